"""What an iLQR control step costs: microseconds per step at k = 1, 2, 4 iterations, with every step planning (m = 1) and under
plan_hold=4, for the single controller and for 32 env-batched instances -- medians of five windows of 200 steps after warm-up in one
process (the protocol of scripts/riccati_cost.py) -- and, in the same process, the yardstick: the MPPI step at N = 4 096 with and
without riccati=True, riccati_feedback=True, whose on-minus-off difference is the same launches as one iteration.  The per-iteration
increment (t_{k=4} - t_{k=1}) / 3 is printed next to it, with the spread of three repeated yardstick measurements.
    python scripts/ilqr_cost.py [--E 32] [--N 4096]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402

KEY = np.array([3, 4], dtype=np.uint32)


def window(step, n=200):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def medians(steps, warm=50):
    """{arm: step} -> {arm: (min, median, max)} of five alternating windows"""
    for s in steps.values():
        for _ in range(warm):
            s()
    us = {k: [] for k in steps}
    for _ in range(5):
        for k, s in steps.items():
            us[k].append(window(s))
    return {k: (min(v), float(np.median(v)), max(v)) for k, v in us.items()}


def show(name, res):
    for k, (lo, med, hi) in res.items():
        print(f"{name:34s} {k:14s}: min {lo:8.2f}  median {med:8.2f}  max {hi:8.2f} us", flush=True)


def zigzag_env(dev):
    return cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                          generate_noisy_state=True, device=dev)


def single_step(env, name, dev, N=4096, **kw):
    c, cp = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=dev, compute_info=False, **kw)
    c.alias_outputs = True
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(1), params)
    st = dict(cp=c.init_control_params)

    def step():
        _, st["cp"], _ = c(obs, state, params, KEY, st["cp"], info)
    return step


def ilqr_single(dev):
    env = zigzag_env(dev)
    out = {}
    for m in (1, 4):
        res = medians({f"k={k}": single_step(env, "ilqr", dev, iters=k, plan_hold=m) for k in (1, 2, 4)})
        show(f"ilqr single m={m}", res)
        out[m] = res
    return out


def ilqr_batched(E, dev):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=dev)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    dp = env.default_params
    th = (dp.m * dp.g / dp.max_thrust) * 2.0 - 1.0
    mean0 = np.tile(np.array([th, 0.0, 0.0, 0.0], dtype=np.float32), 32)
    out = {}
    for m in (1, 4):
        steps = {}
        for k in (1, 2, 4):
            b = cm.controllers.BatchedILQRController(env, E, 32, iters=k, plan_hold=m, a_mean_init=mean0, device=dev)
            b.set_instances([s[2] for s in states], params)
            b([s[1]["noisy_state"] for s in states], keys)
            steps[f"k={k}"] = lambda b=b: b(None, keys)
        res = medians(steps)
        show(f"ilqr batched E={E} m={m}", res)
        out[m] = res
    return out


def yardstick(N, dev, repeats=3):
    """MPPI at N with and without the refinement, `repeats` times: the on-minus-off differences of the medians"""
    env = zigzag_env(dev)
    diffs = []
    for r in range(repeats):
        res = medians({"off": single_step(env, "mppi", dev, N), "on": single_step(env, "mppi", dev, N, riccati=True, riccati_feedback=True)})
        show(f"mppi N={N} (repeat {r})", res)
        diffs.append(res["on"][1] - res["off"][1])
    return diffs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--N", type=int, default=4096)
    a = ap.parse_args()
    dev = "cuda:0"
    s = ilqr_single(dev)
    b = ilqr_batched(a.E, dev)
    y = yardstick(a.N, dev)
    print(f"yardstick (mppi on - off, medians): {['%.2f' % v for v in y]} us; spread {max(y) - min(y):.2f} us", flush=True)
    for name, res in (("single", s[1]), (f"batched E={a.E}", b[1])):
        inc = (res["k=4"][1] - res["k=1"][1]) / 3.0
        print(f"per-iteration increment, {name}: {inc:.2f} us (yardstick median {np.median(y):.2f} us)", flush=True)
