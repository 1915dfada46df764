"""What the ESS floor costs: microseconds per control step without it, with it attached but inactive (lam0 = 5: one solver pass) and
with it active (lam0 = 0.01, ess_min = N / 16: the solver bisects), five alternating windows of 200 steps after warm-up, min /
median / max -- the single covo-online step at N = 65 536 and N = 4 096 and the env-batched covo-online step.
    python scripts/ess_floor_cost.py [--N 65536] [--E 32 --NE 4096]
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

# tag -> (lam0, floor as a fraction of N or None)
ARMS = (("off", "0.01", None), ("off lam0=5", "5.0", None), ("inactive", "5.0", 1 / 16), ("active", "0.01", 1 / 16))


def window(step, n=200):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def report(name, steps, rows):
    for s in steps.values():
        for _ in range(50):
            s()
    us = {k: [] for k in steps}
    for _ in range(5):
        for k, s in steps.items():
            us[k].append(window(s))
    for k, v in us.items():
        r = rows[k]() if rows.get(k) else None
        extra = "" if r is None else f"   lam_eff {r[0]:.5g}  ESS(lam0) {r[2]:.4g}  evaluations {int(r[3])}"
        print(f"{name:34s} floor {k:11s}: min {min(v):8.2f}  median {np.median(v):8.2f}  max {max(v):8.2f} us/step{extra}")


def single(N, dev):
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=dev)
    steps, rows = {}, {}
    for tag, lam, frac in ARMS:
        c, cp = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam{lam}", device=dev, compute_info=False,
                                       ess_min=None if frac is None else frac * N)
        c.alias_outputs = True
        params = env.default_params
        obs, info, state = env.reset(cr.PRNGKey(1), params)
        st = dict(cp=c.init_control_params)

        def step(c=c, st=st, obs=obs, state=state, params=params, info=info):
            _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
        steps[tag] = step
        if frac is not None:
            rows[tag] = lambda c=c: c.core.lam_eff[0].cpu().numpy()
    report(f"covo-online N={N}", steps, rows)


def batched(E, N, dev):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=dev)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    steps, rows = {}, {}
    for tag, lam, frac in ARMS:
        b = cm.controllers.BatchedCoVOController(env, E, N, 32, float(lam), a_mean_init=cp0.a_mean, device=dev,
                                                 ess_min=None if frac is None else frac * N)
        b.set_instances([s[2] for s in states], params)
        noisy = [s[1]["noisy_state"] for s in states]
        b(noisy, keys)
        steps[tag] = lambda b=b: b(None, keys)
        if frac is not None:
            rows[tag] = lambda b=b: b.lam_eff[0].cpu().numpy()
    report(f"batched covo-online E={E} N={N}", steps, rows)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    a = ap.parse_args()
    single(a.N, "cuda:0")
    single(4096, "cuda:0")
    batched(a.E, a.NE, "cuda:0")
