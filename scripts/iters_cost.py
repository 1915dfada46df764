"""What a pass costs: microseconds per control step at iters = 1 (nothing attached: the launches of a step without the option), 2, 4
and 8, five alternating windows of 200 steps after warm-up in one process, min / median / max -- covo-online at the headline
N = 65 536, covo-offline at N = 8 192, MPPI at N = 1 024 and the env-batched step at 32 x 4 096 in its three modes.  The last column
is the median over k times the iters = 1 median of the same config.
    python scripts/iters_cost.py [--N 65536] [--E 32 --NE 4096] [--ks 1 2 4 8]
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


def window(step, n=200):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def report(name, steps, warm=50):
    for s in steps.values():
        for _ in range(warm):
            s()
    us = {k: [] for k in steps}
    for _ in range(5):
        for k, s in steps.items():
            us[k].append(window(s))
    base = np.median(us[min(us)])
    for k, v in us.items():
        print(f"{name:38s} iters {k:2d}: min {min(v):8.2f}  median {np.median(v):8.2f}  max {max(v):8.2f} us/step"
              f"   median / (k x iters-1 median) {np.median(v) / (k * base):5.2f}", flush=True)


def single(name, N, dev, ks):
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=dev)
    steps = {}
    for k in ks:
        c, cp = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=dev, compute_info=False, iters=k)
        c.alias_outputs = True
        params = env.default_params
        obs, info, state = env.reset(cr.PRNGKey(1), params)
        st = dict(cp=c.reset(state, params, c.init_control_params, cr.PRNGKey(2)))

        def step(c=c, st=st, obs=obs, state=state, params=params, info=info):
            _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
        steps[k] = step
    report(f"{name} N={N}", steps)


def batched(name, E, N, dev, ks):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=dev)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    steps, tables = {}, None
    for k in ks:
        if name == "mppi":
            b = cm.controllers.BatchedMPPIController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=dev, iters=k)
        else:
            b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=dev, mode=name.split("-")[1],
                                                     iters=k)
        b.set_instances([s[2] for s in states], params)
        if name == "covo-offline":
            if tables is None:
                tables = b.reset([s[2] for s in states], params, [cr.PRNGKey(400 + e) for e in range(E)])
            else:
                b.set_tables(*tables)
        noisy = [s[1]["noisy_state"] for s in states]
        b(noisy, keys)
        steps[k] = lambda b=b: b(None, keys)
    report(f"batched {name} E={E} N={N}", steps)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 2, 4, 8])
    a = ap.parse_args()
    single("covo-online", a.N, "cuda:0", a.ks)
    single("covo-offline", 8192, "cuda:0", a.ks)
    single("mppi", 1024, "cuda:0", a.ks)
    for mode in ("covo-online", "covo-offline", "mppi"):
        batched(mode, a.E, a.NE, "cuda:0", a.ks)
