"""What the Newton refinement costs: microseconds per control step with refine off and on, five alternating windows of 200 steps after
warm-up in one process, min / median / max -- covo-online at N = 4 096 (where three more launches are the largest share of a step),
at the headline N = 65 536, and the env-batched covo-online step at 32 x 4 096.
    python scripts/refine_cost.py [--N 4096 65536] [--E 32 --NE 4096]
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

ARMS = (("off", False), ("on", True))


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
    for k, v in us.items():
        print(f"{name:38s} refine {k:4s}: min {min(v):8.2f}  median {np.median(v):8.2f}  max {max(v):8.2f} us/step", flush=True)
    print(f"{name:38s} refine costs {np.median(us['on']) - np.median(us['off']):8.2f} us/step (medians)", flush=True)


def single(N, dev):
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=dev)
    steps = {}
    for arm, refine in ARMS:
        c, cp = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False, refine=refine)
        c.alias_outputs = True
        params = env.default_params
        obs, info, state = env.reset(cr.PRNGKey(1), params)
        st = dict(cp=c.init_control_params)

        def step(c=c, st=st, obs=obs, state=state, params=params, info=info):
            _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
        steps[arm] = step
    report(f"covo-online N={N}", steps)


def batched(E, N, dev):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=dev)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    steps = {}
    for arm, refine in ARMS:
        b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=dev, refine=refine)
        b.set_instances([s[2] for s in states], params)
        noisy = [s[1]["noisy_state"] for s in states]
        b(noisy, keys)
        steps[arm] = lambda b=b: b(None, keys)
    report(f"batched covo-online E={E} N={N}", steps)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    a = ap.parse_args()
    for N in a.N:
        single(N, "cuda:0")
    batched(a.E, a.NE, "cuda:0")
