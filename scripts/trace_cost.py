"""What the flight recorder costs: microseconds per control step with and without `compute_plan`, five alternating windows of 200
steps after warm-up, min / median / max -- covo-online at N = 65 536 and 4 096, MPPI at N = 1 024 (where one launch is the largest
share of a step), the env-batched covo-online step; and the device closed loop (run_episode) with and without the trace.
    python scripts/trace_cost.py [--N 65536] [--E 32 --NE 4096]
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


def report(name, steps, warm=50, per_window=1):
    for s in steps.values():
        for _ in range(warm):
            s()
    us = {k: [] for k in steps}
    for _ in range(5):
        for k, s in steps.items():
            us[k].append(window(s, max(200 // per_window, 1)) / per_window)
    for k, v in us.items():
        print(f"{name:38s} plan {k:3s}: min {min(v):8.2f}  median {np.median(v):8.2f}  max {max(v):8.2f} us/step")


def _env(dev):
    return cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                          generate_noisy_state=True, device=dev)


def single(name, N, dev):
    env = _env(dev)
    steps = {}
    for tag, on in (("off", False), ("on", True)):
        c, cp = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=dev, compute_info=False, compute_plan=on)
        c.alias_outputs = True
        params = env.default_params
        obs, info, state = env.reset(cr.PRNGKey(1), params)
        st = dict(cp=c.init_control_params)

        def step(c=c, st=st, obs=obs, state=state, params=params, info=info):
            _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
        steps[tag] = step
    report(f"{name} N={N}", steps)


def batched(E, N, dev):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=dev)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    steps = {}
    for tag, on in (("off", False), ("on", True)):
        b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=dev, compute_plan=on)
        b.set_instances([s[2] for s in states], params)
        noisy = [s[1]["noisy_state"] for s in states]
        b(noisy, keys)
        steps[tag] = lambda b=b: b(None, keys)
    report(f"batched covo-online E={E} N={N}", steps)


def closed_loop(name, N, dev, seg=50):
    """run_episode segments of `seg` steps (control step + device env step, enqueued by one C call), trace attached or not"""
    env = _env(dev)
    steps = {}
    for tag, on in (("off", False), ("on", True)):
        c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=dev, compute_info=False, compute_plan=on)
        c.alias_outputs = True
        params = env.default_params
        st = {}

        def episode(c=c, st=st, params=params):
            if "ep" not in st or st["ep"].n_steps + seg > params.max_steps_in_episode:
                st["ep"] = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (c.core.lib, c.core.h), dev)
                st["cp"] = c.init_control_params
                st["rng"] = cr.PRNGKey(43)
            st["cp"], st["rng"] = c.run_episode(st["ep"], params, st["cp"], st["rng"], seg)
        steps[tag] = episode
    report(f"closed loop {name} N={N}", steps, warm=4, per_window=seg)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    a = ap.parse_args()
    single("covo-online", a.N, "cuda:0")
    single("covo-online", 4096, "cuda:0")
    single("mppi", 1024, "cuda:0")
    batched(a.E, a.NE, "cuda:0")
    closed_loop("mppi", 1024, "cuda:0")
    closed_loop("covo-online", 4096, "cuda:0")
