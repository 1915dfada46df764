"""What the Riccati refinement costs: microseconds per control step with riccati off and on, five alternating windows of 200 steps
after warm-up in one process, min / median / max -- covo-online at N = 4 096 (where the extra launches are the largest share of a
step), at the headline N = 65 536, the env-batched covo-online step at 32 x 4 096 -- and the sweep's launches alone: covo_riccati
(the Hessian's first two launches and the sweep kernel) next to covo_cost_gradient (the Hessian's first launch and the costate walk),
whose difference brackets the sweep kernel itself.
    python scripts/riccati_cost.py [--N 4096 65536] [--E 32 --NE 4096] [--controller covo-online]
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
from covo_mpc_amd.dynamics.dataclass import as_device_state  # noqa: E402

ARMS = (("off", False), ("on", True))


def window(step, n=200):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def report(name, steps, what="riccati", warm=50):
    for s in steps.values():
        for _ in range(warm):
            s()
    us = {k: [] for k in steps}
    for _ in range(5):
        for k, s in steps.items():
            us[k].append(window(s))
    for k, v in us.items():
        print(f"{name:38s} {what} {k:8s}: min {min(v):8.2f}  median {np.median(v):8.2f}  max {max(v):8.2f} us", flush=True)
    a, b = list(steps)
    print(f"{name:38s} {what} {b} - {a}: {np.median(us[b]) - np.median(us[a]):8.2f} us (medians)", flush=True)


def single(name, N, dev):
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=dev)
    steps = {}
    for arm, riccati in ARMS:
        c, cp = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=dev, compute_info=False, riccati=riccati)
        c.alias_outputs = True
        params = env.default_params
        obs, info, state = env.reset(cr.PRNGKey(1), params)
        st = dict(cp=c.init_control_params)
        if name == "covo-offline":
            st["cp"] = c.reset(state, params, st["cp"], cr.PRNGKey(2))

        def step(c=c, st=st, obs=obs, state=state, params=params, info=info):
            _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
        steps[arm] = step
    report(f"{name} N={N}", steps)
    return c, params, info


def batched(E, N, dev):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=dev)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    steps = {}
    for arm, riccati in ARMS:
        b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=dev, riccati=riccati)
        b.set_instances([s[2] for s in states], params)
        noisy = [s[1]["noisy_state"] for s in states]
        b(noisy, keys)
        steps[arm] = lambda b=b: b(None, keys)
    report(f"batched covo-online E={E} N={N}", steps)


def sweep_alone(c, params, info, dev, batches=(1, 32)):
    """the stand-alone launches at the controller's own state and mean: gradient = KB + walk; riccati = KB + chains + sweep"""
    core = c.core
    ds = as_device_state(info["noisy_state"], dev)
    pc = c._params_c(params)
    for n in batches:
        a = c.init_control_params.a_mean.reshape(1, -1).repeat(n, 1).contiguous()
        report(f"stand-alone, batch {n}", {"gradient": lambda a=a: core.cost_gradient(ds, pc, a),
                                           "riccati": lambda a=a: core.riccati(ds, pc, a)}, what="launches")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    ap.add_argument("--controller", default="covo-online")
    a = ap.parse_args()
    for N in a.N:
        c, params, info = single(a.controller, N, "cuda:0")
    batched(a.E, a.NE, "cuda:0")
    sweep_alone(c, params, info, "cuda:0")
