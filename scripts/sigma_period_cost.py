"""What the Sigma period costs and saves: microseconds per control step of a refresh step (the plain covo-online step: the same handle
with the period off), of a reuse step (sigma_period = 64 after its refresh: 63 of 64 steps shift the last factor) and of the covo-offline
step, five alternating windows of 200 steps after warm-up, min / median / max -- the single step at N = 65 536 and N = 4 096 and the
env-batched step at 32 x 4 096 -- and the shift kernel alone next to the batched Cholesky launch (covo_cholesky) that the simpler route
(gather S(Sigma), factor it, scale) would be built on, 1 and 32 matrices, GPU time between two events around 200 launches.
    python scripts/sigma_period_cost.py [--N 65536] [--E 32 --NE 4096]
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

PERIOD = 64  # the longest period: a window of 200 steps holds 3 or 4 refresh steps (reported: their share is subtracted)


def window(step, n=200):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def report(name, steps):
    for s in steps.values():
        for _ in range(70):
            s()
    us = {k: [] for k in steps}
    for _ in range(5):
        for k, s in steps.items():
            us[k].append(window(s))
    med = {k: float(np.median(v)) for k, v in us.items()}
    for k, v in us.items():
        print(f"{name:34s} {k:24s}: min {min(v):8.2f}  median {med[k]:8.2f}  max {max(v):8.2f} us/step")
    if "period 64" in med and "refresh (period off)" in med:
        reuse = (med["period 64"] * PERIOD - med["refresh (period off)"]) / (PERIOD - 1)
        print(f"{name:34s} {'reuse step (derived)':24s}:        median {reuse:8.2f} us/step")
    return med


def _arms(core, step):
    """The two arms of one handle: the period on, and off (covo_set_step_sigma_period with 1: every step is the plain step)."""
    def on():
        if core.sigma_period != PERIOD:
            core.set_sigma_period(PERIOD)
        step()

    def off():
        if core.sigma_period != 1:
            core.set_sigma_period(1)
        step()
    return on, off


def single(N, dev):
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=dev)
    steps = {}
    for name, kw in (("covo-online", dict(sigma_period=PERIOD)), ("covo-offline", {})):
        c, cp = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=dev, compute_info=False, **kw)
        c.alias_outputs = True
        params = env.default_params
        obs, info, state = env.reset(cr.PRNGKey(1), params)
        cp = c.reset(state, params, c.init_control_params, cr.PRNGKey(2))
        st = dict(cp=cp)

        def step(c=c, st=st, obs=obs, state=state, params=params, info=info):
            _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
        if name == "covo-online":
            steps["period 64"], steps["refresh (period off)"] = _arms(c.core, step)
        else:
            steps["covo-offline"] = step
    report(f"single N={N}", steps)


def batched(E, N, dev):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=dev)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=dev, sigma_period=PERIOD)
    b.set_instances([s[2] for s in states], params)
    b([s[1]["noisy_state"] for s in states], keys)
    steps = {}
    steps["period 64"], steps["refresh (period off)"] = _arms(b.core, lambda: b(None, keys))
    report(f"batched covo-online E={E} N={N}", steps)


def kernels(dev):
    """The shift kernel alone and the batched Cholesky launch alone, on the factors / covariances of random SPD matrices."""
    from covo_mpc_amd.controllers._core import SamplingCore
    core = SamplingCore(256, 32, 0.01, 1.0, device=dev, use_graph=False, compute_info=False)
    g = torch.Generator().manual_seed(0)
    for E in (1, 32):
        A = torch.randn(E, 128, 128, generator=g, dtype=torch.float64)
        Sig = (0.05 * A @ A.transpose(1, 2) + 0.2 * torch.eye(128, dtype=torch.float64))
        L = torch.linalg.cholesky(Sig).float().to(dev).contiguous()
        Sig = Sig.float().to(dev).contiguous()
        for name, fn in (("sigma_shift", lambda: core.sigma_shift(L, 0.5)), ("covo_cholesky", lambda: core.cholesky(Sig, 128, E))):
            for _ in range(20):
                fn()
            best = 1e30
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(200):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                best = min(best, e0.elapsed_time(e1) * 1e3 / 200)
            print(f"{'kernel alone, ' + str(E) + ' matrices':34s} {name:24s}: {best:8.2f} us/launch (back to back, with the output allocation)")
    core.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    a = ap.parse_args()
    kernels("cuda:0")
    single(4096, "cuda:0")
    single(a.N, "cuda:0")
    batched(a.E, a.NE, "cuda:0")
