"""What Sigma adapt costs: microseconds per control step of covo-online at sigma_period = 64 with sigma_adapt on and off ON THE SAME
HANDLE (off: the reuse step with the shift kernel and compute_post_cov=True, as before this feature), five alternating windows of 200
steps after warm-up, min / median / max -- the single step at N = 4 096 and N = 65 536 and the env-batched step at 32 x 4 096 -- and
the kernel alone next to the shift kernel, 1 and 32 matrices, GPU time between two events around 200 back-to-back launches.  Switching
an arm restarts the schedule and drops the step graphs: every window starts with a refresh step and holds four of them, in both arms.
    python scripts/sigma_adapt_cost.py [--N 65536] [--E 32 --NE 4096] [--gamma 0.2]
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

PERIOD = 64


def window(step, n=200):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def report(name, core, step, gamma):
    def arm(g):
        def run():
            if core.sigma_adapt_gamma != g:
                core.set_sigma_adapt(g)
            step()
        return run
    steps = {"sigma_adapt off": arm(0.0), f"sigma_adapt {gamma}": arm(gamma)}
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
    on, off = med[f"sigma_adapt {gamma}"], med["sigma_adapt off"]
    print(f"{name:34s} {'on minus off, per reuse step':24s}:        median {(on - off) * 200.0 / 196.0:8.2f} us (196 of a window's 200 steps reuse)")
    rows = core.sigma_adapt_rows.cpu().numpy()
    print(f"{name:34s} {'last rows':24s}: fallback {rows[:, 0].max():.0f}, c in [{rows[:, 1].min():.4f}, {rows[:, 1].max():.4f}]")


def single(N, dev, gamma):
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=dev)
    c, cp = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False, sigma_period=PERIOD,
                                   sigma_adapt=gamma)
    c.alias_outputs = True
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(1), params)
    st = dict(cp=c.reset(state, params, c.init_control_params, cr.PRNGKey(2)))

    def step():
        _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
    report(f"single N={N}", c.core, step, gamma)
    c.core.close()


def batched(E, N, dev, gamma):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=dev)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=dev, sigma_period=PERIOD,
                                             sigma_adapt=gamma)
    b.set_instances([s[2] for s in states], params)
    b([s[1]["noisy_state"] for s in states], keys)
    report(f"batched covo-online E={E} N={N}", b.core, lambda: b(None, keys), gamma)
    b.core.close()


def kernels(dev, gamma):
    """The adapt kernel alone (at gamma and at 0) next to the shift kernel, on the factors of random SPD matrices and a rank-64 C."""
    from covo_mpc_amd.controllers._core import SamplingCore
    core = SamplingCore(256, 32, 0.01, 1.0, device=dev, use_graph=False, compute_info=False)
    g = torch.Generator().manual_seed(0)
    for E in (1, 32):
        A = torch.randn(E, 128, 128, generator=g, dtype=torch.float64)
        Sig = (0.05 * A @ A.transpose(1, 2) + 0.2 * torch.eye(128, dtype=torch.float64))
        L = torch.linalg.cholesky(Sig).float().to(dev).contiguous()
        Y = torch.randn(E, 128, 64, generator=g, dtype=torch.float64) * 0.3
        Cm = (Y @ Y.transpose(1, 2) / 64.0).float().to(dev).contiguous()
        for name, fn in (("sigma_shift", lambda: core.sigma_shift(L, 0.5)), (f"sigma_adapt gamma={gamma}", lambda: core.sigma_adapt(L, Cm, gamma)),
                         ("sigma_adapt gamma=0", lambda: core.sigma_adapt(L, Cm, 0.0))):
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
    ap.add_argument("--gamma", type=float, default=0.2)
    a = ap.parse_args()
    kernels("cuda:0", a.gamma)
    single(4096, "cuda:0", a.gamma)
    single(a.N, "cuda:0", a.gamma)
    batched(a.E, a.NE, "cuda:0", a.gamma)
