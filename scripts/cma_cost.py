"""What a CMA step costs: microseconds per control step of the CMA controller next to MPPI and covo-online IN THE SAME SESSION, five
alternating windows of 200 steps after warm-up, min / median / max -- the single step at N = 4 096 and N = 65 536 and the env-batched
step at 32 x 4 096 -- and the step-size kernel alone (csrc/cma_path.hip) next to the shape kernel it follows (csrc/sigma_adapt.hip), 1 and
32 matrices, GPU time between two events around 200 back-to-back launches.  The controllers step on one fixed state with one fixed key:
the times are those of the launches, not of a closed loop.
    python scripts/cma_cost.py [--N 65536] [--E 32 --NE 4096]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402

NAMES = ("mppi", "covo-online", "cma")


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
    for k, v in us.items():
        print(f"{name:34s} {k:24s}: min {min(v):8.2f}  median {float(np.median(v)):8.2f}  max {max(v):8.2f} us/step")


def single(N, dev):
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=dev)
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(1), params)
    steps, cores = {}, []
    for name in NAMES:
        c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=dev, compute_info=False)
        c.alias_outputs = True
        st = dict(cp=c.reset(state, params, c.init_control_params, cr.PRNGKey(2)))

        def step(c=c, st=st):
            _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
        steps[name] = step
        cores.append(c.core)
    report(f"single N={N}", steps)
    rows = cores[-1].cma_rows.cpu().numpy()
    print(f"{'single N=' + str(N):34s} {'cma, last row':24s}: s {rows[0, 0]:.4f}  |p| {rows[0, 2]:.3f}  mu_eff {rows[0, 4]:.2f}  flags {rows[0, 7]:.0f}")
    for core in cores:
        core.close()


def batched(E, N, dev):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=dev)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    kw = dict(a_mean_init=cp0.a_mean, device=dev)
    bs = {"mppi": cm.controllers.BatchedMPPIController(env, E, N, 32, 0.01, **kw),
          "covo-online": cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, **kw),
          "cma": cm.controllers.BatchedCMAController(env, E, N, 32, 0.01, **kw)}
    steps = {}
    for name, b in bs.items():
        b.set_instances([s[2] for s in states], params)
        b([s[1]["noisy_state"] for s in states], keys)
        steps[name] = (lambda b=b: b(None, keys))
    report(f"batched E={E} N={N}", steps)
    rows = bs["cma"].cma_rows.cpu().numpy()
    print(f"{'batched E=' + str(E):34s} {'cma, last rows':24s}: s in [{rows[:, 0].min():.4f}, {rows[:, 0].max():.4f}]  flags {rows[:, 7].max():.0f}")
    for b in bs.values():
        b.core.close()
    c0.core.close()


def kernels(dev):
    """The step-size kernel alone next to the shape kernel, on the factors of random SPD matrices and a rank-64 C."""
    from covo_mpc_amd.controllers._core import SamplingCore
    core = SamplingCore(256, 32, 0.01, 1.0, device=dev, use_graph=False, compute_info=False)
    g = torch.Generator().manual_seed(0)
    for E in (1, 32):
        A = torch.randn(E, 128, 128, generator=g, dtype=torch.float64)
        Sig = (0.05 * A @ A.transpose(1, 2) + 0.2 * torch.eye(128, dtype=torch.float64))
        L = torch.linalg.cholesky(Sig).float().to(dev).contiguous()
        Y = torch.randn(E, 128, 64, generator=g, dtype=torch.float64) * 0.3
        Cm = (Y @ Y.transpose(1, 2) / 64.0).float().to(dev).contiguous()
        Sh, Lh, srows = core.sigma_adapt(L, Cm, 0.2)
        aux = torch.zeros((E, _lib.COVO_POST_AUX_FLOATS), device=dev)
        aux[:, :128] = (0.05 * torch.randn(E, 128, generator=g)).to(dev)
        aux[:, 128] = 1.0
        ess = torch.full((E,), 7.3, device=dev)
        p, ls = torch.zeros((E, 128), dtype=torch.float64, device=dev), torch.zeros((E,), dtype=torch.float64, device=dev)
        Lo, So, rows = torch.empty_like(Lh), torch.empty_like(Sh), torch.zeros((E, _lib.COVO_CMA_FLOATS), device=dev)
        ptr = _lib.ptr

        def path(on):  # (the C entry itself: the Python wrapper adds small fills of its own)
            _lib.check(core.lib.covo_cma_path(core.h, ptr(L), ptr(aux), _lib.COVO_POST_AUX_FLOATS, ptr(ess), 1, ptr(Lh), ptr(Sh), ptr(srows), E,
                                              256, on, 1.0, 0.1, 4.0, ptr(p), ptr(ls), ptr(Lo), ptr(So), ptr(rows), core.stream()),
                       "covo_cma_path")
        for name, fn in (("sigma_adapt gamma=0.2", lambda: core.sigma_adapt(L, Cm, 0.2)), ("cma_path", lambda: path(1)),
                         ("cma_path, step_size off", lambda: path(0))):
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
            print(f"{'kernel alone, ' + str(E) + ' matrices':34s} {name:24s}: {best:8.2f} us/launch (back to back)")
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
