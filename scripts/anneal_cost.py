"""What the annealed MPPI step costs: microseconds per control step, five alternating windows of 200 steps after warm-up in
one process, min / median / max, for three arms at k = 4 passes --
    dial          DialController(iters=4, beta_pass=0.5, beta_stage=0.9, temp=0.1): schedule launch + standardising solver per pass
    dial-sched    the same with temp=None: the schedule launch alone on top of MPPI's passes (no solver, no staged update)
    mppi          MPPIController(iters=4)
    mppi-ess      MPPIController(iters=4, ess_min=64): the like-for-like arm -- the same staged sequence with the other solver
at N = 4 096 and 65 536, and for 32 x 4 096 env-batched instances against the staged batched MPPI step (with and without ess_min=64).
Then the two solver launches alone on the same costs -- covo_cost_standardise against covo_ess_lambda with the floor inactive (one pass
over the costs) -- as R launches captured into one graph and replayed, device events around the replays.
    python scripts/anneal_cost.py [--Ns 4096 65536] [--E 32 --NE 4096] [--k 4]
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

DEV = "cuda:0"


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
        print(f"{name:28s} {k:12s}: min {min(v):8.2f}  median {np.median(v):8.2f}  max {max(v):8.2f} us/step", flush=True)
    return {k: float(np.median(v)) for k, v in us.items()}


def single(N, k):
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    arms = {"dial": ("dial", dict(iters=k)), "dial-sched": ("dial", dict(iters=k, temp=None)), "mppi": ("mppi", dict(iters=k)),
            "mppi-ess": ("mppi", dict(iters=k, ess_min=64.0))}
    steps = {}
    for arm, (name, kw) in arms.items():
        c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV, compute_info=False, **kw)
        c.alias_outputs = True
        params = env.default_params
        obs, info, state = env.reset(cr.PRNGKey(1), params)
        st = dict(cp=c.reset(state, params, c.init_control_params, cr.PRNGKey(2)))

        def step(c=c, st=st, obs=obs, state=state, params=params, info=info):
            _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
        steps[arm] = step
    m = report(f"single N={N} k={k}", steps)
    print(f"{'':28s} dial - mppi-ess {m['dial'] - m['mppi-ess']:+.2f}   dial-sched - mppi {m['dial-sched'] - m['mppi']:+.2f} us/step "
          f"({(m['dial-sched'] - m['mppi']) / k:+.2f} per pass)", flush=True)


def batched(E, N, k):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=DEV)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "mppi", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    B = cm.controllers
    arms = {"dial": lambda: B.BatchedDialController(env, E, N, 32, 0.01, iters=k, a_mean_init=cp0.a_mean, device=DEV),
            "dial-sched": lambda: B.BatchedDialController(env, E, N, 32, 0.01, iters=k, temp=None, a_mean_init=cp0.a_mean, device=DEV),
            "mppi": lambda: B.BatchedMPPIController(env, E, N, 32, 0.01, iters=k, staged=True, a_mean_init=cp0.a_mean, device=DEV),
            "mppi-ess": lambda: B.BatchedMPPIController(env, E, N, 32, 0.01, iters=k, staged=True, ess_min=64.0, a_mean_init=cp0.a_mean,
                                                        device=DEV)}
    steps = {}
    for arm, make in arms.items():
        b = make()
        b.set_instances([s[2] for s in states], params)
        b([s[1]["noisy_state"] for s in states], keys)
        steps[arm] = lambda b=b: b(None, keys)
    m = report(f"batched E={E} N={N} k={k}", steps)
    print(f"{'':28s} dial - mppi-ess {m['dial'] - m['mppi-ess']:+.2f}   dial-sched - mppi {m['dial-sched'] - m['mppi']:+.2f} us/step",
          flush=True)


def solvers_alone(N, E=1, R=200, replays=10):
    """R launches of each solver in one captured graph; microseconds per launch from device events around `replays` replays"""
    core = cm.controllers._core.SamplingCore(256, 32, 0.01, 1.0, device=DEV, compute_info=False)
    g = torch.Generator(device="cpu").manual_seed(7)
    cost = (5.0 + 3.0 * torch.randn((E, N), generator=g)).to(DEV)
    out = torch.empty((E, 4), dtype=torch.float32, device=DEV)
    lib, h = core.lib, core.h
    calls = {"cost_standardise": lambda s: lib.covo_cost_standardise(h, _lib.ptr(cost), N, E, 0.01, 0.1, _lib.ptr(out), s),
             # lam0 = 10: ESS(lam0) ~ N at these costs, the floor (ess_min = 2) is inactive -> one pass over the costs
             "ess_lambda inactive": lambda s: lib.covo_ess_lambda(h, _lib.ptr(cost), N, E, 10.0, 2.0, _lib.ptr(out), s)}
    for name, call in calls.items():
        _lib.check(call(core.stream()), name)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(R):
                _lib.check(call(core.stream()), name)
        graph.replay()
        torch.cuda.synchronize()
        best = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            best.append(e0.elapsed_time(e1) * 1e3 / (R * replays))
        evals = float(out[0, 3]) if name.startswith("ess") else float("nan")
        print(f"solver alone N={N:6d} E={E:2d} {name:22s}: min {min(best):6.2f}  median {np.median(best):6.2f}  max {max(best):6.2f} us/launch"
              + (f"  (ESS evaluations {evals:.0f})" if name.startswith("ess") else ""), flush=True)
    core.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--Ns", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    ap.add_argument("--k", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("anneal_cost.py measures on the GPU; there is none")
    for N in a.Ns:
        single(N, a.k)
    batched(a.E, a.NE, a.k)
    for N in a.Ns:
        solvers_alone(N)
    solvers_alone(a.NE, E=a.E)
