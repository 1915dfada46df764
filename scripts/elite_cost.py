"""What the elite-set update costs: microseconds per control step without it (the same handle, detached), with elite = N / 16 and,
in the same session, with the ESS floor active (lam0 = 0.01, ess_min = N / 16: the solver bisects), five alternating windows of 200
steps after warm-up, min / median / max -- the single covo-online step at N = 65 536 and N = 4 096, MPPI at N = 1 024 and the
env-batched covo-online step.
    python scripts/elite_cost.py [--N 65536] [--E 32 --NE 4096]
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

from covo_mpc_amd import _lib  # noqa: E402

FRAC = 1 / 16  # elite = ess_min = N / 16


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
        print(f"{name:34s} {k:14s}: min {min(v):8.2f}  median {np.median(v):8.2f}  max {max(v):8.2f} us/step   {rows[k]() if k in rows else ''}")


def _elite_row(t):
    r = t[0].cpu().numpy()
    return f"cost_min {r[2]:.5g}  cost_kth {r[3]:.5g}  K {int(r[4])}  ties {int(r[5])}"


def _arms(core, step, elite_K):
    """The three arms of one elite handle: attached, detached (covo_set_step_elite with K = 0: the softmax update), attached."""
    def attach(K):
        _lib.check(core.lib.covo_set_step_elite(core.h, K, _lib.ptr(core.elite_rows), int(core.elite_rows.shape[0])), "covo_set_step_elite")

    def on():
        if not on.state:
            attach(elite_K)
            on.state = True
        step()

    def off():
        if on.state:
            attach(0)
            on.state = False
        step()
    on.state = True
    return on, off


def single(name, N, dev):
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=dev)
    steps, rows = {}, {}
    for tag, kw in (("elite", dict(elite=int(FRAC * N))), ("ess_min active", dict(ess_min=FRAC * N))):
        c, cp = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=dev, compute_info=False, **kw)
        c.alias_outputs = True
        params = env.default_params
        obs, info, state = env.reset(cr.PRNGKey(1), params)
        st = dict(cp=c.init_control_params)

        def step(c=c, st=st, obs=obs, state=state, params=params, info=info):
            _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
        if tag == "elite":
            steps["elite"], steps["detached"] = _arms(c.core, step, int(FRAC * N))
            rows["elite"] = lambda c=c: _elite_row(c.core.elite_rows)
        else:
            steps[tag] = step
            rows[tag] = lambda c=c: "lam_eff %.5g  evaluations %d" % tuple(c.core.lam_eff[0].cpu().numpy()[[0, 3]])
    report(f"{name} N={N}", steps, rows)


def batched(E, N, dev):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=dev)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    steps, rows = {}, {}
    for tag, kw in (("elite", dict(elite=int(FRAC * N))), ("ess_min active", dict(ess_min=FRAC * N))):
        b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=dev, **kw)
        b.set_instances([s[2] for s in states], params)
        noisy = [s[1]["noisy_state"] for s in states]
        b(noisy, keys)
        step = lambda b=b: b(None, keys)
        if tag == "elite":
            steps["elite"], steps["detached"] = _arms(b.core, step, int(FRAC * N))
            rows["elite"] = lambda b=b: _elite_row(b.elite)
        else:
            steps[tag] = step
            rows[tag] = lambda b=b: "lam_eff %.5g  evaluations %d" % tuple(b.lam_eff[0].cpu().numpy()[[0, 3]])
    report(f"batched covo-online E={E} N={N}", steps, rows)


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
