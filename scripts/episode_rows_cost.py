"""What the episode logs of the attachments' rows (covo_set_episode_rows) cost: milliseconds per 300-step episode run by the device
closed loop with the logs attached and detached ON THE SAME HANDLE, five alternating windows after warm-up, min / median / max; a window
is one episode, the host clock around run_episode and a synchronise (the episode's construction -- a reset on the host -- is outside it).
  single   covo-online N = 4 096, ess_min = 64: the temperature log
  batched  covo-online 32 x 4 096, sigma_period = 4, sigma_adapt = 0.1: the Sigma log and the posterior covariance's side row (one launch)
    python scripts/episode_rows_cost.py [--steps 300] [--E 32 --NE 4096]
--off-only times the detached arm alone, 2 x 5 windows.  It asks nothing of the library that a build without the logs lacks: run from
two checkouts in turn it shows whether the drivers' null check costs an episode without logs anything.
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
from covo_mpc_amd.controllers._core import EPISODE_LOGS  # noqa: E402

HAS_ROWS = hasattr(_lib, "COVO_HAS_EPISODE_ROWS")
ROW_LOGS = {name: entry[3] for name, entry in EPISODE_LOGS.items() if HAS_ROWS and entry[3] is not None}


def set_arm(core, attached):
    """attached: the core binds every log it fills (its own attach_log); else the row logs are unbound and stay so."""
    core.__dict__.pop("attach_log", None)
    if attached or not HAS_ROWS:
        return
    for kind in ROW_LOGS.values():
        _lib.check(core.lib.covo_set_episode_rows(core.h, kind, None, 0), "covo_set_episode_rows")
    attach = core.attach_log
    core.attach_log = lambda name, episode, rows_left: None if name in ROW_LOGS else attach(name, episode, rows_left)


def report(name, core, episode, arms):
    """episode(): builds one and returns the function that runs it"""
    def window(attached):
        set_arm(core, attached)
        run = episode()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ep = run()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        filled = [n for n in ROW_LOGS if getattr(ep, n, None) is not None]
        assert bool(filled) == bool(attached and HAS_ROWS), (attached, filled)
        return ms, filled
    for _, attached in arms:  # the first episodes capture the step graphs
        window(attached)
        window(attached)
    ms = {k: [] for k, _ in arms}
    logs = {}
    for _ in range(5):
        for k, attached in arms:
            t, logs[k] = window(attached)
            ms[k].append(t)
    for k, v in ms.items():
        print(f"{name:34s} {k:12s}: min {min(v):8.3f}  median {np.median(v):8.3f}  max {max(v):8.3f} ms/episode  {' '.join(logs[k])}")
    if len(arms) == 2 and arms[0][1] != arms[1][1]:
        on, off = (np.median(ms[k]) for k, a in sorted(arms, key=lambda x: not x[1]))
        print(f"{name:34s} {'on minus off':12s}:        median {(on - off) * 1e3 / STEPS:8.3f} us/step")


def single(N, dev, arms):
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=dev)
    c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False, ess_min=64)
    c.alias_outputs = True
    params = env.default_params

    def episode():
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(21), params, (c.core.lib, c.core.h), c.core.device)
        cp = c.reset(ep.state0, params, c.init_control_params, cr.PRNGKey(22))

        def run():
            c.run_episode(ep, params, cp, cr.PRNGKey(23), STEPS)
            return ep
        return run
    report(f"single covo-online N={N}", c.core, episode, arms)
    c.core.close()


def batched(E, N, dev, arms):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=dev)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False)
    c0.core.close()
    b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=dev, sigma_period=4, sigma_adapt=0.1)
    a_mean0 = b.a_mean.clone()
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])

    def episode():
        ep = cm.envs.BatchedDeviceEpisode(env, [cr.PRNGKey(200 + e) for e in range(E)], params, (b.core.lib, b.core.h), b.core.device)
        b.a_mean.copy_(a_mean0)
        b.reset(None, None, None)  # the Sigma schedule restarts

        def run():
            b.run_episode(ep, keys, STEPS)
            return ep
        return run
    report(f"batched covo-online E={E} N={N}", b.core, episode, arms)
    b.core.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    ap.add_argument("--off-only", action="store_true")
    a = ap.parse_args()
    STEPS = a.steps
    arms = [("off (a)", False), ("off (b)", False)] if a.off_only else [("detached", False), ("attached", True)]
    print(f"episode logs of the attachments' rows: {'present' if HAS_ROWS else 'not in this build'}; {STEPS} steps per episode")
    single(4096, "cuda:0", arms)
    batched(a.E, a.NE, "cuda:0", arms)
