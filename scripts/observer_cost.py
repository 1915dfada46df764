"""What the force observer costs (csrc/force_observer.hip), on one build and in one process; the measuring loops are
scripts/estimator_cost.py's.
  the launch alone   covo_observe_force for 1 and for 32 instances next to covo_estimate, the 13-state filter whose products run on the
                     vector unit (the comparison DESIGN.md 4.33 left open): five alternating windows of 2 000 back-to-back launches
                     between device events (min / median / max of the windows), and one launch synchronised on its own by the host
                     clock (median of 200: launch, run and synchronisation)
  per step in an episode   run_episode with the observer attached against not attached: single covo-online at N = 4 096 and the
                     env-batched covo-online step at 32 x 4 096; five alternating segments of 100 steps, host clock around the
                     segment and its synchronisation
    python scripts/observer_cost.py [--N 4096] [--E 32 --NE 4096] [--no-episodes]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from estimator_cost import DEV, alone, episodes, event_windows  # noqa: E402


def launches(E):
    """{name: a callable that enqueues one launch for E instances}.  Both filters are timed on their update path: a launch leaves
    t_prev = the row's time word, so the next one on the same row would re-initialise; each call therefore first copies t_prev =
    time - 1 back into the filter's meta words, and that small copy is timed on its own as `meta copy` -- subtract it.  The observer
    overwrites the row's kinematic floats with its estimate: the next launch measures that estimate, still an update."""
    import torch
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.dynamics.dataclass import EnvParams3D
    core = SamplingCore(64, 32, 0.01, 1.0, device=DEV, use_graph=False, compute_info=False)
    f32, f64 = dict(dtype=torch.float32, device=DEV), dict(dtype=torch.float64, device=DEV)
    pc = EnvParams3D().to_c()

    def fresh_rows():
        rows = torch.zeros((E, 32), **f32)
        rows[:, 9] = 1.0
        rows[:, 25:26] = torch.tensor([7], dtype=torch.int32, device=DEV).view(torch.float32)
        return rows
    u = torch.zeros((E, 4), **f32)
    obs = (0.0125, 0.025, 0.001, 0.025)
    # the state estimator
    rows_e, side_e = fresh_rows(), torch.zeros((E, 8), **f32)
    xhat, Pe, meta_e = torch.zeros((E, 16), **f64), torch.zeros((E, 13, 13), **f64), torch.zeros((E, 2), dtype=torch.int32, device=DEV)
    kw_e = dict(rows=side_e, obs_std=obs, proc_std=(0.0, -1.0, 0.0, 0.0), force_std=0.05)
    core.estimate(rows_e, u, pc, xhat, Pe, meta_e, reset=True, **kw_e)
    # the force observer
    rows_o, side_o = fresh_rows(), torch.zeros((E, 8), **f32)
    xi, Po, meta_o = torch.zeros((E, 16), **f64), torch.zeros((E, 16, 16), **f64), torch.zeros((E, 2), dtype=torch.int32, device=DEV)
    kw_o = dict(rows=side_o, obs_std=obs, force_walk_std=0.05, force_init_std=0.2 / 3 ** 0.5)
    core.observe_force(rows_o, u, pc, xi, Po, meta_o, reset=True, **kw_o)
    due = meta_e.clone()
    due[:, 1] = 6  # (the row's time word is 7: every launch behind this copy is an update)
    scratch = torch.zeros_like(due)

    def put_back():
        scratch.copy_(due, non_blocking=True)

    def estimate():
        meta_e.copy_(due, non_blocking=True)
        core.estimate(rows_e, u, pc, xhat, Pe, meta_e, **kw_e)

    def observe():
        meta_o.copy_(due, non_blocking=True)
        core.observe_force(rows_o, u, pc, xi, Po, meta_o, **kw_o)
    estimate()
    observe()
    torch.cuda.synchronize()
    assert int(side_e[0, 0:1].view(torch.int32)[0]) == 0 and int(side_o[0, 0:1].view(torch.int32)[0]) == 0, "the timed launches must be updates"
    return core, {"meta copy": put_back, "estimate": estimate, "observe": observe}


def report_launches(E):
    core, calls = launches(E)
    for k, v in event_windows(calls).items():
        print(f"{E:3d} instances  back-to-back  {k:10s}: min {min(v):7.2f}  median {np.median(v):7.2f}  max {max(v):7.2f} us per call", flush=True)
    for k, v in alone(calls).items():
        print(f"{E:3d} instances  synchronised  {k:10s}: median {np.median(v):7.2f}  min {min(v):7.2f} us", flush=True)
    core.close()


def single(N):
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    params = env.default_params
    arms = {}
    for arm in ("plain", "attached"):
        c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
        c.alias_outputs = True
        if arm == "attached":
            cm.controllers.ForceObserver(env).attach(c)
        st = dict(rng=cr.PRNGKey(3))

        def prep(c=c):
            ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (c.core.lib, c.core.h), DEV)
            return ep, c.reset(ep.state0, params, c.init_control_params, cr.PRNGKey(42))

        def go(ctx, n, c=c, st=st):
            c.run_episode(ctx[0], params, ctx[1], st["rng"], n)
        arms[arm] = (prep, go)
    episodes(f"covo-online N={N}", arms)


def batched(E, N):
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=DEV)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    keys = [cr.PRNGKey(200 + e) for e in range(E)]
    rngs = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    arms = {}
    for arm in ("plain", "attached"):
        b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=DEV)
        if arm == "attached":
            cm.controllers.ForceObserver(env, n_inst=E).attach(b)

        def prep(b=b):
            ep = cm.envs.BatchedDeviceEpisode(env, keys, params, (b.core.lib, b.core.h), DEV)
            b.reset(None, None, None)
            return ep

        def go(ep, n, b=b):
            b.run_episode(ep, rngs.copy(), n)
        arms[arm] = (prep, go)
    episodes(f"batched covo-online E={E} N={N}", arms)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    ap.add_argument("--no-episodes", action="store_true")
    a = ap.parse_args()
    for E in (1, a.E):
        report_launches(E)
    if not a.no_episodes:
        single(a.N)
        batched(a.E, a.NE)
