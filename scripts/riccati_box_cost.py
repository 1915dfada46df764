"""What the Riccati box costs: microseconds per control step with riccati_box off and on -- both arms with riccati=True, on the same
commit, five alternating windows of 200 steps after warm-up in one process, min / median / max -- covo-online at N = 4 096 and at
the headline N = 65 536, the env-batched covo-online step at 32 x 4 096, the iLQR controller at k = 1 / 2 / 4 iterations, and the
sweep's launches alone (covo_riccati next to covo_riccati_box, batch 1 and 32).  Every line of an "on" arm also says how many
coordinates the last sweep clamped: a stage whose unconstrained step is feasible costs one wave-uniform test, a stage that leaves the
box the pattern search and a second factorisation.
    python scripts/riccati_box_cost.py [--N 4096 65536] [--E 32 --NE 4096] [--iters 1 2 4]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.dynamics.dataclass import as_device_state  # noqa: E402
from riccati_cost import report  # noqa: E402

ARMS = (("off", False), ("on", True))
KEY = np.array([3, 4], dtype=np.uint32)


def clamped(masks):
    m = masks.reshape(-1, 1).cpu().numpy()
    return int(((m >> np.arange(8)) & 1).sum())


def quad(dev, **kw):
    return cm.envs.Quad3D(**{**dict(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian",
                                    disable_rollover_terminate=True, generate_noisy_state=True, device=dev), **kw})


def single(name, spec, dev, what, **kw):
    env = quad(dev)
    steps, cores = {}, {}
    for arm, box in ARMS:
        c, cp = cm.envs.get_controller(env, name, spec, device=dev, compute_info=False, riccati_box=box, **kw)
        c.alias_outputs = True
        params = env.default_params
        obs, info, state = env.reset(cr.PRNGKey(1), params)
        st = dict(cp=c.init_control_params)

        def step(c=c, st=st, obs=obs, state=state, params=params, info=info):
            _, st["cp"], _ = c(obs, state, params, KEY, st["cp"], info)
        steps[arm], cores[arm] = step, c.core
    report(what, steps, what="riccati_box")
    print(f"{what:38s} clamped coordinates of the last sweep: {clamped(cores['on'].riccati_box_masks)}", flush=True)
    return c, params, info


def batched(E, N, dev):
    env = quad(dev, task="tracking", obs_type="quad_params", enable_randomizer=True)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    steps, ctl = {}, {}
    for arm, box in ARMS:
        b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=dev, riccati=True, riccati_box=box)
        b.set_instances([s[2] for s in states], params)
        b([s[1]["noisy_state"] for s in states], keys)
        steps[arm], ctl[arm] = (lambda b=b: b(None, keys)), b
    what = f"batched covo-online E={E} N={N}"
    report(what, steps, what="riccati_box")
    print(f"{what:38s} clamped coordinates of the last sweeps: {clamped(ctl['on'].riccati_box)}", flush=True)


def sweep_alone(c, params, info, dev, batches=(1, 32)):
    """the stand-alone launches at the controller's own state and its initial (hover) mean"""
    core = c.core
    ds = as_device_state(info["noisy_state"], dev)
    pc = c._params_c(params)
    for n in batches:
        a = c.init_control_params.a_mean.reshape(1, -1).repeat(n, 1).contiguous()
        report(f"stand-alone, batch {n}", {"riccati": lambda a=a: core.riccati(ds, pc, a),
                                           "riccati_box": lambda a=a: core.riccati(ds, pc, a, box=True)}, what="launches")
        print(f"{'stand-alone, batch %d' % n:38s} clamped coordinates: {clamped(core.riccati(ds, pc, a, box=True)['box'])}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    ap.add_argument("--iters", type=int, nargs="+", default=[1, 2, 4])
    a = ap.parse_args()
    for N in a.N:
        c, params, info = single("covo-online", f"N{N}_H32_lam0.01", "cuda:0", f"covo-online N={N}", riccati=True)
    batched(a.E, a.NE, "cuda:0")
    for k in a.iters:
        single("ilqr", "N64_H32_lam0.01", "cuda:0", f"ilqr k={k}", iters=k)
    sweep_alone(c, params, info, "cuda:0")
