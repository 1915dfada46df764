"""What Riccati feedback costs on top of the Riccati refinement: microseconds per control step with riccati=True against riccati=True,
riccati_feedback=True on the same build, by scripts/riccati_cost.py's protocol (five alternating windows of 200 steps after warm-up in
one process, min / median / max) and at its shapes -- covo-online at N = 4 096 and 65 536, the env-batched covo-online step at
32 x 4 096 -- and the generator's launch alone: covo_feedback_rollout at the ladder's 16 step sizes next to an empty pass over the same
Python call path (host time: its kernel time is what `rocprofv3 --kernel-trace --stats -- python scripts/feedback_cost.py --alone`
reports for feedback_rollout_kernel).
    python scripts/feedback_cost.py [--N 4096 65536] [--E 32 --NE 4096] [--controller covo-online] [--alone]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.dynamics.dataclass import as_device_state  # noqa: E402
from riccati_cost import report  # noqa: E402

ARMS = (("riccati", False), ("feedback", True))
WHAT = "feedback"


def single(name, N, dev):
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=dev)
    steps = {}
    for arm, feedback in ARMS:
        c, cp = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=dev, compute_info=False, riccati=True,
                                       riccati_feedback=feedback)
        c.alias_outputs = True
        params = env.default_params
        obs, info, state = env.reset(cr.PRNGKey(1), params)
        st = dict(cp=c.init_control_params)
        if name == "covo-offline":
            st["cp"] = c.reset(state, params, st["cp"], cr.PRNGKey(2))

        def step(c=c, st=st, obs=obs, state=state, params=params, info=info):
            _, st["cp"], _ = c(obs, state, params, np.array([3, 4], dtype=np.uint32), st["cp"], info)
        steps[arm] = step
    report(f"{name} N={N}", steps, what=WHAT)
    return c, params, info


def batched(E, N, dev):
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=dev)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=dev, compute_info=False)
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    steps = {}
    for arm, feedback in ARMS:
        b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=dev, riccati=True,
                                                 riccati_feedback=feedback)
        b.set_instances([s[2] for s in states], params)
        noisy = [s[1]["noisy_state"] for s in states]
        b(noisy, keys)
        steps[arm] = lambda b=b: b(None, keys)
    report(f"batched covo-online E={E} N={N}", steps, what=WHAT)


def generator_alone(c, params, info, dev):
    """the generator's launch at the controller's own state and mean, under the gains of one stand-alone sweep there"""
    core = c.core
    ds = as_device_state(info["noisy_state"], dev)
    pc = c._params_c(params)
    a = c.init_control_params.a_mean.reshape(1, -1).contiguous()
    sw = core.riccati(ds, pc, a)
    torch.cuda.synchronize()
    report("stand-alone generator, 16 step sizes", {"sweep": lambda: core.riccati(ds, pc, a),
                                                    "generator": lambda: core.feedback_rollout(ds, pc, a, sw["K"], sw["kff"], sw["x"])},
           what="launches")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--E", type=int, default=32)
    ap.add_argument("--NE", type=int, default=4096)
    ap.add_argument("--controller", default="covo-online")
    ap.add_argument("--alone", action="store_true", help="only the stand-alone generator calls (for a kernel trace)")
    a = ap.parse_args()
    if a.alone:
        env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                             generate_noisy_state=True, device="cuda:0")
        c, _ = cm.envs.get_controller(env, a.controller, "N4096_H32_lam0.01", device="cuda:0", compute_info=False)
        params = env.default_params
        _, info, _ = env.reset(cr.PRNGKey(1), params)
        generator_alone(c, params, info, "cuda:0")
        sys.exit(0)
    for N in a.N:
        c, params, info = single(a.controller, N, "cuda:0")
    batched(a.E, a.NE, "cuda:0")
    generator_alone(c, params, info, "cuda:0")
