"""What the staged env-batched MPPI / covo-offline step (staged=True, covo_set_step_batched_staged) costs, by the method of
scripts/batched_modes.py: open loop on fixed states with changing keys, every arm replaying graphs, the arms of one comparison
alternating `--rounds` times in one process after warm-up, the host clock around `--steps` steps that end in a synchronise;
min / median / max of the per-step time.

  staged-vs-fused   MPPI and covo-offline under the gaussian disturbance (a configuration the fused launch takes): the staged batched
                    step against the fused one -- what switching it on costs where it is not needed
  staged-vs-loop    MPPI-periodic and MPPI with gamma_sigma = 0.2 (configurations the fused launch refuses): the staged batched step
                    against the loop over n_envs single controllers' C calls, the only other way to run them
  fused             the fused batched step alone, staged off (to compare one commit with another: run it on both)

  python scripts/batched_staged_cost.py [--arms staged-vs-fused staged-vs-loop fused] [--n-envs 32] [--N 4096]
Prints one JSON line per comparison.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARMS = ["staged-vs-fused", "staged-vs-loop", "fused"]
ap = argparse.ArgumentParser()
ap.add_argument("--arms", nargs="+", choices=ARMS, default=ARMS)
ap.add_argument("--n-envs", type=int, default=32)
ap.add_argument("--N", type=int, default=4096)
ap.add_argument("--lam", default="0.01")
ap.add_argument("--steps", type=int, default=200, help="steps per timed window")
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()

import torch  # noqa: E402

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.dynamics.dataclass import DeviceState  # noqa: E402

os.environ["COVO_GRAPH"] = "1"  # every arm replays graphs
DEV = "cuda:0"
E, N, lam = args.n_envs, args.N, args.lam
keys_seq = np.random.default_rng(1).integers(0, 2 ** 32, size=(args.steps, E, 2), dtype=np.uint32)
STAGED = hasattr(cm._lib, "COVO_HAS_BATCHED_STAGED")  # (the `fused` arm also runs on a commit without the switch)


def stat(x):
    return dict(min=round(min(x), 2), median=round(float(np.median(x)), 2), max=round(max(x), 2))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) / args.steps * 1e6


class Setup:
    """E domain-randomised instances a few steps into their episodes under `disturb`, and what builds controllers on them."""

    def __init__(self, mode, disturb):
        self.mode = mode
        self.env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type=disturb,
                                  disable_rollover_terminate=True, generate_noisy_state=True, device=DEV)
        self.params = [self.env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
        c0, _ = cm.envs.get_controller(self.env, mode, f"N{N}_H32_lam{lam}", device=DEV, compute_info=False)
        self.cp0 = c0.init_control_params
        b = self.batched(staged=False) if disturb == "gaussian" else self.batched(staged=True)
        self.ep = cm.envs.BatchedDeviceEpisode(self.env, [cr.PRNGKey(200 + e) for e in range(E)], self.params, (b.core.lib, b.core.h), DEV)
        self.tables = None
        if mode == "covo-offline":
            self.tables = b.reset(self.ep.states0, self.params, [cr.PRNGKey(300 + e) for e in range(E)])
        b.run_episode(self.ep, np.stack([np.asarray(cr.PRNGKey(400 + e)) for e in range(E)]), 5)  # off the reset point
        torch.cuda.synchronize()
        self.noisy = self.ep.noisy.clone()

    def batched(self, staged, gamma_sigma=0.0):
        cp0 = self.cp0
        kw = dict(discount=cp0.discount, gamma_mean=cp0.gamma_mean, a_mean_init=cp0.a_mean, device=DEV)
        if STAGED:
            kw["staged"] = staged
        if self.mode == "mppi":
            if gamma_sigma:
                kw["gamma_sigma"] = gamma_sigma
            return cm.controllers.BatchedMPPIController(self.env, E, N, 32, float(lam), sigmas=cp0.sample_sigma, **kw)
        return cm.controllers.BatchedCoVOController(self.env, E, N, 32, float(lam), sample_sigma=cp0.sample_sigma, mode="offline", **kw)

    def open_loop(self, staged, gamma_sigma=0.0):
        """-> a function that runs args.steps batched steps on the fixed states and synchronises"""
        b = self.batched(staged, gamma_sigma)
        if self.tables is not None:
            b.set_tables(*self.tables)
        b.set_instances(self.ep.states0, self.params)

        def run():
            for t in range(args.steps):
                b(self.noisy, keys_seq[t])
            torch.cuda.synchronize()
        return run

    def loop_of_singles(self, gamma_sigma=0.0):
        """-> the same work as E single controllers' C calls (core.step = covo_mpc_step) one after the other, as in batched_modes.py"""
        singles = []
        for e in range(E):
            c, _ = cm.envs.get_controller(self.env, self.mode, f"N{N}_H32_lam{lam}", device=DEV, compute_info=False)
            c.alias_outputs = True
            cp = c.init_control_params
            ds = DeviceState(packed=self.noisy[e].clone(), pos_traj=self.ep.pos_traj[e], vel_traj=self.ep.vel_traj[e], time=None)
            kw = dict(gamma_mean=cp.gamma_mean, sample_sigma=cp.sample_sigma, want_stats=False, derive_keys=True,
                      a_cov=cp.a_cov.clone(), rollout_deterministic=False, gamma_sigma=gamma_sigma)
            singles.append(dict(c=c, ds=ds, pc=c._params_c(self.params[e]), am=cp.a_mean.reshape(-1).clone(), kw=kw))

        def run():
            for t in range(args.steps):
                for e, s in enumerate(singles):
                    s["am"], cov = s["c"].core.step(cm._lib.MODE_MPPI, s["ds"], s["pc"], s["am"], keys_seq[t, e], **s["kw"])
                    if cov is not None:
                        s["kw"]["a_cov"] = cov
            torch.cuda.synchronize()
        return run


def compare(what, config, arms):
    """arms: {name: run}; all warmed up (eager call, capture, replays), then alternating args.rounds times"""
    for run in arms.values():
        run()
    times = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, run in arms.items():
            times[name].append(timed(run))
    out = dict(what=what, config=config, n_envs=E, N=N, steps=args.steps, rounds=args.rounds,
               **{f"{name}_us": stat(t) for name, t in times.items()})
    names = list(arms)
    if len(names) == 2:
        a, b = times[names[0]], times[names[1]]
        out[f"{names[0]}_over_{names[1]}_median"] = round(float(np.median(a)) / float(np.median(b)), 3)
        out[f"{names[0]}_max_below_{names[1]}_min"] = bool(max(a) < min(b))
    print(json.dumps(out), flush=True)


if "fused" in args.arms:
    for mode in ("mppi", "covo-offline"):
        compare("fused", f"{mode} gaussian, staged off", dict(fused=Setup(mode, "gaussian").open_loop(False)))
if "staged-vs-fused" in args.arms:
    for mode in ("mppi", "covo-offline"):
        s = Setup(mode, "gaussian")
        compare("staged-vs-fused", f"{mode} gaussian", dict(staged=s.open_loop(True), fused=s.open_loop(False)))
if "staged-vs-loop" in args.arms:
    s = Setup("mppi", "periodic")
    compare("staged-vs-loop", "mppi periodic", dict(staged=s.open_loop(True), loop=s.loop_of_singles()))
    s = Setup("mppi", "gaussian")
    compare("staged-vs-loop", "mppi gaussian gamma_sigma=0.2", dict(staged=s.open_loop(True, 0.2), loop=s.loop_of_singles(0.2)))
