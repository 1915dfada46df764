"""Time the env-batched control step per controller (mppi | covo-offline | covo-online) for n_envs domain-randomised instances.

  open loop    one batched step (graph replay) on fixed states, keys changing, against the same work done by n_envs
               single-instance controllers stepped one after the other in the same process (each on its one-launch fused path,
               graph replay) -- the two alternate `--rounds` times after warm-up; min / median / max of the per-step time
  closed loop  covo_run_episode_batched(_mode): control step + env step on the device, one host sync per segment -> env-steps/s

  python scripts/batched_modes.py --mode mppi --n-envs 32 --N 1024
Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["mppi", "covo-offline", "covo-online"], default="mppi")
ap.add_argument("--n-envs", type=int, default=32)
ap.add_argument("--N", type=int, default=4096)
ap.add_argument("--lam", default="0.01")
ap.add_argument("--steps", type=int, default=200, help="steps per timed window")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--no-loop", action="store_true", help="skip the per-instance baseline")
ap.add_argument("--episode-steps", type=int, default=300)
ap.add_argument("--diag", action="store_true", help="the batched controllers also form the per-step sampling diagnostics (compute_diag)")
args = ap.parse_args()

import torch  # noqa: E402

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402

os.environ["COVO_GRAPH"] = "1"  # both sides replay graphs
DEV = "cuda:0"
E, N, lam = args.n_envs, args.N, args.lam
env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                     disable_rollover_terminate=True, generate_noisy_state=True, device=DEV)
params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
reset_keys = [cr.PRNGKey(200 + e) for e in range(E)]
c0, _ = cm.envs.get_controller(env, args.mode, f"N{N}_H32_lam{lam}", device=DEV, compute_info=False)
cp0 = c0.init_control_params


def make_batched():
    kw = dict(discount=cp0.discount, gamma_mean=cp0.gamma_mean, a_mean_init=cp0.a_mean, device=DEV, compute_diag=args.diag)
    if args.mode == "mppi":
        return cm.controllers.BatchedMPPIController(env, E, N, 32, float(lam), sigmas=cp0.sample_sigma, **kw)
    return cm.controllers.BatchedCoVOController(env, E, N, 32, float(lam), sample_sigma=cp0.sample_sigma,
                                                mode="offline" if args.mode == "covo-offline" else "online", **kw)


b = make_batched()
ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
table_keys = [cr.PRNGKey(300 + e) for e in range(E)]
if args.mode == "covo-offline":
    b.reset(ep.states0, params, table_keys)
rngs = np.stack([np.asarray(cr.PRNGKey(400 + e)) for e in range(E)])
rngs = b.run_episode(ep, rngs, 5)  # off the reset point
torch.cuda.synchronize()
noisy = ep.noisy.clone()
states = [None] * E
keys_seq = np.random.default_rng(1).integers(0, 2 ** 32, size=(args.steps, E, 2), dtype=np.uint32)

# ---- open loop
bo = make_batched()
if args.mode == "covo-offline":
    bo.set_tables(b.a_cov_offline, b.a_chol_offline)
bo.set_instances(ep.states0, params)


def run_batched():
    for t in range(args.steps):
        bo(noisy, keys_seq[t])
    torch.cuda.synchronize()


singles = []
if not args.no_loop and args.mode != "covo-online":
    from covo_mpc_amd.dynamics.dataclass import DeviceState
    for e in range(E):
        c, _ = cm.envs.get_controller(env, args.mode, f"N{N}_H32_lam{lam}", device=DEV, compute_info=False)
        c.alias_outputs = True
        cp = c.init_control_params
        if args.mode == "covo-offline":
            cp = cp.replace(a_cov_offline=b.a_cov_offline[e], a_chol_offline=b.a_chol_offline[e])
        ds = DeviceState(packed=noisy[e].clone(), pos_traj=ep.pos_traj[e], vel_traj=ep.vel_traj[e], time=None)
        # the controller's C call alone (core.step = covo_mpc_step), without the Python wrapper's bookkeeping: the baseline is the
        # launches, not the host code around them
        kw = dict(gamma_mean=cp.gamma_mean, sample_sigma=cp.sample_sigma, want_stats=False, derive_keys=True)
        if args.mode == "mppi":
            kw.update(a_cov=cp.a_cov.clone(), rollout_deterministic=False, gamma_sigma=0.0)
            mode = cm._lib.MODE_MPPI
        else:
            kw.update(L_table=cp.a_chol_offline)
            mode = cm._lib.MODE_COVO_OFFLINE
        singles.append(dict(c=c, mode=mode, ds=ds, pc=c._params_c(params[e]), am=cp.a_mean.reshape(-1).clone(), kw=kw))


def run_loop():
    for t in range(args.steps):
        for e, s in enumerate(singles):
            s["am"], cov = s["c"].core.step(s["mode"], s["ds"], s["pc"], s["am"], keys_seq[t, e], **s["kw"])
            if cov is not None:
                s["kw"]["a_cov"] = cov
    torch.cuda.synchronize()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) / args.steps * 1e6


run_batched()
if singles:
    run_loop()
tb, tl = [], []
for _ in range(args.rounds):
    tb.append(timed(run_batched))
    if singles:
        tl.append(timed(run_loop))
stat = lambda x: dict(min=round(min(x), 2), median=round(float(np.median(x)), 2), max=round(max(x), 2))
out = dict(what="open_loop", mode=args.mode, n_envs=E, N=N, steps=args.steps, rounds=args.rounds, batched_step_us=stat(tb),
           batched_us_per_env_step=round(float(np.median(tb)) / E, 3))
if tl:
    out["loop_of_singles_us"] = stat(tl)
    out["speedup_median"] = round(float(np.median(tl)) / float(np.median(tb)), 2)
    out["faster_beyond_spreads"] = bool(min(tl) - max(tb) > 0 and (np.median(tl) - np.median(tb)) > (max(tl) - min(tl)) + (max(tb) - min(tb)))
print(json.dumps(out))

# ---- closed loop
rates = []
for _ in range(3):
    ep2 = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b.run_episode(ep2, rngs, args.episode_steps)
    ep2.read_log()
    dt = time.perf_counter() - t0
    rates.append(E * args.episode_steps / dt)
print(json.dumps(dict(what="closed_loop", mode=args.mode, n_envs=E, N=N, episode_steps=args.episode_steps,
                      env_steps_per_s=stat(rates), us_per_batched_step=round(1e6 * E / float(np.median(rates)), 2))))
