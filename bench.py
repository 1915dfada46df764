#!/usr/bin/env python
"""bench.py -- MPC control-steps/s of the MI355X-native sampling-MPC inner loop.

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

`--gpus N` without a torchrun environment launches its own N ranks: the parent, before any GPU call, starts
`python -m torch.distributed.run --nproc-per-node N bench.py ...` as a CHILD process, relays its output (rank 0's JSON
line) and exits with its code.

A "step" is one controller __call__ (quadjax/controllers/covo.py:187-283), teacher-forced on the inputs of ONE closed-loop
episode of the SAME controller ("averaged over a 300-step tracking_zigzag episode",
quadjax/envs/quadrotor.py:506-579): an untimed recording pass runs the controller in closed loop (Python env on the
host) and keeps, per step, the noisy state, the control_params.a_mean that went in and the controller key; the timed
steps replay those inputs (resident in HBM) at indices spread evenly over all 300 steps, so K timed steps cover the
whole episode and every one of them runs exactly the launches (the Sigma chain's data-dependent iteration counts
included) that step of the closed loop ran.  Workload (BASELINE.json north_star / configs[3]):
covo-online, tracking_zigzag, N = 65536 samples x H = 32, lambda = 0.01, sigma = 0.5; with G > 1 ranks
the sample axis is sharded (N/G per GPU, "strong" scaling: total work fixed) and ONE exchange of the
516-float rank records (online-softmax partial + position sums) crosses xGMI per step (RCCL all-gather; COVO_EXCHANGE=peer:
direct peer writes, csrc/exchange.hip).

A plain run sets up (recording pass), warms up, times the K steps, writes the last timed step's outputs under
`--dump-outputs DIR` and prints the headline line (`value`, `ms_per_step`, ...).  Everything else below is measured only with
`--full`: rank 0's line then also holds `roofline` (the fused rollout kernel in the variant the timed step runs -- it also
leaves the softmax records --, HBM bound, 516 B/sample algorithmic, mean launch duration measured live with events on
the launch stream; `traffic` / `counters` from the committed PMC passes of this command, dropped when the kernel
sources changed since), `roofline_gemm` (the noise GEMM against the fp32 MFMA peak: as a launch of its own, and what it adds to the
Sigma chain streamed inside its finalize launch, which is how the timed steps run it), `value_with_pos_info` (the same
steps with covo.py:281's pos_mean / pos_std computed) and, at N=1, `cpu_baseline` (the plain-C oracle port of the same
step on the host cores).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_F32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: dense fp32 matrix peak (v_mfma_f32_32x32x2_f32: 256 flop/clk/CU)
ROLLOUT_BYTES_PER_SAMPLE = 516  # 32 x 16 B action read + 4 B cost write
GEMM_FLOP_PER_SAMPLE_DENSE = 2 * 128 * 128  # dense-equivalent 2 n^2
GEMM_FLOP_PER_SAMPLE_ISSUED = 20480         # lower-triangular k-skip in 32-wide groups: (1 + 2 + 3 + 4)/16 of the dense MFMAs
DUMP_LIMIT_BYTES = 64 << 20                 # --dump-outputs: all files together


def dump_outputs(dirname, arrays):
    """--dump-outputs: the arrays the last timed step handed its caller, one DIR/<name>.npy each, float64 where the output is
    float64 and float32 otherwise.  An array above its share of DUMP_LIMIT_BYTES is cut to a fixed sample (seed 0) of its
    flattened elements, so two runs with the same arguments write the same elements."""
    import torch
    os.makedirs(dirname, exist_ok=True)
    share = DUMP_LIMIT_BYTES // max(len(arrays), 1)
    for name, t in arrays.items():
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, name + ".npy"), a)


def record_episode(env, controller, params, T, with_counts):
    """The recording pass (untimed): one closed-loop episode of `controller` itself -- quadjax's eval_env loop
    (quadrotor.py:506-579: rng -> rng_act, rng_step; controller; env.step) with the Python env on the host, seeds as in
    closed_loop()'s host leg.  Per step it keeps what the controller __call__ was given: the noisy state (packed + host
    object), control_params.a_mean and rng_act; for covo-online also the Sigma chain's (squarings, Newton-Schulz iterations).
    -> dict(packed [T,32], states [T], a_means [T,128] device tensor, keys [T], counts [T,2] or None, s_reset, cp_reset)"""
    import torch
    from covo_mpc_amd import random as cr
    obs, info, state = env.reset(cr.PRNGKey(21), params)
    s_reset = state
    cp = cp_reset = controller.reset(state, params, controller.init_control_params, cr.PRNGKey(22))
    key = cr.PRNGKey(23)
    packed, states, a_means, keys, counts, errs = [], [], [], [], [], []
    alias = controller.alias_outputs
    controller.alias_outputs = False  # the recorded means must not alias the controller's buffer
    for _ in range(T):
        key, k_act, k_step = cr.split(key, 3)
        packed.append(info["noisy_state"].pack())
        states.append(info["noisy_state"])
        a_means.append(cp.a_mean.reshape(-1).clone())
        keys.append(k_act)
        u, cp, _ = controller(obs, state, params, k_act, cp, info)
        if with_counts:
            counts.append(sigma_chain_counts(controller.core))
        obs, state, reward, done, info = env.step(k_step, state, u.cpu().numpy(), params)
        errs.append(info["err_pos"])
    controller.alias_outputs = alias
    return {"packed": np.stack(packed), "states": states, "a_means": torch.stack(a_means), "keys": keys,
            "counts": np.asarray(counts) if with_counts else None, "s_reset": s_reset, "cp_reset": cp_reset,
            "err_pos_mean_m": float(np.mean(errs))}


def make_states(env, params, n_states, seed):
    """Noisy states of a PID-tracked tracking_zigzag episode (rounds 1-4's teacher-forced inputs).  NOT used by the bench any more
    (its timed steps replay the controller's own closed-loop episode, record_episode); scripts/ still draw their states from it."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    obs, info, state = env.reset(cr.PRNGKey(seed), params)
    pid = cm.controllers.PIDController(env, cm.controllers.PIDParams(Kp=10.0, Kd=5.0, Ki=0.0, Kp_att=10.0))
    cp, key = pid.init_control_params, cr.PRNGKey(seed + 1)
    packed, states = [], []
    for _ in range(n_states):
        packed.append(info["noisy_state"].pack())
        states.append(info["noisy_state"])
        a, cp, _ = pid(obs, state, params, key, cp)
        key, k = cr.split(key)
        obs, state, reward, done, info = env.step_env(k, state, a, params)
    return state, np.stack(packed), states


def spread_indices(K, T):
    """K indices spread evenly over [0, T): the centres of K equal strata (K <= T), or the episode repeated (K > T)."""
    if K <= T:
        return [min(T - 1, (2 * i + 1) * T // (2 * K)) for i in range(K)]
    return [i % T for i in range(K)]


def cpu_baseline(states, params, N, H, lam, budget_s=15.0):
    """The oracle's C port of the WHOLE covo-online step on this box's host cores: hyper-dual Hessian (fp64, OpenMP
    over the 8 256 action pairs) -> LAPACK eigh/cholesky for Sigma -> noise GEMM -> rollout -> softmax update (fp32,
    OpenMP over samples).  epsilon is drawn once outside the loop (the reference's threefry draw is not ported)."""
    from oracle import c_oracle as CO
    from oracle import ref_np as R
    cores = int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count() or 1)  # a thread count the caller set is kept
    os.environ["OMP_NUM_THREADS"] = str(cores)
    ns = states[40]
    so = R.State(pos=ns.pos, vel=ns.vel, quat=ns.quat, omega=ns.omega, f_disturb=ns.f_disturb, pos_tar=ns.pos_tar,
                 vel_tar=ns.vel_tar, acc_tar=ns.acc_tar, time=ns.time, pos_traj=ns.pos_traj, vel_traj=ns.vel_traj,
                 acc_traj=ns.acc_traj).astype(np.float32)
    so64 = so.astype(np.float64)
    p = R.Params()
    rng = np.random.default_rng(0)
    eps = rng.standard_normal((N, H * 4), dtype=np.float32)
    a_mean = R.hover_action(p, H, np.float32)
    n_done, t_h, t0 = 0, 0.0, time.perf_counter()
    while True:
        th = time.perf_counter()
        Rm = CO.hessian(so64, p.fp32(), R.shift_mean(a_mean.astype(np.float64)).reshape(-1), H)  # covo.py:134-185
        t_h += time.perf_counter() - th
        Sigma = R.optimize_sigma(Rm, 0.5, H, 4)                      # covo.py:116-132 (LAPACK)
        L = np.linalg.cholesky(Sigma).astype(np.float32)             # covo.py:216
        a_mean, cost, _ = CO.sampling_step(so, p, L, R.shift_mean(a_mean), eps, lam)  # covo.py:201-278
        n_done += 1
        el = time.perf_counter() - t0
        if el > budget_s or n_done >= 200:
            break
    return {"value": n_done / el, "unit": "control-steps/s", "cores": cores, "kind": "port",
            "sample": f"{n_done} full-size covo-online control steps (N={N}, H={H}) of the C oracle port: fp64 hyper-dual "
                      f"Hessian ({1e3 * t_h / n_done:.1f} ms/step) + fp64 LAPACK eigh/cholesky + fp32 noise GEMM, rollout and "
                      f"softmax update, OpenMP on {cores} host threads; {el:.1f} s of CPU work"}


def sigma_chain_counts(core):
    """(squarings, Newton-Schulz iterations) of the Sigma chain of the LAST covo-online step (scalar slots of its workspace;
    synchronises).  The length of a step's chain is data dependent: these are what make two values comparable.  `squarings` =
    the filter iterate lambda_min was taken from (SC_KWIN: the first one whose Ritz pair passes its residual test); the chain
    itself runs up to two squarings further while that iterate is being evaluated."""
    import torch
    from covo_mpc_amd import _lib
    out = torch.zeros(24, dtype=torch.float64).pin_memory()
    _lib.check(core.lib.covo_debug_sigma_workspace(core.h, _lib.ptr(out), 11 * 128 * 128, 24, core.stream()), "sigma workspace")
    torch.cuda.synchronize()
    o = out.numpy()
    return float(o[7]), float(o[6])  # SC_KWIN, SC_ITERS (csrc/sigma_ns.hip)


def closed_loop(env, controller, params, T, rec=None):
    """the same controller in CLOSED loop for one episode (env step included): with the env step as a
    device kernel and the whole episode enqueued by one C call (covo_run_episode: one host sync per episode) and with the Python env on the host (one sync and
    one 128-B upload per step) -- reported next to the teacher-forced `value`, never in place of it."""
    import torch
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    core = controller.core
    res = {"unit": "control-steps/s", "steps": int(T)}
    # --- warm-up (first-use module loads of the env kernel and of torch's gather kernels), untimed
    ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(20), params, (core.lib, core.h), core.device)
    cp = controller.reset(ep.state0, params, controller.init_control_params, cr.PRNGKey(22))
    cp, _ = controller.run_episode(ep, params, cp, cr.PRNGKey(19), 5)
    # --- device env
    ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(21), params, (core.lib, core.h), core.device)
    cp = controller.reset(ep.state0, params, controller.init_control_params, cr.PRNGKey(22))
    key = cr.PRNGKey(23)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cp, key = controller.run_episode(ep, params, cp, key, T)  # ONE C call enqueues T x {control step, env step}
    log = ep.read_log()                                        # the one host sync of the episode
    res["device_env"] = T / (time.perf_counter() - t0)
    res["device_env_err_pos_mean_m"] = float(log[:, 1].mean())
    # --- host env
    obs, info, state = env.reset(cr.PRNGKey(21), params)
    cp = controller.reset(state, params, controller.init_control_params, cr.PRNGKey(22))
    key = cr.PRNGKey(23)
    errs = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(T):
        key, k_act, k_step = cr.split(key, 3)
        u, cp, _ = controller(obs, state, params, k_act, cp, info)
        obs, state, reward, done, info = env.step(k_step, state, u.cpu().numpy(), params)
        errs.append(info["err_pos"])
    torch.cuda.synchronize()
    res["host_env"] = T / (time.perf_counter() - t0)
    res["host_env_err_pos_mean_m"] = float(np.mean(errs))
    if rec is not None and rec["counts"] is not None:
        # the Sigma chain's data-dependent iteration counts over the recorded closed-loop episode (same seeds as the host leg)
        res["sigma_chain_mean_squarings"] = float(rec["counts"][:, 0].mean())
        res["sigma_chain_mean_newton_schulz_iterations"] = float(rec["counts"][:, 1].mean())
    return res


PMC_SUMMARY = os.path.join("profiles", "r06_bench_pmc_summary.json")
# every file the rollout kernel and the noise GEMM are built from: the hash that decides whether committed PMC counters still
# describe the kernels of this tree (scripts/pmc_summary.py imports this list)
KERNEL_SRCS = ["covo_mpc_amd/csrc/" + f for f in (
    "rollout_pipe.hpp", "rollout_common.hpp", "rollout_launch.hpp", "rollout.hip", "rollout_var_r0.hip", "rollout_var_r1.hip",
    "quad_model.hpp", "disturb_model.hpp", "covo_common.hpp", "wave_reduce.hpp", "noise_gemm.hip", "noise_gemm_body.hpp",
    "softmax_merge.hpp", "eps_tiles.hpp", "rng_device.hpp", "Makefile")]


def rollout_sweep(kstate, pc, lam, device, sizes=(65536, 131072, 262144, 1048576), reps=100):
    """SURVEY.md 7 ("configs 2-4 must be reported honestly with a size sweep showing the asymptote"): the judged rollout kernel
    stand-alone (rollout_pipe3_kernel<..., REC = false>: covo_rollout_cost) at growing sample counts on the timed mid-episode
    state -- 3 x `reps` back-to-back launches issued from C between HIP events on the launch stream (covo_debug_time_rollout),
    actions = clip(mean + 0.5 eps) drawn on the device.  516 B per sample / launch duration against 8 TB/s."""
    import torch
    from covo_mpc_amd.controllers._core import SamplingCore
    out = []
    for n in sizes:
        core = None
        try:
            core = SamplingCore(n, 32, lam, 1.0, device=device, compute_info=False, trust_clipped=True, use_graph=False)
            am = torch.tensor([-0.3378, 0.0, 0.0, 0.0], device=device).repeat(32)
            L = (0.5 * torch.eye(128, device=device)).contiguous()
            core.noise_gemm_philox(L, am, (1, 2))
            torch.cuda.synchronize()
            us, us_min = core.time_rollout(kstate, pc, reps=reps, with_records=False)
            ach = n * ROLLOUT_BYTES_PER_SAMPLE / (us * 1e-6) / 1e9
            out.append({"N": int(n), "launch_us": us, "launch_us_min": us_min, "achieved": ach, "frac": ach / HBM_PEAK_GBS,
                        "frac_fastest_batch": n * ROLLOUT_BYTES_PER_SAMPLE / (us_min * 1e-6) / 1e9 / HBM_PEAK_GBS})
        except Exception as e:  # noqa: BLE001
            out.append({"N": int(n), "error": str(e)})
        finally:
            if core is not None:
                core.close()
                del core
            torch.cuda.empty_cache()
    return out


def kernel_src_sha():
    import hashlib
    h = hashlib.sha256()
    for f in KERNEL_SRCS:
        with open(os.path.join(ROOT, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def pmc_counters(args, n_local):
    """PMC-derived numbers per launch.  Counters cannot be read inside this process; they come from the separate
    `rocprofv3 --pmc` passes over THIS command that scripts/profile_bench.sh committed (profiles/, with the commit and the
    hash of the kernel sources they were taken at).  Attached only when the run is that command's workload (default
    controller, N_local = 65 536, no --info) AND the kernel sources are unchanged since -- otherwise null (stale counters
    would describe another kernel).  -> (summary dict or None, provenance or None)."""
    if args.controller != "covo-online" or args.info or n_local != 65536:
        return None, None
    try:
        with open(os.path.join(ROOT, PMC_SUMMARY)) as f:
            d = json.load(f)
        src = {"kind": "committed_profile", "file": PMC_SUMMARY, "command": d.get("command"), "commit": d.get("commit"),
               "kernel_src_sha": d.get("kernel_src_sha")}
        if d.get("kernel_src_sha") != kernel_src_sha():
            src["stale"] = "kernel sources changed since the profile was taken: counters dropped"
            return None, src
        return d, src
    except Exception:
        return None, None


def bench_envs(args, world, rank, device, backend):
    """--config envs = BASELINE.json configs[4]: covo-online on the lissajous `tracking` task with domain randomisation
    (quadjax/envs/quadrotor.py:132-171), E env instances x N = 4096 samples per GPU in ONE batched graph (covo_mpc_step_batched),
    the 256 instances of the config env-sharded 32 per rank over 8 GPUs -- "replicas only": complete independent MPC problems,
    NO collective on the data path (the process group only brackets the timed region).  weak scaling: per-GPU work is fixed.
    A step = one batched control step = E_local controller __call__s; value = instances x steps / s over all ranks,
    teacher-forced on the instances' noisy states after a short closed-loop warm-up (means carried), like the default config.
    Extra: closed_loop (covo_run_episode_batched: control + env step of all instances, one host sync per episode), the step's
    launch groups, and the batched rollout kernel against the HBM roofline."""
    import torch
    import torch.distributed as dist
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    H, E = 32, args.envs_per_gpu
    N = args.N if args.N is not None else 4096
    env = cm.envs.Quad3D(task="tracking", obs_type="quad_params", enable_randomizer=True, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=device)
    c0, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H{H}_lam{args.lam}", device=device, compute_info=False)
    cp0 = c0.init_control_params
    c0.core.close()
    del c0
    gids = [rank * E + e for e in range(E)]  # global instance ids of this rank
    params = [env.sample_params(cr.PRNGKey(1000 + g)) for g in gids]
    b = cm.controllers.BatchedCoVOController(env, E, N, H, args.lam, discount=cp0.discount, gamma_mean=cp0.gamma_mean,
                                             sample_sigma=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=device)
    ep = cm.envs.BatchedDeviceEpisode(env, [cr.PRNGKey(2000 + g) for g in gids], params, (b.core.lib, b.core.h), device)
    rngs = np.stack([np.asarray(cr.PRNGKey(3000 + g)) for g in gids])
    rngs = b.run_episode(ep, rngs, 20)          # off the reset point, on the device
    torch.cuda.synchronize()
    keys = np.stack([np.asarray(cr.PRNGKey(4000 + g)) for g in gids]).astype(np.uint32)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        keys[:, 1] += 1
        b(None, keys)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        keys[:, 1] += 1
        u = b(None, keys)
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if backend == "gloo" else device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    assert torch.isfinite(b.a_mean).all(), "non-finite a_mean after the timed region"
    out = {
        "metric": "mpc_control_steps_per_sec", "value": world * E * args.steps / elapsed,
        "unit": "control-steps/s (env instances x steps)", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"covo-online `tracking` with domain randomisation, {world * E} env instances x N={N} H={H} "
                               f"lam={args.lam} sigma=0.5: {E} instances per GPU in one batched graph (covo_mpc_step_batched), "
                               f"env-sharded over {world} rank(s), no collective (BASELINE.json configs[4]; teacher-forced noisy "
                               "states after a 20-step closed-loop warm-up)",
                   "controller": "covo-online", "envs_total": world * E, "envs_per_gpu": E, "N_per_env": N, "H": H},
    }
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"u": u, "a_mean": b.a_mean, "a_cov": b.a_cov})
    if not args.full:
        if rank == 0:
            print(json.dumps(out))
        b.core.close()
        if world > 1:
            dist.destroy_process_group()
        return
    # launch groups of the step (graph replays of 10 copies each, GPU time per copy)
    phases = {}
    try:
        t_all = b.time_phases(2 | 4 | 8 | 16 | 32)
        phases = {"hessian_us": b.time_phases(2), "sigma_us": b.time_phases(4), "noise_gemm_us": b.time_phases(8),
                  "rollout_us": b.time_phases(16), "update_us": b.time_phases(32), "all_but_begin_us": t_all}
    except Exception as e:  # noqa: BLE001
        phases = {"error": str(e)}
    # closed loop: one 300-step episode of all instances, controller and env on the device
    closed = None
    if not args.no_closed_loop:
        ep2 = cm.envs.BatchedDeviceEpisode(env, [cr.PRNGKey(5000 + g) for g in gids], params, (b.core.lib, b.core.h), device)
        b.a_mean.copy_(torch.as_tensor(cp0.a_mean, device=device).reshape(1, -1).expand(E, -1))
        r2 = np.stack([np.asarray(cr.PRNGKey(6000 + g)) for g in gids])
        r2 = b.run_episode(ep2, r2, 5)            # first-use costs (re-capture on the new buffers), untimed
        T = params[0].max_steps_in_episode - 5
        barrier()
        t0 = time.perf_counter()
        b.run_episode(ep2, r2, T)
        log = ep2.read_log()
        barrier()
        el = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64, device="cpu" if backend == "gloo" else device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        closed = {"unit": "control-steps/s (env instances x steps, control + env step on the device)", "value": world * E * T / el,
                  "steps_per_instance": int(T), "err_pos_mean_m": float(log[:, 5:, 1].mean()),
                  "err_pos_median_instance_m": float(np.median(log[:, 5:, 1].mean(axis=1))),
                  "err_pos_max_instance_m": float(log[:, 5:, 1].mean(axis=1).max()),
                  # an instance whose lissajous trajectory itself leaves the 3 m box (38 of 3 072 `tracking` trajectories do) terminates
                  # there (quadrotor.py:484) and is auto-reset on the device as BaseEnvironment.step does (base.py:22-40): counted here
                  "auto_reset": True, "instances_done_before_T": int((log[:, :, 3].sum(axis=1) > 0).sum()),
                  "resets": int(log[:, :, 3].sum()),
                  "instances_above_0.3_m": int((log[:, 5:, 1].mean(axis=1) > 0.3).sum())}
    if rank == 0:
        alg_bytes = E * N * ROLLOUT_BYTES_PER_SAMPLE
        ro_us = phases.get("rollout_us")
        out["phases_us_per_batched_step"] = phases
        traffic = traffic_src = None
        try:  # the committed counter passes of THIS command (scripts/profile_bench.sh), dropped when the kernel sources changed
            with open(os.path.join(ROOT, "profiles", "r06_bench_envs_pmc_summary.json")) as f:
                pm = json.load(f)
            traffic_src = {"kind": "committed_profile", "file": "profiles/r06_bench_envs_pmc_summary.json", "commit": pm.get("commit"),
                           "kernel_src_sha": pm.get("kernel_src_sha")}
            if pm.get("kernel_src_sha") == kernel_src_sha() and E == 32 and N == 4096:
                traffic = pm.get("traffic_bytes_per_launch")
            else:
                traffic_src["stale"] = "kernel sources or workload changed since the profile was taken: counters dropped"
        except Exception:
            pass
        if ro_us:
            ach = alg_bytes / (ro_us * 1e-6) / 1e9
            out["roofline"] = {"bound": "hbm", "kernel": "rollout_pipe3_kernel<..., BATCHED = true, REC = true> (all instances, one launch)",
                               "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": traffic,
                               "counters_source": traffic_src,
                               "algorithmic_bytes_per_launch": alg_bytes, "launch_us": ro_us,
                               "launch_us_statistic": "graph replay of 10 copies of the batched rollout launch on the step's buffers "
                                                      "(covo_debug_time_batched), fastest of 3 replays"}
        if closed is not None:
            out["closed_loop"] = closed
        print(json.dumps(out))
    b.core.close()
    if world > 1:
        dist.destroy_process_group()


def self_launch(n, argv):
    """Start `python -m torch.distributed.run --nnodes=1 --nproc-per-node n --master-addr 127.0.0.1 --master-port <free>
    bench.py <argv>` as a child process (the driver's own N > 1 command line) and wait for it -> its exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL / peer mappings between the ranks
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.run(cmd, env=env).returncode


def rendezvous_only(args, world, rank):
    """--rendezvous-only: everything of the N-rank bench except the GPU work -- process group (gloo), the barrier bracket, the
    max-over-ranks reduction, ONE line from rank 0."""
    import torch
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("gloo")
        dist.barrier()
    t0 = time.perf_counter()
    if world > 1:
        dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank == 0:
        print(json.dumps({"metric": "mpc_control_steps_per_sec", "value": None, "unit": "control-steps/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "rendezvous_only": True, "barrier_bracket_s": float(t.item()),
                          "scaling": "weak" if args.config == "envs" else "strong"}))
    if world > 1:
        dist.destroy_process_group()


def headline(args, world, elapsed, H, n_states, idx_timed, n_local, exchange_name):
    """--config samples: the fields of the result line every run prints; --full adds its measurements to them."""
    return {
        "metric": "mpc_control_steps_per_sec", "value": args.steps / elapsed, "unit": "control-steps/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{args.controller} {args.task} N={args.N} H={H} lam={args.lam} sigma=0.5 "
                               f"(teacher-forced on the recorded inputs -- noisy state, a_mean, key -- of this controller's own "
                               f"{n_states}-step closed-loop episode, timed steps spread evenly over the episode; samples sharded "
                               f"{world}x{n_local}, one exchange of the 516-float rank records per step: {exchange_name})",
                   "controller": args.controller, "task": args.task, "N_global": args.N, "N_local": n_local, "H": H,
                   "timed_episode_steps": idx_timed if len(idx_timed) <= 64 else f"{len(idx_timed)} indices, stride "
                                                                                f"{n_states / len(idx_timed):.2f}",
                   "pos_stats_info": bool(args.info)},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", default="samples", choices=["samples", "envs"],
                    help="samples: BASELINE configs[3] (default; the headline: N samples sharded over the GPUs); envs: configs[4] "
                         "(domain-randomised env instances, env-sharded, no collective)")
    ap.add_argument("--envs-per-gpu", type=int, default=32, help="--config envs: instances per GPU (256 / 8)")
    ap.add_argument("--controller", default="covo-online", choices=["covo-online", "covo-offline", "mppi"])
    ap.add_argument("--N", type=int, default=None, help="global number of samples (default 65536; --config envs: per instance, default 4096)")
    ap.add_argument("--lam", type=float, default=0.01)
    ap.add_argument("--info", action="store_true", help="also compute pos_mean/pos_std (covo.py:281); XLA drops "
                    "them as dead code in the reference's eval loop (quadrotor.py:523-538)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure everything beside the headline: roofline and GEMM figures, Sigma chain "
                         "counts, closed loop, the pos_info leg, the rollout sweep, the CPU baseline (the --no-* switches below "
                         "drop single parts of it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32 / float64, 64 MB at most)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-closed-loop", action="store_true", help="skip the closed-loop episodes (profiler counter passes)")
    ap.add_argument("--no-info-leg", action="store_true", help="skip the second timed loop with pos_mean/pos_std on")
    ap.add_argument("--no-sweep", action="store_true", help="skip roofline.sweep (the stand-alone rollout at 65 536 ... 1 048 576 samples)")
    ap.add_argument("--cpu-budget", type=float, default=15.0)
    ap.add_argument("--task", default="tracking_zigzag", help="--config samples: the env task (BASELINE configs[0] is `hovering`)")
    ap.add_argument("--rendezvous-only", action="store_true",
                    help="launch the ranks, form the process group, bracket an empty timed region and print the line's launch "
                         "fields (n_gpus, ...) with value null: the N > 1 launcher on a box without GPUs (tests)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` as the driver's 1-GPU command is spelled: this process becomes the launcher.  It has made NO
        # GPU call (torch is not even imported) and makes none: the ranks are CHILD processes of torch.distributed.run, whose
        # output (rank 0's one JSON line) passes through and whose exit code is returned.
        sys.exit(self_launch(args.gpus, sys.argv[1:]))

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.rendezvous_only:
        return rendezvous_only(args, world, rank)
    assert torch.cuda.is_available(), "bench.py needs the MI355X (no CPU fallback)"
    # COVO_BENCH_BACKEND=gloo: rehearsal of the N > 1 code path on a box with fewer GPUs than ranks (ranks share devices,
    # the 528-byte records are staged through the host); the product backend is nccl = RCCL over xGMI, one rank per GPU
    backend = os.environ.get("COVO_BENCH_BACKEND", "nccl")
    if backend == "gloo":
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    device = f"cuda:{local_rank}"
    pg = None
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "gloo":
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device(device))
        pg = dist.group.WORLD
    if args.config == "envs":
        return bench_envs(args, world, rank, device, backend)
    if args.N is None:
        args.N = 65536

    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    from covo_mpc_amd.dynamics.dataclass import DeviceState

    H = 32
    env = cm.envs.Quad3D(task=args.task, obs_type="quad", enable_randomizer=False, disturb_type="gaussian",
                         disable_rollover_terminate=True, generate_noisy_state=True, device=device)
    params = env.default_params
    controller, cp = cm.envs.get_controller(env, args.controller, f"N{args.N}_H{H}_lam{args.lam}", device=device,
                                            process_group=pg, compute_info=args.info)
    n_states = params.max_steps_in_episode
    online = args.controller == "covo-online"
    # ---- untimed recording pass: the controller's OWN closed-loop episode (every rank runs the same replicated env)
    rec = record_episode(env, controller, params, n_states, with_counts=online and args.full)
    host_states, s_reset = rec["states"], rec["s_reset"]
    cp = rec["cp_reset"]  # offline: the Sigma table of this episode's reset state
    packed_d = torch.from_numpy(rec["packed"]).to(device)
    a_means_d = rec["a_means"].contiguous()  # [T, 128] on the device: control_params.a_mean of every recorded call
    dref = s_reset.to_device(device)
    dstates = [DeviceState(packed=packed_d[i], pos_traj=dref.pos_traj, vel_traj=dref.vel_traj, time=int(host_states[i].time))
               for i in range(n_states)]
    controller.alias_outputs = True  # returned tensors alias the controller's buffers: no per-step clones
    core = controller.core
    # the timed steps' inputs: indices spread evenly over the whole episode (warm-up: its own spread)
    idx_warm, idx_timed = spread_indices(args.warmup, n_states), spread_indices(args.steps, n_states)
    a_mean_rows = [a_means_d[i].view(H, 4) for i in range(n_states)]

    def step(i, cp_prev):
        """One teacher-forced controller __call__ on the recorded inputs of closed-loop step i: noisy state, a_mean, key.
        (Everything else of control_params is what the previous call returned: covo-online's a_cov is an output only, covo-offline's
        table is per episode, MPPI's a_cov -- gamma_sigma = 0: H identical blocks, invariant under the shift -- equals the recorded.)
        -> (u, control_params, info) as the controller returns them."""
        return controller(None, None, params, rec["keys"][i], cp_prev.replace(a_mean=a_mean_rows[i]), {"noisy_state": dstates[i]})

    for i in idx_warm:
        cp = step(i, cp)[1]
    torch.cuda.synchronize()

    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in idx_timed:
        u, cp, info = step(i, cp)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if backend == "gloo" else device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    assert torch.isfinite(cp.a_mean).all(), "non-finite a_mean after the timed region"
    if args.dump_outputs and rank == 0:  # right here: the returned tensors alias the controller's buffers, which --full reuses
        outs = {"u": u, "a_mean": cp.a_mean, "a_cov": cp.a_cov}
        outs.update({k: v for k, v in info.items() if torch.is_tensor(v)})
        dump_outputs(args.dump_outputs, outs)
    n_local, exchange_name = core.n_local, core.exchange
    if not args.full:
        if rank == 0:
            print(json.dumps(headline(args, world, elapsed, H, n_states, idx_timed, n_local, exchange_name)))
        if world > 1:
            dist.destroy_process_group()
        return
    kstate = dstates[idx_timed[len(idx_timed) // 2]]  # the state the stand-alone kernel timings below run on

    # The rollout kernel of the timed steps runs inside the fused step and cannot be bracketed individually from the host.
    # `launch_us` = MEAN duration of back-to-back launches of the SAME kernel variant the step runs (with the softmax
    # records; with the position statistics under --info) on the SAME buffers, measured right here with events on the launch
    # stream, 3 x 100 launches issued from C (covo_debug_time_rollout; `launch_us_min` = the fastest batch of 100);
    # `in_step_us` = graph-replay time of the (noise GEMM -> rollout) pair minus the GEMM alone (covo_debug_time_step: 20
    # copies in one graph), i.e. the rollout reading stripes the GEMM has just written; `standalone_*` = the variant WITHOUT
    # the records (covo_rollout_cost as a stand-alone call).  The rocprofv3 kernel trace of this command (profiles/) lists
    # the two variants under their own names (last template argument).
    pc = params.to_c()
    standalone = None
    if args.info:  # position statistics + finalize launch: two launches per call, timed from Python with events
        reps = 50
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            core.rollout(kstate, pc, (0.0, 0.0, 0.0), True)
        e0.record()
        for _ in range(reps):
            core.rollout(kstate, pc, (0.0, 0.0, 0.0), True)
        e1.record()
        torch.cuda.synchronize()
        launch_us = launch_us_min = 1e3 * e0.elapsed_time(e1) / reps
        kernel_name = "rollout_pipe3_kernel<STATS> + pos_stats_finalize_kernel"
    else:
        launch_us, launch_us_min = core.time_rollout(kstate, pc, reps=100, with_records=True)
        standalone = core.time_rollout(kstate, pc, reps=100, with_records=False)
        kernel_name = "rollout_pipe3_kernel<..., REC = true>"
    in_step_us = gemm_in_step_us = in_step_rounds = gemm_in_step_rounds = in_step_rejected = gemm_added_us = gemm_added_rounds = None
    in_step_by_index = None
    if world == 1:
        try:
            # covo_debug_time_step replays the LAST step: make that a mid-episode one (the replays below), and take the rollout's
            # in-step duration at three indices spread over the episode -- it is DATA dependent through the softmax-record epilogue:
            # in an episode's last ~30 steps (time + k >= 300 freezes the rewards, quadrotor.py:483) the samples' costs nearly
            # coincide, every sample carries weight and the epilogue walks whole waves: 16.5 us there against 11.6 elsewhere
            probe_idx = [idx_timed[(2 * q + 1) * len(idx_timed) // 6] for q in range(3)] if len(idx_timed) >= 3 else [idx_timed[0]]
            cp = step(probe_idx[1], cp)[1]
            # every figure is a DIFFERENCE of two graph-replay times; for covo-online both carry the ~135 us Sigma chain, so 1 % of
            # clock wander between the two replays would move the 10 us rollout by 1.4 us (r03: the driver's 20-step command read
            # frac 0.34 ... 0.43 run to run).  The selections are therefore replayed interleaved, four times each, and the
            # fastest replay of each is used: both then sit at the same (highest) clock.
            def rounds_of(*masks, rounds=4):
                return [[core.time_phases(m) for m in masks] for _ in range(rounds)]

            def spread(v):
                v = sorted(v)
                return {"min": v[0], "median": 0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2]), "max": v[-1]}
            if args.controller == "covo-online":
                # the product order: the noise GEMM rides INSIDE the Sigma chain's last launch, streamed under the factorisation
                # (sigma_ns.hip: ns_finalize_stream_kernel); mask 4 alone runs the chain with its plain finalize launch
                rr = rounds_of(4, 4 | 8, 4 | 8 | 16)
                t_sig, t_sig_gemm, t_all = (min(r[i] for r in rr) for i in range(3))
                gemm_added_us = t_sig_gemm - t_sig               # what the streamed GEMM adds to the chain
                in_step_us = t_all - t_sig_gemm
                in_step_rounds = spread([r[2] - r[1] for r in rr])       # the same difference WITHIN each round
                gemm_added_rounds = spread([r[1] - r[0] for r in rr])
                # the GEMM as a launch of its own (rounds 1-4: epsilon drawn under the finalize launch, tiled GEMM behind it): the
                # kernel-quality figure -- every one of its MFMAs, its start-up and its write-back uncovered
                from covo_mpc_amd import _lib as _l
                _l.check(core.lib.covo_debug_set_stream_gemm(core.h, 0), "stream_gemm")
                try:
                    rs = rounds_of(4, 4 | 8)
                    gemm_in_step_us = min(r[1] for r in rs) - min(r[0] for r in rs)
                    gemm_in_step_rounds = spread([r[1] - r[0] for r in rs])
                finally:
                    _l.check(core.lib.covo_debug_set_stream_gemm(core.h, 1), "stream_gemm")
            else:
                rr = rounds_of(8, 8 | 16)
                gemm_in_step_us, t_both = (min(r[i] for r in rr) for i in range(2))
                in_step_us = t_both - gemm_in_step_us
                in_step_rounds = spread([r[1] - r[0] for r in rr])
                gemm_in_step_rounds = spread([r[0] for r in rr])
            # a difference of two independently minimised ~150 us replays standing in for a ~10 us kernel: only accepted when it is
            # positive AND agrees with the per-round differences (else the warm back-to-back figure is the judged duration)
            if not (in_step_us > 0 and in_step_rounds["min"] > 0 and
                    0.7 * in_step_rounds["median"] <= in_step_us <= 1.3 * in_step_rounds["median"]):
                in_step_rejected = in_step_us
                in_step_us = None
            if in_step_us is not None:
                def rollout_in_step():
                    ro = rounds_of(*((4 | 8, 4 | 8 | 16) if args.controller == "covo-online" else (8, 8 | 16)), rounds=3)
                    return min(r[1] for r in ro) - min(r[0] for r in ro)
                in_step_by_index = {str(probe_idx[1]): in_step_us}
                for q in (0, 2):
                    if q < len(probe_idx):
                        cp = step(probe_idx[q], cp)[1]
                        in_step_by_index[str(probe_idx[q])] = rollout_in_step()
                in_step_us = float(np.mean(list(in_step_by_index.values())))  # the judged figure: the mean over the three indices
            if not (gemm_in_step_us and gemm_in_step_us > 0):
                gemm_in_step_us = None
        except Exception:
            in_step_us = gemm_in_step_us = None

    # ---- what the timed steps ran, for comparing values like for like: the Sigma chain's data-dependent
    # squaring / Newton-Schulz counts on the timed states (an untimed replay, one read-back per step), and the step's launch
    # groups split into what every rank of a sample-sharded run REPEATS (Hessian + Sigma chain) and what shrinks with 1 / G
    # (noise GEMM, rollout, update): the expected strong scaling is on the line, not left to be discovered (item 5)
    chain_counts = split = None
    if online and rank == 0:
        try:
            cnt = []
            for i in idx_timed[:100]:
                cp = step(i, cp)[1]
                cnt.append(sigma_chain_counts(core))
            chain_counts = {"mean_squarings": float(np.mean([c[0] for c in cnt])),
                            "mean_newton_schulz_iterations": float(np.mean([c[1] for c in cnt])), "steps": len(cnt),
                            "episode_mean_squarings": float(rec["counts"][:, 0].mean()),
                            "episode_mean_newton_schulz_iterations": float(rec["counts"][:, 1].mean()),
                            "note": "untimed replay of the timed steps with one read-back each; episode_* = all 300 steps of the "
                                    "recorded closed-loop episode the timed inputs were taken from"}
        except Exception as e:  # noqa: BLE001
            chain_counts = {"error": str(e)}
    if world == 1:
        try:
            rep = core.time_phases(2 | 4) if args.controller == "covo-online" else 0.0
            sh = core.time_phases(8 | 16 | 32)
            split = {"replicated_us": rep, "sharded_us": sh,
                     "note": "graph replay of the launch groups of one step at N_local = N: Hessian + Sigma chain are repeated by every "
                             "rank of a sample-sharded run (north_star: the eigendecomposition stays single-GPU), noise GEMM + "
                             "rollout + update shrink with 1 / G and ONE ~10-20 us exchange of the 2 064-byte rank records is added: "
                             f"expected speed-up at G = 8 about {(rep + sh) / (rep + sh / 8 + 15.0):.2f}x (unmeasured: no multi-GPU box)"}
        except Exception as e:  # noqa: BLE001
            split = {"error": str(e)}

    closed = closed_loop(env, controller, params, n_states, rec) if (world == 1 and rank == 0 and not args.no_closed_loop) else None

    # ---- the same steps with covo.py:281's pos_mean / pos_std (a22) computed: a second controller, same inputs, same keys,
    # same barrier + sync bracket; reported NEXT to `value` (the reference's jitted eval loop drops the info as dead code,
    # a plain controller __call__ returns it)
    # The first controller is destroyed first: two live handles per process are harmless on a GPU of one's own, but with
    # several ranks SHARING one GPU (the single-box rehearsal of --gpus N) every launch of the second handle ran 2.3x
    # slower (hardware-queue oversubscription) -- r03 measurement, DESIGN.md 6.
    elapsed_other = None
    if not args.no_info_leg:
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()  # peers map this rank's exchange buffer: everybody is done with it before anybody frees it
        core.close()
        del controller, core, cp
        ctrl2, cp2 = cm.envs.get_controller(env, args.controller, f"N{args.N}_H{H}_lam{args.lam}", device=device,
                                            process_group=pg, compute_info=not args.info)
        cp2 = ctrl2.reset(s_reset, params, ctrl2.init_control_params, cr.PRNGKey(22))
        ctrl2.alias_outputs = True

        def step2(i, cp_prev):
            u, cp_out, _ = ctrl2(None, None, params, rec["keys"][i], cp_prev.replace(a_mean=a_mean_rows[i]), {"noisy_state": dstates[i]})
            return cp_out

        for i in idx_warm:
            cp2 = step2(i, cp2)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in idx_timed:
            cp2 = step2(i, cp2)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        elapsed_other = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([elapsed_other], dtype=torch.float64, device="cpu" if backend == "gloo" else device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed_other = float(t.item())
        del ctrl2, cp2

    sweep = None
    if rank == 0 and world == 1 and not args.no_sweep:
        try:
            sweep = rollout_sweep(kstate, pc, args.lam, device)
        except Exception as e:  # noqa: BLE001
            sweep = [{"error": str(e)}]
    if rank == 0:
        alg_bytes = n_local * ROLLOUT_BYTES_PER_SAMPLE
        # the judged duration is the kernel's IN-STEP duration (what the timed region ran and what the rocprofv3 kernel trace
        # of this command averages, cold stripes fresh from the GEMM); the warm back-to-back figure rides along
        b2b_us, b2b_min_us = launch_us, launch_us_min
        if in_step_us:
            launch_us = in_step_us
        achieved = alg_bytes / (launch_us * 1e-6) / 1e9
        pmc, pmc_src = pmc_counters(args, n_local)
        kin = (pmc or {}).get("kernels", {})
        out = {**headline(args, world, elapsed, H, n_states, idx_timed, n_local, exchange_name),
            "roofline": {"bound": "hbm", "kernel": kernel_name,
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": (pmc or {}).get("traffic_bytes_per_launch"), "counters_source": pmc_src,
                         "algorithmic_bytes_per_launch": alg_bytes, "launch_us": launch_us, "launch_us_statistic":
                         ("in-step: graph replay of 20 x (Sigma chain, GEMM, rollout) minus 20 x (Sigma chain, GEMM), events around "
                          "the replay, fastest replay of each selection over 4 interleaved rounds; in_step_us_per_round = the "
                          "same difference within each round (min / median / max); mean over three steps of the episode "
                          "(in_step_us_by_episode_step: the record epilogue is data dependent)" if in_step_us
                          else "mean of 3 x 100 back-to-back launches (events on the launch stream)"),
                         "in_step_us": in_step_us, "in_step_us_per_round": in_step_rounds,
                         "in_step_us_by_episode_step": in_step_by_index,
                         "in_step_us_rejected": in_step_rejected,
                         "back_to_back": {"launch_us": b2b_us, "launch_us_min": b2b_min_us,
                                          "frac": alg_bytes / (b2b_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                                          "statistic": "mean / fastest batch of 3 x 100 back-to-back launches on warm stripes"},
                         "standalone_without_records": None if standalone is None else {
                             "kernel": "rollout_pipe3_kernel<..., REC = false>", "launch_us": standalone[0],
                             "launch_us_min": standalone[1],
                             "frac": alg_bytes / (standalone[0] * 1e-6) / 1e9 / HBM_PEAK_GBS},
                         "counters": (kin.get("rollout_in_step") or {}).get("derived"),
                         "sweep": sweep, "sweep_statistic": "stand-alone rollout_pipe3_kernel<..., REC = false> on the timed "
                         "mid-episode state, mean (launch_us) / fastest batch (launch_us_min) of 3 x 100 back-to-back launches "
                         "between HIP events on the launch stream; frac = 516 B x N / launch_us / 8 TB/s"},
        }
        if args.controller != "covo-online" and n_local <= 16384 and not args.info and args.task in ("tracking_zigzag", "hovering"):
            out["config"]["one_launch_step"] = ("the timed steps run as ONE launch per control step (csrc/step_small.hip: begin + noise draw + "
                                                "rollout + softmax records + merge); the roofline figures below time the staged kernels")
        if elapsed_other is not None:
            v2 = args.steps / elapsed_other
            out["value_with_pos_info" if not args.info else "value_without_pos_info"] = v2
        if gemm_in_step_us:
            dense = n_local * GEMM_FLOP_PER_SAMPLE_DENSE / (gemm_in_step_us * 1e-6) / 1e12
            issued = n_local * GEMM_FLOP_PER_SAMPLE_ISSUED / (gemm_in_step_us * 1e-6) / 1e12
            out["roofline_gemm"] = {"bound": "mfma", "kernel": "noise_gemm_kernel", "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                                    "in_step_us": gemm_in_step_us, "in_step_us_per_round": gemm_in_step_rounds,
                                    "achieved_dense_equivalent": dense,
                                    "frac_dense_equivalent": dense / MFMA_F32_PEAK_TFLOPS, "achieved": issued,
                                    "frac": issued / MFMA_F32_PEAK_TFLOPS,
                                    "flop_per_sample": {"dense_equivalent": GEMM_FLOP_PER_SAMPLE_DENSE,
                                                        "issued": GEMM_FLOP_PER_SAMPLE_ISSUED},
                                    "counters": (kin.get("noise_gemm") or {}).get("derived")}
            if gemm_added_us is not None:
                out["roofline_gemm"]["statistic"] = (
                    "the noise GEMM as a launch of its own behind the Sigma chain (covo_debug_set_stream_gemm(handle, 0): graph replay of 20 x "
                    "(chain, GEMM) minus 20 x (chain)); the timed steps run it STREAMED inside the chain's finalize launch, where it "
                    "adds streamed_added_us to the chain (same replays, product mode)")
                out["roofline_gemm"]["streamed_added_us"] = gemm_added_us
                out["roofline_gemm"]["streamed_added_us_per_round"] = gemm_added_rounds
                out["roofline_gemm"]["counters_streamed_launch"] = (kin.get("finalize_stream") or {}).get("derived")
        if chain_counts is not None:
            out["sigma_chain"] = chain_counts
        if split is not None:
            out["sample_sharding_split"] = split
        if closed is not None:
            out["closed_loop"] = closed
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(host_states, params, args.N, H, args.lam, args.cpu_budget)
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
