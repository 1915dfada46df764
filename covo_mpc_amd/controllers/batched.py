"""The sampling controllers for E independent env instances in one call (BASELINE.json configs[4]).

The reference runs its `--mode render` / eval loop on one env instance and reaches many instances through
`jax.vmap` of the whole controller (quadjax/envs/quadrotor.py:497-538 is written per instance and vmap-clean).
Here that is `covo_mpc_step_batched` / `covo_mpc_step_batched_mode` (include/covo_hip.h, csrc/step.hip):
  covo-online   one hipGraph holding ONE batched Hessian + Sigma launch set for all instances and the per-instance sampling path;
  covo-offline, MPPI   the key upload plus ONE fused launch for all instances (csrc/step_small.hip, instance = grid dimension);
                       with staged=True the launch sequence of a single staged step with the instance as a grid dimension
                       (covo_set_step_batched_staged), which takes every step option and disturbance model the single controllers take.
Every instance has its own state, reference trajectory, (domain-randomised) parameters, mean, key (and, per mode, Sigma table or
block covariances); instance e's result is bit-identical to the single controller's `__call__` on that instance alone
(tests/test_gpu_parity.py::test_batched_step_equals_replicas, tests/test_gpu_batched_modes.py).
Instances never exchange data ("replicas only"): to use G GPUs give each rank E/G instances.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from .._lib import COVO_H, COVO_NA, check
from ..dynamics.dataclass import as_device_state
from ._core import SamplingCore
from ._options import check_sigma_nodes, check_step_options, check_step_switches, take, take_switches

# (controller attribute, core attribute) of the attachment buffers the batched controllers hand out
CORE_BUFFERS = (("diag", "diag"), ("plan", "plan"), ("fan", "fan"), ("arbiter", "arbiter"), ("lam_eff", "lam_eff"), ("elite", "elite_rows"),
                ("iter_cost_min", "iter_cost_min"), ("post_cov", "post_cov"), ("post_aux", "post_aux"),
                ("sigma_adapt_rows", "sigma_adapt_rows"), ("refine", "refine_rows"), ("riccati", "riccati_rows"),
                ("riccati_feedback", "riccati_feedback_rows"), ("plan_hold_rows", "plan_hold_rows"),
                ("riccati_box", "riccati_box_masks"), ("sigma_nodes_rows", "sigma_nodes_rows"))


class BatchedCoVOController:
    """CoVO-MPC for E instances.  mode="online" (default): Sigma from every instance's own Hessian at every step;
    mode="offline": Sigma looked up in a per-instance table built by `reset` (covo.py:44-112, per instance)."""
    MODE = None  # subclasses with a fixed mode (BatchedMPPIController)

    def __init__(self, env, n_envs: int, N: int, H: int, lam: float, *, discount: float = 1.0, gamma_mean: float = 1.0,
                 sample_sigma: float = 0.5, a_mean_init=None, device=None, mode: str = "online", compute_diag: bool = False,
                 compute_plan: bool = False, ess_min=None, compute_fan=None, update: str = "softmax", iters: int = 1, elite=None,
                 sigma_period: int = 1, compute_post_cov: bool = False, sigma_adapt: float = 0.0, staged: bool = False,
                 refine: bool = False, riccati: bool = False, riccati_feedback: bool = False, plan_hold: int = 1,
                 riccati_box: bool = False, sigma_nodes=None, node_interp: str = "linear"):
        opts, switches = take(locals()), take_switches(locals())
        moded = self.MODE is not None or mode != "online"  # the MPPI / covo-offline step
        if staged and not moded:
            raise ValueError("staged=True with mode=\"online\": the env-batched covo-online step is a staged launch sequence already; "
                             "staged= belongs to BatchedMPPIController and BatchedCoVOController(mode=\"offline\")")
        # staged (not a step option: a switch of these two controllers, off by default): the step runs as the launch sequence of a
        # single staged step with the instance as a grid dimension instead of the one fused launch -- also where the fused launch
        # would do -- and takes what that launch refuses
        self.staged = bool(staged)
        fused = moded and not self.staged  # one fused launch for all instances
        what = ("online" if not moded else
                "the env-batched MPPI controller" if self.MODE is not None else f"the env-batched covo-{mode} controller")
        check_step_options(N, what, fused_batched=fused, **opts)
        check_step_switches(what, sigma_period=sigma_period, disturb_type=getattr(env, "disturb_type", None), **switches)
        # sigma_nodes=M (covo-online only; _options.check_sigma_nodes): .sigma_nodes_rows [E, 8] after a call
        check_sigma_nodes(sigma_nodes, node_interp, what=what, sigma_period=sigma_period, sigma_adapt=sigma_adapt, refine=refine)
        if self.MODE is not None:
            self.mode = self.MODE
        elif mode in ("online", "offline"):
            self.mode = _lib.MODE_COVO_ONLINE if mode == "online" else _lib.MODE_COVO_OFFLINE
        else:
            raise NotImplementedError(mode)  # covo.py:113-114
        if not 0 < n_envs <= _lib.COVO_MAX_ENVS:
            raise ValueError(f"n_envs={n_envs} outside (0, {_lib.COVO_MAX_ENVS}]")
        self.env, self.E, self.N, self.H = env, int(n_envs), int(N), int(H)
        self.gamma_mean, self.sample_sigma = float(gamma_mean), float(sample_sigma)
        self.rollover_terminate = not getattr(env, "disable_rollover_terminate", True)  # quadrotor.py:486
        # every disturbance model of the env is taken: for periodic / sin / drag / mixed covo_mpc_step_batched builds each
        # instance's per-step tables (csrc/disturb.hip) from its state, raw key and disturb_params inside the graph
        # one call advances all instances: the ~56 launches are worth a graph (same GPU time as eager, 40 us instead of
        # 150-270 us of host time per call)
        self.core = SamplingCore(N, H, lam, discount, device=device, compute_info=False, trust_clipped=True, use_graph=True,
                                 diag_rows=int(n_envs), **switches, **opts, sigma_nodes=sigma_nodes, node_interp=node_interp)
        if moded:
            check(self.core.lib.covo_set_step_batched_staged(self.core.h, int(self.staged)), "covo_set_step_batched_staged")
        # after a call, row e of each of the core's attachment buffers holds instance e's result of that step; None for what is off
        # (the options: _options.py; the rows: where SamplingCore allocates them; include/covo_hip.h).  sigma_period: the batch shares
        # one age -- self.sigma_age is the age the last call ran at (0 = refresh), reset() restarts the schedule
        for mine, cores in CORE_BUFFERS:
            setattr(self, mine, getattr(self.core, cores))
        torch = self.core.torch
        f32 = dict(dtype=torch.float32, device=self.core.device)
        E, n = self.E, self.N
        self.a_mean = torch.zeros((E, COVO_NA), **f32)
        if a_mean_init is not None:
            self.a_mean.copy_(torch.as_tensor(a_mean_init, **f32).reshape(1, COVO_NA).expand(E, COVO_NA))
        # online: the Sigma every instance sampled from (out); MPPI: the H 4x4 blocks (in/out, shifted in place each step)
        self.a_cov = torch.zeros((E, COVO_H, 4, 4) if self.mode == _lib.MODE_MPPI else (E, COVO_NA, COVO_NA), **f32)
        self.a_cov_offline = self.a_chol_offline = None  # offline: [E][T][128][128] tables, built by reset()
        self.gamma_sigma = 0.0
        self._a = torch.empty((E, COVO_H, n, 4), **f32)
        self._cost = torch.empty((E, n), **f32)
        self._groupmin = torch.empty((E, (n + 63) // 64), **f32)
        self._states = torch.zeros((E, _lib.COVO_STATE_FLOATS), **f32)
        self._traj = None  # (pos [E,T,3], vel [E,T,3], source ptrs)
        self._params = None
        self._args = None

    def set_instances(self, env_states, env_params):
        """Bind the E instances' reference trajectories and parameters (once per episode)."""
        torch = self.core.torch
        ds = [as_device_state(s, self.core.device) for s in env_states]
        T = ds[0].T
        if any(d.T != T for d in ds):
            raise ValueError("all instances must share the trajectory length T")
        pos = torch.stack([d.pos_traj.reshape(T, 3) for d in ds]).contiguous()
        vel = torch.stack([d.vel_traj.reshape(T, 3) for d in ds]).contiguous()
        self._traj = (pos, vel, T)
        from .base import env_model_params_c
        self._params = (_lib.EnvParamsC * self.E)(*[env_model_params_c(self.env, p) for p in env_params])
        self._args = self._make_args(self._states, pos, vel, T)
        self._states_buf = self._states
        self._episode = None

    def _make_args(self, states, pos, vel, T):
        """struct covo_batch_mode_args over the controller's buffers; its `base` is the covo_batch_args of the covo-online entries."""
        m = _lib.BatchModeArgsC()
        a = m.base
        a.n_envs, a.n_samples, a.T = self.E, self.N, T
        a.states, a.pos_traj, a.vel_traj = states.data_ptr(), pos.data_ptr(), vel.data_ptr()
        a.a_mean, a.a_cov = self.a_mean.data_ptr(), self.a_cov.data_ptr()
        a.a, a.cost, a.groupmin = self._a.data_ptr(), self._cost.data_ptr(), self._groupmin.data_ptr()
        a.gamma_mean, a.sample_sigma = self.gamma_mean, self.sample_sigma
        m.mode, m.gamma_sigma = self.mode, self.gamma_sigma
        self._fill_table(m)
        return m

    def _fill_table(self, m):
        if self.mode == _lib.MODE_COVO_OFFLINE and self.a_chol_offline is not None:
            L = self.a_chol_offline
            m.L_table, m.n_table, m.L_table_stride = L.data_ptr(), int(L.shape[1]), int(L.shape[1]) * COVO_NA * COVO_NA

    def reset(self, env_states, env_params, keys):
        """covo-offline: instance e's Sigma table and its Cholesky factors from instance e's own start state, parameters and key,
        through CoVOController.reset_a_cov_offline (covo.py:58-104; once per episode, a host loop over the instances).
        -> (a_cov_offline, a_chol_offline) [E, T, 128, 128].  The other modes have nothing to build."""
        self.core.restart_plan_hold()  # (plan_hold: the episode's first step plans)
        self.core.estimator_reset()
        self.core.force_observer_reset()
        if self.mode != _lib.MODE_COVO_OFFLINE:
            if self.core.sigma_period > 1:  # the schedule restarts: the episode's first step refreshes Sigma
                self.core.set_sigma_period(self.core.sigma_period)
            return None
        from .covo import CoVOController, CoVOParams
        torch = self.core.torch
        cp = CoVOParams(gamma_mean=self.gamma_mean, gamma_sigma=0.0, discount=self.core.discount, sample_sigma=self.sample_sigma,
                        a_mean=None, a_cov=None, a_cov_offline=None)
        if getattr(self, "_builder", None) is None:
            self._builder = CoVOController(self.env, cp, self.N, self.H, self.core.lam, "offline", device=self.core.device,
                                           compute_info=False)
        Sig, L = [], []
        for st, p, k in zip(env_states, env_params, keys):
            out = self._builder.reset_a_cov_offline(st, p, cp, k)
            Sig.append(out.a_cov_offline.clone())
            L.append(out.a_chol_offline.clone())
        if len(Sig) != self.E:
            raise ValueError(f"{len(Sig)} instances given, controller has {self.E}")
        return self.set_tables(torch.stack(Sig), torch.stack(L))

    def set_tables(self, a_cov_offline, a_chol_offline):
        """covo-offline: take ready-made per-instance tables [E, T, 128, 128] (Sigma and its lower Cholesky factors)."""
        if self.mode != _lib.MODE_COVO_OFFLINE:
            raise ValueError("only the covo-offline controller has Sigma tables")
        if tuple(a_chol_offline.shape[:1] + a_chol_offline.shape[2:]) != (self.E, COVO_NA, COVO_NA):
            raise ValueError(f"a_chol_offline {tuple(a_chol_offline.shape)} is not [{self.E}, T, {COVO_NA}, {COVO_NA}]")
        self.a_cov_offline, self.a_chol_offline = a_cov_offline.contiguous(), a_chol_offline.contiguous()
        if self._args is not None:
            self._fill_table(self._args)
        return self.a_cov_offline, self.a_chol_offline

    def _check_ready(self):
        if self._args is None:
            raise RuntimeError("call set_instances(env_states, env_params) first")
        if self.mode == _lib.MODE_COVO_OFFLINE and self.a_chol_offline is None:
            raise RuntimeError("covo-offline: call controller.reset(...) first (a_cov_offline table missing)")

    def __call__(self, noisy_states, rng_acts):
        """One control step of every instance.  noisy_states: E env states (or a float32 [E, 32] device tensor of
        packed states); rng_acts: uint32 [E, 2] raw controller keys.  -> first actions [E, 4] (view of a_mean)."""
        self._check_ready()
        torch = self.core.torch
        buf = self._states_buf  # the tensor args.states points at: the controller's own, or a bound episode's noisy states
        if noisy_states is None or noisy_states is buf:
            pass  # a bound BatchedDeviceEpisode: the env step kernel has already written them
        elif torch.is_tensor(noisy_states):
            buf.copy_(noisy_states, non_blocking=True)
        else:
            packed = [as_device_state(s, self.core.device).packed for s in noisy_states]
            torch.stack(packed, out=buf)
        self.core.estimated(buf, self.a_mean, self._params)  # (an attached StateEstimator: in place on the rows the step reads)
        keys = np.ascontiguousarray(np.asarray(rng_acts, dtype=np.uint32).reshape(self.E, 2))
        if self.mode == _lib.MODE_COVO_ONLINE:
            check(self.core.lib.covo_mpc_step_batched(self.core.h, C.byref(self._args.base), self._params,
                                                      keys.ctypes.data_as(C.POINTER(C.c_uint32)), self.core.stream()),
                  "covo_mpc_step_batched")
        else:
            check(self.core.lib.covo_mpc_step_batched_mode(self.core.h, C.byref(self._args), self._params,
                                                           keys.ctypes.data_as(C.POINTER(C.c_uint32)), self.core.stream()),
                  "covo_mpc_step_batched_mode")
        return self.a_mean.view(self.E, COVO_H, 4)[:, 0]

    @property
    def sigma_age(self) -> int:
        """The age the last call ran at under sigma_period (0 = it refreshed every instance's Sigma; always 0 without a period)."""
        return self.core._sigma_ages()[1]

    @property
    def plan_age(self) -> int:
        """The age the last call ran at under plan_hold (0 = every instance planned; always 0 without it)."""
        return self.core._plan_ages()[1]

    def time_phases(self, step_mask: int, reps: int = 10) -> float:
        """GPU microseconds of the selected launch groups of the LAST batched step (2 Hessian, 4 Sigma, 8 GEMM, 16 rollout,
        32 update), replayed `reps` times from one graph (covo_debug_time_batched)."""
        us = C.c_float(0.0)
        self.core.torch.cuda.synchronize()
        check(self.core.lib.covo_debug_time_batched(self.core.h, int(step_mask), int(reps), C.byref(us), self.core.stream()),
              "covo_debug_time_batched")
        return float(us.value)

    def bind_episode(self, episode):
        """Plan from a BatchedDeviceEpisode's buffers: its noisy states ARE the controller's input (rewritten by every env step on
        the device), its trajectories and parameters the instances' (once per episode)."""
        if episode.E != self.E:
            raise ValueError(f"episode has {episode.E} instances, controller {self.E}")
        self._traj = (episode.pos_traj, episode.vel_traj, episode.T)
        self._params = episode.params_c
        self._args = self._make_args(episode.noisy, episode.pos_traj, episode.vel_traj, episode.T)
        self._states_buf = episode.noisy
        self._episode = episode

    def run_episode(self, episode, rngs, n_steps: int):
        """covo_run_episode_batched: n_steps x { batched control step on the noisy states -> batched env step }, all enqueued by
        ONE C call; every instance's key chain threaded like eval_env's run_one_step (quadrotor.py:520-538).  rngs: uint32
        [E, 2] -> the chains' keys after the segment.  Asynchronous; episode.read_log() synchronises."""
        if getattr(self, "_episode", None) is not episode:
            self.bind_episode(episode)
        self._check_ready()
        env = self.env
        keys = np.ascontiguousarray(np.asarray(rngs, dtype=np.uint32).reshape(self.E, 2)).copy()
        # rows n_steps .. of the [E, T + 1, 8] diagnostic log, [E, T + 1, 168] trace, [E, T + 1, K, 100] fan log, [E, T + 1, 8] arbiter log
        # and the logs of the attachments' rows (temperature, elite, iterations, Sigma, posterior covariance)
        self.core.attach_episode_logs(episode, int(episode.log.shape[1]))
        online = self.mode == _lib.MODE_COVO_ONLINE
        fn = self.core.lib.covo_run_episode_batched if online else self.core.lib.covo_run_episode_batched_mode
        check(fn(
            self.core.h, C.byref(self._args.base) if online else C.byref(self._args), self._params, _lib.ptr(episode.true), _lib.ptr(episode.acc_traj),
            1 if env.generate_noisy_state else 0, float(env.default_params.obs_noise_scale), _lib.ptr(episode.log),
            int(episode.log.shape[1]), int(episode.n_steps), keys.ctypes.data_as(C.POINTER(C.c_uint32)), int(n_steps),
            self.core.stream()), "covo_run_episode_batched" if online else "covo_run_episode_batched_mode")
        episode.n_steps += int(n_steps)
        return keys


class BatchedMPPIController(BatchedCoVOController):
    """MPPI (mppi.py:11-134) for E instances: the same methods as BatchedCoVOController; `a_cov` [E, H, 4, 4] starts as
    diag(sigmas**2) tiled over the horizon (quadrotor.py:705-720, as controllers/mppi.py for one instance) and is shifted in
    place by every step (mppi.py:43-49).  sigmas: one standard deviation for all four action components, or four of them."""
    MODE = _lib.MODE_MPPI

    def __init__(self, env, n_envs: int, N: int, H: int, lam: float, *, sigmas=0.5, discount: float = 1.0, gamma_mean: float = 1.0,
                 gamma_sigma: float = 0.0, a_mean_init=None, device=None, compute_diag: bool = False, compute_plan: bool = False,
                 ess_min=None, compute_fan=None, update: str = "softmax", iters: int = 1, elite=None, sigma_period: int = 1,
                 compute_post_cov: bool = False, sigma_adapt: float = 0.0, staged: bool = False):
        opts = take(locals())
        # (ahead of gamma_sigma's refusal; under staged gamma_sigma is taken and has its say in the elite check, as for MPPIController)
        s = check_step_options(N, "the env-batched MPPI controller", fused_batched=not staged,
                               gamma_sigma=gamma_sigma if staged else None, **opts)
        if float(gamma_sigma) != 0.0 and not staged:
            raise NotImplementedError(f"gamma_sigma={gamma_sigma}: MPPI's covariance adaptation (mppi.py:119-125) is not batched; "
                                      "the batched fused launch needs gamma_sigma == 0 (the reference's default), or pass staged=True")
        if float(gamma_sigma) != 0.0 and (s.elite_K or s.ess_min != 0.0):
            with_what = f"elite={elite}" if s.elite_K else f"ess_min={ess_min}"
            raise NotImplementedError(f"gamma_sigma={gamma_sigma} together with {with_what}: the staged env-batched MPPI step adapts "
                                      "a_cov under the softmax weights at the configured lam only (that covariance update has no "
                                      "instance dimension); MPPIController takes both")
        sig = np.broadcast_to(np.asarray(sigmas, dtype=np.float32).reshape(-1), (4,)).copy()
        super().__init__(env, n_envs, N, H, lam, discount=discount, gamma_mean=gamma_mean, sample_sigma=float(sig[0]),
                         a_mean_init=a_mean_init, device=device, staged=staged, **opts)
        self.gamma_sigma = float(gamma_sigma)  # (non-zero under staged only: a_cov[e] is adapted in place, mppi.py:119-125)
        torch = self.core.torch
        blk = torch.diag(torch.as_tensor(sig, dtype=torch.float32, device=self.core.device) ** 2)
        self.a_cov.copy_(blk.expand(self.E, COVO_H, 4, 4))


class BatchedILQRController(BatchedCoVOController):
    """iLQR (controllers/ilqr.py) for E instances: the same methods as BatchedCoVOController -- set_instances / bind_episode, __call__
    (also as .step), run_episode, reset -- through covo_mpc_step_batched_mode / covo_run_episode_batched_mode in COVO_MODE_ILQR.  Every
    iteration's launches take the instance as a grid dimension; instance e's result is bit-identical to ILQRController's on that
    instance alone (tests/test_gpu_ilqr.py).  After a call: .ilqr_rows / .ilqr_feedback_rows [E, iters, 8] (every iteration's Riccati /
    feedback row), .ilqr_summary [E, 8] (SamplingCore.attach_ilqr), .riccati / .riccati_feedback (the last iteration's rows),
    .plan_hold_rows and .plan (None for what is off); under riccati_box .riccati_box [E, 32] (the last sweep's clamp masks) and
    .ilqr_box_count [E, iters] (every iteration's clamped coordinates)."""
    MODE = _lib.MODE_ILQR

    def __init__(self, env, n_envs: int, H: int, *, iters: int = 2, riccati_feedback=None, plan_hold: int = 1,
                 compute_plan: bool = False, discount: float = 1.0, a_mean_init=None, device=None, riccati_box: bool = False):
        from .ilqr import ILQR_N, build_ilqr_core
        from ._options import check_ilqr
        self.iters, self.riccati_feedback_on, self.plan_hold = check_ilqr(
            iters, riccati_feedback=riccati_feedback, plan_hold=plan_hold, disturb_type=getattr(env, "disturb_type", None),
            compute_plan=compute_plan, what="the env-batched iLQR controller", riccati_box=riccati_box)
        if not 0 < n_envs <= _lib.COVO_MAX_ENVS:
            raise ValueError(f"n_envs={n_envs} outside (0, {_lib.COVO_MAX_ENVS}]")
        self.mode, self.staged = self.MODE, False
        self.env, self.E, self.N, self.H = env, int(n_envs), ILQR_N, int(H)
        self.gamma_mean, self.sample_sigma, self.gamma_sigma = 1.0, 0.5, 0.0  # (fields of the argument block an iLQR step never reads)
        self.rollover_terminate = not getattr(env, "disable_rollover_terminate", True)
        # (eager: the iterations are eager launches; nothing of an iLQR step is captured)
        switches = dict(riccati_feedback=self.riccati_feedback_on, plan_hold=self.plan_hold, riccati_box=riccati_box)
        self.core = build_ilqr_core(self.E, H, discount, iters=self.iters, switches=switches, compute_plan=bool(compute_plan),
                                    device=device, use_graph=False)
        for mine, cores in CORE_BUFFERS:
            setattr(self, mine, getattr(self.core, cores))
        self.ilqr_rows, self.ilqr_feedback_rows, self.ilqr_summary = (self.core.ilqr_rows, self.core.ilqr_feedback_rows,
                                                                      self.core.ilqr_summary)
        self.ilqr_box_count = self.core.ilqr_box_count  # [E, iters] int32 under riccati_box, else None
        torch = self.core.torch
        f32 = dict(dtype=torch.float32, device=self.core.device)
        E, n = self.E, self.N
        self.a_mean = torch.zeros((E, COVO_NA), **f32)
        if a_mean_init is not None:
            self.a_mean.copy_(torch.as_tensor(a_mean_init, **f32).reshape(1, COVO_NA).expand(E, COVO_NA))
        # the sample buffers of the argument block, at the smallest size it takes: never launched on
        self.a_cov = torch.zeros((E, 1), **f32)
        self.a_cov_offline = self.a_chol_offline = None
        self._a = torch.empty((E, COVO_H, n, 4), **f32)
        self._cost = torch.empty((E, n), **f32)
        self._groupmin = torch.empty((E, (n + 63) // 64), **f32)
        self._states = torch.zeros((E, _lib.COVO_STATE_FLOATS), **f32)
        self._traj = self._params = self._args = None

    def step(self, noisy_states, rng_acts):
        """One control step of every instance (= __call__) -> first actions [E, 4] (view of a_mean)."""
        return self(noisy_states, rng_acts)


class BatchedCMAController(BatchedCoVOController):
    """CMA-MPC (controllers/cma.py) for E instances: the same methods as BatchedCoVOController -- set_instances / bind_episode, __call__
    (also as .step), run_episode, reset -- through covo_mpc_step_batched_mode / covo_run_episode_batched_mode in COVO_MODE_CMA: covo-online's
    staged batch without its Hessian and Sigma chain, the shape and step-size launches with the instance as a grid dimension.  Every
    instance keeps its own factor, path and step size; instance e's result is bit-identical to CMAController's on that instance alone
    (tests/test_gpu_cma.py).  After a call: .cma_rows [E, 8], .cma_path [E, 128] float64, .a_cov [E, 128, 128] (the covariances the
    step sampled from), .diag, .post_cov, .post_aux and the other step options' buffers (None for what is off)."""
    MODE = _lib.MODE_CMA

    def __init__(self, env, n_envs: int, N: int, H: int, lam: float, *, gamma: float = 0.2, step_size: bool = True, damping: float = 1.0,
                 s_min: float = 0.1, s_max: float = 4.0, discount: float = 1.0, gamma_mean: float = 1.0, sample_sigma: float = 0.5,
                 a_mean_init=None, device=None, compute_plan: bool = False, compute_fan=None, update: str = "softmax", ess_min=None,
                 elite=None, iters: int = 1, sigma_period: int = 1, sigma_adapt: float = 0.0, sigma_nodes=None, refine: bool = False,
                 riccati: bool = False, riccati_feedback: bool = False, plan_hold: int = 1, riccati_box: bool = False):
        from ._options import check_cma
        what = "the env-batched CMA controller"
        self.cma = check_cma(gamma=gamma, step_size=step_size, damping=damping, s_min=s_min, s_max=s_max, sigma_period=sigma_period,
                             sigma_adapt=sigma_adapt, sigma_nodes=sigma_nodes, refine=refine, riccati=riccati,
                             riccati_feedback=riccati_feedback, plan_hold=plan_hold, riccati_box=riccati_box, what=what)
        opts = dict(compute_diag=True, compute_plan=compute_plan, ess_min=ess_min, compute_fan=compute_fan, update=update, iters=iters,
                    elite=elite, compute_post_cov=True)
        check_step_options(N, what, **opts)
        if not 0 < n_envs <= _lib.COVO_MAX_ENVS:
            raise ValueError(f"n_envs={n_envs} outside (0, {_lib.COVO_MAX_ENVS}]")
        self.mode, self.staged = self.MODE, False
        self.env, self.E, self.N, self.H = env, int(n_envs), int(N), int(H)
        self.gamma_mean, self.sample_sigma, self.gamma_sigma = float(gamma_mean), float(sample_sigma), 0.0
        self.rollover_terminate = not getattr(env, "disable_rollover_terminate", True)
        self.core = SamplingCore(N, H, lam, discount, device=device, compute_info=False, trust_clipped=True, use_graph=True,
                                 diag_rows=int(n_envs), **opts)
        self.core.attach_cma(self.cma)
        for mine, cores in CORE_BUFFERS:
            setattr(self, mine, getattr(self.core, cores))
        self.cma_rows, self.cma_path = self.core.cma_rows, self.core.cma_p
        torch = self.core.torch
        f32 = dict(dtype=torch.float32, device=self.core.device)
        E, n = self.E, self.N
        self.a_mean = torch.zeros((E, COVO_NA), **f32)
        if a_mean_init is not None:
            self.a_mean.copy_(torch.as_tensor(a_mean_init, **f32).reshape(1, COVO_NA).expand(E, COVO_NA))
        self.a_cov = torch.zeros((E, COVO_NA, COVO_NA), **f32)
        self.a_cov_offline = self.a_chol_offline = None
        self._a = torch.empty((E, COVO_H, n, 4), **f32)
        self._cost = torch.empty((E, n), **f32)
        self._groupmin = torch.empty((E, (n + 63) // 64), **f32)
        self._states = torch.zeros((E, _lib.COVO_STATE_FLOATS), **f32)
        self._traj = self._params = self._args = None

    def reset(self, env_states=None, env_params=None, keys=None):
        """Episode start: every instance's L = sample_sigma I, p = 0, log s = 0 -- the next step samples from sample_sigma^2 I."""
        self.core.cma_reset()
        self.core.estimator_reset()
        self.core.force_observer_reset()
        return None

    def step(self, noisy_states, rng_acts):
        """One control step of every instance (= __call__) -> first actions [E, 4] (view of a_mean)."""
        return self(noisy_states, rng_acts)


class BatchedDialController(BatchedMPPIController):
    """Annealed MPPI (controllers/dial.py) for E instances: the same methods as BatchedMPPIController -- set_instances / bind_episode,
    __call__ (also as .step), run_episode, reset -- always on the staged env-batched MPPI step (the fused launch shifts and factors
    a_cov itself and needs the temperature before all costs exist).  Every instance runs the same schedule; instance e's result is
    bit-identical to DialController's on that instance alone (tests/test_gpu_anneal.py).  After a call: .anneal_rows [E, iters, 4]
    (every pass's solver row; {lam, 1 / lam, 0, 0} without temp), .anneal_sigma [iters, 32], and the step options' buffers as for
    BatchedMPPIController.  beta_pass = beta_stage = 1 with temp=None attaches nothing: BatchedMPPIController(staged=True, iters=k).
    nodes=M / node_interp: the spline-node perturbations of check_dial, one table for all instances (.anneal_sigma is then sigma_e)."""

    def __init__(self, env, n_envs: int, N: int, H: int, lam: float, *, iters: int = 4, beta_pass: float = 0.5, beta_stage: float = 0.9,
                 temp=0.1, sigmas=0.5, discount: float = 1.0, gamma_mean: float = 1.0, a_mean_init=None, device=None,
                 compute_diag: bool = False, compute_plan: bool = False, compute_fan=None, update: str = "softmax",
                 compute_post_cov: bool = False, nodes=None, node_interp: str = "linear"):
        from ._options import check_dial
        sig = np.broadcast_to(np.asarray(sigmas, dtype=np.float32).reshape(-1), (4,))
        if not (sig == sig[0]).all():
            raise ValueError(f"sigmas={sigmas!r}: the schedule scales ONE standard deviation for all four action components")
        self.anneal = check_dial(iters, beta_pass=beta_pass, beta_stage=beta_stage, temp=temp, sample_sigma=float(sig[0]),
                                 what="the env-batched annealed MPPI controller", nodes=nodes, node_interp=node_interp)
        super().__init__(env, n_envs, N, H, lam, sigmas=float(sig[0]), discount=discount, gamma_mean=gamma_mean, gamma_sigma=0.0,
                         a_mean_init=a_mean_init, device=device, compute_diag=compute_diag, compute_plan=compute_plan,
                         compute_fan=compute_fan, update=update, iters=iters, compute_post_cov=compute_post_cov, staged=True)
        if self.anneal is not None:
            self.core.attach_anneal(self.anneal)
        self.anneal_rows, self.anneal_sigma = self.core.anneal_rows, self.core.anneal_sigma

    def step(self, noisy_states, rng_acts):
        """One control step of every instance (= __call__) -> first actions [E, 4] (view of a_mean)."""
        return self(noisy_states, rng_acts)
