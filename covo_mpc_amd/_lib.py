"""ctypes binding of csrc/libcovo_hip.so (C ABI: include/covo_hip.h).

Fails loudly: a missing library is an ImportError-class failure at first use, never a silent
fallback to another backend.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("COVO_HIP_LIB") or os.path.join(_HERE, "csrc", "libcovo_hip.so")  # COVO_HIP_LIB: A/B builds
_lib = None

COVO_H = 32
COVO_DU = 4
COVO_NA = COVO_H * COVO_DU
COVO_STATE_FLOATS = 32
COVO_PARTIAL_FLOATS = 132
COVO_POS_STATS_DOUBLES = COVO_H * 6
COVO_RANK_RECORD_FLOATS = COVO_PARTIAL_FLOATS + 2 * COVO_POS_STATS_DOUBLES  # 516: {m, s, v[128], pad} + 192 fp64 position sums
COVO_COV_FLOATS = COVO_H * 10
COVO_RANK_RECORD_COV_FLOATS = COVO_PARTIAL_FLOATS + COVO_COV_FLOATS + 2 * COVO_POS_STATS_DOUBLES  # 836: with MPPI's second moments
COVO_EXCHANGE_HANDLE_BYTES = 128
ABI_VERSION = 10
COVO_DIAG_FLOATS = 8  # per-step sampling diagnostics of one instance (covo_set_step_diag)
DIAG_FIELDS = ("ess", "cost_min", "cost_weighted", "cost_mean", "weight_sum", "n_samples")
COVO_PLAN_FLOATS = 100   # the plan of a step: {cost_plan, 0, 0, 0, pos_plan[H][3]} (covo_set_step_plan)
COVO_TRACE_FLOATS = 168  # a trace row: true state[32], noisy state[32], u[4], the step's plan row (covo_set_episode_trace)
COVO_LAM_FLOATS = 4  # the ESS floor's solver row of one instance: lam_eff, 1 / lam_eff, ESS(lam0), evaluations (covo_set_step_ess_floor)
COVO_HAS_SAMPLE_FAN = 1
COVO_FAN_FLOATS = 100  # a fan row: {cost_s, bits(int32 n_s), 0, 0, pos_s[H][3]} (covo_set_step_fan): the layout of a plan row
COVO_FAN_MAX = 64      # rows of a fan: one 64-sample group of the rollout
COVO_HAS_UPDATE_ARBITER = 1
COVO_HAS_STEP_ITERS = 1
COVO_ARB_FLOATS = 8  # an arbiter row: {cost_softmax, cost_nominal, cost_best, cost_chosen, bits(int32 choice), bits(int32 n_best), 0, 0}
COVO_MAX_STEP_ITERS = 16  # iters= of the controllers: sample-rollout-update passes per control step (covo_hip.h: COVO_HAS_STEP_ITERS)
UPDATE_MASKS = {"softmax": 0, "best": 0b110, "guarded": 0b111}  # update= of the controllers -> the arbiter's candidate mask (0: detached)
LAM_FIELDS = ("lam_eff", "inv_lam_eff", "ess_lam0", "evaluations")
COVO_HAS_STEP_ANNEAL = 1  # the "dial" controller (covo_set_step_anneal, covo_cost_standardise): per-pass noise schedule, standardised weights
# the standardising solver's row: {lam_eff, 1 / lam_eff, std, bits(int32 |F| | fallback << 31)}, F the pass's finite costs
ANNEAL_FIELDS = ("lam_eff", "inv_lam_eff", "std", "n_finite")
ANNEAL_FALLBACK_BIT = 0x80000000
COVO_HAS_STEP_NODES = 1  # the annealed controllers' nodes=M (covo_set_step_nodes, covo_noise_nodes_philox): spline-node perturbations
# sigma_nodes=M of the covo-online controllers (covo_set_step_sigma_nodes, covo_sigma_nodes, covo_noise_factor_philox): Sigma in node space
COVO_HAS_SIGMA_NODES = 1
COVO_SIGMA_NODES_MAX = 16
COVO_SIGMA_NODES_FLOATS = 8  # the side row: {lam_min, lam_max, eig_max, eig_min of Sigma_M, log det Sigma_M, sweeps, flags, d}
SIGMA_NODES_FIELDS = ("lam_min", "lam_max", "eig_max", "eig_min", "log_det", "sweeps", "flags", "d")
SIGMA_NODES_NONFINITE, SIGMA_NODES_NO_CONVERGENCE, SIGMA_NODES_PIVOT = 1, 2, 4
COVO_HAS_ELITE_UPDATE = 1
COVO_ELITE_FLOATS = 8  # the elite-set update's selector row of one instance (covo_set_step_elite)
ELITE_FIELDS = ("threshold_cost_word", "threshold_index_word", "cost_min", "cost_kth", "K", "ties")  # words: uint32 bits
COVO_HAS_SIGMA_PERIOD = 1
COVO_MAX_SIGMA_PERIOD = 64  # sigma_period= of the covo-online controllers: every m-th step refreshes Sigma (covo_set_step_sigma_period)
COVO_HAS_POST_COV = 1
COVO_POST_AUX_FLOATS = 132  # the posterior covariance's side row of one instance: {shift d[128], W, 0, 0, 0} (covo_set_step_post_cov)
COVO_HAS_SIGMA_ADAPT = 1
COVO_SIGMA_ADAPT_FLOATS = 4  # Sigma adapt's row of one instance: {fallback, c, log det M, 0} (covo_set_step_sigma_adapt)
COVO_HAS_EPISODE_ROWS = 1
COVO_HAS_BATCHED_STAGED = 1  # staged= of the env-batched MPPI / covo-offline controllers (covo_set_step_batched_staged)
COVO_HAS_NEWTON_REFINE = 1  # refine= of the covo-online controllers (covo_set_step_refine, covo_newton_refine, covo_cost_gradient)
# a refine row: {cost_base, cost_chosen, bits(int32 choice), alpha, |g|_2, g.d, 0, bits(int32 flags)}; the candidates clip(b) and
# clip(b + 2^(3 - j) d), j = 1 .. 16
COVO_REFINE_FLOATS = 8
COVO_REFINE_CANDIDATES = 17
COVO_HAS_RICCATI_REFINE = 1  # riccati= of every sampling controller (covo_set_step_riccati, covo_riccati_refine, covo_riccati)
# a riccati row: a refine row whose last two words are {mu, bits(int32 flags | rung << 8)}; flags bit 0: g not finite, 1: d not finite,
# 3: no rung of the ladder mu_j = reg0 4^j, j < COVO_RICCATI_RUNGS, positive definite.  The sweep's side row: COVO_RICCATI_SIDE
# doubles {mu, rung, smallest pivot, flags}
COVO_RICCATI_FLOATS = 8
COVO_RICCATI_SIDE = 4
COVO_RICCATI_RUNGS = 8
COVO_RICCATI_REG0 = 1e-2
COVO_HAS_RICCATI_FEEDBACK = 1  # riccati_feedback= on top of riccati= (covo_set_step_riccati_feedback, covo_riccati_refine_feedback, covo_feedback_rollout)
# a feedback row: {cheapest of candidates 0 .. 16, cheapest valid closed-loop candidate (+inf: none), bits(int32 index of the former),
# bits(int32 index of the latter, 0: none), its max |K dx|_inf, bits(int32 its clipped count), bits(int32 mask of invalid ones), 0}; the
# candidates 17 .. 32 are the closed-loop sequences under the sweep's gains at the ladder's step sizes 2^(3 - j), j = 1 .. 16.  The
# generator's aux row: {max |K dx|_inf, bits(int32 clipped count), bits(int32 first k with a v that is not finite, -1: none), 0}
COVO_FEEDBACK_FLOATS = 8
COVO_FEEDBACK_CANDIDATES = 33
FEEDBACK_AUX_FLOATS = 4
FEEDBACK_MAX_ALPHAS = 64
FEEDBACK_LADDER = tuple(2.0 ** (3 - j) for j in range(1, 17))
COVO_HAS_PLAN_HOLD = 1  # plan_hold= on top of riccati= (covo_set_step_plan_hold, covo_plan_hold, covo_set_episode_hold_log)
# a hold row: {bits(int32 age j), alpha, max |v - v0| (the feedback term as it entered the action), bits(int32 clipped count),
# bits(int32 flags), |dx_pos|_2, bits(int32 the state's time word), 0}; flags bit 0: the sweep is flagged (its side row), 1: a v
# that is not finite, 2: the state's time is not the plan's + j.  A plan step's row: {0, 0, 0, 0, 0, 0, bits(time), 0}
COVO_HOLD_FLOATS = 8
COVO_MAX_PLAN_HOLD = 16  # plan_hold= of the controllers: every m-th control step plans, the others hold
HOLD_FIELDS = ("age", "alpha", "gain", "clipped", "flags", "dpos", "time")
HOLD_FLAG_SWEEP, HOLD_FLAG_NOT_FINITE, HOLD_FLAG_TIME = 1, 2, 4
COVO_HAS_ILQR = 1  # the "ilqr" controller (COVO_MODE_ILQR, covo_set_step_ilqr): Riccati sweeps and the line search, nothing sampled
# a summary row: {row_0.cost_base, row_{k-1}.cost_chosen, bits(int32 iterations with choice != 0), bits(int32 first j with choice 0; k:
# none), bits(int32 iterations with choice > 16), bits(OR of the rows' flag words), |g|_2 of the last iteration, 0}
COVO_ILQR_FLOATS = 8
COVO_HAS_CMA = 1  # the "cma" controller (COVO_MODE_CMA, covo_set_step_cma): a learned full covariance with step-size control
COVO_CMA_FLOATS = 8  # its row of one instance: {s, log s, |p|, |z|, mu_eff, c_sigma, d_sigma, flags}
# controllers.StateEstimator (covo_set_step_estimator, covo_estimate, covo_set_episode_estimator_log): an EKF between env step and control
# step.  Its side row: {bits(int32 flags), nis, |nu_pos|, |x - z|_pos, tr P_pos, tr P_vel, smallest pivot of S, bits(int32 time word)};
# flags 1: initialised, 2: re-initialised (time word), 4: a measured coordinate not finite, 8: the update failed
COVO_HAS_STATE_ESTIMATOR = 1
COVO_EST_FLOATS = 8
COVO_EST_STATE_DOUBLES = 16  # per instance: the estimate [13], then the force of the row last seen [3]
COVO_EST_META_INTS = 2       # {valid, the time word of the row last seen}
COVO_EST_LOG_FLOATS = 34     # a row of the episode log: measured [13], written [13], the side row [8]
# controllers.ForceObserver (covo_set_step_force_observer, covo_observe_force, covo_set_episode_force_observer_log): a 16-state EKF that
# estimates the disturbance force from the kinematic measurements and writes floats 0 .. 15 of the row.  Its side row: {bits(int32
# flags), nis, |nu_pos|, |f^|, tr P_pos, tr P_force, smallest pivot of S, bits(int32 time word)}; the flags are the state estimator's
COVO_HAS_FORCE_OBSERVER = 1
COVO_OBS_FLOATS = 8
COVO_OBS_STATE_DOUBLES = 16  # per instance: x [13], then the force estimate [3]
COVO_OBS_META_INTS = 2       # {valid, the time word of the row last seen}
COVO_OBS_LOG_FLOATS = 40     # a row of the episode log: measured [16] (slots 13 .. 15: the true force), written [16], the side row [8]
ILQR_FIELDS = ("cost_first", "cost", "moved", "fixed_at", "closed", "flags", "grad_norm")
# riccati_box= on top of riccati= (covo_set_step_riccati_box, covo_riccati_box, covo_riccati_refine_box): the sweep's stages solve the
# box QP on -1 <= clip(b) + du <= 1.  A mask word per stage: bits 0-3 coordinate i clamped at the lower bound, bits 4-7 at the upper
COVO_HAS_RICCATI_BOX = 1
# the episode logs of the attachments' rows (covo_set_episode_rows): the kinds, and the Sigma log's row {age, fallback, c, log det M}
COVO_EPLOG_LAM, COVO_EPLOG_ELITE, COVO_EPLOG_ITERS, COVO_EPLOG_SIGMA, COVO_EPLOG_POST_AUX, COVO_EPLOG_POST_COV = range(6)
COVO_EPLOG_KINDS = 6
COVO_SIGMA_LOG_FLOATS = 4
SIGMA_LOG_FIELDS = ("age", "fallback", "scale", "logdet")
COVO_POST_COV_FLOATS = COVO_NA * COVO_NA  # a row of the posterior covariance log: the matrix [128][128]
COVO_FLAG_ACTIONS_CLIPPED = 1


class CovoError(RuntimeError):
    pass


class EnvParamsC(C.Structure):
    """struct covo_env_params (include/covo_hip.h)."""
    _fields_ = [
        ("max_thrust", C.c_float), ("max_torque", C.c_float * 3), ("max_omega", C.c_float * 3),
        ("dt", C.c_float), ("g", C.c_float), ("m", C.c_float), ("action_scale", C.c_float),
        ("alpha_bodyrate", C.c_float), ("max_steps_in_episode", C.c_int32), ("pos_limit", C.c_float),
        ("rollover_terminate", C.c_int32), ("reward_kind", C.c_int32), ("disturb_kind", C.c_int32),
        ("disturb_period", C.c_int32), ("disturb_scale", C.c_float), ("disturb_params", C.c_float * 6),
        ("dyn_noise_scale", C.c_float),
        ("reset_traj", C.c_int32), ("reserved0", C.c_int32), ("reset_dt", C.c_double), ("reset_disturb_scale", C.c_double),
    ]


class ConfigC(C.Structure):
    """struct covo_config (include/covo_hip.h)."""
    _fields_ = [("n_local", C.c_int32), ("H", C.c_int32), ("du", C.c_int32), ("lam", C.c_float),
                ("discount", C.c_float), ("flags", C.c_int32)]


_P = C.c_void_p


class StepArgsC(C.Structure):
    """struct covo_step_args (include/covo_hip.h)."""
    _fields_ = [("mode", C.c_int32), ("n_samples", C.c_int32), ("T", C.c_int32), ("n_table", C.c_int32),
                ("state", _P), ("pos_traj", _P), ("vel_traj", _P), ("a_mean", _P), ("a_mean_shift", _P), ("a_cov", _P),
                ("L_table", _P), ("a", _P), ("cost", _P), ("groupmin", _P), ("pos_stats", _P), ("partial_out", _P),
                ("sample_offset", C.c_int64), ("gamma_mean", C.c_float), ("sample_sigma", C.c_float),
                ("derive_keys", C.c_int32), ("rollout_deterministic", C.c_int32), ("gamma_sigma", C.c_float),
                ("pad_", C.c_int32), ("a_mean_in", _P)]


class BatchArgsC(C.Structure):
    """struct covo_batch_args (include/covo_hip.h)."""
    _fields_ = [("n_envs", C.c_int32), ("n_samples", C.c_int32), ("T", C.c_int32), ("pad_", C.c_int32),
                ("states", _P), ("pos_traj", _P), ("vel_traj", _P), ("a_mean", _P), ("a_cov", _P), ("a", _P), ("cost", _P),
                ("groupmin", _P), ("gamma_mean", C.c_float), ("sample_sigma", C.c_float)]


class BatchModeArgsC(C.Structure):
    """struct covo_batch_mode_args (include/covo_hip.h): the batched step with a mode, for the *_mode entry points."""
    _fields_ = [("base", BatchArgsC), ("mode", C.c_int32), ("n_table", C.c_int32), ("L_table", _P),
                ("L_table_stride", C.c_int64), ("gamma_sigma", C.c_float), ("pad_", C.c_int32)]


REWARD_KINDS = {"penyaw": 0, "realworld": 1}                 # COVO_REWARD_*
DISTURB_KINDS = {"none": 0, "gaussian": 1, "periodic": 2, "sin": 3, "drag": 4, "mixed": 5}  # COVO_DISTURB_*
TRAJ_KINDS = {None: 0, "hovering": 1, "tracking": 2, "tracking_slow": 3, "tracking_zigzag": 4}  # COVO_TRAJ_* by Quad3D task
STATE_DISTURB_KINDS = (4, 5)                                  # drag / mixed: the force is a state (16-state plants)
TABLE_DISTURB_KINDS = (2, 3, 4, 5)                            # models that need covo_disturb_table's per-step table
DISTURB_KEYS_SHARED, DISTURB_KEYS_HESSIAN, DISTURB_KEYS_NOMINAL = 0, 1, 2
COVO_MAX_ENVS = 64
MODE_MPPI, MODE_COVO_ONLINE, MODE_COVO_OFFLINE = 0, 1, 2
MODE_ILQR = 3
MODE_CMA = 5  # the "cma" controller (COVO_MODE_CMA; 4 stays an invalid mode)
COVO_FLAG_NO_GRAPH = 2
COVO_FLAG_SHARED_DEVICE = 4
COVO_FLAG_PROPAGATE_NAN = 8
COVO_E_DEVICE = -4
COVO_DEVSTAT_GRID_BARRIER = 1
COVO_DEVSTAT_EXCHANGE = 2
COVO_DEVSTAT_ADJOINT = 4
_SIGS = {
    "covo_last_error": (C.c_char_p, []),
    "covo_abi_version": (C.c_int, []),
    "covo_create": (C.c_int, [C.POINTER(ConfigC), C.POINTER(_P)]),
    "covo_destroy": (C.c_int, [_P]),
    "covo_device_status": (C.c_int, [_P, C.c_int32]),
    "covo_debug_raise_device_status": (C.c_int, [_P, C.c_int32, _P]),
    "covo_randn": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
    "covo_randn_jax": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _P, _P]),
    "covo_noise_gemm": (C.c_int, [_P, _P, _P, _P, C.c_int32, _P, _P]),
    "covo_noise_blockdiag": (C.c_int, [_P, _P, _P, _P, C.c_int32, _P, _P]),
    "covo_noise_gemm_philox": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_int64, C.c_int32, _P, _P]),
    "covo_noise_blockdiag_philox": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_int64, C.c_int32, _P, _P]),
    "covo_rollout_cost": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), C.POINTER(C.c_float), _P, _P,
                                    C.c_int32, _P, _P, _P, _P]),
    "covo_disturb_table": (C.c_int, [_P, C.POINTER(EnvParamsC), _P, C.c_int32, _P, C.c_uint32, C.c_uint32, C.c_int32,
                                     C.c_int32, _P, _P]),
    "covo_pos_info": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P]),
    "covo_debug_time_rollout": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), C.POINTER(C.c_float), _P, _P,
                                          C.c_int32, _P, _P, C.c_int32, C.c_int32, C.POINTER(C.c_float), _P]),
    "covo_softmax_reduce": (C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P]),
    "covo_softmax_update": (C.c_int, [_P, _P, _P, C.c_int32, _P, _P, C.c_float, _P, _P]),
    "covo_softmax_update_cov": (C.c_int, [_P, _P, _P, C.c_int32, _P, _P, C.c_float, _P, C.c_float, _P, _P, _P]),
    "covo_merge": (C.c_int, [_P, _P, C.c_int32, _P, C.c_float, _P, _P]),
    "covo_merge_ranks": (C.c_int, [_P, _P, C.c_int32, _P, C.c_float, _P, _P, _P]),
    "covo_merge_ranks_wide": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_float, _P, _P, _P]),
    "covo_exchange_create": (C.c_int, [_P, C.c_int32, C.c_int32, _P]),
    "covo_exchange_connect": (C.c_int, [_P, _P]),
    "covo_exchange_set_timeout": (C.c_int, [_P, C.c_double]),
    "covo_device_bus_id": (C.c_int, [C.c_int32, C.c_char_p, C.c_int32]),
    "covo_exchange_records": (C.c_int, [_P, _P, _P, _P]),
    "covo_exchange_records_cov": (C.c_int, [_P, _P, _P, _P]),
    "covo_softmax_reduce_cov": (C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, _P]),
    "covo_merge_ranks_cov": (C.c_int, [_P, _P, C.c_int32, _P, C.c_float, _P, C.c_float, _P, _P, _P, _P]),
    "covo_shift_mean": (C.c_int, [_P, _P, _P, _P]),
    "covo_hessian": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), _P, _P, C.c_int32, _P, _P]),
    "covo_hessian_pairs": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), _P, _P, C.c_int32, _P, _P]),
    "covo_sigma": (C.c_int, [_P, _P, C.c_int32, C.c_float, _P, _P, _P]),
    "covo_debug_sigma_workspace": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P]),
    "covo_debug_hess_workspace": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P]),
    "covo_debug_batched_hessians": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P]),
    "covo_env_step": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), _P, C.POINTER(C.c_uint32),
                                C.c_int32, C.c_float, _P, C.c_int32, _P]),
    "covo_pid_nominal": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), C.POINTER(EnvParamsC), C.c_float,
                                   C.c_float, C.c_float, C.c_uint32, C.c_uint32, C.c_int32, _P, _P, _P, _P]),
    "covo_run_episode": (C.c_int, [_P, C.POINTER(EnvParamsC), C.POINTER(StepArgsC), _P, _P, C.c_int32,
                                   C.c_float, _P, C.POINTER(C.c_uint32), C.c_int32, _P]),
    "covo_mpc_step_batched": (C.c_int, [_P, C.POINTER(BatchArgsC), C.POINTER(EnvParamsC), C.POINTER(C.c_uint32), _P]),
    "covo_env_step_batched": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), _P,
                                        C.POINTER(C.c_uint32), C.c_int32, C.c_float, _P, C.c_int32, C.c_int32, _P]),
    "covo_run_episode_batched": (C.c_int, [_P, C.POINTER(BatchArgsC), C.POINTER(EnvParamsC), _P, _P, C.c_int32, C.c_float, _P,
                                           C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.c_int32, _P]),
    "covo_mpc_step_batched_mode": (C.c_int, [_P, C.POINTER(BatchModeArgsC), C.POINTER(EnvParamsC), C.POINTER(C.c_uint32), _P]),
    "covo_run_episode_batched_mode": (C.c_int, [_P, C.POINTER(BatchModeArgsC), C.POINTER(EnvParamsC), _P, _P, C.c_int32, C.c_float,
                                                _P, C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.c_int32, _P]),
    "covo_debug_set_ns_deflate": (C.c_int, [_P, C.c_int]),             # per-handle experiment switches (covo_hip.h)
    "covo_debug_set_fuse_small": (C.c_int, [_P, C.c_int]),
    "covo_debug_set_fold_begin": (C.c_int, [_P, C.c_int]),
    "covo_debug_set_stream_gemm": (C.c_int, [_P, C.c_int]),
    "covo_debug_set_ns_coherence": (C.c_int, [_P, C.c_int]),
    "covo_debug_set_ns_merged": (C.c_int, [_P, C.c_int]),
    "covo_set_step_diag": (C.c_int, [_P, _P, C.c_int32]),             # per-step sampling diagnostics (covo_hip.h)
    "covo_set_episode_diag_log": (C.c_int, [_P, _P, C.c_int32]),
    "covo_set_step_batched_staged": (C.c_int, [_P, C.c_int32]),  # the staged batched step (covo_hip.h: COVO_HAS_BATCHED_STAGED)
    "covo_set_step_ess_floor": (C.c_int, [_P, C.c_float, _P, C.c_int32]),  # the ESS floor (covo_hip.h: COVO_HAS_ESS_FLOOR)
    "covo_ess_lambda": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P]),
    # the annealed step (covo_hip.h: COVO_HAS_STEP_ANNEAL)
    "covo_set_step_anneal": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int32, C.c_float, _P, C.c_int32]),
    "covo_cost_standardise": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P]),
    # the spline nodes of the annealed step (covo_hip.h: COVO_HAS_STEP_NODES)
    "covo_set_step_nodes": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int32, C.c_int32]),
    "covo_step_nodes": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "covo_noise_nodes_philox": (C.c_int, [_P, _P, C.c_int32, _P, C.c_uint32, C.c_uint32, C.c_int64, C.c_int32, _P, _P]),
    # Sigma in node space (covo_hip.h: COVO_HAS_SIGMA_NODES)
    "covo_set_step_sigma_nodes": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int32, _P, C.c_int32]),
    "covo_step_sigma_nodes": (C.c_int, [_P, C.POINTER(C.c_int32), _P, _P, C.c_int32, _P]),
    "covo_sigma_nodes": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_float, _P, _P, _P, _P, _P]),
    "covo_noise_factor_philox": (C.c_int, [_P, _P, C.c_int32, _P, C.c_uint32, C.c_uint32, C.c_int64, C.c_int32, _P, _P]),
    "covo_set_step_elite": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),  # the elite-set update (covo_hip.h: COVO_HAS_ELITE_UPDATE)
    "covo_elite_select": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "covo_set_step_sigma_period": (C.c_int, [_P, C.c_int32]),  # the Sigma period (covo_hip.h: COVO_HAS_SIGMA_PERIOD)
    "covo_step_sigma_age": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "covo_sigma_shift": (C.c_int, [_P, _P, C.c_int32, C.c_float, _P, _P, _P]),
    "covo_debug_sigma_factor": (C.c_int, [_P, C.c_int32, _P, C.c_int64, _P]),
    "covo_set_step_post_cov": (C.c_int, [_P, _P, _P, C.c_int32]),  # the posterior covariance (covo_hip.h: COVO_HAS_POST_COV)
    "covo_weighted_cov": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, _P, _P]),
    "covo_set_step_sigma_adapt": (C.c_int, [_P, C.c_float, _P, C.c_int32]),  # Sigma adapt (covo_hip.h: COVO_HAS_SIGMA_ADAPT)
    "covo_sigma_adapt": (C.c_int, [_P, _P, _P, C.c_int32, C.c_float, C.c_float, _P, _P, _P, _P]),
    "covo_set_episode_rows": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),  # the attachments' episode logs (covo_hip.h: COVO_HAS_EPISODE_ROWS)
    "covo_set_step_plan": (C.c_int, [_P, _P, C.c_int32]),             # the flight recorder (covo_hip.h: COVO_HAS_PLAN_TRACE)
    "covo_set_episode_trace": (C.c_int, [_P, _P, C.c_int32]),
    "covo_rollout_fan": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), C.POINTER(C.c_float), _P, _P,
                                   C.c_int32, _P, C.c_int32, _P, _P]),  # the sample fan (covo_hip.h: COVO_HAS_SAMPLE_FAN)
    "covo_set_step_fan": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32]),
    "covo_set_episode_fan": (C.c_int, [_P, _P, C.c_int32]),
    "covo_set_step_arbiter": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),  # the update arbiter (covo_hip.h: COVO_HAS_UPDATE_ARBITER)
    "covo_set_episode_arbiter_log": (C.c_int, [_P, _P, C.c_int32]),
    "covo_set_step_iters": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),  # iterations per control step (covo_hip.h: COVO_HAS_STEP_ITERS)
    "covo_arbitrate": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), C.POINTER(C.c_float), _P, _P, _P, C.c_int32,
                                 _P, _P, C.c_int32, _P, _P]),
    # the Newton refinement (covo_hip.h: COVO_HAS_NEWTON_REFINE)
    "covo_cost_gradient": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), _P, _P, C.c_int32, _P, _P]),
    "covo_newton_refine": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), C.POINTER(C.c_float), _P, _P, _P, _P, _P, _P,
                                     C.c_int32, _P, _P, _P]),
    "covo_set_step_refine": (C.c_int, [_P, _P, C.c_int32]),
    # the Riccati refinement (covo_hip.h: COVO_HAS_RICCATI_REFINE)
    "covo_riccati": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), _P, _P, C.c_int32, C.c_double, _P, _P, _P, _P, _P, _P]),
    "covo_riccati_refine": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), C.POINTER(C.c_float), _P, _P, _P, C.c_double,
                                      C.c_int32, _P, _P, _P]),
    "covo_set_step_riccati": (C.c_int, [_P, _P, C.c_int32]),
    # Riccati feedback (covo_hip.h: COVO_HAS_RICCATI_FEEDBACK)
    "covo_feedback_rollout": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), C.POINTER(C.c_float), _P, _P, _P, _P, _P,
                                        C.POINTER(C.c_double), C.c_int32, C.c_int32, _P, _P, _P]),
    "covo_riccati_refine_feedback": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), C.POINTER(C.c_float), _P, _P, _P,
                                               C.c_double, C.c_int32, _P, _P, _P, _P]),
    "covo_set_step_riccati_feedback": (C.c_int, [_P, _P, C.c_int32]),
    "covo_debug_feedback_gain": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_double]),
    # the plan hold (covo_hip.h: COVO_HAS_PLAN_HOLD)
    "covo_set_step_plan_hold": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "covo_step_plan_age": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "covo_plan_hold": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, _P]),
    "covo_set_episode_hold_log": (C.c_int, [_P, _P, C.c_int32]),
    "covo_debug_plan_latch": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    # the iLQR controller's per-iteration logs (covo_hip.h: COVO_HAS_ILQR)
    "covo_set_step_ilqr": (C.c_int, [_P, _P, _P, _P, C.c_int32]),
    # the CMA controller (covo_hip.h: COVO_HAS_CMA)
    "covo_set_step_cma": (C.c_int, [_P, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_float, _P, _P, C.c_int32]),
    "covo_cma_reset": (C.c_int, [_P]),
    "covo_cma_path": (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                C.c_float, _P, _P, _P, _P, _P, _P]),
    "covo_debug_ilqr_costs": (C.c_int, [_P, _P, C.c_int32]),
    # the state estimator (covo_hip.h: COVO_HAS_STATE_ESTIMATOR)
    "covo_set_step_estimator": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, _P, _P, _P, _P, C.c_int32]),
    "covo_estimator_reset": (C.c_int, [_P]),
    "covo_estimate": (C.c_int, [_P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, _P,
                                _P, _P, _P, C.c_int32, C.c_int32, _P]),
    "covo_set_episode_estimator_log": (C.c_int, [_P, _P, C.c_int32]),
    # the force observer (covo_hip.h: COVO_HAS_FORCE_OBSERVER)
    "covo_set_step_force_observer": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double, _P, _P, _P, _P,
                                               C.c_int32]),
    "covo_force_observer_reset": (C.c_int, [_P]),
    "covo_observe_force": (C.c_int, [_P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                                     C.c_double, _P, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    "covo_set_episode_force_observer_log": (C.c_int, [_P, _P, C.c_int32]),
    # the Riccati box (covo_hip.h: COVO_HAS_RICCATI_BOX)
    "covo_riccati_box": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), _P, _P, C.c_int32, C.c_double, _P, _P, _P, _P, _P, _P,
                                   _P]),
    "covo_riccati_refine_box": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(EnvParamsC), C.POINTER(C.c_float), _P, _P, _P, C.c_double,
                                          C.c_int32, _P, _P, _P, C.c_int32, _P, _P]),
    "covo_set_step_riccati_box": (C.c_int, [_P, _P, C.c_int32]),
    "covo_set_step_ilqr_box": (C.c_int, [_P, _P, C.c_int32]),
    "covo_debug_time_step": (C.c_int, [_P, C.POINTER(EnvParamsC), C.POINTER(StepArgsC), C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.POINTER(C.c_float), _P]),
    "covo_debug_time_batched": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_float), _P]),
    "covo_sigma_jacobi": (C.c_int, [_P, _P, C.c_int32, C.c_float, _P, _P, _P]),
    "covo_sigma_profile": (C.c_int, [_P, _P, C.c_float, _P, _P, _P, _P]),
    "covo_mpc_step": (C.c_int, [_P, C.POINTER(EnvParamsC), C.POINTER(StepArgsC), C.c_uint32, C.c_uint32,
                                C.POINTER(C.c_float), _P]),
    "covo_cholesky": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
}
EXPORTS = tuple(_SIGS)


def lib_path() -> str:
    return _SO


def load_library():
    """Load libcovo_hip.so and declare every prototype of include/covo_hip.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise CovoError(
            f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C covo_mpc_amd/csrc`).  covo_mpc_amd has no CPU/torch fallback.")
    # torch bundles its own ROCm runtime (libamdhip64): load it FIRST so this library binds to the
    # runtime instance that owns torch's device context and streams (two runtimes in one process do
    # not see each other's devices).
    import torch  # noqa: F401
    lib = C.CDLL(_SO)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError = ABI mismatch, surfaced as is
        fn.restype = res
        fn.argtypes = args
    if lib.covo_abi_version() != ABI_VERSION:
        raise CovoError(f"libcovo_hip.so ABI {lib.covo_abi_version()} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load_library().covo_last_error()
        raise CovoError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


def check_fan(compute_fan, N) -> int:
    """compute_fan= of the controllers -> the fan size K (0: off): None / False / 0 given as the default mean off; anything else
    must be an integer in [1, COVO_FAN_MAX] and <= N."""
    if compute_fan is None or compute_fan is False:
        return 0
    K = int(compute_fan)
    if isinstance(compute_fan, bool) or K != compute_fan or not 1 <= K <= COVO_FAN_MAX:
        raise ValueError(f"compute_fan={compute_fan!r} outside [1, {COVO_FAN_MAX}] (the fan size K; None = off)")
    if K > int(N):
        raise ValueError(f"compute_fan={K} > N={N}: the fan takes K of the step's N samples")
    return K


def check_update(update) -> int:
    """update= of the controllers -> the arbiter's candidate mask (0: "softmax", nothing attached); anything but "softmax" / "best" /
    "guarded" raises ValueError."""
    if not isinstance(update, str) or update not in UPDATE_MASKS:
        raise ValueError(f"update={update!r} (softmax | best | guarded)")
    return UPDATE_MASKS[update]


def check_iters(iters) -> int:
    """iters= of the controllers -> the number of sample-rollout-update passes per control step: an integer in
    [1, COVO_MAX_STEP_ITERS] (1, the default: today's step); anything else raises ValueError."""
    import numbers
    if isinstance(iters, bool) or not isinstance(iters, numbers.Integral) or not 1 <= int(iters) <= COVO_MAX_STEP_ITERS:
        raise ValueError(f"iters={iters!r} outside [1, {COVO_MAX_STEP_ITERS}] (an integer number of passes per control step; 1 = off)")
    return int(iters)


def check_elite(elite, N, ess_min=None, gamma_sigma=None) -> int:
    """elite= of the controllers -> the elite count K (0: off): None / False / 0 mean off; anything else must be an integer in [1, N].
    With ess_min set as well: ValueError (both define the update's weights).  gamma_sigma (MPPI): a full refit, gamma_sigma >= 1,
    from K < 5 samples raises ValueError -- a 4 x 4 block refitted from K samples about their own mean has rank <= K - 1."""
    import numbers
    if elite is None or elite is False or (isinstance(elite, numbers.Integral) and not isinstance(elite, bool) and int(elite) == 0):
        return 0
    if isinstance(elite, bool) or not isinstance(elite, numbers.Integral) or not 1 <= int(elite) <= int(N):
        raise ValueError(f"elite={elite!r} outside [1, N={N}] (an integer number of elite samples; None = off)")
    K = int(elite)
    if ess_min is not None and float(ess_min) != 0.0:
        raise ValueError(f"elite={K} together with ess_min={ess_min}: both define the update's weights; give one of them")
    if gamma_sigma is not None and float(gamma_sigma) >= 1.0 and K < 5:
        raise ValueError(f"elite={K} with gamma_sigma={gamma_sigma}: a 4 x 4 covariance block refitted from K < 5 samples about their "
                         "own mean is singular (rank <= K - 1); take K >= 5 or gamma_sigma < 1")
    return K


def check_sigma_period(sigma_period, mode="online") -> int:
    """sigma_period= of the controllers -> the period m: an integer in [1, COVO_MAX_SIGMA_PERIOD] (1, the default: every step computes
    its own Sigma); anything else raises ValueError.  mode: what the controller is ("online", "offline", "mppi", ...): m > 1 with
    anything but covo-online raises ValueError -- only covo-online decides a Sigma per step."""
    import numbers
    if (isinstance(sigma_period, bool) or not isinstance(sigma_period, numbers.Integral) or
            not 1 <= int(sigma_period) <= COVO_MAX_SIGMA_PERIOD):
        raise ValueError(f"sigma_period={sigma_period!r} outside [1, {COVO_MAX_SIGMA_PERIOD}] (an integer number of control steps per "
                         "Sigma refresh; 1 = off)")
    m = int(sigma_period)
    if m > 1 and mode != "online":
        raise ValueError(f"sigma_period={m} with {mode}: the Sigma period belongs to covo-online, the one mode that computes a Sigma per "
                         "step (CoVOController(mode=\"online\"), BatchedCoVOController(mode=\"online\")); give sigma_period=1")
    return m


def check_sigma_adapt(sigma_adapt, sigma_period=None, mode="online") -> float:
    """sigma_adapt= of the controllers -> gamma, the weight of the posterior covariance in a reuse step's Sigma': a real number in
    [0, 1) (0.0, the default: off); anything else raises ValueError.  gamma > 0 with a mode other than "online" raises ValueError --
    only covo-online has reuse steps -- and so does gamma > 0 with sigma_period == 1 (given): every step refreshes, nothing would
    ever adapt."""
    import math
    import numbers
    if (isinstance(sigma_adapt, bool) or not isinstance(sigma_adapt, numbers.Real) or math.isnan(float(sigma_adapt)) or
            not 0.0 <= float(sigma_adapt) < 1.0):
        raise ValueError(f"sigma_adapt={sigma_adapt!r} outside [0, 1) (the weight gamma of the posterior covariance in a reuse step's "
                         "Sigma', a real number; 0 = off)")
    g = float(sigma_adapt)
    if g > 0.0 and mode != "online":
        raise ValueError(f"sigma_adapt={g} with {mode}: Sigma adapt belongs to the reuse steps of covo-online "
                         "(CoVOController(mode=\"online\"), BatchedCoVOController(mode=\"online\")); give sigma_adapt=0")
    if g > 0.0 and sigma_period is not None and int(sigma_period) == 1:
        raise ValueError(f"sigma_adapt={g} with sigma_period=1: every step refreshes Sigma and nothing would ever adapt; give "
                         "sigma_period > 1 or sigma_adapt=0")
    return g


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
