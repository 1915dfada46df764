"""Quadrotor environment plumbing + experiment drivers: quadjax/envs/quadrotor.py.

Host-side (numpy fp32) mirror of `Quad3D` (quadrotor.py:23-503) -- same constructor, attributes,
`step_env` / `raw_step` / `reset_env` / `get_info` / `get_obs*` / `is_terminal` -- plus
`get_controller` (:670-752), `eval_env` (:506-591), `Args` (:755-766) and `main` (:769-803).
No kernels live here: one state per control step is serial scalar math; the
N x H rollouts the controllers need run in csrc/rollout.hip.  The controllers receive
`info["noisy_state"]` exactly like the reference's (covo.py:198).
"""
from __future__ import annotations

import argparse
import os
import pickle
import time as time_module
from dataclasses import dataclass as pydataclass
from functools import partial

import numpy as np

from .. import controllers
from .. import random as crandom
from ..controllers._options import (STEP_OPTION_DEFAULTS, STEP_SWITCH_DEFAULTS, check_dial, check_ilqr, check_step_options, check_step_switches,
                                    take, take_switches)
from ..dynamics import utils
from ..dynamics.dataclass import Action3D, DeviceState, EnvParams3D, EnvState3D
from ..dynamics.free import get_quadrotor_1st_order_dyn
from .base import BaseEnvironment

f32 = np.float32


class Quad3D(BaseEnvironment):
    def __init__(self, task: str = "tracking", obs_type: str = "quad", enable_randomizer: bool = True,
                 lower_controller: str = "base", disturb_type: str = "periodic",
                 disable_rollover_terminate: bool = False, generate_noisy_state: bool = False, device=None):
        super().__init__()
        self.task = task
        self.disable_rollover_terminate = disable_rollover_terminate
        self.generate_noisy_state = generate_noisy_state
        self.disturb_type = disturb_type
        self.device = device
        dp = self.default_params
        gens = {  # quadrotor.py:49-84
            "tracking": (utils.generate_lissa_traj, utils.tracking_penyaw_reward_fn),
            "tracking_slow": (utils.generate_lissa_traj_slow, utils.tracking_realworld_reward_fn),
            "tracking_zigzag": (utils.generate_zigzag_traj, utils.tracking_penyaw_reward_fn),
            "hovering": (utils.generate_fixed_traj, utils.tracking_penyaw_reward_fn),
        }
        if task not in gens:
            raise NotImplementedError(task)
        gen, self.reward_fn = gens[task]
        self.generate_traj = partial(gen, dp.max_steps_in_episode, dp.dt)
        self.get_init_state = self.get_zero_state
        self.step_fn, self.dynamics_fn = get_quadrotor_1st_order_dyn(disturb_type=disturb_type)  # :87-89
        self.get_err_pos = lambda state: np.linalg.norm(state.pos_tar - state.pos)
        self.get_err_vel = lambda state: np.linalg.norm(state.vel_tar - state.vel)
        if lower_controller != "base":  # the L1 lower controllers live on the reference's `rl` branch only
            raise NotImplementedError(lower_controller)
        self.default_control_params = 0.0
        self.control_fn = lambda obs, state, env_params, rng_act, input_action: (input_action, None, state)
        self.sim_dt = dp.dt
        self.substeps = 1
        self.enable_randomizer = enable_randomizer
        if enable_randomizer and "params" not in obs_type:
            print("Warning: enable domain randomziation without params in obs_type")
        if obs_type == "quad_params":
            self.get_obs = self.get_obs_quad_params
            self.obs_dim = 39 + dp.traj_obs_len * 6
        elif obs_type == "quad":
            self.get_obs = self.get_obs_quadonly
            self.obs_dim = 19 + dp.traj_obs_len * 6
        else:
            raise NotImplementedError(obs_type)
        self.equib = np.array([0.0] * 6 + [1.0] + [0.0] * 9, dtype=f32)
        self.action_dim = 4
        self.adapt_obs_dim = 22 * dp.adapt_horizon
        self.param_obs_dim = 20

    @property
    def default_params(self) -> EnvParams3D:
        return EnvParams3D()

    # ---- domain randomisation (quadrotor.py:132-171) ------------------------------------------------
    def sample_params(self, key) -> EnvParams3D:
        p = self.default_params
        if self.enable_randomizer:
            param_key = crandom.split(key)[0]
            r = crandom.uniform(param_key, (17,), -1.0, 1.0)
            I_diag = p.I_diag_mean + r[1:4] * p.I_diag_std
            return EnvParams3D(m=float(p.m_mean + r[0] * p.m_std), I=np.diag(I_diag).astype(f32),
                               action_scale=float(p.action_scale_mean + r[4] * p.action_scale_std),
                               alpha_bodyrate=float(p.alpha_bodyrate_mean + r[5] * p.alpha_bodyrate_std),
                               disturb_params=(r[6:12] * p.disturb_scale).astype(f32))
        return EnvParams3D(disturb_params=crandom.uniform(key, (6,), -1.0, 1.0))

    # ---- key methods ----------------------------------------------------------------------------------
    def step_env(self, key, state: EnvState3D, action, params: EnvParams3D, deterministic: bool = False,
                 need_info: bool = True):
        """quadrotor.py:215-248: reward/done of the PRE-step state, one raw_step."""
        action = np.clip(np.asarray(action, dtype=f32), -1.0, 1.0)
        params = params.replace(dyn_noise_scale=params.dyn_noise_scale * (1.0 - float(deterministic)))  # :234-235
        sub_action, _, state = self.control_fn(None, state, params, key, action)
        next_state = self.raw_step(key, state, sub_action, params)
        reward = self.reward_fn(state, params)
        done = bool(self.is_terminal(state, params))
        if not need_info:
            return None, next_state, reward, done, None
        info_key, key = crandom.split(key)
        info = self.get_info(info_key, state, next_state, params)
        return self.get_obs(next_state, params), next_state, reward, done, info

    def raw_step(self, key, state, sub_action, params):
        """quadrotor.py:250-263."""
        sub_action = np.clip(np.asarray(sub_action, dtype=f32), -1.0, 1.0)
        thrust = (sub_action[0] + f32(1.0)) / f32(2.0) * f32(params.max_thrust)
        torque = sub_action[1:] * params.max_torque
        key, step_key = crandom.split(key)
        return self.step_fn(params, state, Action3D(thrust=thrust, torque=torque.astype(f32)), step_key, self.sim_dt)

    def rollout_disturbance(self, step_key, params, deterministic: bool, rng=crandom):
        """The single f_disturb vector every sample/step of a controller rollout receives under 'none' / 'gaussian': all
        N x H step_env calls share `step_key` (covo.py:225,231 / mppi.py:69,74), so free.py:147's draw is one vector.  Key
        derivation follows step_env -> raw_step -> step_fn (quadrotor.py:262, free.py:136,144); `rng`: the key module
        (covo_mpc_amd.random, or random_jax for jax's own bitstream).  The other models (periodic / sin / drag / mixed) are
        per-step or per-sample: csrc/disturb.hip builds their table on the device (SamplingCore.disturb_table)."""
        if self.disturb_type == "none":
            return np.zeros(3, dtype=f32)
        if self.disturb_type == "gaussian":
            scale = params.dyn_noise_scale * (1.0 - float(deterministic))
            _, k = rng.split(step_key)      # raw_step: key, step_key = split(key)
            k, _ = rng.split(k)             # step_fn:  key, key_dyn = split(key)
            disturb_key, _ = rng.split(k)   #           disturb_key, key = split(key)
            return (f32(scale) * np.asarray(rng.normal(disturb_key, (3,)), dtype=f32)).astype(f32)
        raise NotImplementedError(f"disturb_type={self.disturb_type!r}: no single shared vector (use SamplingCore.disturb_table)")

    def rollout_disturbance_table(self, key, params, time: int, f_disturb0, key_mode: int, deterministic: bool, rng=crandom,
                                  H: int = 32):
        """Host restatement of csrc/disturb.hip: the per-step disturbance table of a controller rollout, float32 [H][4] with
        row k = {g_k[3], c_k}, f_k = c_drag drag(vel_{k-1}) + c_k f_{k-1} + g_k for k >= 1 (row 0 unused: step 0 integrates the
        state's own f_disturb).  `rng`: the key module -- covo_mpc_amd.random (then the rows are the device kernel's), or
        random_jax for jax's own bitstream (noise_stream = "jax": keys split and uniforms / normals drawn as jax.random does).
        key_mode (covo_mpc_amd._lib.DISTURB_KEYS_*): who calls step_env with which key -- SHARED: every step the same `key`
        (covo.py:225,231; mppi.py:69,74); HESSIAN: rng_k, key = split(key) per step (covo.py:150-153); NOMINAL: _, key = split(key);
        rng_step, key = split(key) (covo.py:58-70)."""
        from .. import _lib
        kind = self.disturb_type
        tab = np.zeros((H, 4), dtype=f32)
        dp = np.asarray(params.disturb_params, dtype=f32)
        period = int(params.disturb_period) if int(params.disturb_period) > 0 else 1
        scale = f32(params.disturb_scale)
        held = np.asarray(f_disturb0, dtype=f32).copy()
        key = np.asarray(key)

        def disturb_key(k):  # raw_step: key, step_key = split(k); step_fn: key, key_dyn = split(step_key); disturb_key, key = split(key)
            _, a = rng.split(k)
            b, _ = rng.split(a)
            d, _ = rng.split(b)
            return d

        def sin_term(t):  # free.py:27-38 in fp32, like the env
            amp = dp[:3] * scale
            per = dp[:3] * f32(period / 3) + f32(period)
            return (amp * np.sin(f32(2 * np.pi) / per * f32(t) + dp[3:6] * f32(2 * np.pi))).astype(f32)

        for k in range(H - 1):
            if key_mode == _lib.DISTURB_KEYS_HESSIAN:
                sk, key = rng.split(key)
            elif key_mode == _lib.DISTURB_KEYS_NOMINAL:
                _, key = rng.split(key)
                sk, key = rng.split(key)
            else:
                sk = key
            t = int(time) + k
            hit = t % period == 0
            g, c = np.zeros(3, dtype=f32), f32(0.0)
            if kind == "gaussian":
                if not deterministic:
                    g = (f32(params.dyn_noise_scale) * np.asarray(rng.normal(disturb_key(sk), (3,)), dtype=f32)).astype(f32)
            elif kind == "periodic":
                if hit:
                    held = np.asarray(rng.uniform(disturb_key(sk), (3,), -scale, scale), dtype=f32)
                g = held.copy()
            elif kind == "sin":
                g = sin_term(t)
            elif kind == "mixed":
                u = np.asarray(rng.uniform(disturb_key(sk), (3,), -scale, scale), dtype=f32) if hit else np.zeros(3, dtype=f32)
                g = ((sin_term(t) + u) / f32(3)).astype(f32)
                c = f32(0.0) if hit else f32(1.0) / f32(3.0)
            tab[k + 1, :3] = g
            tab[k + 1, 3] = c
        return tab

    def get_zero_state(self, key, params) -> EnvState3D:
        """quadrotor.py:265-312."""
        traj_key, disturb_key, key = crandom.split(key, 3)
        pos_traj, vel_traj, acc_traj = self.generate_traj(traj_key)
        z3 = np.zeros(3, dtype=f32)
        hist = self.default_params.adapt_horizon + 2
        traj_dev = None
        if self.device is not None:
            import torch
            traj_dev = (torch.from_numpy(pos_traj).to(self.device), torch.from_numpy(vel_traj).to(self.device))
        return EnvState3D(
            pos=z3.copy(), vel=z3.copy(), omega=z3.copy(), omega_tar=z3.copy(), quat=np.array([0, 0, 0, 1], dtype=f32),
            pos_tar=pos_traj[0], vel_tar=vel_traj[0], acc_tar=acc_traj[0],
            pos_traj=pos_traj, vel_traj=vel_traj, acc_traj=acc_traj, last_thrust=0.0, last_torque=z3.copy(), time=0,
            f_disturb=crandom.uniform(disturb_key, (3,), -params.disturb_scale, params.disturb_scale),
            vel_hist=np.zeros((hist, 3), f32), omega_hist=np.zeros((hist, 3), f32), action_hist=np.zeros((hist, 4), f32),
            control_params=self.default_control_params, traj_dev=traj_dev)

    def get_info(self, rng, state, next_state, params) -> dict:
        """quadrotor.py:314-361."""
        if self.generate_noisy_state:
            rng_pos, rng_vel, rng_quat, rng_omega, rng = crandom.split(rng, 5)
            s = f32(self.default_params.obs_noise_scale)
            noisy_state = next_state.replace(
                pos=(next_state.pos + crandom.normal(rng_pos, (3,)) * s * f32(0.25)).astype(f32),
                vel=(next_state.vel + crandom.normal(rng_vel, (3,)) * s * f32(0.5)).astype(f32),
                quat=(next_state.quat + crandom.normal(rng_quat, (4,)) * s * f32(0.02)).astype(f32),
                omega=(next_state.omega + crandom.normal(rng_omega, (3,)) * s * f32(0.5)).astype(f32))
        else:
            noisy_state = None
        return {"discount": 1.0, "err_pos": self.get_err_pos(state), "err_vel": self.get_err_vel(state),
                "obs_param": self.get_obs_paramsonly(state, params), "noisy_state": noisy_state}

    def reset_env(self, key, params):
        """quadrotor.py:363-370 (note the (obs, info, state) order)."""
        state = self.get_init_state(key, params)
        info_key, key = crandom.split(key)
        info = self.get_info(info_key, state, state, params)
        return self.get_obs(state, params), info, state

    def get_obs_quadonly(self, state, params):
        """quadrotor.py:372-394."""
        dp = self.default_params
        idx = np.clip(state.time + 1 + np.arange(dp.traj_obs_len) * dp.traj_obs_gap, 0, state.pos_traj.shape[0] - 1)
        return np.concatenate([state.pos, state.vel / 3.0, state.quat, state.omega / 5.0, state.pos_tar,
                               state.vel_tar / 3.0, state.pos_traj[idx].flatten(),
                               state.vel_traj[idx].flatten() / 3.0]).astype(f32)

    def get_obs_paramsonly(self, state, params):
        """quadrotor.py:425-452."""
        return np.concatenate([
            (np.diag(params.I) - params.I_diag_mean) / params.I_diag_std, state.f_disturb / params.disturb_scale,
            (params.hook_offset - params.hook_offset_mean) / params.hook_offset_std, params.disturb_params,
            [(params.m - params.m_mean) / params.m_std,
             (params.action_scale - params.action_scale_mean) / params.action_scale_std,
             (params.alpha_bodyrate - params.alpha_bodyrate_mean) / params.alpha_bodyrate_std]]).astype(f32)

    def get_obs_quad_params(self, state, params):
        """quadrotor.py:465-470."""
        return np.concatenate([self.get_obs_quadonly(state, params), self.get_obs_paramsonly(state, params)])

    def is_terminal(self, state, params) -> bool:
        """quadrotor.py:479-490."""
        done = (state.time >= params.max_steps_in_episode) or bool(np.any(np.abs(state.pos) > 3.0))
        if not self.disable_rollover_terminate:
            done = done or (state.quat[3] < np.cos(np.pi / 4.0)) or bool(np.any(np.abs(state.omega) > 100.0))
        return done



def split_trace_rows(rows: np.ndarray) -> dict:
    """Trace rows [.., n, 168] (include/covo_hip.h: covo_set_episode_trace) -> {state [.., n, 32], noisy [.., n, 32], u [.., n, 4],
    cost_plan [.., n], pos_plan [.., n, H, 3]} as numpy views."""
    H = (rows.shape[-1] - 72) // 3
    return {"state": rows[..., 0:32], "noisy": rows[..., 32:64], "u": rows[..., 64:68], "cost_plan": rows[..., 68],
            "pos_plan": rows[..., 72:].reshape(rows.shape[:-1] + (H, 3))}


def split_fan_rows(rows: np.ndarray) -> dict:
    """Fan rows [.., K, 100] (include/covo_hip.h: covo_set_step_fan) -> {pos [.., K, H, 3], cost [.., K], idx [.., K] int32} (numpy;
    pos and cost are views)."""
    H = (rows.shape[-1] - 4) // 3
    return {"pos": rows[..., 4:].reshape(rows.shape[:-1] + (H, 3)), "cost": rows[..., 0],
            "idx": np.ascontiguousarray(rows[..., 1]).view(np.int32)}


def split_arbiter_rows(rows: np.ndarray) -> dict:
    """Arbiter rows [.., 8] (include/covo_hip.h: covo_set_step_arbiter) -> {cost [.., 3] (softmax mean, nominal, best sample; +inf:
    masked out or absent), cost_chosen [..], choice [..] int32, best [..] int32 (the best sample's index, -1: none)} (numpy)."""
    return {"cost": rows[..., 0:3], "cost_chosen": rows[..., 3], "choice": np.ascontiguousarray(rows[..., 4]).view(np.int32),
            "best": np.ascontiguousarray(rows[..., 5]).view(np.int32)}


def _split_fields(rows: np.ndarray, fields, words=()) -> dict:
    """Rows [.., len(fields) or more] -> {field: rows[.., i]}; the fields named in `words` hold uint32 bits and come back as such."""
    out = {}
    for i, name in enumerate(fields):
        col = rows[..., i]
        out[name] = np.ascontiguousarray(col).view(np.uint32) if name in words else col
    return out


def split_lam_rows(rows: np.ndarray) -> dict:
    """Temperature rows [.., 4] (include/covo_hip.h: covo_set_step_ess_floor) -> {lam_eff, inv_lam_eff, ess_lam0, evaluations}, each [..]."""
    from .. import _lib
    return _split_fields(rows, _lib.LAM_FIELDS)


def split_elite_rows(rows: np.ndarray) -> dict:
    """Selector rows [.., 8] (include/covo_hip.h: covo_set_step_elite) -> {threshold_cost_word, threshold_index_word (uint32), cost_min,
    cost_kth, K, ties}, each [..]."""
    from .. import _lib
    return _split_fields(rows, _lib.ELITE_FIELDS, words=("threshold_cost_word", "threshold_index_word"))


def split_sigma_rows(rows: np.ndarray) -> dict:
    """Sigma log rows [.., 4] (include/covo_hip.h: covo_set_episode_rows) -> {age (int32: 0 = the step refreshed Sigma), fallback, scale,
    logdet}, each [..]; {fallback, scale, logdet} are Sigma adapt's {fallback, c, log det M}, {0, 1, 0} without it."""
    from .. import _lib
    out = _split_fields(rows, _lib.SIGMA_LOG_FIELDS)
    out["age"] = out["age"].astype(np.int32)
    return out


def split_post_rows(rows: np.ndarray) -> dict:
    """Side rows [.., 132] (include/covo_hip.h: covo_set_step_post_cov) -> {shift [.., 128], weight [..]}."""
    return {"shift": rows[..., :128], "weight": rows[..., 128]}


def unpack_state_row(row: np.ndarray) -> dict:
    """One packed state float32[32] (include/covo_hip.h "Data layouts") -> the EnvState3D fields it carries."""
    return {"pos": row[0:3].copy(), "vel": row[3:6].copy(), "quat": row[6:10].copy(), "omega": row[10:13].copy(),
            "f_disturb": row[13:16].copy(), "pos_tar": row[16:19].copy(), "vel_tar": row[19:22].copy(),
            "acc_tar": row[22:25].copy(), "time": int(np.ascontiguousarray(row[25:26]).view(np.int32)[0])}


class _EpisodeLogs:
    """The logs an episode driver can fill next to the env log, one row per enqueued step: `diag_log` (sampling diagnostics),
    `trace` (the flight recorder), `fanlog` (the sample fan), `arblog` (the update arbiter), and the rows of the step attachments
    (covo_set_episode_rows): `lamlog` (the ESS floor's temperature), `elitelog` (the elite set's selector), `iterlog` (the passes' cost
    minima), `sigmalog` (the Sigma period's age, Sigma adapt's row), `postlog` (the posterior covariance's side row) and `postcovlog`
    (its matrix: 64 KiB per step and instance, kept only by an episode built with log_post_cov=True).  Each is None until a controller
    built with its option runs the episode (SamplingCore.attach_log allocates it on first use), shaped like the env log `self.log` with
    the log's own row in place of the 4 floats: [T + 1, ...] for one instance, [E, T + 1, ...] for E (STEP_AXIS: the step axis)."""
    STEP_AXIS = 0
    log_post_cov = False
    # attribute: (the row's width in _lib -- None: alloc_log's argument is the width --, what splits the rows read back, what the log is
    # called, the option that fills it)
    LOGS = {"diag_log": ("COVO_DIAG_FLOATS", None, "diagnostic log", "compute_diag=True"),         # rows [8]
            "trace": ("COVO_TRACE_FLOATS", split_trace_rows, "trace", "compute_plan=True"),          # rows [168]
            "fanlog": ("COVO_FAN_FLOATS", split_fan_rows, "fan log", "compute_fan=K"),               # rows [K, 100]: alloc_log("fanlog", K)
            "arblog": ("COVO_ARB_FLOATS", split_arbiter_rows, "arbiter log", "update='best' or 'guarded'"),  # rows [8]
            "lamlog": ("COVO_LAM_FLOATS", split_lam_rows, "temperature log", "ess_min"),            # rows [4]
            "elitelog": ("COVO_ELITE_FLOATS", split_elite_rows, "elite log", "elite=K"),              # rows [8]
            "iterlog": (None, None, "iteration log", "iters=k > 1"),                                  # rows [k]: alloc_log("iterlog", k)
            "sigmalog": ("COVO_SIGMA_LOG_FLOATS", split_sigma_rows, "Sigma log", "sigma_period=m > 1"),  # rows [4]
            "postlog": ("COVO_POST_AUX_FLOATS", split_post_rows, "posterior side-row log", "compute_post_cov=True"),  # rows [132]
            "postcovlog": ("COVO_POST_COV_FLOATS", None, "posterior covariance log",
                           "compute_post_cov=True, in an episode built with log_post_cov=True")}      # rows [128 * 128]

    def alloc_log(self, name, *inner):
        import torch
        width = self.LOGS[name][0]
        shape = tuple(self.log.shape[:-1]) + tuple(int(n) for n in inner) + ((getattr(self._lib, width),) if width else ())
        setattr(self, name, torch.zeros(shape, dtype=torch.float32, device=self.device))

    # the hold log of plan_hold > 1 -- [.., T + 1, 8], None until such a controller runs the episode -- is not one of LOGS: the hold
    # launch, and the latch on plan steps, write its rows themselves (SamplingCore.attach_hold_log)
    holdlog = None

    def alloc_hold_log(self):
        import torch
        self.holdlog = torch.zeros(tuple(self.log.shape[:-1]) + (self._lib.COVO_HOLD_FLOATS,), dtype=torch.float32, device=self.device)

    def read_hold(self):
        """-> {age [n] (int32: 0 = the step planned), alpha [n], gain [n] (max |K dx|_inf as it entered the action), clipped [n] (int32),
        flags [n] (int32: 1 the sweep is flagged, 2 a command that is not finite, 4 the state's time is not the plan's + age),
        dpos [n], time [n] (int32)}: per enqueued step its hold row (include/covo_hip.h: covo_set_step_plan_hold), under a controller
        built with plan_hold > 1."""
        if self.holdlog is None:
            raise RuntimeError("no hold log: run_episode under a controller built with plan_hold=m > 1")
        self.read_log()  # synchronises and checks the device status
        rows = self.holdlog.narrow(self.STEP_AXIS, 0, self.n_steps).cpu().numpy()
        as_int = lambda i: np.ascontiguousarray(rows[..., i]).view(np.int32)
        return {"age": as_int(0), "alpha": rows[..., 1], "gain": rows[..., 2], "clipped": as_int(3), "flags": as_int(4),
                "dpos": rows[..., 5], "time": as_int(6)}

    # the estimator log of an attached controllers.StateEstimator -- [.., T + 1, 34], None until a controller with one attached runs the
    # episode -- is not one of LOGS either: the estimator's launch writes its rows itself (SamplingCore.attach_estimator_log)
    estlog = None

    def alloc_estimator_log(self):
        import torch
        self.estlog = torch.zeros(tuple(self.log.shape[:-1]) + (self._lib.COVO_EST_LOG_FLOATS,), dtype=torch.float32, device=self.device)

    def read_estimate(self):
        """-> {measured [n, 13], estimate [n, 13], flags [n] (int32: 1 initialised, 2 re-initialised on the time word, 4 a measured
        coordinate not finite, 8 the update failed), nis [n], innov_pos [n], moved_pos [n], trace_pos [n], trace_vel [n], pivot_min [n],
        time [n] (int32)}: per enqueued step what the env step measured, what the estimator wrote over it and its side row
        (include/covo_hip.h: covo_set_step_estimator), under a controller with a controllers.StateEstimator attached."""
        if self.estlog is None:
            raise RuntimeError("no estimator log: run_episode under a controller with a StateEstimator attached (StateEstimator.attach)")
        self.read_log()  # synchronises and checks the device status
        rows = self.estlog.narrow(self.STEP_AXIS, 0, self.n_steps).cpu().numpy()
        as_int = lambda i: np.ascontiguousarray(rows[..., i]).view(np.int32)
        return {"measured": rows[..., 0:13], "estimate": rows[..., 13:26], "flags": as_int(26), "nis": rows[..., 27],
                "innov_pos": rows[..., 28], "moved_pos": rows[..., 29], "trace_pos": rows[..., 30], "trace_vel": rows[..., 31],
                "pivot_min": rows[..., 32], "time": as_int(33)}

    # the observer log of an attached controllers.ForceObserver -- [.., T + 1, 40], None until a controller with one attached runs the
    # episode --: like estlog, written by the filter's launch itself (SamplingCore.attach_force_observer_log)
    obslog = None

    def alloc_force_observer_log(self):
        import torch
        self.obslog = torch.zeros(tuple(self.log.shape[:-1]) + (self._lib.COVO_OBS_LOG_FLOATS,), dtype=torch.float32, device=self.device)

    def read_force(self):
        """-> {measured [n, 13], written [n, 16], force_true [n, 3], force_est [n, 3], rows [n, 8]}: per enqueued step what the env step
        measured, the 16 floats the row held behind the observer's launch, the force the env step left in the row (the one the NEXT
        plant step integrates), the observer's estimate of it (written[:, 13:16]) and its side row (include/covo_hip.h:
        covo_set_step_force_observer; words 0 and 7 are int32 bits), under a controller with a controllers.ForceObserver attached."""
        if self.obslog is None:
            raise RuntimeError("no observer log: run_episode under a controller with a ForceObserver attached (ForceObserver.attach)")
        self.read_log()  # synchronises and checks the device status
        rows = self.obslog.narrow(self.STEP_AXIS, 0, self.n_steps).cpu().numpy()
        return {"measured": rows[..., 0:13], "written": rows[..., 16:32], "force_true": rows[..., 13:16], "force_est": rows[..., 29:32],
                "rows": rows[..., 32:40]}

    def log_segment(self, name):
        """What the episode driver binds of log `name` for the next segment: one instance -- the rows from n_steps on (covo_run_episode
        counts its rows from 0); E instances -- the whole buffer (the batched drivers take the first row of a segment as log_index)."""
        buf = getattr(self, name)
        return buf if self.STEP_AXIS else buf[self.n_steps:]

    def _read(self, name):
        _, split, label, option = self.LOGS[name]
        buf = getattr(self, name)
        if buf is None:
            raise RuntimeError(f"no {label}: run_episode under a controller built with {option}")
        self.read_log()  # synchronises and checks the device status
        rows = buf.narrow(self.STEP_AXIS, 0, self.n_steps).cpu().numpy()
        return split(rows) if split else rows

    # the read_* below: numpy, n = n_steps rows per instance ([E, n, ...] for E instances), synchronising and checking the device status
    # like read_log
    def read_diag(self):
        """-> float32 [n, 8]: per enqueued step its sampling diagnostics (include/covo_hip.h: covo_set_step_diag), under a controller
        built with compute_diag."""
        return self._read("diag_log")

    def read_trace(self):
        """-> {state [n, 32], noisy [n, 32], u [n, 4], cost_plan [n], pos_plan [n, H, 3]}: per enqueued step the true and the noisy
        state ENTERING its env step, the action it received and the controller's plan (include/covo_hip.h: covo_set_episode_trace),
        under a controller built with compute_plan."""
        return self._read("trace")

    def read_fan(self):
        """-> {pos [n, K, H, 3], cost [n, K], idx [n, K]}: per enqueued step the K sampled rollouts of its fan (include/covo_hip.h:
        covo_set_step_fan), under a controller built with compute_fan."""
        return self._read("fanlog")

    def read_arbiter(self):
        """-> {cost [n, 3], cost_chosen [n], choice [n], best [n]}: per enqueued step the update arbiter's row (include/covo_hip.h:
        covo_set_step_arbiter), under a controller built with update="best" / "guarded"."""
        return self._read("arblog")

    def read_lam(self):
        """-> {lam_eff [n], inv_lam_eff [n], ess_lam0 [n], evaluations [n]}: per enqueued step the ESS floor's solver row
        (include/covo_hip.h: covo_set_step_ess_floor), under a controller built with ess_min."""
        return self._read("lamlog")

    def read_elite(self):
        """-> {threshold_cost_word [n], threshold_index_word [n] (uint32), cost_min [n], cost_kth [n], K [n], ties [n]}: per enqueued
        step the elite set's selector row (include/covo_hip.h: covo_set_step_elite; the last pass's under iters), under a controller
        built with elite."""
        return self._read("elitelog")

    def read_iters(self):
        """-> float32 [n, k]: per enqueued step the minimum sample cost of each of its k passes (include/covo_hip.h:
        covo_set_step_iters), under a controller built with iters=k > 1."""
        return self._read("iterlog")

    def read_sigma(self):
        """-> {age [n] (int32: 0 = the step refreshed Sigma), fallback [n], scale [n], logdet [n]}: per enqueued step the age it ran at
        and Sigma adapt's row (include/covo_hip.h: covo_set_episode_rows; {0, 1, 0} without sigma_adapt), under a controller built with
        sigma_period > 1."""
        return self._read("sigmalog")

    def read_post(self):
        """-> {shift [n, 128], weight [n]} and, in an episode built with log_post_cov=True, cov [n, 128, 128]: per enqueued step the
        posterior covariance's side row and matrix (include/covo_hip.h: covo_set_step_post_cov), under a controller built with
        compute_post_cov (or sigma_adapt)."""
        out = self._read("postlog")
        if self.postcovlog is not None:
            cov = self._read("postcovlog")
            out["cov"] = cov.reshape(cov.shape[:-1] + (128, 128))
        return out


class DeviceEpisode(_EpisodeLogs):
    """One episode whose env state lives on the device: the true state, its noisy copy (what the
    controller plans from), the reference trajectory and the per-step log {reward, err_pos, err_vel, done}.
    `reset` is host plumbing (trajectory generation, quadrotor.py:265-312) followed by one upload; `step` launches
    covo_env_step, which derives the five noise keys of `Quad3D.step` from the step key on the device -- no sync,
    so an episode is 300 x (controller graph + this launch) with one read-back of the log at the end.
    auto_reset (default, as BaseEnvironment.step: quadjax/envs/base.py:22-40): when the pre-step state is terminal the kernel
    stores reset_env(key_reset)'s state, noisy copy and a NEW trajectory (written over pos_traj / vel_traj / acc_traj in place);
    the log row then carries the reset state's errors and done = 1.  `state0` keeps the first reset's host state."""

    def __init__(self, env: "Quad3D", key, params, lib_handle, device, auto_reset: bool = True, log_post_cov: bool = False):
        import torch
        from .. import _lib
        self.env, self.params, self.device = env, params, device
        self.log_post_cov = bool(log_post_cov)  # also keep every step's posterior covariance matrix (19.7 MB per 300 steps)
        self.lib, self.h = lib_handle
        self._lib = _lib
        obs, info, state = env.reset(key, params)
        self.state0 = state
        ns = info["noisy_state"] if info["noisy_state"] is not None else state
        self.true = torch.from_numpy(state.pack()).to(device)
        self.noisy = torch.from_numpy(ns.pack()).to(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
        self.pos_traj, self.vel_traj, self.acc_traj = up(state.pos_traj), up(state.vel_traj), up(state.acc_traj)
        self.T = int(state.pos_traj.shape[0])
        self.log = torch.zeros((params.max_steps_in_episode + 1, 4), dtype=torch.float32, device=device)
        from ..controllers.base import env_model_params_c
        # incl. the env's reward, disturbance model and reset generator (env_step.hip runs all of them)
        self.params_c = env_model_params_c(env, params, auto_reset=auto_reset)
        self.n_steps = 0
        for name in self.LOGS:  # allocated when a controller with the log's option runs the episode
            setattr(self, name, None)

    @property
    def noisy_state(self) -> DeviceState:
        return DeviceState(packed=self.noisy, pos_traj=self.pos_traj, vel_traj=self.vel_traj, time=None)

    @staticmethod
    def leaf_keys(step_key):
        """(disturb, pos, vel, quat, omega) keys of Quad3D.step(step_key, ...): base.py:22 -> step_env (split for
        raw_step and for get_info from the same key, quadrotor.py:262 / :246) -> free.py:136,144 -> quadrotor.py:324."""
        k = crandom.split(step_key)[0]            # base.step: key, key_reset = split(key)
        info_key, raw_key = crandom.split(k)      # step_env: info_key = split(key)[0]; raw_step: step_key = split(key)[1]
        dk = crandom.split(crandom.split(raw_key)[0])[0]   # step_fn: key, key_dyn = split(key); disturb_key, key = split(key)
        return np.concatenate([dk[None], crandom.split(info_key, 5)[:4]]).astype(np.uint32)

    def step(self, step_key, action, stream=None):
        """action: float32[4] device tensor (the controller's u).  Asynchronous."""
        import ctypes as C
        import torch
        keys = np.ascontiguousarray(np.asarray(step_key).reshape(-1)[:2], dtype=np.uint32)  # leaf keys derived on the device
        ptr = self._lib.ptr
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
        self._lib.check(self.lib.covo_env_step(
            self.h, ptr(self.true), ptr(self.noisy), ptr(self.pos_traj), ptr(self.vel_traj), ptr(self.acc_traj), self.T,
            C.byref(self.params_c), ptr(action), keys.ctypes.data_as(C.POINTER(C.c_uint32)),
            1 if self.env.generate_noisy_state else 0, float(self.env.default_params.obs_noise_scale), ptr(self.log),
            self.n_steps, st), "covo_env_step")
        self._keep = (keys, action)
        self.n_steps += 1

    def read_log(self):
        """-> float32[n_steps, 4] = reward, err_pos, err_vel, done (pre-step state); synchronises, then checks the handle's
        sticky device status: a kernel of the enqueued steps that failed (a starved grid barrier of the Sigma chain, see
        SamplingCore.shared_device) has poisoned every later step of the segment -- raise instead of returning its log."""
        out = self.log[:self.n_steps].cpu().numpy()
        st = int(self.lib.covo_device_status(self.h, 0))
        if st != 0:
            raise self._lib.CovoError(f"device status 0x{st:x} after the episode segment (covo_device_status): a kernel of an "
                                      "enqueued step failed; its mean / Sigma and everything after it are invalid.  "
                                      "Build the controller with shared_device=True when the GPU is shared.")
        return out


class BatchedDeviceEpisode(_EpisodeLogs):
    """E independent env instances on the device (BASELINE configs[4]): instance e has its own (domain-randomised,
    quadrotor.py:132-171) parameters, reset key, true state, noisy copy, reference trajectory and log.  `step` launches
    covo_env_step_batched -- every instance's Quad3D.step in ONE launch; BatchedCoVOController.run_episode enqueues whole
    episodes (control step + env step for all instances) from one C call.  auto_reset: as DeviceEpisode, per instance."""
    STEP_AXIS = 1

    def __init__(self, env: "Quad3D", keys, params_list, lib_handle, device, auto_reset: bool = True, log_post_cov: bool = False):
        import torch
        from .. import _lib
        from ..controllers.base import env_model_params_c
        self.env, self.params, self.device = env, list(params_list), device
        self.log_post_cov = bool(log_post_cov)  # also keep every step's posterior covariance matrices (19.7 MB per instance and 300 steps)
        self.lib, self.h = lib_handle
        self._lib = _lib
        self.E = len(self.params)
        if not 0 < self.E <= _lib.COVO_MAX_ENVS or len(keys) != self.E:
            raise ValueError(f"{self.E} instances (1..{_lib.COVO_MAX_ENVS}), {len(keys)} keys")
        states, noisy = [], []
        for k, p in zip(keys, self.params):
            obs, info, st = env.reset(k, p)
            states.append(st)
            noisy.append(info["noisy_state"] if info["noisy_state"] is not None else st)
        self.states0 = states
        T = int(states[0].pos_traj.shape[0])
        if any(int(s.pos_traj.shape[0]) != T for s in states):
            raise ValueError("all instances must share the trajectory length T")
        if any(p.max_steps_in_episode != self.params[0].max_steps_in_episode for p in self.params):
            raise ValueError("all instances must share max_steps_in_episode")
        self.T = T
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
        self.true = up(np.stack([s.pack() for s in states]))
        self.noisy = up(np.stack([s.pack() for s in noisy]))
        self.pos_traj = up(np.stack([s.pos_traj for s in states]))
        self.vel_traj = up(np.stack([s.vel_traj for s in states]))
        self.acc_traj = up(np.stack([s.acc_traj for s in states]))
        self.log = torch.zeros((self.E, self.params[0].max_steps_in_episode + 1, 4), dtype=torch.float32, device=device)
        self.params_c = (_lib.EnvParamsC * self.E)(*[env_model_params_c(env, p, auto_reset=auto_reset) for p in self.params])
        self.n_steps = 0
        for name in self.LOGS:  # allocated when a controller with the log's option runs the episode
            setattr(self, name, None)

    def step(self, step_keys, a_mean, stream=None):
        """step_keys: uint32 [E, 2] (the key Quad3D.step receives, per instance); a_mean: float32 [E, 128] device tensor whose first
        four entries per instance are the action.  Asynchronous."""
        import ctypes as C
        import torch
        keys = np.ascontiguousarray(np.asarray(step_keys, dtype=np.uint32).reshape(self.E, 2))
        ptr = self._lib.ptr
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
        self._lib.check(self.lib.covo_env_step_batched(
            self.h, self.E, ptr(self.true), ptr(self.noisy), ptr(self.pos_traj), ptr(self.vel_traj), ptr(self.acc_traj), self.T,
            self.params_c, ptr(a_mean), keys.ctypes.data_as(C.POINTER(C.c_uint32)), 1 if self.env.generate_noisy_state else 0,
            float(self.env.default_params.obs_noise_scale), ptr(self.log), int(self.log.shape[1]), self.n_steps, st),
            "covo_env_step_batched")
        self._keep = (keys, a_mean)
        self.n_steps += 1

    def read_log(self):
        """-> float32 [E, n_steps, 4] = reward, err_pos, err_vel, done (pre-step states); synchronises and checks the device status."""
        out = self.log[:, :self.n_steps].cpu().numpy()
        st = int(self.lib.covo_device_status(self.h, 0))
        if st != 0:
            raise self._lib.CovoError(f"device status 0x{st:x} after the batched episode segment (covo_device_status)")
        return out


def eval_env_batched(env: Quad3D, n_envs: int, controller_params: str = "N4096_H32_lam0.01", n_steps=None, seed: int = 1, device=None,
                     verbose: bool = True, diag: bool = False, trace: bool = False, fan=None, update: str = "softmax",
                     arbiter: bool = False, iters: int = 1, elite=None, sigma_period: int = 1, sigma_adapt: float = 0.0,
                     rows: bool = False, staged: bool = False, controller: str = "covo-online", refine: bool = False,
                     riccati: bool = False, riccati_feedback: bool = False, plan_hold: int = 1, riccati_box: bool = False,
                     beta_pass: float = 0.5, beta_stage: float = 0.9, temp=0.1, *, nodes=None, node_interp: str = "linear"):
    """BASELINE configs[4] as a driver: `n_envs` domain-randomised instances of `env` (each with parameters from
    env.sample_params, its own reset key and key chain, quadrotor.py:132-171 + 506-591 per instance) run one episode under
    `controller` (covo-online by default), controller and env on the device, ONE host sync.  -> mean position error per instance
    [n_envs]; with trace=True
    -> (that, ep.read_trace()): every instance's states, actions and plans of the episode; with fan=K ep.read_fan() -- K sampled
    rollouts of every step of every instance -- is appended to the returned tuple.  update: the controller's update rule ("softmax" |
    "best" | "guarded"); arbiter=True (with "best" / "guarded") appends ep.read_arbiter(), every step's arbiter row.  diag / trace / fan
    are the step options compute_diag / compute_plan / compute_fan, update / iters / elite / sigma_period / sigma_adapt the options of
    those names (controllers/_options.py).  rows=True appends one dict {"elite": ep.read_elite(), "iters": ep.read_iters(), "sigma":
    ep.read_sigma(), "post": ep.read_post()} -- every step's rows of the attachments -- holding the entries whose option is on.
    controller: "covo-online" (the default), or one of the two baselines on the same instances and keys -- "mppi"
    (BatchedMPPIController) and "covo-offline" (BatchedCoVOController(mode="offline"), every instance's Sigma table built by its
    reset() from the episode's start states).  staged=True runs the baselines' staged batched step, which takes elite / update with
    iters / every disturb_type / tracking_slow (controllers/batched.py); with "covo-online", whose batch is staged already, it is a
    ValueError.  refine=True ("covo-online" only; not a step option: controllers/_options.py: check_refine): every control step ends
    with the Newton line search on its committed mean; the trace's u and cost_plan then show the refined mean.  riccati=True
    ("covo-online" only here: the env-batched MPPI / covo-offline steps refuse it; check_riccati): the same line search along the
    Riccati sweep's direction; riccati_feedback=True on top of it: the closed-loop candidates under the sweep's gains compete in that
    line search (check_riccati_feedback).  plan_hold=m > 1 on top of riccati: every m-th step plans, the others apply the sweep's law to
    the measured state (check_plan_hold); rows=True then also holds "hold": ep.read_hold().  riccati_box=True on top of riccati (implied
    by "ilqr"): every sweep solves the control-limited stage problem (check_riccati_box).  controller="dial": BatchedDialController
    (annealed MPPI, always staged) under iters / beta_pass / beta_stage / temp (check_dial; the other controllers ignore the last three);
    rows=True then also holds "lam": ep.read_lam(), the last pass's solver rows, when temp is given.  nodes=M / node_interp (keyword-only,
    "dial" only): the spline-node perturbations of check_dial.  controller="cma": BatchedCMAController at its defaults (this signature
    carries none of its keywords; _eval_cma_batched); rows=True then also holds "cma", the instances' last rows."""
    if controller not in ("covo-online", "mppi", "covo-offline", "ilqr", "dial", "cma"):
        raise ValueError(f"controller={controller!r}: eval_env_batched runs 'covo-online', 'mppi', 'covo-offline', 'ilqr', 'dial' or 'cma'")
    opts = take({**STEP_OPTION_DEFAULTS, **locals(), "compute_diag": diag, "compute_plan": trace, "compute_fan": fan})
    switches = take_switches(locals())
    if controller == "cma":
        return _eval_cma_batched(env, n_envs, controller_params, n_steps, seed, device, verbose, trace, fan, arbiter, rows, staged, switches,
                                 opts)
    if controller == "ilqr":
        return _eval_ilqr_batched(env, n_envs, controller_params, n_steps, seed, device, verbose, trace, rows, staged, arbiter, switches,
                                  opts)
    dial = controller == "dial"
    if dial:
        dial_opts = _check_dial_keywords({**opts, "ess_min": None, "compute_post_cov": False}, switches, None, beta_pass, beta_stage, temp,
                                         nodes, node_interp)
        if staged:
            raise ValueError("staged=True with controller='dial': the annealed batch is always staged")
    online, batch = controller == "covo-online", f"the env-batched {controller} controller"
    check_step_options(None, "online" if online else ("MPPI" if dial else controller), **opts)  # ValueError before anything is built
    check_step_switches(batch, mode_what="online" if online else controller, riccati_what="online" if online else batch,
                        sigma_period=sigma_period, disturb_type=getattr(env, "disturb_type", None), **switches)
    if arbiter and update == "softmax":
        raise ValueError("arbiter=True needs update='best' or 'guarded': under 'softmax' no arbiter is attached")
    from .. import controllers
    rng = crandom.PRNGKey(seed)
    ks = crandom.split(rng, 3 * n_envs + 1)
    params = [env.sample_params(ks[e]) for e in range(n_envs)]
    N, H, lam = (lambda p: (int(p[0][1:]), int(p[1][1:]), float(p[2][3:])))(controller_params.split("_"))
    c0, cp0 = get_controller(env, "mppi" if dial else controller, controller_params, device=device, compute_info=False)
    cp0 = c0.init_control_params
    kw = dict(discount=cp0.discount, gamma_mean=cp0.gamma_mean, a_mean_init=cp0.a_mean, device=c0.core.device, staged=staged, **opts)
    if dial:
        b = controllers.BatchedDialController(env, n_envs, N, H, lam, sigmas=cp0.sample_sigma, beta_pass=beta_pass, beta_stage=beta_stage,
                                              temp=temp, discount=cp0.discount, gamma_mean=cp0.gamma_mean, a_mean_init=cp0.a_mean,
                                              device=c0.core.device, nodes=nodes, node_interp=node_interp, **dial_opts)
    elif controller == "mppi":  # (it takes no switch: check_riccati has refused riccati, which the others need, for the two baselines)
        b = controllers.BatchedMPPIController(env, n_envs, N, H, lam, sigmas=cp0.sample_sigma, **kw)
    else:
        b = controllers.BatchedCoVOController(env, n_envs, N, H, lam, sample_sigma=cp0.sample_sigma,
                                              mode="offline" if controller == "covo-offline" else "online", **switches, **kw)
    del c0
    ep = BatchedDeviceEpisode(env, ks[n_envs:2 * n_envs], params, (b.core.lib, b.core.h), b.core.device)
    if controller == "covo-offline":  # (the table keys: children of the instances' control keys, which stay what they were)
        b.reset(ep.states0, params, [crandom.split(k)[1] for k in ks[2 * n_envs:3 * n_envs]])
    T = params[0].max_steps_in_episode if n_steps is None else int(n_steps)
    t0 = time_module.time()
    b.run_episode(ep, ks[2 * n_envs:3 * n_envs], T)
    log = ep.read_log()
    if verbose:
        el = time_module.time() - t0
        print(f"{n_envs} instances x {T} steps in {el:.2f}s = {n_envs * T / el:.0f} env-steps/s; "
              f"err_pos mean over instances: {log[:, :, 1].mean():.3f} (min {log[:, :, 1].mean(axis=1).min():.3f}, "
              f"max {log[:, :, 1].mean(axis=1).max():.3f})")
        if diag:  # ess > 0.9 N: the costs do not discriminate -- the controller is blind (state outside the box, episode tail)
            ess = ep.read_diag()[:, :, 0]
            blind = (ess > 0.9 * N).sum(axis=1)
            print("ESS median per instance: " + " ".join(f"{v:.0f}" for v in np.median(ess, axis=1)) +
                  f"; steps with ess > 0.9 N per instance: {' '.join(str(int(v)) for v in blind)} (of {T})")
    out = ((log[:, :, 1].mean(axis=1),) + ((ep.read_trace(),) if trace else ()) + ((ep.read_fan(),) if fan else ()) +
           ((ep.read_arbiter(),) if arbiter else ()))
    if rows:
        reads = {"elite": ("elitelog", ep.read_elite), "iters": ("iterlog", ep.read_iters), "sigma": ("sigmalog", ep.read_sigma),
                 "post": ("postlog", ep.read_post)}
        reads["hold"] = ("holdlog", ep.read_hold)
        if dial:
            reads["lam"] = ("lamlog", ep.read_lam)
        out += ({name: read() for name, (attr, read) in reads.items() if getattr(ep, attr) is not None},)
    return out if len(out) > 1 else out[0]


def _eval_cma_batched(env, n_envs, controller_params, n_steps, seed, device, verbose, trace, fan, arbiter, rows, staged, switches, opts):
    """eval_env_batched(controller="cma"): BatchedCMAController (controllers/cma.py) at its defaults -- gamma=0.2, step_size=True,
    damping=1, s_min=0.1, s_max=4: eval_env_batched's signature is pinned and carries none of them -- on the same instances and keys.
    diag and compute_post_cov are implied; trace / fan / update (with arbiter) / iters / elite pass through; sigma_period, sigma_adapt, a
    switch or staged=True is a ValueError (check_cma).  rows=True then also holds "cma": the instances' last rows [n_envs, 8]."""
    from .. import controllers
    from ..controllers._options import check_cma
    check_cma(sigma_period=opts["sigma_period"], sigma_adapt=opts["sigma_adapt"], **switches, what="the env-batched CMA controller")
    if staged:
        raise ValueError("staged=True with controller='cma': its batch is a staged launch sequence already")
    if arbiter and opts["update"] == "softmax":
        raise ValueError("arbiter=True needs update='best' or 'guarded': under 'softmax' no arbiter is attached")
    kw = dict(compute_plan=opts["compute_plan"], compute_fan=opts["compute_fan"], update=opts["update"], iters=opts["iters"],
              elite=opts["elite"])
    check_step_options(None, "the env-batched CMA controller", **kw)
    rng = crandom.PRNGKey(seed)
    ks = crandom.split(rng, 3 * n_envs + 1)
    params = [env.sample_params(ks[e]) for e in range(n_envs)]
    N, H, lam = (lambda p: (int(p[0][1:]), int(p[1][1:]), float(p[2][3:])))(controller_params.split("_"))
    device = device if device is not None else (env.device if env.device is not None else "cuda")
    dp = env.default_params
    import torch
    a_mean = torch.tensor([(dp.m * dp.g / dp.max_thrust) * 2.0 - 1.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=device).repeat(H, 1)
    b = controllers.BatchedCMAController(env, n_envs, N, H, lam, a_mean_init=a_mean, device=device, **kw)
    ep = BatchedDeviceEpisode(env, ks[n_envs:2 * n_envs], params, (b.core.lib, b.core.h), b.core.device)
    b.reset()
    T = params[0].max_steps_in_episode if n_steps is None else int(n_steps)
    t0 = time_module.time()
    b.run_episode(ep, ks[2 * n_envs:3 * n_envs], T)
    log = ep.read_log()
    if verbose:
        el = time_module.time() - t0
        s = b.cma_rows[:, 0].cpu().numpy()
        print(f"{n_envs} instances x {T} steps in {el:.2f}s = {n_envs * T / el:.0f} env-steps/s; err_pos mean over instances: "
              f"{log[:, :, 1].mean():.3f}; last step sizes in [{s.min():.3f}, {s.max():.3f}]")
    out = ((log[:, :, 1].mean(axis=1),) + ((ep.read_trace(),) if trace else ()) + ((ep.read_fan(),) if fan else ()) +
           ((ep.read_arbiter(),) if arbiter else ()))
    if rows:
        reads = {"elite": ("elitelog", ep.read_elite), "iters": ("iterlog", ep.read_iters), "post": ("postlog", ep.read_post)}
        found = {name: read() for name, (attr, read) in reads.items() if getattr(ep, attr) is not None}
        found["cma"] = b.cma_rows.cpu().numpy()
        out += (found,)
    return out if len(out) > 1 else out[0]


def _check_dial_keywords(opts, switches, process_group, beta_pass, beta_stage, temp, nodes=None, node_interp="linear"):
    """check_dial on the keywords get_controller and eval_env_batched carry -> the step options DialController / BatchedDialController
    take.  The objections, in a fixed order: check_dial's own; then ValueError for ess_min, elite, sigma_period, sigma_adapt, a step
    switch or a process_group away from its default, naming it."""
    check_dial(opts["iters"], beta_pass=beta_pass, beta_stage=beta_stage, temp=temp, nodes=nodes, node_interp=node_interp)
    for name in ("ess_min", "elite", "sigma_period", "sigma_adapt"):
        v, default = opts[name], STEP_OPTION_DEFAULTS[name]
        if not ((not v) if default is None else v == default):
            raise ValueError(f"{name}={v!r} with the annealed MPPI controller: it defines its own weights and noise scale; leave it at "
                             "its default")
    for name, default in STEP_SWITCH_DEFAULTS.items():
        if switches[name] != default:
            raise ValueError(f"{name}={switches[name]!r} with the annealed MPPI controller: it takes no step switch; leave it at its "
                             "default")
    if process_group is not None:
        raise ValueError("process_group with the annealed MPPI controller: a sample-sharded rank sees only its shard's costs; run it on "
                         "one rank")
    return {o: opts[o] for o in ("compute_diag", "compute_plan", "compute_fan", "update", "iters", "compute_post_cov")}


def _check_ilqr_switches(env, switches, opts, process_group=None):
    """check_ilqr on the sampling controllers' keywords, as get_controller and eval_env_batched carry them: riccati is implied, and
    riccati_feedback=False (those signatures' default) leaves the choice to the plant -> (iters, riccati_feedback, plan_hold)."""
    sw = {s: v for s, v in switches.items() if s != "riccati"}
    return check_ilqr(opts["iters"], disturb_type=getattr(env, "disturb_type", None), process_group=process_group,
                      **{**sw, "riccati_feedback": sw["riccati_feedback"] or None}, **{o: v for o, v in opts.items() if o != "iters"})


def _eval_ilqr_batched(env, n_envs, controller_params, n_steps, seed, device, verbose, trace, rows, staged, arbiter, switches, opts):
    """eval_env_batched(controller="ilqr"): the same instances, reset keys and key chains under BatchedILQRController (H from
    controller_params; N and lam are ignored; riccati_feedback as for get_controller).  rows=True appends {"hold": ep.read_hold()}
    under plan_hold > 1 (else {})."""
    k, feedback, m = _check_ilqr_switches(env, switches, opts)
    if staged or arbiter:
        raise ValueError(f"{'staged' if staged else 'arbiter'}=True with controller='ilqr': a switch of the sampling batches")
    from .. import controllers
    ks = crandom.split(crandom.PRNGKey(seed), 3 * n_envs + 1)
    params = [env.sample_params(ks[e]) for e in range(n_envs)]
    H = int(controller_params.split("_")[1][1:]) if controller_params else 32
    dp = env.default_params
    th = (dp.m * dp.g / dp.max_thrust) * 2.0 - 1.0
    b = controllers.BatchedILQRController(env, n_envs, H, iters=k, riccati_feedback=feedback, plan_hold=m, compute_plan=trace,
                                          a_mean_init=np.tile(np.array([th, 0.0, 0.0, 0.0], dtype=np.float32), H), device=device,
                                          riccati_box=switches["riccati_box"])
    ep = BatchedDeviceEpisode(env, ks[n_envs:2 * n_envs], params, (b.core.lib, b.core.h), b.core.device)
    T = params[0].max_steps_in_episode if n_steps is None else int(n_steps)
    t0 = time_module.time()
    b.run_episode(ep, ks[2 * n_envs:3 * n_envs], T)
    log = ep.read_log()
    if verbose:
        el = time_module.time() - t0
        print(f"{n_envs} instances x {T} steps in {el:.2f}s = {n_envs * T / el:.0f} env-steps/s; "
              f"err_pos mean over instances: {log[:, :, 1].mean():.3f} (min {log[:, :, 1].mean(axis=1).min():.3f}, "
              f"max {log[:, :, 1].mean(axis=1).max():.3f})")
    out = (log[:, :, 1].mean(axis=1),) + ((ep.read_trace(),) if trace else ())
    if rows:
        out += ({"hold": ep.read_hold()} if ep.holdlog is not None else {},)
    return out if len(out) > 1 else out[0]


def eval_env_device(env: Quad3D, controller, total_steps=30000, num_trajs=4, seed=1, verbose=True, on_episode=None):
    """eval_env (quadrotor.py:506-591) with the env step on the device: same key threading, same protocol (num_trajs
    reset keys x episodes x max_steps_in_episode steps, mean/std over episodes of the mean position error), one host
    sync per EPISODE instead of one per step.  on_episode(ep): called with every finished DeviceEpisode, its log read -- where a caller
    reads the episode's other logs (read_lam, read_sigma, read_iters, ...)."""
    rng = crandom.PRNGKey(seed)
    T = env.default_params.max_steps_in_episode
    core = controller.core
    keep_alias = getattr(controller, "alias_outputs", False)
    controller.alias_outputs = True  # u stays a view of the controller's mean buffer: nothing leaves the device

    def run_one_ep(rng_reset, rng):
        env_params = env.default_params  # :543 (default params even under DR)
        ep = DeviceEpisode(env, rng_reset, env_params, (core.lib, core.h), core.device)
        rng_control, rng = crandom.split(rng)
        control_params = controller.reset(ep.state0, env_params, controller.init_control_params, rng_control)
        if hasattr(controller, "run_episode") and core.world == 1:
            # the whole episode is enqueued by ONE C call (covo_run_episode), keys threaded as run_one_step does
            control_params, rng = controller.run_episode(ep, env_params, control_params, rng, T)
        else:
            for _ in range(T):  # run_one_step, :520-538
                rng, rng_act, rng_step, rng_control = crandom.split(rng, 4)
                action, control_params, _ = controller(None, None, env_params, rng_act, control_params,
                                                       {"noisy_state": ep.noisy_state})
                ep.step(rng_step, action)
                rng, rng_control = crandom.split(rng)
        log = ep.read_log()
        if on_episode is not None:
            on_episode(ep)
        # info["err_pos"] of step t is the error of the state BEFORE that step (quadrotor.py:352); the host loop
        # records it after each env.step, i.e. rows 0..T-1 of the log
        return rng, log[:, 1]

    t0 = time_module.time()
    num_eps = int(total_steps // T)
    err_pos_ep = []
    rng, rng_reset_meta = crandom.split(rng)
    for i, rng_reset in enumerate(crandom.split(rng_reset_meta, num_trajs)):
        for _ in range(max(num_eps // num_trajs, 1)):
            rng, err_pos = run_one_ep(rng_reset, rng)
            err_pos_ep.append(err_pos.mean())
    controller.alias_outputs = keep_alias
    err_pos_ep = np.asarray(err_pos_ep)
    if verbose:
        print(f"env running time: {time_module.time()-t0:.2f}s")
        print(f"err_pos mean: {err_pos_ep.mean():.3f}, std: {err_pos_ep.std():.3f}")
    return err_pos_ep


def eval_env(env: Quad3D, controller, total_steps=30000, filename="", num_trajs=4, seed=1, save=True, verbose=True):
    """quadrotor.py:506-591: `num_trajs` reset keys x (episodes) x max_steps_in_episode steps; reports the
    mean/std over episodes of the mean position error."""
    rng = crandom.PRNGKey(seed)
    T = env.default_params.max_steps_in_episode

    def run_one_ep(rng_reset, rng):
        env_params = env.default_params  # :543 (default params even under DR)
        obs, info, env_state = env.reset(rng_reset, env_params)
        rng_control, rng = crandom.split(rng)
        control_params = controller.reset(env_state, env_params, controller.init_control_params, rng_control)
        errs = []
        for _ in range(T):  # run_one_step, :520-538
            rng, rng_act, rng_step, rng_control = crandom.split(rng, 4)
            action, control_params, control_info = controller(obs, env_state, env_params, rng_act, control_params, info)
            if hasattr(action, "detach"):
                action = action.detach().cpu().numpy()
            obs, env_state, reward, done, info = env.step(rng_step, env_state, action, env_params)
            rng, rng_control = crandom.split(rng)
            errs.append(info["err_pos"])
        return rng, np.asarray(errs)

    t0 = time_module.time()
    num_eps = int(total_steps // T)
    err_pos_ep = []
    rng, rng_reset_meta = crandom.split(rng)
    for i, rng_reset in enumerate(crandom.split(rng_reset_meta, num_trajs)):
        if verbose:
            print(f"[DEBUG] test traj {i+1}")
        for _ in range(max(num_eps // num_trajs, 1)):
            rng, err_pos = run_one_ep(rng_reset, rng)
            err_pos_ep.append(err_pos.mean())
    err_pos_ep = np.asarray(err_pos_ep)
    pos_mean, pos_std = err_pos_ep.mean(), err_pos_ep.std()
    if verbose:
        print(f"env running time: {time_module.time()-t0:.2f}s")
        print(f"err_pos mean: {pos_mean:.3f}, std: {pos_std:.3f}")
        print(f"${pos_mean*100:.2f} \\pm {pos_std*100:.2f}$")
    if save:
        from .. import get_package_path
        save_path = f"{get_package_path()}/../results"
        os.makedirs(save_path, exist_ok=True)
        with open(f"{save_path}/eval_err_pos_{filename}.pkl", "wb") as f:
            pickle.dump(np.array(err_pos_ep), f)
    return err_pos_ep


def get_controller(env, controller_name, controller_params=None, debug=False, device=None, process_group=None,
                   compute_info=True, compute_diag=False, compute_plan=False, ess_min=None, compute_fan=None, update="softmax",
                   iters=1, elite=None, sigma_period=1, compute_post_cov=False, sigma_adapt=0.0, refine=False,
                   riccati=False, riccati_feedback=False, plan_hold=1, riccati_box=False, beta_pass=0.5, beta_stage=0.9, temp=0.1, *,
                   nodes=None, node_interp="linear"):
    """quadrotor.py:670-752.  compute_diag, compute_plan, ess_min, compute_fan, update, iters, elite, sigma_period, compute_post_cov and
    sigma_adapt are the sampling controllers' step options -- what each does and what it adds to the controller's info dict:
    controllers/_options.py.  refine (covo-online only): the Newton line search behind every step -- a switch, not a step option
    (controllers/_options.py: check_refine).  riccati (mppi, covo-offline, covo-online): the same line search along the Riccati sweep's
    direction, which needs neither R nor Sigma (controllers/_options.py: check_riccati).  riccati_feedback (on top of riccati): the
    closed-loop candidates under the sweep's gains compete in that line search (controllers/_options.py: check_riccati_feedback).
    plan_hold (on top of riccati): every plan_hold-th control step plans, the others track the last plan under the sweep's gains
    (controllers/_options.py: check_plan_hold).  riccati_box (on top of riccati; "ilqr" takes it as it is): every stage of the sweep
    solves the control-limited box QP (controllers/_options.py: check_riccati_box).
    controller_name "ilqr": the sampling-free controller (controllers/ilqr.py; controllers/_options.py: check_ilqr) -- H is taken from
    controller_params, N and lam are ignored; iters, plan_hold and compute_plan pass through, riccati is implied, riccati_feedback=True
    asks for the closed-loop candidates and False (this signature's default) leaves the choice to the plant (ILQRController's None);
    every other step option away from its default is a ValueError.
    controller_name "dial": the annealed MPPI controller (controllers/dial.py; controllers/_options.py: check_dial) -- MPPI's control
    parameters; iters, beta_pass, beta_stage, temp and the keyword-only nodes / node_interp (spline-node perturbations) are its own
    keywords (every other controller name ignores all but iters at their defaults), compute_diag / compute_plan / compute_fan / update / compute_post_cov pass through; ess_min, elite, sigma_period,
    sigma_adapt, a switch or a process_group away from the default is a ValueError."""
    opts, switches = take(locals()), take_switches(locals())
    if controller_name == "ilqr":  # ValueError / NotImplementedError before anything is built
        k, feedback, m = _check_ilqr_switches(env, switches, opts, process_group=process_group)
    if controller_name == "dial":
        dial_opts = _check_dial_keywords(opts, switches, process_group, beta_pass, beta_stage, temp, nodes, node_interp)
    import torch
    if controller_name == "cma":
        # the CMA controller at its defaults (gamma=0.2, step_size=True, damping=1, s_min=0.1, s_max=4: this signature is pinned and
        # carries none of them; build controllers.CMAController for others).  check_cma refuses sigma_period, sigma_adapt, the switches
        # and a process_group; compute_diag and compute_post_cov are implied
        from ..controllers._options import check_cma
        check_cma(sigma_period=sigma_period, sigma_adapt=sigma_adapt, process_group=process_group, **switches)
        N, H, lam = ((lambda p: (int(p[0][1:]), int(p[1][1:]), float(p[2][3:])))(controller_params.split("_")) if controller_params
                     else (8192, 32, 0.01))
        device = device if device is not None else (env.device if env.device is not None else "cuda")
        dp = env.default_params
        th = (dp.m * dp.g / dp.max_thrust) * 2.0 - 1.0
        control_params = controllers.CMAParams(
            gamma_mean=1.0, discount=1.0, sample_sigma=0.5,
            a_mean=torch.tensor([th, 0.0, 0.0, 0.0], dtype=torch.float32, device=device).repeat(H, 1),
            a_cov=torch.eye(H * env.action_dim, dtype=torch.float32, device=device) * 0.25)
        return controllers.CMAController(env=env, control_params=control_params, N=N, H=H, lam=lam, device=device,
                                         compute_info=compute_info, compute_plan=compute_plan, compute_fan=compute_fan, update=update,
                                         ess_min=ess_min, elite=elite, iters=iters), control_params
    if controller_name == "ilqr":
        H = int(controller_params.split("_")[1][1:]) if controller_params else 32
        device = device if device is not None else (env.device if env.device is not None else "cuda")
        dp = env.default_params
        th = (dp.m * dp.g / dp.max_thrust) * 2.0 - 1.0
        control_params = controllers.ILQRParams(
            a_mean=torch.tensor([th, 0.0, 0.0, 0.0], dtype=torch.float32, device=device).repeat(H, 1), discount=1.0)
        cls = controllers.ILQRBoxController if riccati_box else controllers.ILQRController
        return cls(env=env, control_params=control_params, H=H, iters=k, riccati_feedback=feedback, plan_hold=m,
                   compute_plan=compute_plan, device=device), control_params
    # ValueError before anything is built; the controller's own check, with N, follows
    what = "online" if ("covo" in controller_name and "offline" not in controller_name) else controller_name
    what = "MPPI" if controller_name == "dial" else what
    check_step_options(None, what, **opts)
    check_step_switches(what, sigma_period=sigma_period, disturb_type=getattr(env, "disturb_type", None), **switches)

    def parse_sample_params(param_text):
        if not param_text:
            return 8192, 32, 0.01, 0.5
        parts = param_text.split("_")
        return int(parts[0][1:]), int(parts[1][1:]), float(parts[2][3:]), 0.5

    device = device if device is not None else (env.device if env.device is not None else "cuda")

    def get_sample_mean(H):
        dp = env.default_params
        th = (dp.m * dp.g / dp.max_thrust) * 2.0 - 1.0
        return torch.tensor([th, 0.0, 0.0, 0.0], dtype=torch.float32, device=device).repeat(H, 1)

    if controller_name == "pid":
        control_params = controllers.PIDParams(Kp=10.0, Kd=5.0, Ki=0.0, Kp_att=10.0)
        return controllers.PIDController(env, control_params=control_params), control_params
    if controller_name == "random":
        return controllers.RandomController(env, None), None
    if controller_name == "mppi":
        N, H, lam, sigma = parse_sample_params(controller_params)
        a_cov = (torch.eye(env.action_dim, dtype=torch.float32, device=device) * sigma ** 2).repeat(H, 1, 1)
        control_params = controllers.MPPIParams(gamma_mean=1.0, gamma_sigma=0.0, discount=1.0, sample_sigma=sigma,
                                                a_mean=get_sample_mean(H), a_cov=a_cov)
        return controllers.MPPIController(env=env, control_params=control_params, N=N, H=H, lam=lam, device=device,
                                          process_group=process_group, compute_info=compute_info,  # (MPPI has no refine: refused above)
                                          **{s: v for s, v in switches.items() if s != "refine"}, **opts), control_params
    if controller_name == "dial":
        N, H, lam, sigma = parse_sample_params(controller_params)
        a_cov = (torch.eye(env.action_dim, dtype=torch.float32, device=device) * sigma ** 2).repeat(H, 1, 1)
        control_params = controllers.MPPIParams(gamma_mean=1.0, gamma_sigma=0.0, discount=1.0, sample_sigma=sigma,
                                                a_mean=get_sample_mean(H), a_cov=a_cov)
        return controllers.DialController(env=env, control_params=control_params, N=N, H=H, lam=lam, device=device,
                                          compute_info=compute_info, beta_pass=beta_pass, beta_stage=beta_stage, temp=temp,
                                          nodes=nodes, node_interp=node_interp, **dial_opts), control_params
    if "covo" in controller_name:
        N, H, lam, sigma = parse_sample_params(controller_params)
        mode = "offline" if "offline" in controller_name else "online"
        if "online" not in controller_name and "offline" not in controller_name:
            print("[DEBUG] unset mode, CoVO mode set to online")
        control_params = controllers.CoVOParams(
            gamma_mean=1.0, gamma_sigma=0.0, discount=1.0, sample_sigma=sigma, a_mean=get_sample_mean(H),
            a_cov=torch.eye(H * env.action_dim, dtype=torch.float32, device=device) * sigma ** 2,
            a_cov_offline=torch.zeros((H, env.action_dim, env.action_dim), dtype=torch.float32, device=device))
        return controllers.CoVOController(env=env, control_params=control_params, N=N, H=H, lam=lam, mode=mode,
                                          device=device, process_group=process_group, compute_info=compute_info, **switches,
                                          **opts), control_params
    raise NotImplementedError(controller_name)


def render_env(env: Quad3D, controller, control_params, repeat_times=1, filename="", save=True, host_env=False):
    """quadrotor.py:594-667 without the plots: ONE closed-loop run from PRNGKey(1) -- the params, reset and control keys split off
    in that order (:599-611) -- whose STATE SEQUENCE is returned and, with `save`, pickled to results/state_seq_<filename>.pkl
    (relative to the working directory): a list with one dict per step, the env state ENTERING that step (:616), up to and
    including the step whose `done` fires (`repeat_times` of them).  The dicts are keyed by EnvState3D's field names (s.__dict__,
    :656; the device handle `traj_dev` left out) plus `reward`, and -- under a controller built with compute_plan -- `u`,
    `pos_plan` [H, 3] and `cost_plan`: the action the step applied and the controller's own plan (include/covo_hip.h); under one built with compute_fan=K also
    `fan_pos` [K, H, 3], `fan_cost` [K] and `fan_idx` [K]: K of the step's sampled rollouts around that plan; under one built with
    compute_post_cov also `post_cov` [128, 128] and `post_shift` [128] (such a controller takes the host path: moving it onto the
    episode drivers' matrix log would change the noise realisation of the command, see DEVIATION below).  No plotting
    (utils.plot_states, :661, stays out of scope).
    Host path (controllers without a `core` or without compute_plan, host_env=True, repeat_times > 1): the Python loop with the
    reference's per-step keys (rng, rng_act, rng_step = split(rng, 3), :617); on `done` the parameters are re-sampled and the
    controller reset as :633-640.
    Device path (sampling controllers built with compute_plan, repeat_times == 1): ONE run_episode segment of
    max_steps_in_episode + 1 steps with the trace attached, one sync, rows cut at the first `done` of the env log; the states are
    unpacked from the trace rows (the fields the device state carries: pos, vel, quat, omega, f_disturb, pos_tar, vel_tar, acc_tar,
    time), the trajectories come from the episode's reset state.  DEVIATION: the episode drivers thread the per-step keys as
    eval_env's run_one_step does (split(rng, 4), then one more split; quadrotor.py:520-538), not as :617 -- another realisation of
    the same noise; the Philox stream is build-defined anyway (random.py)."""
    rng = crandom.PRNGKey(1)
    rng, rng_params = crandom.split(rng)
    env_params = env.sample_params(rng_params)
    rng, rng_reset = crandom.split(rng)
    core = getattr(controller, "core", None)
    device_path = (not host_env and repeat_times == 1 and core is not None and getattr(core, "compute_plan", False)
                   and hasattr(controller, "run_episode") and core.world == 1 and not getattr(core, "compute_post_cov", False))
    t0 = time_module.time()
    seq = []
    if device_path:
        ep = DeviceEpisode(env, rng_reset, env_params, (core.lib, core.h), core.device)
        rng, rng_control = crandom.split(rng)
        control_params = controller.reset(ep.state0, env_params, controller.init_control_params, rng_control)
        controller.run_episode(ep, env_params, control_params, rng, env_params.max_steps_in_episode + 1)
        tr = ep.read_trace()
        fan = ep.read_fan() if getattr(core, "compute_fan", 0) else None
        log = ep.read_log()
        dones = np.nonzero(log[:, 3] > 0.5)[0]
        n = int(dones[0]) + 1 if len(dones) else int(log.shape[0])
        s0 = ep.state0
        for k in range(n):
            d = unpack_state_row(tr["state"][k])
            d.update(pos_traj=s0.pos_traj, vel_traj=s0.vel_traj, acc_traj=s0.acc_traj, reward=float(log[k, 0]),
                     u=tr["u"][k].copy(), pos_plan=tr["pos_plan"][k].copy(), cost_plan=float(tr["cost_plan"][k]))
            if fan is not None:
                d.update(fan_pos=fan["pos"][k].copy(), fan_cost=fan["cost"][k].copy(), fan_idx=fan["idx"][k].copy())
            seq.append(d)
    else:
        obs, info, env_state = env.reset(rng_reset, env_params)
        rng, rng_control = crandom.split(rng)
        control_params = controller.reset(env_state, env_params, controller.init_control_params, rng_control)
        n_dones = 0
        to_np = lambda v: v.detach().cpu().numpy() if hasattr(v, "detach") else v
        while n_dones < repeat_times:
            d = {k: v for k, v in env_state.__dict__.items() if k != "traj_dev"}
            rng, rng_act, rng_step = crandom.split(rng, 3)
            action, control_params, control_info = controller(obs, env_state, env_params, rng_act, control_params, info)
            action = to_np(action)
            next_obs, next_env_state, reward, done, info = env.step(rng_step, env_state, action, env_params)
            d["reward"] = reward
            if isinstance(control_info, dict) and "pos_plan" in control_info:
                d.update(u=np.array(action, copy=True), pos_plan=to_np(control_info["pos_plan"]).copy(),
                         cost_plan=float(to_np(control_info["cost_plan"])))
            if isinstance(control_info, dict) and "fan_pos" in control_info:
                d.update(fan_pos=to_np(control_info["fan_pos"]).copy(), fan_cost=to_np(control_info["fan_cost"]).copy(),
                         fan_idx=to_np(control_info["fan_idx"]).copy())
            if isinstance(control_info, dict) and "post_cov" in control_info:
                d.update(post_cov=to_np(control_info["post_cov"]).copy(), post_shift=to_np(control_info["post_shift"]).copy())
            seq.append(d)
            if done:
                rng, rng_params = crandom.split(rng)
                env_params = env.sample_params(rng_params)
                rng, rng_control = crandom.split(rng)
                control_params = controller.reset(env_state, env_params, control_params, rng_control)
                n_dones += 1
            obs, env_state = next_obs, next_env_state
    print(f"env running time: {time_module.time()-t0:.2f}s")
    if save:
        os.makedirs("results", exist_ok=True)
        path = os.path.join("results", f"state_seq_{filename}.pkl")
        with open(path, "wb") as f:
            pickle.dump(seq, f)
        print("[DEBUG] state sequence saved to ", path)
    return seq


@pydataclass
class Args:
    """quadrotor.py:755-766."""
    task: str = "tracking"
    controller: str = "lqr"
    controller_params: str = ""
    obs_type: str = "quad"
    debug: bool = False
    mode: str = "render"
    lower_controller: str = "base"
    noDR: bool = False
    disturb_type: str = "gaussian"
    name: str = ""
    host_env: bool = False  # (not in quadjax) eval with the Python env step instead of the device one
    fan: int = 0            # (not in quadjax) render: K sampled rollouts of every step next to the plan (compute_fan); 0 = off
    update: str = "softmax"  # (not in quadjax) the sampling controllers' update rule: softmax | best | guarded (the update arbiter)
    iters: int = 1          # (not in quadjax) the sampling controllers' sample-rollout-update passes per control step; 1 = one pass
    elite: int = 0          # (not in quadjax) the sampling controllers' elite-set update: the K cheapest samples with weight 1; 0 = off
    sigma_period: int = 1   # (not in quadjax) covo-online: every m-th control step refreshes Sigma, the others shift the last factor; 1 = off
    post_cov: bool = False  # (not in quadjax) render: the posterior covariance of every step next to the plan (compute_post_cov)
    sigma_adapt: float = 0.0  # (not in quadjax) covo-online under a Sigma period: the posterior covariance's weight in a reuse step's Sigma'; 0 = off
    refine: bool = False    # (not in quadjax) covo-online: every control step ends with a Newton line search on its committed mean
    riccati: bool = False   # (not in quadjax) mppi / covo: every control step ends with that line search along the Riccati sweep's direction
    riccati_feedback: bool = False  # (not in quadjax) on top of riccati: the closed-loop candidates under the sweep's gains compete too
    plan_hold: int = 1      # (not in quadjax) on top of riccati: every m-th control step plans, the others track the plan under the sweep's gains; 1 = off
    riccati_box: bool = False  # (not in quadjax) on top of riccati / with ilqr: the sweep's stages solve the control-limited box QP
    beta_pass: float = 0.5  # (not in quadjax) --controller dial: the noise scale's factor per pass of a control step's --iters passes
    beta_stage: float = 0.9  # (not in quadjax) --controller dial: the noise scale's factor per stage towards the front of the horizon
    temp: float = 0.1       # (not in quadjax) --controller dial: a pass's temperature in standard deviations of its costs; 0 = the configured lam
    nodes: int = 0          # (not in quadjax) --controller dial: spline nodes the perturbations are drawn at, 2 .. 32; 0 = a draw per stage
    node_interp: str = "linear"  # (not in quadjax) --controller dial --nodes M: "linear" or "cubic" interpolation between the nodes


def main(args: Args):
    """quadrotor.py:769-803: `eval`, and `render` as the state sequence without its plots (render_env)."""
    env = Quad3D(task=args.task, obs_type=args.obs_type, lower_controller=args.lower_controller,
                 enable_randomizer=not args.noDR, disturb_type=args.disturb_type, disable_rollover_terminate=True,
                 generate_noisy_state=True, device="cuda")
    print("starting test...")
    # eval never reads the controller's info dict: quadjax's jitted run_one_step drops pos_mean / pos_std as dead code
    # (quadrotor.py:523-538), here the per-step position statistics are simply not requested
    render = args.mode == "render"
    controller, control_params = get_controller(env, args.controller, args.controller_params, compute_info=args.mode != "eval",
                                                compute_plan=render, compute_fan=(args.fan or None) if render else None,
                                                update=args.update, iters=args.iters, elite=args.elite or None,
                                                sigma_period=args.sigma_period, compute_post_cov=args.post_cov and render,
                                                sigma_adapt=args.sigma_adapt, **take_switches(vars(args)), beta_pass=args.beta_pass,
                                                beta_stage=args.beta_stage, temp=args.temp if args.temp > 0.0 else None,
                                                nodes=args.nodes or None, node_interp=args.node_interp)
    if render:  # the reference's default mode (:798-799); the plan rides along for the sampling controllers
        return render_env(env, controller=controller, control_params=control_params, repeat_times=1, filename=args.name,
                          host_env=args.host_env)
    if args.mode == "eval":
        if not args.host_env and hasattr(controller, "core"):
            # same protocol, env step on the device, whole episodes enqueued by one C call (eval_env_device)
            return eval_env_device(env, controller=controller, total_steps=300 * 4 * 10)
        return eval_env(env, controller=controller, total_steps=300 * 4 * 10, filename=args.name)
    raise NotImplementedError(args.mode)


def _cli():
    ap = argparse.ArgumentParser(description="quadjax-compatible driver (same flag names as quadrotor.py:755-766)")
    for f, default in Args().__dict__.items():
        if f == "post_cov":
            ap.add_argument("--post-cov", "--post_cov", dest="post_cov", action="store_true")
        elif isinstance(STEP_SWITCH_DEFAULTS.get(f), bool):  # --name-with-dashes, and --name_as_it_is where that is another spelling
            ap.add_argument(*dict.fromkeys((f"--{f.replace('_', '-')}", f"--{f}")), dest=f, action="store_true")
        elif f == "plan_hold":
            ap.add_argument("--plan-hold", "--plan_hold", dest="plan_hold", type=int, default=default)
        elif isinstance(default, bool):
            ap.add_argument(f"--{f}", action="store_true")
        elif f == "update":
            ap.add_argument("--update", choices=("softmax", "best", "guarded"), default=default)
        elif f == "sigma_period":
            ap.add_argument("--sigma-period", "--sigma_period", dest="sigma_period", type=int, default=default)
        elif f == "sigma_adapt":
            ap.add_argument("--sigma-adapt", "--sigma_adapt", dest="sigma_adapt", type=float, default=default)
        elif f in ("beta_pass", "beta_stage"):
            ap.add_argument(f"--{f.replace('_', '-')}", f"--{f}", dest=f, type=float, default=default)
        elif f == "node_interp":
            ap.add_argument("--node-interp", "--node_interp", dest=f, choices=("linear", "cubic"), default=default)
        else:
            ap.add_argument(f"--{f}", type=type(default), default=default)
    main(Args(**vars(ap.parse_args())))


if __name__ == "__main__":
    _cli()
