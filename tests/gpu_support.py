"""What the GPU tests share: the device, state / action layouts, and the factories of envs, controllers and instance sets.  Imports
torch and the package, so a tests/test_gpu_*.py imports it below its module-level importorskip / is_available skip, never above."""
import ctypes as C

import numpy as np
import torch

import covo_mpc_amd as cm
from covo_mpc_amd import _lib
from covo_mpc_amd import random as cr
from covo_mpc_amd.dynamics.dataclass import DeviceState, EnvParams3D
from oracle import ref_np as R

DEV = "cuda:0"
H = 32
f32 = np.float32


# ------------------------------------------------------------------------------------------ envs, controllers, instance sets
def quad_env(*, task, randomizer=False, rollover=False, disturb="gaussian", obs_type=None, **kw):
    """Quad3D on DEV with a noisy state.  `task` has no default: the tests disagree on it (tracking_zigzag, tracking, hovering).
    obs_type None: "quad_params" with the randomizer, else "quad" (Quad3D's own default)."""
    if obs_type is None:
        obs_type = "quad_params" if randomizer else "quad"
    return cm.envs.Quad3D(task=task, obs_type=obs_type, enable_randomizer=randomizer, disturb_type=disturb,
                          disable_rollover_terminate=not rollover, generate_noisy_state=True, device=DEV, **kw)


_OFFLINE = {}  # covo-offline's Sigma table per (task, randomizer, rollover, disturbance, seed): it depends on nothing else


def single_controller(env, name, N, *, lam="0.01", seed=1, offline_table=True, **step_options):
    """A single controller at the start of an episode: (controller, control params, obs, info, state, params).  The episode is
    env.reset(PRNGKey(seed)) at the default parameters.  covo-offline's control params carry the Sigma table of
    controller.reset(..., PRNGKey(seed + 1)), built once per env variant and seed (offline_table=False: the caller resets)."""
    c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam{lam}", device=DEV, compute_info=False, **step_options)
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(seed), params)
    cp = c.init_control_params
    if name == "covo-offline" and offline_table:
        k = (env.task, env.enable_randomizer, env.disable_rollover_terminate, env.disturb_type, seed)
        if k not in _OFFLINE:
            t = c.reset(state, params, cp, cr.PRNGKey(seed + 1))
            _OFFLINE[k] = (t.a_cov_offline, t.a_chol_offline)
        cp = cp.replace(a_cov_offline=_OFFLINE[k][0], a_chol_offline=_OFFLINE[k][1])
    return c, cp, obs, info, state, params


def instances(env, name, N, lam, E, *, seed=0, warm=True, controllers=True, gamma_sigma=0.0, **step_options):
    """E domain-randomised instances, each with its own trajectory (reset key), a state a few steps into the episode (reached
    with its own random actions), its own key chain and -- controllers=True -- its own single-instance controller, built with the
    step options; gamma_sigma goes into its control params.  Seeds per instance e: params 100+e, reset 200+e, key chain 300+e,
    reset_key 400+e, warm-up actions 1000+e, warm-up env steps 5000+10e+k (all + seed)."""
    inst = []
    for e in range(E):
        params = env.sample_params(cr.PRNGKey(seed + 100 + e))
        i = dict(params=params)
        if controllers:
            i["c"], _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam{lam}", device=DEV, compute_info=False, **step_options)
            i["cp"] = i["c"].init_control_params
            if gamma_sigma:
                i["cp"] = i["cp"].replace(gamma_sigma=gamma_sigma)
        obs, info, state = env.reset(cr.PRNGKey(seed + 200 + e), params)
        rng = np.random.default_rng(seed + 1000 + e)
        for k in range((2 + e % 4) if warm else 0):
            u = (0.3 * rng.standard_normal(4)).clip(-1, 1).astype(np.float32)
            obs, state, _, _, info = env.step(cr.PRNGKey(seed + 5000 + 10 * e + k), state, u, params)
        i.update(obs=obs, info=info, state=state, key=cr.PRNGKey(seed + 300 + e), reset_key=cr.PRNGKey(seed + 400 + e))
        inst.append(i)
    return inst


def batched_controller(env, name, inst_or_cp0, E, N, lam, *, set_instances=False, check_cov=False, gamma_sigma=None, **kw):
    """The env-batched controller of `name` for E instances, its constants taken from one single-instance control params: those of
    instance 0 of an instances() list, or a cp0 handed in as it is.  gamma_sigma (MPPI only) and everything in kw (staged=,
    iters=, compute_*=...) go to the constructor; set_instances=True also hands it the list's states and parameters; check_cov=True
    asserts that MPPI's initial a_cov is the single factory's (cp0 must then come from an MPPI controller)."""
    inst = inst_or_cp0 if isinstance(inst_or_cp0, list) else None
    cp0 = inst[0]["cp"] if inst is not None else inst_or_cp0
    if name == "mppi":
        if gamma_sigma is not None:
            kw = dict(kw, gamma_sigma=gamma_sigma)
        b = cm.controllers.BatchedMPPIController(env, E, N, H, float(lam), sigmas=cp0.sample_sigma, discount=cp0.discount,
                                                 gamma_mean=cp0.gamma_mean, a_mean_init=cp0.a_mean, device=DEV, **kw)
        assert not check_cov or torch.equal(b.a_cov[0], cp0.a_cov)  # quadrotor.py:705-720: diag(sigma^2) tiled over H
    else:
        b = cm.controllers.BatchedCoVOController(env, E, N, H, float(lam), discount=cp0.discount, gamma_mean=cp0.gamma_mean,
                                                 sample_sigma=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=DEV,
                                                 mode=name.split("-")[1], **kw)
    if set_instances:
        b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    return b


# ------------------------------------------------------------------------------------------ layouts and bit views
def dev_state(s) -> DeviceState:
    x = np.zeros(32, dtype=np.float32)
    x[0:3], x[3:6], x[6:10], x[10:13], x[13:16] = s.pos, s.vel, s.quat, s.omega, s.f_disturb
    x[16:19], x[19:22], x[22:25] = s.pos_tar, s.vel_tar, s.acc_tar
    x[25:26] = np.asarray([s.time], dtype=np.int32).view(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return DeviceState(packed=t(x), pos_traj=t(s.pos_traj), vel_traj=t(s.vel_traj))


def to_stripes(a_nh4):
    """(N,H,4) -> device stripe layout (H,N,4)."""
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a_nh4, (1, 0, 2)), dtype=np.float32)).to(DEV)


def sample_actions(p, rng, N, H=32, sigma=0.5):
    a = np.clip(R.hover_action(p, H, np.float64)[None] + sigma * rng.normal(size=(N, H, 4)), -1, 1)
    return a.astype(np.float32)


def ulps(a, b):
    """max distance in fp32 ulps between two float32 arrays (0 where both are 0)"""
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    scale = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(f32))
    d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / scale
    return float(np.max(np.where(a == b, 0.0, d)))


def bits(x):
    """float32 array or device tensor -> its uint32 words (numpy)"""
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    assert x.dtype == np.float32
    return np.ascontiguousarray(x).view(np.uint32)


# ------------------------------------------------------------------------------------------ model parameters and keys (csrc/disturb.hip)
# disturb_params: every component live (dataclass.py:88; DR / reset draw them); fp32 numbers, like every parameter of the reference
DP = tuple(float(np.float32(x)) for x in (0.7, -0.4, 0.9, 0.15, -0.35, 0.6))


def params_c(p: R.Params, kind="none", reward="penyaw", rollover=False):
    e = EnvParams3D(disturb_params=np.asarray(p.disturb_params, dtype=np.float32), disturb_period=p.disturb_period,
                    disturb_scale=p.disturb_scale, dyn_noise_scale=p.dyn_noise_scale)
    return e.to_c(rollover_terminate=rollover, reward=reward, disturb_type=kind)


def disturb_key(k):
    """disturb_key of step_env(k): quadrotor.py:262, free.py:136,144"""
    return cr.split(cr.split(cr.split(k)[1])[0])[0]


def step_keys(key, mode, H=32):
    """the key step_env receives at every rollout step (include/covo_hip.h: COVO_DISTURB_KEYS_*)"""
    out = []
    for _ in range(H):
        if mode == _lib.DISTURB_KEYS_SHARED:
            out.append(key)
        elif mode == _lib.DISTURB_KEYS_HESSIAN:  # covo.py:151
            rk, key = cr.split(key)
            out.append(rk)
        else:  # covo.py:60,66
            _, key = cr.split(key)
            rs, key = cr.split(key)
            out.append(rs)
    return out


def uniform_draws(p, key, mode, H=32):
    """(H,3): uniform(disturb_key, (3,), -scale, scale) of every step (free.py:16-21)"""
    return np.stack([cr.uniform(disturb_key(k), (3,), -p.disturb_scale, p.disturb_scale) for k in step_keys(key, mode, H)])


# ------------------------------------------------------------------------------------------ one step of a single controller
def build_with_discount(env, name, N, lam="0.01", discount=1.0, plan=True, diag=False):
    """(controller, control params) with the given discount (get_controller fixes 1.0: the controller is rebuilt around it)"""
    c, cp = cm.envs.get_controller(env, name, f"N{N}_H32_lam{lam}", device=DEV, compute_info=False, compute_diag=diag,
                                   compute_plan=plan)
    if discount == 1.0:
        return c, c.init_control_params
    c.core.close()
    cp = cp.replace(discount=discount)
    if name == "mppi":
        c = cm.controllers.MPPIController(env=env, control_params=cp, N=N, H=H, lam=float(lam), device=DEV, compute_info=False,
                                          compute_diag=diag, compute_plan=plan)
    else:
        c = cm.controllers.CoVOController(env=env, control_params=cp, N=N, H=H, lam=float(lam), device=DEV, compute_info=False,
                                          mode="offline" if "offline" in name else "online", compute_diag=diag, compute_plan=plan)
    return c, c.init_control_params


def start_episode(env, c, cp, name, seed=1):
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(seed), params)
    if name == "covo-offline":
        cp = c.reset(state, params, cp, cr.PRNGKey(seed + 1))
    return cp, obs, info, state, params


def step_inputs(env, c, name, params, k_act, dstate, core1):
    """The disturbance inputs the sample rollouts of a step with raw key k_act had: (f_shared host 3-vector, device table or None),
    formed as the controllers' kernel-by-kernel path forms them (covo.py:212,225,231 / mppi.py:53,69,74)."""
    step_key = cr.split(cr.split(k_act)[0])[1]
    pc = c._params_c(params)
    det = name != "mppi"
    if pc.disturb_kind in _lib.TABLE_DISTURB_KINDS:
        return (0.0, 0.0, 0.0), core1.disturb_table(pc, dstate.packed, key=step_key, key_mode=_lib.DISTURB_KEYS_SHARED, deterministic=det)
    if det:
        return (0.0, 0.0, 0.0), None
    return tuple(float(x) for x in env.rollout_disturbance(step_key, params, deterministic=False)), None


def shared_vector(env, name, params, k_act):
    """the one shared vector of a step's sample rollouts under the gaussian model: MPPI's draw, 0 for CoVO (deterministic)"""
    if name != "mppi":
        return np.zeros(3)
    step_key = cr.split(cr.split(k_act)[0])[1]
    return np.asarray(env.rollout_disturbance(step_key, params, deterministic=False), dtype=np.float64)


def finite_step(core, pc, args):
    _lib.check(core.lib.covo_mpc_step(core.h, C.byref(pc), C.byref(args), 7, 9, None, core.stream()), "covo_mpc_step")
    torch.cuda.synchronize()
    assert core.device_status() == 0
    assert bool(torch.isfinite(core._bufs["a_mean"]).all())


def perturbed_hover_mean(p, rng, scale):
    a = (R.hover_action(p, 32, np.float64) + scale * rng.normal(size=(32, 4))).astype(f32)
    a[3, 1] = 1.0    # exact clip ties (tests/test_gpu_parity.py::test_hessian_vs_ad_oracle)
    a[5, 2] = -1.0
    return a.reshape(-1)


# ------------------------------------------------------------------------------------------ the sample fan's rows
POS_BAR = 2e-5


def split_rows(rows):
    """fan rows [K, 100] (device tensor) -> (cost [K] f32, idx [K] i32, words 2..3 [K, 2], pos [K, H, 3]) as numpy"""
    r = rows.detach().cpu().numpy()
    return r[:, 0].copy(), np.ascontiguousarray(r[:, 1]).view(np.int32).copy(), r[:, 2:4], r[:, 4:].reshape(-1, H, 3)


def want_idx(N, K, idx=None):
    if idx is None:
        return np.asarray([(s * N) // K for s in range(K)], dtype=np.int32)
    return np.clip(np.asarray(idx, dtype=np.int64), 0, N - 1).astype(np.int32)


# ------------------------------------------------------------------------------------------ env-batched steps and episodes
_TABLES = {}


def offline_tables(env, inst, tag):
    """Every instance's Sigma table from a single CoVOController.reset on it (cached: the same instances come back in every case)."""
    out = []
    for e, i in enumerate(inst):
        k = (tag, e)
        if k not in _TABLES:
            cp = i["c"].reset(i["state"], i["params"], i["c"].init_control_params, i["reset_key"])
            _TABLES[k] = (cp.a_cov_offline, cp.a_chol_offline)
        out.append(_TABLES[k])
        i["cp"] = i["cp"].replace(a_cov_offline=out[-1][0], a_chol_offline=out[-1][1])
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


ST_TIME = 25  # packed state: the step counter's int32 bits (include/covo_hip.h)


def set_time(ep, e, t):
    """Instance e of a batched episode starts at step t (true and noisy state: the counter's int32 bits)."""
    bits = torch.tensor([t], dtype=torch.int32, device=DEV).view(torch.float32)
    ep.true[e, ST_TIME:ST_TIME + 1] = bits
    ep.noisy[e, ST_TIME:ST_TIME + 1] = bits
