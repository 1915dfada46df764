"""GPU tests (-m gpu) off hover: the kernels of tests/test_gpu_parity.py, test_gpu_models.py, test_gpu_fan.py, test_gpu_trace.py and
test_gpu_reset.py again, through the same C ABI and against the same oracles, from the upset states of tests/state_atlas.py --
every octant and the kink of the reward's yaw atan2 (quad_model.hpp: atan2abs_), its near-singular attitude, inverted / tumbling /
far and fast starts, a non-unit and a negated stored quaternion, and the rollover branch of is_terminal taken at step 0.

Bars.  Rollout cost, rule (a): with e_dev = rel_err(cost, c64) and e32 = rel_err(c32, c64) (the C oracle run in fp32 on the same
inputs), over ALL samples
    max(e_dev) <= max(1e-5, M max(e32)),  q99(e_dev) <= max(1e-5, M q99(e32)),  median(e_dev) <= max(2e-6, M median(e32)),  M = 2:
the kernel's rsq / sqrt / log / rcp are 1-ulp hardware operations and its atan is ~1 ulp of pi/4 where the oracle's are correctly
rounded (0.5 ulp), so operation for operation it may lose at most twice what the fp32 oracle loses; 1e-5 and 2e-6 are the existing
bars of tests/test_gpu_parity.py.  Positions (statistics, fan): max(2e-5, 2 x the fp32 oracle's own loss).  Hessian: 1e-9 relative to
max(1, max|ref|), exactly symmetric; with a force table 1e-9 against the oracle fed the same rows and 2e-8 against the model
functions.  Sigma: 1e-6 relative Frobenius (benign entries).  Env step: 2e-5 max(1, |x|); reset: as tests/test_gpu_reset.py.  PID
nominal: 5e-5 states, 2e-4 means.  Production steps: tests/gpu_cases.py::_oracle_check_of_a_fused_step.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from covo_mpc_amd.dynamics.dataclass import EnvParams3D  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from tests.conftest import make_problem  # noqa: E402
from tests.gpu_cases import _oracle_check_of_a_fused_step, _run_rollout, check_plan_against_oracle  # noqa: E402
from tests.gpu_support import (DEV, DP, POS_BAR, build_with_discount, dev_state, params_c, perturbed_hover_mean, quad_env,  # noqa: E402
                               sample_actions, split_rows, start_episode, to_stripes, ulps, uniform_draws, want_idx)
from tests.state_atlas import (BENIGN, NAMES, ROLLOUT_SEED, ROLLOVER_AT_0, atlas_state, euler_quat, loss3, rel_err,  # noqa: E402
                               rollout_case)

f32 = np.float32
M = 2.0  # see the header


def rule_a(e_dev, e32, where):
    """the three assertions of rule (a); prints the ratios e_dev / e32 -> them"""
    d, o = loss3(e_dev), loss3(e32)
    ratio = d / np.maximum(o, 1e-300)
    w = int(np.argmax(e_dev))
    print(f"  {where}: e_dev max {d[0]:.2e} q99 {d[1]:.2e} median {d[2]:.2e} | e32 {o[0]:.2e} {o[1]:.2e} {o[2]:.2e} | "
          f"e_dev/e32 {ratio[0]:.2f} {ratio[1]:.2f} {ratio[2]:.2f} | worst sample {w}: e32 there {e32[w]:.2e}")
    assert d[0] <= max(1e-5, M * o[0]), (where, "max", d[0], o[0])
    assert d[1] <= max(1e-5, M * o[1]), (where, "q99", d[1], o[1])
    assert d[2] <= max(2e-6, M * o[2]), (where, "median", d[2], o[2])
    return ratio


def oracle_costs(s, p, a, discount, rollover=False, poses=False):
    """(c64, c32[, poses64, poses32]) of the C oracle in fp64 and fp32 on the same fp32 inputs -- the discount among them: the handle
    holds float(0.97), and 0.97 in fp64 instead would put a common 3e-8 k per step (5e-6 of a cost) into e_dev and e32 alike"""
    z, discount = np.zeros(3), float(f32(discount))
    r64 = CO.rollout(s, p, a.astype(np.float64), discount, z, dtype=np.float64, rollover=rollover, want_poses=poses)
    r32 = CO.rollout(s.astype(f32), p, a, discount, z.astype(f32), dtype=f32, rollover=rollover, want_poses=poses)
    if poses:
        return r64[0], r32[0].astype(np.float64), r64[1], r32[1].astype(np.float64)
    return r64, r32.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _core(N, discount):
    return SamplingCore(N, 32, 0.01, discount, device=DEV)


# ------------------------------------------------------------------------------------------ a: rollout
@pytest.mark.parametrize("name", NAMES)
def test_rollout_at_every_entry(name):
    """N = 1024, sigma = 0.5, discount 1 and 0.97, statistics off and on.  The inputs are state_atlas.rollout_case's, the ones whose
    conditioning tests/test_state_atlas.py measures in fp64 (roll_120_spin draws from seed 1: see state_atlas.ROLLOUT_SEED)."""
    N = 1024
    s, p, rng = atlas_state(name, seed=ROLLOUT_SEED.get(name, 0))
    a = sample_actions(p, rng, N)
    assert np.array_equal(a, rollout_case(name, N)[2])
    for discount in (1.0, 0.97):
        core = _core(N, discount)
        c64, c32, p64, p32 = oracle_costs(s, p, a, discount, poses=True)
        cost = _run_rollout(core, s, p, a, np.zeros(3)).copy()
        rule_a(rel_err(cost, c64), rel_err(c32, c64), f"{name} disc={discount}")
        bm = core.blockmin.cpu().numpy()
        assert np.array_equal(bm, np.array([cost[i:i + 64].min() for i in range(0, N, 64)], dtype=f32))
        cost_s = _run_rollout(core, s, p, a, np.zeros(3), want_stats=True).copy()
        assert np.array_equal(cost_s, cost)  # the STATS variant: the same arithmetic
        assert np.array_equal(core.blockmin.cpu().numpy(), bm)
        info = core.info(dev_state(s))
        (pm, ps), (pm32, ps32) = R.pos_stats(p64), R.pos_stats(p32)
        bar = max(2e-5, 2 * max(np.abs(pm32 - pm).max(), np.abs(ps32 - ps).max()))
        dm, dsd = np.abs(info["pos_mean"].cpu().numpy() - pm).max(), np.abs(info["pos_std"].cpu().numpy() - ps).max()
        print(f"  {name} disc={discount}: pos_mean {dm:.2e} pos_std {dsd:.2e} (bar {bar:.2e})")
        assert dm <= bar and dsd <= bar, (name, dm, dsd, bar)


# ------------------------------------------------------------------------------------------ b: yaw sweep
def test_rollout_yaw_sweep():
    """73 start yaws around the circle, +-pi, +-pi/2, +-pi/4, +-3pi/4 and 0 exactly (5 degree steps from -pi: k pi / 36); level,
    N = 64 each.  An octant or sign error of atan2abs_ is O(0.1) in the cost here."""
    N = 64
    s0, p, rng = make_problem(0, 37)
    core = _core(N, 1.0)
    yaws = np.arange(-36, 37) * np.pi / 36
    assert len(yaws) == 73 and all(np.any(yaws == y) for y in (-np.pi, np.pi, np.pi / 2, -np.pi / 2, np.pi / 4, -np.pi / 4,
                                                               3 * np.pi / 4, -3 * np.pi / 4, 0.0))
    e_dev, e32 = [], []
    for yaw in yaws:
        s = s0.replace(quat=euler_quat(0.0, 0.0, yaw)).astype(f32).astype(np.float64)
        a = sample_actions(p, rng, N, sigma=0.3)
        c64, c32 = oracle_costs(s, p, a, 1.0)
        cost = _run_rollout(core, s, p, a, np.zeros(3))
        e_dev.append(rel_err(cost, c64))
        e32.append(rel_err(c32, c64))
    worst = yaws[int(np.argmax([e.max() for e in e_dev]))]
    print(f"  worst yaw {worst:.4f} rad")
    rule_a(np.concatenate(e_dev), np.concatenate(e32), "yaw sweep")


# ------------------------------------------------------------------------------------------ c: rollover at step 0
@pytest.mark.parametrize("name", ROLLOVER_AT_0)
def test_rollout_rollover_at_step_0(name):
    """is_terminal's rollover branch true on the start state: every sample freezes at step 0 (no threshold coin flip), so rule (a)
    holds against the rollover=True oracles; with the flag off the same launch is the un-frozen rollout."""
    N = 256
    s, p, rng = atlas_state(name)
    a = sample_actions(p, rng, N)
    core = _core(N, 0.97)
    _, rew = CO.rollout(s, p, a.astype(np.float64), 0.97, np.zeros(3), dtype=np.float64, rollover=True, want_rewards=True)
    assert np.all(rew == rew[:, :1])
    for rollover in (True, False):
        c64, c32 = oracle_costs(s, p, a, 0.97, rollover=rollover)
        for stats in (False, True):
            cost = _run_rollout(core, s, p, a, np.zeros(3), want_stats=stats, rollover=rollover)
            rule_a(rel_err(cost, c64), rel_err(c32, c64), f"{name} rollover={rollover} stats={stats}")
    frozen, free = oracle_costs(s, p, a, 0.97, rollover=True)[0], c64
    assert np.abs(frozen - free).max() > 1e-3  # the flag matters


# ------------------------------------------------------------------------------------------ d: sample fan and plan trace
@pytest.mark.parametrize("name", ["inverted", "far_fast", "near_singular"])
def test_rollout_fan_positions(name):
    N, K = 256, 64
    s, p, rng = atlas_state(name)
    a = sample_actions(p, rng, N)
    core = _core(N, 1.0)
    ds, pc = dev_state(s), EnvParams3D().to_c()
    core.a.copy_(to_stripes(a))
    cost = core.rollout(ds, pc, (0.0, 0.0, 0.0), False).clone()
    rows = core.rollout_fan(ds, pc, None, f_shared=(0.0, 0.0, 0.0), K=K)
    torch.cuda.synchronize()
    _, _, p64, p32 = oracle_costs(s, p, a, 1.0, poses=True)
    fcost, n, pad, pos = split_rows(rows)
    assert np.array_equal(n, want_idx(N, K)) and np.all(pad == 0.0)
    assert torch.equal(rows[:, 0], cost[torch.from_numpy(n.astype(np.int64)).to(DEV)])  # bit-equal to the rollout's
    loss32 = np.abs(p32 - p64).max()
    dpos = np.abs(pos - np.transpose(p64[:, n], (1, 0, 2))).max()
    print(f"  {name}: |fan_pos - poses| {dpos:.2e}, fp32 oracle's own {loss32:.2e}")
    assert dpos <= max(POS_BAR, 2 * loss32), (name, dpos, loss32)


def _env_state(template, s, traj=True):
    """the host env state `template` with the oracle state s in it (fp32); traj: s's trajectories as well"""
    kw = dict(pos=s.pos, vel=s.vel, quat=s.quat, omega=s.omega, f_disturb=s.f_disturb, pos_tar=s.pos_tar, vel_tar=s.vel_tar,
              acc_tar=s.acc_tar)
    if traj:
        kw.update(pos_traj=s.pos_traj, vel_traj=s.vel_traj, acc_traj=s.acc_traj)
    kw = {k: np.ascontiguousarray(v, dtype=f32) for k, v in kw.items()}
    return template.replace(time=int(s.time), **kw, **(dict(traj_dev=None) if traj else {}))


def test_plan_trace_at_far_fast():
    """One step of a compute_plan controller planning from far_fast: the plan row through tests/test_gpu_trace.py's checker."""
    env = quad_env(task="tracking_zigzag")
    c, cp = build_with_discount(env, "mppi", 1024)
    cp, obs, info, state, params = start_episode(env, c, cp, "mppi")
    ns = _env_state(info["noisy_state"], atlas_state("far_fast")[0])
    k_act = cr.split(cr.PRNGKey(7), 3)[1]
    u, cp, cinfo = c(obs, state, params, k_act, cp, dict(info, noisy_state=ns))
    torch.cuda.synchronize()
    check_plan_against_oracle(env, "mppi", params, ns, k_act, cp, cinfo, "mppi N=1024 far_fast")
    assert c.core.device_status() == 0
    c.core.close()


# ------------------------------------------------------------------------------------------ e: Hessian
@functools.lru_cache(maxsize=None)
def _hessian_case(name, scale):
    """(s, a, ref, {method: device Hessian}) -- computed once, shared by the Hessian, batch and Sigma tests"""
    s, p, rng = atlas_state(name)
    a = perturbed_hover_mean(p, rng, scale)
    ref = CO.hessian(s, p, a.astype(np.float64), 32)
    core = _core(256, 1.0)
    ds = dev_state(s)
    dev = {m: core.hessian(ds.packed, ds, EnvParams3D().to_c(), torch.from_numpy(a).to(DEV), method=m)[0].cpu().numpy()
           for m in ("adjoint", "pairs")}
    return s, a, ref, dev


def _check_hessian(Rm, ref, where, rel=1e-9):
    err, big = np.abs(Rm - ref).max(), np.abs(ref).max()
    print(f"  {where}: |R - ref| {err:.2e}, max|ref| {big:.3g}, relative {err / max(1.0, big):.2e}")
    assert np.all(np.isfinite(ref)), where
    assert np.array_equal(Rm, Rm.T), where
    assert np.all(Rm[124:] == 0.0) and np.all(Rm[:, 124:] == 0.0), where
    assert err < rel * max(1.0, big), (where, err, big)


@pytest.mark.parametrize("scale", [0.1, 0.5])
@pytest.mark.parametrize("name", NAMES)
def test_hessian_at_every_entry(name, scale):
    s, a, ref, dev = _hessian_case(name, scale)
    assert np.abs(ref[13]).max() > 0  # the tie rows are live
    for method in ("adjoint", "pairs"):
        _check_hessian(dev[method], ref, f"{name} scale={scale} {method}")


@pytest.mark.parametrize("kind,reward", [("drag", "penyaw"), ("periodic", "realworld")])
@pytest.mark.parametrize("name", ["far_fast", "roll_120_spin", "yaw_cross"])
def test_hessian_model_variants_off_hover(name, kind, reward):
    """drag: the adjoint kernels' 16-component instantiation (the force is part of the differentiated state, |rel| kink); periodic
    + realworld: a held / redrawn force table and the other reward.  The force-table plumbing and bars of
    tests/test_gpu_models.py::test_hessian_reward_and_disturbance_variants_vs_ad_oracle."""
    s, p, rng = atlas_state(name)
    p = p.replace(disturb_params=DP)
    a = perturbed_hover_mean(p, rng, 0.1)
    key = cr.PRNGKey(21)
    core = _core(256, 1.0)
    ds, pc = dev_state(s), params_c(p, kind, reward)
    tab = core.disturb_table(pc, ds.packed, key=key, key_mode=_lib.DISTURB_KEYS_HESSIAN, deterministic=True)
    draws = uniform_draws(p, key, _lib.DISTURB_KEYS_HESSIAN).astype(np.float64)
    ref = CO.hessian(s, p, a.astype(np.float64), 32, reward=reward, kind=kind, draws=draws)
    ref_t = CO.hessian(s, p, a.astype(np.float64), 32, reward=reward, kind=kind, table=tab[0].cpu().numpy())
    other = CO.hessian(s, p, a.astype(np.float64), 32)
    assert np.abs(other - ref).max() > 1e-6  # the variant matters
    for method in ("adjoint", "pairs"):
        Rm = core.hessian(ds.packed, ds, pc, torch.from_numpy(a).to(DEV), method=method, f_steps=tab)[0].cpu().numpy()
        _check_hessian(Rm, ref_t, f"{name} {kind} {reward} {method} (oracle on the table)")
        _check_hessian(Rm, ref, f"{name} {kind} {reward} {method} (oracle on the model functions)", rel=2e-8)


def test_hessian_batch_of_all_entries_equals_single_calls():
    """All 12 entries as one batch (>= 8: the split adj_hd_kernel launches): bit-equal to the 12 single calls."""
    cases = [_hessian_case(name, 0.1) for name in NAMES]
    core = _core(256, 1.0)
    packed = torch.stack([dev_state(c[0]).packed for c in cases])
    am = torch.stack([torch.from_numpy(c[1]).to(DEV) for c in cases])
    for method in ("adjoint", "pairs"):
        Rb = core.hessian(packed, dev_state(cases[0][0]), EnvParams3D().to_c(), am, batch=len(cases), method=method).cpu().numpy()
        for i, name in enumerate(NAMES):
            assert np.array_equal(Rb[i], cases[i][3][method]), (method, name, np.abs(Rb[i] - cases[i][3][method]).max())
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ f: Sigma
@pytest.mark.parametrize("method", ["ns", "jacobi"])
def test_sigma_of_the_atlas_hessians(method):
    """The device Hessians of the 11 benign entries as one batched covo_sigma call against eigh-based optimize_sigma of the same
    matrices: 1e-6 relative Frobenius.  near_singular (cond(Sigma)^2 ~ 1e5..1e6, outside the range the suite covers): printed,
    finite and symmetric only."""
    mats = [_hessian_case(name, 0.1)[3]["adjoint"] for name in BENIGN]
    core = _core(256, 1.0)
    Sigma, L = core.sigma(torch.from_numpy(np.ascontiguousarray(np.stack(mats))).to(DEV), 0.5, batch=len(mats), method=method)
    Sigma, L = Sigma.cpu().numpy(), L.cpu().numpy()
    for i, name in enumerate(BENIGN):
        ref = R.optimize_sigma(mats[i], 0.5, 32, 4)
        err = np.linalg.norm(Sigma[i] - ref) / np.linalg.norm(ref)
        w = np.linalg.eigvalsh(ref)
        print(f"  {name} {method}: Sigma rel err {err:.2e}, cond(Sigma)^2 {(w[-1] / w[0]) ** 2:.3g}")
        assert err < 1e-6, (name, err)
        assert np.array_equal(Sigma[i], Sigma[i].T) and np.all(np.triu(L[i], 1) == 0), name
    Rn = _hessian_case("near_singular", 0.1)[3]["adjoint"]
    Sn, Ln = core.sigma(torch.from_numpy(np.ascontiguousarray(Rn[None])).to(DEV), 0.5, batch=1, method=method)
    Sn = Sn[0].cpu().numpy()
    ref = R.optimize_sigma(Rn, 0.5, 32, 4)
    w = np.linalg.eigvalsh(ref)
    print(f"  near_singular {method}: Sigma rel err {np.linalg.norm(Sn - ref) / np.linalg.norm(ref):.2e}, "
          f"cond(Sigma)^2 {(w[-1] / w[0]) ** 2:.3g} (not asserted)")
    assert np.all(np.isfinite(Sn)) and np.array_equal(Sn, Sn.T)
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ g: env step
@pytest.mark.parametrize("name", ["inverted", "roll_120_spin", "far_fast", "near_singular", "yaw_pi_minus", "yaw_3quarter_neg"])
def test_env_step_kernel_vs_host_env_off_hover(name):
    """tests/test_gpu_parity.py::test_env_step_kernel_vs_host_env from the atlas state with actions the env's clip cuts.  The two
    yaw entries keep yd < 0 for the whole run: the logged reward is the only user of the fp32 qm::atan2abs_ (the rollouts have
    rollout_pipe.hpp's own body), and a roll or a decaying spin alone never takes it into its x < 0 branch."""
    import covo_mpc_amd as cm
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    core = _core(256, 1.0)
    ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(11), params, (core.lib, core.h), DEV)
    obs, info, state = env.reset(cr.PRNGKey(11), params)
    state = _env_state(state, atlas_state(name)[0], traj=False)
    ep.true.copy_(torch.from_numpy(state.pack()).to(DEV))
    rng = np.random.default_rng(5)
    key = cr.PRNGKey(12)
    rewards, errs, dones, worst, clipped = [], [], [], 0.0, 0
    for t in range(20):
        key, k_step = cr.split(key)
        u = np.clip(np.array([-0.3378, 0, 0, 0]) + 0.8 * rng.normal(size=4), -1.2, 1.2).astype(f32)
        clipped += int(np.any(np.abs(u) > 1.0))
        ep.step(k_step, torch.from_numpy(u).to(DEV))
        obs, state, reward, done, info = env.step(k_step, state, u, params)
        rewards.append(reward)
        errs.append(info["err_pos"])
        dones.append(float(done))
        t_dev, n_dev = ep.true.cpu().numpy(), ep.noisy.cpu().numpy()
        want, want_n = state.pack(), info["noisy_state"].pack()
        assert t_dev[25:26].view(np.int32)[0] == state.time
        d = max((np.abs(t_dev[:25] - want[:25]) / np.maximum(1.0, np.abs(want[:25]))).max(),
                (np.abs(n_dev[:25] - want_n[:25]) / np.maximum(1.0, np.abs(want_n[:25]))).max())
        worst = max(worst, d)
        assert d < 2e-5, (name, t, d)
        kp, kv, kq, ko = cr.split(cr.split(cr.split(k_step)[0])[0], 5)[:4]  # the noise itself is bit-exact (see the test named above)
        s_ = f32(params.obs_noise_scale)
        for sl, kk, n_, c_ in ((slice(0, 3), kp, 3, 0.25), (slice(3, 6), kv, 3, 0.5), (slice(6, 10), kq, 4, 0.02), (slice(10, 13), ko, 3, 0.5)):
            assert np.array_equal(n_dev[sl], (t_dev[sl] + cr.normal(kk, (n_,)) * s_ * f32(c_)).astype(f32)), (name, t, sl)
    log = ep.read_log()
    dr, de = np.abs(log[:, 0] - np.asarray(rewards)).max(), np.abs(log[:, 1] - np.asarray(errs)).max()
    print(f"  {name}: state {worst:.2e} reward {dr:.2e} err_pos {de:.2e}; {clipped} of 20 actions clipped")
    assert log.shape == (20, 4) and dr < 2e-5 and de < 2e-5 and np.array_equal(log[:, 3], np.asarray(dones, dtype=f32))
    assert clipped > 0


@pytest.mark.parametrize("trial,name", [(0, "inverted"), (1, "double_cover"), (2, "yaw_pi_plus")])
def test_env_step_rollover_triggers_the_auto_reset(trial, name):
    """disable_rollover_terminate=False and a pre-step state that is terminal by quat[3] < cos(pi/4) alone (inside the box, inside
    the episode): covo_env_step stores reset_env(key_reset)'s state, its noisy copy, a new trajectory and done = 1 -- compared with
    the Python env's step on the same key as tests/test_gpu_reset.py::test_device_reset_vs_host_reset_env compares its box resets
    (same keys as its trials 0, 1 and 2, hence the same new trajectories and the same cap on elements one ulp apart)."""
    import covo_mpc_amd as cm
    env = quad_env(task="tracking_zigzag", rollover=True)
    params = env.default_params.replace(disturb_scale=0.3)
    core = _core(256, 1.0)
    ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(11 + trial), params, (core.lib, core.h), DEV)
    obs, info, state = env.reset(cr.PRNGKey(11 + trial), params)
    s = atlas_state(name)[0]
    state = _env_state(state, s, traj=False)
    assert np.abs(state.pos).max() < 3.0 and state.time < 300 and state.quat[3] < np.cos(np.pi / 4) and env.is_terminal(state, params)
    ep.true.copy_(torch.from_numpy(state.pack()).to(DEV))
    k_step = cr.split(cr.PRNGKey(500 + trial))[1]
    u = np.array([-0.3, 0.1, -0.1, 0.05], dtype=f32)
    ep.step(k_step, torch.from_numpy(u).to(DEV))
    obs, st_h, reward, done, info = env.step(k_step, state, u, params)
    assert done and st_h.time == 0
    traj_d = [t.cpu().numpy() for t in (ep.pos_traj, ep.vel_traj, ep.acc_traj)]
    differing = 0
    for d, h in zip(traj_d, [st_h.pos_traj, st_h.vel_traj, st_h.acc_traj]):
        assert d.shape == h.shape and ulps(d, h) <= 1.0, (name, ulps(d, h))
        differing += int(np.sum(d != h))
    assert differing <= 2, differing
    t_dev, n_dev = ep.true.cpu().numpy(), ep.noisy.cpu().numpy()
    want = st_h.pack()
    assert np.array_equal(t_dev[:16], want[:16]) and np.array_equal(t_dev[25:], want[25:]), name
    assert np.array_equal(t_dev[6:10], np.array([0, 0, 0, 1], dtype=f32)) and np.abs(t_dev[13:16]).max() > 0
    assert np.array_equal(t_dev[16:25], np.concatenate([traj_d[0][0], traj_d[1][0], traj_d[2][0]]))
    n_host = info["noisy_state"].pack()
    assert np.array_equal(n_dev[:16], n_host[:16]) and np.array_equal(n_dev[16:], t_dev[16:]), name
    log = ep.read_log()
    assert log.shape == (1, 4) and log[0, 3] == 1.0
    assert abs(log[0, 0] - reward) < 2e-5 * max(1.0, abs(reward)), (log[0, 0], reward)  # the reward of the TERMINAL state
    assert abs(log[0, 1] - info["err_pos"]) < 1e-6 and abs(log[0, 2] - info["err_vel"]) < 1e-6  # errors of the RESET state
    assert not np.array_equal(traj_d[0], ep.state0.pos_traj)  # a NEW trajectory
    # the same state with the rollover test off is not terminal: the vehicle flies on
    env0 = quad_env(task="tracking_zigzag")
    ep0 = cm.envs.DeviceEpisode(env0, cr.PRNGKey(11 + trial), params, (core.lib, core.h), DEV)
    ep0.true.copy_(torch.from_numpy(state.pack()).to(DEV))
    ep0.step(k_step, torch.from_numpy(u).to(DEV))
    assert ep0.read_log()[0, 3] == 0.0 and ep0.true.cpu().numpy()[25:26].view(np.int32)[0] == state.time + 1


# ------------------------------------------------------------------------------------------ h: PID nominal
@pytest.mark.parametrize("name", ["inverted", "far_fast", "unnorm_q"])
def test_pid_nominal_device_vs_host_off_hover(name):
    """tests/test_gpu_parity.py::test_offline_nominal_trajectory_device_vs_host with the reset state's attitude, body rates, position
    and velocity replaced (its own trajectory and targets kept): the PID law with the thrust clipped at 0, a large e3 x z_d angle,
    an inverted / non-unit Q."""
    import covo_mpc_amd as cm
    env = quad_env(task="tracking_zigzag")
    controller, cp = cm.envs.get_controller(env, "covo-offline", "N1024_H32_lam0.01", device=DEV)
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(31), params)
    s = atlas_state(name)[0]
    state = state.replace(**{k: np.ascontiguousarray(getattr(s, k), dtype=f32) for k in ("quat", "omega", "pos", "vel")})
    ph, ah = controller._nominal_host(state, params, cr.PRNGKey(32))
    pd, ad, _ = controller._nominal_device(state, params, cr.PRNGKey(32))
    pd, ad = pd.cpu().numpy(), ad.cpu().numpy()
    assert np.array_equal(pd[:, 25].view(np.int32), ph[:, 25].view(np.int32))      # time
    ds_, da_ = np.abs(pd[:, :25] - ph[:, :25]).max(), np.abs(ad - ah).max()
    clips = int(np.sum(ah[:, 0::4] == -1.0))
    print(f"  {name}: states {ds_:.2e} means {da_:.2e}; thrust clipped at 0 in {clips} nominal steps; max |action| {np.abs(ah).max():.1f}")
    assert ds_ < 5e-5, ds_
    assert da_ < 2e-4, da_
    assert clips > 0 and np.any(ad[:, 0::4] == -1.0)  # not vacuous: the thrust clip at 0 is live on both sides
    assert np.abs(ph[:, 0:3]).max() < 3.0  # the chain stays inside the box
    controller.core.close()


# ------------------------------------------------------------------------------------------ i: one production step per mode
@pytest.mark.parametrize("state_name", ["inverted", "far_fast", "yaw_pi_minus"])
@pytest.mark.parametrize("name,N", [("covo-online", 4096), ("mppi", 1024)])
def test_production_step_from_an_upset_state(name, N, state_name):
    """One fused control step (the plumbing of tests/test_gpu_parity.py::test_controller_step_teacher_forced, production path) whose
    noisy state is the atlas entry: cost, Sigma and mean through _oracle_check_of_a_fused_step."""
    import covo_mpc_amd as cm
    env = quad_env(task="tracking_zigzag")
    controller, cp = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV)
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(1), params)
    cp = controller.reset(state, params, controller.init_control_params, cr.PRNGKey(2))
    ns = _env_state(info["noisy_state"], atlas_state(state_name)[0])
    k_act = cr.split(cr.PRNGKey(3), 3)[1]
    am_before = cp.a_mean.cpu().numpy().copy()
    u, cp_new, cinfo = controller(obs, state, params, k_act, cp, dict(info, noisy_state=ns))
    torch.cuda.synchronize()
    assert controller.core.device_status() == 0
    _oracle_check_of_a_fused_step(name, env, params, ns, am_before, k_act, controller.core, cp_new, "0.01")
    assert np.array_equal(u.cpu().numpy(), cp_new.a_mean[0].cpu().numpy()) and np.all(np.isfinite(cinfo["pos_mean"].cpu().numpy()))
    controller.core.close()
