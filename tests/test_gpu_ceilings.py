"""GPU tests (-m gpu) at the documented ceilings of the step options: 64 env instances (COVO_MAX_ENVS; and 33, the first count above
what the other modules run), 16 passes per step (COVO_MAX_STEP_ITERS), a Sigma period of 64 (COVO_MAX_SIGMA_PERIOD: 63 reuse steps
in a row, shifted or adapted), a fan of 64 inside a batched step (COVO_FAN_MAX).  The subject is the instance, pass or period axis:
the sample counts are the smallest the other modules use (N = 40, 100, 256), the bodies are theirs, called with the larger argument.

Bars.  Everything in a step is equality of bits, as in the modules the bodies come from.  The stand-alone chains:
  one step    against the fp64 restatement of the step's OWN fp32 input at the one-step bars of tests/test_gpu_sigma_period.py
              (L' 3e-6, Sigma' 1e-6), at k = 1, 2, 3, 16, 30, 31, 32, 63
  log det     |2 sum log L'_ii - 2 n log sigma| <= 2 n 2^-24 at EVERY k: the bar is derived per step (each diagonal entry of the
              fp32 L' within 2^-24 relative of an fp64 one whose log det is exact) and every step renormalises -- nothing accumulates
  k shifts    against the closed form c_k S^k(Sigma) of the ORIGINAL fp32 factor (tests/sigma_shift_oracle.py::shift_power_ref):
              one one-step bar plus twice what the restatement's own fp32 chain (shift_chain_ref) is off by at the same k.  Two
              chains that round L' to fp32 at every step, each started from the same factor, are both that far from the exact answer;
              the kernel gets one more one-step bar for its own arithmetic.  The bar is computed, not chosen: the module fixture
              measures the reference chain first.
The worst ratios are printed and quoted in DESIGN.md 4.16 / 4.18."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from tests.gpu_cases import (CASES, _batched_iters_case, _batched_period_case, _batched_step_equals_replicas,  # noqa: E402
                             _definition_case, _mode_step_equals_replicas, _period_case, _run_episode_case, check_shift,
                             check_structure, errors, g32)
from tests.gpu_support import DEV, ST_TIME, batched_controller, instances, quad_env  # noqa: E402
from tests.sigma_shift_oracle import (BAR_L, BAR_LOGDET, BAR_SIGMA, N_A, adapt_ref, chain_ratios, decoupled_rows,  # noqa: E402
                                      off_structure, random_spd_factors, shift_chain_ref, shift_factor_ref, shift_power_ref)

HERE = os.path.dirname(os.path.abspath(__file__))
SIGMA = 0.5
E_MAX, K_MAX, M_MAX, FAN_MAX = _lib.COVO_MAX_ENVS, _lib.COVO_MAX_STEP_ITERS, _lib.COVO_MAX_SIGMA_PERIOD, _lib.COVO_FAN_MAX
CHAIN = M_MAX - 1                       # reuse steps in a row at the largest period
ONE_STEP_AT = (1, 2, 3, 16, 30, 31, 32, 63)
GOLDEN = (0, 5, 9, 13)
NAMES = ["sigma I"] + [f"golden {i}" for i in GOLDEN] + ["random_spd 6e2", "random_spd 7e4"]
ADAPT_CLOUDS = ((257, 0.5), (5, 0.05))  # (samples, lam) of the posterior covariance; 5 samples: rank <= 4


def test_the_ceilings_are_the_documented_ones():
    assert (E_MAX, K_MAX, M_MAX, FAN_MAX) == (64, 16, 64, 64) and _lib.check_iters(K_MAX) == K_MAX and _lib.check_fan(FAN_MAX, 256) == FAN_MAX
    for bad in (lambda: _lib.check_iters(K_MAX + 1), lambda: _lib.check_fan(FAN_MAX + 1, 256), lambda: _lib.check_sigma_period(M_MAX + 1)):
        with pytest.raises(ValueError):
            bad()


# ---- a, b: 63 reuse steps in a row, stand-alone ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core():
    c = SamplingCore(256, 32, 0.01, 1.0, device=DEV, use_graph=False, compute_info=False)
    yield c
    c.close()


@pytest.fixture(scope="module")
def chain_inputs(core):
    """L [7] fp32: sigma I, covo_sigma's factors of golden Hessians 0, 5, 9, 13, the two random_spd factors; per input and k <= 63 the
    closed form (Sigma_k, L_k) of the original factor and what the restatement's own fp32 chain is off it by, (L', Sigma') as
    multiples of the one-step bars -- computed once."""
    g = np.load(os.path.join(HERE, "golden", "hessians_r03.npz"))
    Rm = np.stack([np.ascontiguousarray(m) for k in g.files for m in g[k]])[list(GOLDEN)]
    _, Lg = core.sigma(torch.from_numpy(Rm).to(DEV), SIGMA, batch=len(GOLDEN))
    torch.cuda.synchronize()
    L = np.concatenate([(SIGMA * np.eye(N_A, dtype=np.float32))[None], Lg.cpu().numpy(), np.stack(random_spd_factors())])
    assert L.shape == (len(NAMES), N_A, N_A) and L.dtype == np.float32
    closed, own = [], np.zeros((len(L), CHAIN + 1, 2))
    for i, l in enumerate(L):
        Sigma0 = l.astype(np.float64) @ l.astype(np.float64).T
        refs = [None]
        for k, (Sp, Lp) in enumerate(shift_chain_ref(l, CHAIN, SIGMA, every=True), start=1):
            Sref = shift_power_ref(Sigma0, k, SIGMA)
            Lref = np.linalg.cholesky(Sref)
            refs.append((Sref, Lref))
            own[i, k] = chain_ratios(Sp.astype(np.float32), Lp.astype(np.float32), Sref, Lref, SIGMA)[1:]
        closed.append(refs)
    return L, closed, own


def test_63_shifts_in_place_against_the_closed_form(core, chain_inputs):
    """The seven factors as one batch through covo_sigma_shift in place 63 times (what a step at sigma_period = 64 does between two
    refreshes).  Every k: the exact zero structure -- after k shifts the trailing min(k, 31) stages are decoupled 4 x 4 blocks --,
    Sigma' symmetric bit for bit, the log det bar, and L', Sigma' against the closed form of the original factor.  The listed k: the
    step against the restatement of its own input.  k = 63: a batch row is the single launch bit for bit."""
    L, closed, own = chain_inputs
    n = len(L)
    Lb = torch.from_numpy(L).to(DEV).contiguous()
    So = torch.empty_like(Lb)
    worst_bar, worst_one, worst_ld = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n)
    for k in range(1, CHAIN + 1):
        L_in = Lb.clone()
        _lib.check(core.lib.covo_sigma_shift(core.h, _lib.ptr(Lb), n, SIGMA, _lib.ptr(So), _lib.ptr(Lb), core.stream()), "covo_sigma_shift")
        torch.cuda.synchronize()
        Sh, Lh = So.cpu().numpy(), Lb.cpu().numpy()
        m, off = decoupled_rows(k), off_structure(k)
        for i in range(n):
            where = (NAMES[i], k)
            assert np.all(np.isfinite(Sh[i])) and np.all(np.isfinite(Lh[i])) and np.all(np.diag(Lh[i]) > 0), where
            assert np.all(np.triu(Lh[i], 1) == 0.0) and np.all(Lh[i][m:, :m] == 0.0) and not Lh[i][off].any(), where
            assert np.array_equal(Sh[i], Sh[i].T) and not Sh[i][off].any(), where
            Sref, Lref = closed[i][k]
            r = chain_ratios(Sh[i], Lh[i], Sref, Lref, SIGMA)
            worst_ld[i] = max(worst_ld[i], r[0])
            assert r[0] <= 1.0, (where, r[0] * BAR_LOGDET)
            bars = 1.0 + 2.0 * own[i, k]  # in one-step bars
            worst_one[i] = np.maximum(worst_one[i], r[1:])
            worst_bar[i] = np.maximum(worst_bar[i], r[1:] / bars)
            assert np.all(r[1:] <= bars), (where, r[1:] * (BAR_L, BAR_SIGMA), bars * (BAR_L, BAR_SIGMA))
        if k in ONE_STEP_AT:
            Lih = L_in.cpu().numpy()
            for i in range(n):
                check_shift(Sh[i], Lh[i], shift_factor_ref(Lih[i], SIGMA), (NAMES[i], "step", k))
        if k == CHAIN:
            for i in range(n):
                S1, L1 = core.sigma_shift(L_in[i].contiguous(), SIGMA)
                assert torch.equal(S1, So[i]) and torch.equal(L1, Lb[i]), NAMES[i]
    assert np.abs(Sh[0] - SIGMA ** 2 * np.eye(N_A)).max() < 1e-6  # sigma^2 I stays what it is
    for i in range(n):
        print(f"  {NAMES[i]}: 63 shifts against the closed form, worst over k -- L' {worst_one[i, 0]:.2f}, Sigma' {worst_one[i, 1]:.2f} "
              f"one-step bars (own fp32 chain of the restatement: {own[i, :, 0].max():.2f}, {own[i, :, 1].max():.2f}); of the bar "
              f"1 + 2 x that: {worst_bar[i, 0]:.2f}, {worst_bar[i, 1]:.2f}; log det {worst_ld[i]:.2f}")
    assert core.device_status() == 0


@pytest.fixture(scope="module")
def adapt_clouds(core, chain_inputs):
    """Per cloud (N, lam) one posterior covariance per factor (core.weighted_cov of N samples clip(L eps) under random costs, as
    tests/test_gpu_sigma_adapt.py builds them), fixed over the chain."""
    L = torch.from_numpy(chain_inputs[0]).to(DEV).contiguous()
    n = L.shape[0]
    gen = torch.Generator(device=DEV).manual_seed(5)
    Cs = {}
    for N, lam in ADAPT_CLOUDS:
        eps = torch.randn((n, N, N_A), device=DEV, generator=gen)
        x = torch.clamp(eps @ L.transpose(1, 2), -1.0, 1.0)
        a = x.view(n, N, 32, 4).permute(0, 2, 1, 3).contiguous()
        cost = torch.randn((n, N), device=DEV, generator=gen)
        Cs[(N, lam)] = core.weighted_cov(a, cost, torch.zeros((n, N_A), device=DEV), lam=lam)[0].contiguous()
    torch.cuda.synchronize()
    sv = np.linalg.svd(Cs[(5, 0.05)][1].double().cpu().numpy(), compute_uv=False)
    # five samples about their weighted mean: rank <= 4 up to the fp32 rounding of the entries.  The samples are clipped to [-1, 1], so
    # an entry of sum w y y^T / W is at most 1 and carries a few 2^-24 of rounding; 128 such entries bound the spectral norm of the noise
    assert sv[4] <= 4 * N_A * 2.0 ** -24, sv[:6]
    return L, Cs


@pytest.mark.parametrize("gamma", [0.5, 0.9])
@pytest.mark.parametrize("cloud", ADAPT_CLOUDS, ids=lambda c: f"N{c[0]}-lam{c[1]}")
def test_63_adapts_in_place(core, adapt_clouds, cloud, gamma):
    """covo_sigma_adapt in place 63 times with a fixed C per factor.  Every step: no fallback, everything finite, the zero structure,
    symmetry, the log det bar.  The listed k: the step against the restatement of its own fp32 input at the one-step bars.  The
    rank-4 C at gamma = 0.9 drives cond(Sigma') from below 3e2 to 1.9e6 over the chain (golden Hessian 13): the factorisation inside the
    kernel is the one thing between two reuse steps, and this is the hardest matrix it gets."""
    L0, Cs = adapt_clouds
    Cb = Cs[cloud]
    Ch = Cb.cpu().numpy()
    n = L0.shape[0]
    Lb = L0.clone()
    worst, worst_ld, cond = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    for k in range(1, CHAIN + 1):
        L_in = Lb.clone() if k in ONE_STEP_AT else None
        Sp, Lout, rows = core.sigma_adapt(Lb, Cb, gamma, SIGMA, L_out=Lb)
        torch.cuda.synchronize()
        assert Lout is Lb
        Sh, Lh, rh = Sp.cpu().numpy(), Lb.cpu().numpy(), rows.cpu().numpy()
        assert np.all(rh[:, 0] == 0.0) and np.all(np.isfinite(rh)), (cloud, gamma, k, rh[:, 0])
        for i in range(n):
            where = (cloud, gamma, NAMES[i], k)
            check_structure(Sh[i], Lh[i], where)
            e_ld = abs(2.0 * np.log(np.diag(Lh[i].astype(np.float64))).sum() - 2.0 * N_A * np.log(SIGMA))
            worst_ld[i] = max(worst_ld[i], e_ld / BAR_LOGDET)
            assert e_ld <= BAR_LOGDET, (where, e_ld)
            if L_in is not None:
                ref = adapt_ref(L_in[i].cpu().numpy(), Ch[i], g32(gamma), SIGMA)
                assert ref[2] == 0, where
                e = np.array(errors(Sh[i], Lh[i], ref))
                worst[i] = np.maximum(worst[i], e)
                assert e.max() <= 1.0, (where, e)
                cond[i] = max(cond[i], np.linalg.cond(ref[0]))
    i = int(np.argmax(cond))
    print(f"  C of {cloud}, gamma {gamma}: 63 adapts of {n} factors, worst ratio to the one-step bars at k in {ONE_STEP_AT} -- log det "
          f"{worst[:, 0].max():.2f} (every k: {worst_ld.max():.2f}), L' {worst[:, 1].max():.2f}, Sigma' {worst[:, 2].max():.2f}; "
          f"cond(Sigma') up to {cond[i]:.1e} ({NAMES[i]})")
    assert core.device_status() == 0


# ---- c: sigma_period = 64 inside the step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_period_64_over_two_periods(graph, monkeypatch):
    """130 steps at m = 64, N = 256: sigma_age == step % 64; each of the 2 x 63 + 1 reuse steps is core.sigma_shift of the previous
    factor and covo_noise_gemm_philox with it, bit for bit; steps 0, 64 and 128 are a plain controller's from the same mean."""
    _period_case(M_MAX, 2 * M_MAX + 2, graph, monkeypatch)


@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_period_64_adapting_over_two_periods(graph, monkeypatch):
    """The same run with sigma_adapt = 0.9: every reuse step is core.sigma_adapt of the previous factor and the previous step's
    posterior covariance bit for bit, reports that call's flag and scale, and leaves a finite mean."""
    _period_case(M_MAX, 2 * M_MAX + 2, graph, monkeypatch, gamma=0.9)


def test_period_64_batched_equals_single():
    """E = 2, m = 64, 66 steps -- through one whole period and the next refresh."""
    _batched_period_case(2, 256, M_MAX, M_MAX + 2)


# ---- d: iters = 16 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["graph", "eager"])
@pytest.mark.parametrize("name,N", [("mppi", 100), ("covo-offline", 40), ("covo-online", 256)])
def test_16_pass_step_equals_its_definition(name, N, graph, monkeypatch):
    """One captured graph holding 16 passes; the [1, 16] iteration log; the key walked 15 times on the device."""
    _definition_case(name, N, K_MAX, graph, monkeypatch)


@pytest.mark.parametrize("name,N", [("mppi", 100), ("covo-offline", 40), ("covo-online", 256)])
def test_batched_16_passes_equal_replicas(name, N):
    _batched_iters_case(name, N, 2, K_MAX)


def test_run_episode_with_16_passes_equals_the_python_loop():
    _run_episode_case(K_MAX, 4)


# ---- e: 64 (and 33) env instances ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [33, E_MAX])
@pytest.mark.parametrize("name,N,lam,rollover", [c for c in CASES if c[1] <= 100])
def test_batched_mode_step_equals_replicas_at_the_ceiling(name, N, lam, rollover, E, monkeypatch):
    """MPPI N = 100 and covo-offline N = 40: instance e of 3 batched steps (eager, capture, replay) is the single controller's."""
    _mode_step_equals_replicas(name, N, lam, rollover, E, "graph", monkeypatch)


@pytest.mark.parametrize("E", [33, E_MAX])
def test_batched_online_step_equals_replicas_at_the_ceiling(E):
    _batched_step_equals_replicas(256, E, 3)


def test_batched_env_step_of_64_equals_the_single_kernel():
    """covo_env_step_batched, E = 64, 4 steps: every instance's true and noisy state and log equal covo_env_step on it alone."""
    E = E_MAX
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(900 + e)) for e in range(E)]
    core = SamplingCore(256, 32, 0.01, 1.0, device=DEV)
    keys0 = [cr.PRNGKey(1000 + e) for e in range(E)]
    ep = cm.envs.BatchedDeviceEpisode(env, keys0, params, (core.lib, core.h), DEV)
    singles = [cm.envs.DeviceEpisode(env, keys0[e], params[e], (core.lib, core.h), DEV) for e in range(E)]
    rng = np.random.default_rng(7)
    key = cr.PRNGKey(77)
    a_mean = torch.zeros((E, 128), dtype=torch.float32, device=DEV)
    for t in range(4):
        key, sub = cr.split(key)
        step_keys = np.asarray(cr.split(sub, E))
        u = np.clip(np.array([-0.3378, 0, 0, 0]) + 0.3 * rng.normal(size=(E, 4)), -1.2, 1.2).astype(np.float32)
        a_mean[:, :4] = torch.from_numpy(u).to(DEV)
        ep.step(step_keys, a_mean)
        for e, se in enumerate(singles):
            se.step(step_keys[e], a_mean[e, :4].contiguous())
        torch.cuda.synchronize()
        for e, se in enumerate(singles):
            assert torch.equal(se.true, ep.true[e]) and torch.equal(se.noisy, ep.noisy[e]), (t, e)
    log = ep.read_log()
    assert log.shape == (E, 4, 4) and np.all(np.isfinite(log))
    for e, se in enumerate(singles):
        assert np.array_equal(se.read_log(), log[e]), e
    assert not np.array_equal(log[E - 1], log[0])
    core.close()


def test_run_episode_batched_of_64_equals_per_instance_episodes():
    """covo_run_episode_batched, covo-online N = 256, E = 64, 8 steps; instance 40 starts at step 294 of its episode, terminates
    and auto-resets inside the run.  Per instance: log, mean, Sigma, state, trajectory and key chain of covo_run_episode alone."""
    E, N, n, late_e = E_MAX, 256, 8, 40
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    c0, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    cp0 = c0.init_control_params
    c0.core.close()
    b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, discount=cp0.discount, gamma_mean=cp0.gamma_mean,
                                             sample_sigma=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=DEV)
    reset_keys = [cr.PRNGKey(150 + e) for e in range(E)]
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    late = torch.tensor([294], dtype=torch.int32, device=DEV).view(torch.float32)
    ep.true[late_e, ST_TIME:ST_TIME + 1] = late
    ep.noisy[late_e, ST_TIME:ST_TIME + 1] = late
    rngs0 = np.stack([np.asarray(cr.PRNGKey(160 + e)) for e in range(E)])
    rngs = b.run_episode(ep, rngs0, n)
    log = ep.read_log()
    assert log.shape == (E, n, 4)
    assert [int(log[e, :, 3].sum()) for e in range(E)] == [int(e == late_e) for e in range(E)]
    for e in range(E):
        c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
        c.alias_outputs = True
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        if e == late_e:
            se.true[ST_TIME:ST_TIME + 1] = late
            se.noisy[ST_TIME:ST_TIME + 1] = late
        cp = c.reset(se.state0, params[e], c.init_control_params, cr.PRNGKey(2))
        cp, rng = c.run_episode(se, params[e], cp, rngs0[e], n)
        assert np.array_equal(se.read_log(), log[e]), e
        assert torch.equal(cp.a_mean.reshape(-1), b.a_mean[e]) and torch.equal(cp.a_cov, b.a_cov[e]), e
        assert torch.equal(se.true, ep.true[e]) and torch.equal(se.pos_traj, ep.pos_traj[e]), e
        assert np.array_equal(np.asarray(rng, dtype=np.uint32), rngs[e]), e
        assert c.core.device_status() == 0
        c.core.close()
    assert b.core.device_status() == 0
    b.core.close()


ATTACHED = dict(compute_diag=True, compute_plan=True, compute_fan=FAN_MAX, update="guarded", compute_post_cov=True)
ROWS = (("diag", "diag"), ("plan", "plan"), ("fan", "fan"), ("arbiter", "arbiter"), ("lam_eff", "lam_eff"), ("elite", "elite_rows"),
        ("post_cov", "post_cov"), ("post_aux", "post_aux"))


@pytest.mark.parametrize("weights", [dict(ess_min=16.0), dict(elite=32)], ids=["ess_min", "elite"])
def test_one_step_of_64_with_every_attachment(weights):
    """One covo-online step of E = 64, N = 256 with diagnostics, plan, a fan of K = 64 ([64, 64, 100]), update="guarded", the posterior
    covariance and the ESS floor (or the elite set of 32) all attached: every [E, ...] row, the mean, Sigma, the costs and the
    actions of instance e are the single controller's with the same options on instance e alone, bit for bit."""
    E, N = E_MAX, 256
    opts = dict(ATTACHED, **weights)
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "covo-online", N, "0.01", E, **opts)
    b = batched_controller(env, "covo-online", inst, len(inst), N, 0.01, **opts)
    b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    assert tuple(b.fan.shape) == (E, FAN_MAX, _lib.COVO_FAN_FLOATS) == (64, 64, 100) and tuple(b.core.fan_idx.shape) == (E, FAN_MAX)
    assert tuple(b.post_cov.shape) == (E, N_A, N_A) and tuple(b.arbiter.shape) == (E, _lib.COVO_ARB_FLOATS) and b.diag.shape[0] == E
    assert (b.lam_eff is None) == ("elite" in weights) and (b.elite is None) == ("ess_min" in weights)
    k_acts = np.stack([np.asarray(cr.split(i["key"], 3)[1]) for i in inst])
    u_b = b([i["info"]["noisy_state"] for i in inst], k_acts).clone()
    torch.cuda.synchronize()
    for e, i in enumerate(inst):
        u, cp, _ = i["c"](i["obs"], i["state"], i["params"], k_acts[e], i["cp"], i["info"])
        torch.cuda.synchronize()
        core = i["c"].core
        assert torch.equal(u_b[e], u) and torch.equal(b.a_mean[e], cp.a_mean.reshape(-1)) and torch.equal(b.a_cov[e], cp.a_cov), e
        assert torch.equal(b._a[e], core.a) and torch.equal(b._cost[e], core.cost), e
        for mine, cores in ROWS:
            rows = getattr(b, mine)
            if rows is not None:
                got, want = rows[e].contiguous().view(torch.int32), getattr(core, cores)[0].contiguous().view(torch.int32)
                assert torch.equal(got, want), (e, mine)
        assert torch.equal(b.core.fan_idx[e], core.fan_idx[0]), e
        core.close()
    for mine, _ in ROWS:
        rows = getattr(b, mine)
        if rows is not None:
            assert bool(torch.isfinite(rows).all()) or mine in ("fan", "arbiter", "elite"), mine  # (those carry integer bit patterns)
            assert not torch.equal(rows[0], rows[E - 1]), mine  # different plants, different rows
    assert bool(torch.isfinite(b.a_mean).all()) and b.core.device_status() == 0
    b.core.close()
