"""GPU tests (-m gpu) of Sigma adapt (covo_set_step_sigma_adapt / covo_sigma_adapt; `sigma_adapt=gamma`): a reuse step of the Sigma
period samples from the shifted blend c ((1 - gamma) S(Sigma) + gamma S(C)) of the covariance the previous step sampled from and the
posterior covariance that step left (csrc/sigma_adapt.hip).

The reference is the fp64 numpy restatement of tests/test_sigma_adapt_abi.py, fed the kernel's own fp32 inputs L and C.  The bars are
the Sigma period's for the same quantities (tests/test_gpu_sigma_period.py) -- the kernel computes in fp64 and rounds
every output to fp32 once:
  L'      max |L' - L'_ref| / max |L'_ref| <= 3e-6
  Sigma'  max |Sigma' - Sigma'_ref| / max |Sigma'_ref| <= 1e-6
  log det |2 sum log L'_ii - 2 n log sigma| <= 2 n 2^-24 = 1.53e-5 (every diagonal entry of the fp32 L' is within 2^-24 relative of
          the fp64 one: at most n 2^-24 in the sum of logs, twice that in the log det)
The restatement itself, with L' rounded to fp32, is held to the same bars first, for every input.  Everything else is equality of
bits: batch against single launches, in place against out of place, a guarded instance against its own gamma = 0 launch, a reuse step
against the stand-alone call on the previous step's factor and posterior covariance, a batched row against the single controller,
the device episode against the Python loop."""
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
from tests.gpu_cases import check_structure, errors, g32  # noqa: E402
from tests.gpu_support import DEV, quad_env, single_controller  # noqa: E402
from tests.sigma_shift_oracle import BAR_L, BAR_LOGDET, BAR_SIGMA, N_A, adapt_ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SIGMA = 0.5
GAMMAS = (0.05, 0.5, 0.9)
CLOUDS = ((257, 0.5), (257, 0.05), (5, 0.5), (5, 0.05))  # (samples, lam) of the posterior covariances; 5 samples: rank <= 4
NL = 15


# ---- 1. the stand-alone kernel -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core():
    c = SamplingCore(256, 32, 0.01, 1.0, device=DEV, use_graph=False, compute_info=False)
    yield c
    c.close()


@pytest.fixture(scope="module")
def inputs(core):
    """L [15]: sigma I and covo_sigma's factors of the 14 matrices of tests/golden/hessians_r03.npz.  C: per cloud (N, lam), the
    posterior covariance (core.weighted_cov) of N samples clip(L eps) under random costs, one per L; plus C = 0.  The fp64 reference
    of every (C, gamma, L) -- computed once."""
    g = np.load(os.path.join(HERE, "golden", "hessians_r03.npz"))
    Rm = np.stack([np.ascontiguousarray(m) for k in g.files for m in g[k]])
    assert Rm.shape == (14, N_A, N_A)
    _, L = core.sigma(torch.from_numpy(Rm).to(DEV), SIGMA, batch=14)
    L = torch.cat([SIGMA * torch.eye(N_A, device=DEV)[None], L]).contiguous()
    gen = torch.Generator(device=DEV).manual_seed(5)
    Cs = {"zero": torch.zeros_like(L)}
    for N, lam in CLOUDS:
        eps = torch.randn((NL, N, N_A), device=DEV, generator=gen)
        x = torch.clamp(eps @ L.transpose(1, 2), -1.0, 1.0)                          # [15, N, 128], mean 0
        a = x.view(NL, N, 32, 4).permute(0, 2, 1, 3).contiguous()                     # [15, H, N, 4]
        cost = torch.randn((NL, N), device=DEV, generator=gen)
        Cs[(N, lam)] = core.weighted_cov(a, cost, torch.zeros((NL, N_A), device=DEV), lam=lam)[0].contiguous()
    torch.cuda.synchronize()
    Lh = L.cpu().numpy()
    refs = {(k, gm): [adapt_ref(Lh[i], Ch[i], g32(gm), SIGMA) for i in range(NL)]
            for k, Ch in ((k, v.cpu().numpy()) for k, v in Cs.items()) for gm in GAMMAS}
    return L, Cs, refs


def test_the_restatement_rounded_to_fp32_stays_inside_the_bars(inputs):
    """The reference's own L' and Sigma' after one rounding to fp32 against itself: what the bars leave to the kernel."""
    _, _, refs = inputs
    worst = np.zeros(3)
    for key, rs in refs.items():
        for i, r in enumerate(rs):
            assert r[2] == 0, (key, i)  # no input here makes the guard fire
            e = errors(r[0].astype(np.float32), r[1].astype(np.float32), r)
            worst = np.maximum(worst, e)
            assert max(e) <= 1.0, (key, i, e)
    print(f"  restatement in fp32, worst ratio to the bars: log det {worst[0]:.3f}, L' {worst[1]:.3f}, Sigma' {worst[2]:.3f}")


def test_adapt_alone_against_the_fp64_restatement(core, inputs):
    """Every C (four clouds and zero), every gamma, the 15 factors in one launch: bars against the restatement, the zero structure,
    symmetry, and rows = {0, c, log det M, 0}; each matrix launched alone gives the bits of its batch row."""
    L, Cs, refs = inputs
    worst = np.zeros(3)
    for key, Cb in Cs.items():
        for gm in GAMMAS:
            Sp, Lp, rows = core.sigma_adapt(L, Cb, gm, SIGMA)
            for i in range(NL):
                S1, L1, r1 = core.sigma_adapt(L[i].contiguous(), Cb[i].contiguous(), gm, SIGMA)
                assert torch.equal(S1, Sp[i]) and torch.equal(L1, Lp[i]) and torch.equal(r1, rows[i]), (key, gm, i)
            Sh, Lh, rh = Sp.cpu().numpy(), Lp.cpu().numpy(), rows.cpu().numpy()
            for i in range(NL):
                where = (key, gm, i)
                ref = refs[(key, gm)][i]
                check_structure(Sh[i], Lh[i], where)
                e = errors(Sh[i], Lh[i], ref)
                worst = np.maximum(worst, e)
                assert max(e) <= 1.0, (where, e)
                assert rh[i, 0] == 0.0 and rh[i, 3] == 0.0, where
                assert abs(rh[i, 1] - ref[3]) <= 1e-6 * ref[3] and abs(rh[i, 2] - ref[4]) <= 1e-6 * max(abs(ref[4]), 1.0), where
    print(f"  kernel, worst ratio to the bars: log det {worst[0]:.3f}, L' {worst[1]:.3f}, Sigma' {worst[2]:.3f}")
    # sigma^2 I with C = 0 stays sigma^2 I
    Sp, _, _ = core.sigma_adapt(L[0].contiguous(), Cs["zero"][0].contiguous(), 0.5, SIGMA)
    assert np.abs(Sp.cpu().numpy() - SIGMA ** 2 * np.eye(N_A)).max() < 1e-7


def test_gamma_zero_agrees_with_the_shift_kernel(core, inputs):
    """Two algorithms for one matrix (a fresh factorisation here, a rank-4 update there), each within one bar of the same reference:
    within two bars of each other.  C is not read at gamma = 0: NaNs there change nothing."""
    L, Cs, _ = inputs
    Sa, La, rows = core.sigma_adapt(L, torch.full_like(L, float("nan")), 0.0, SIGMA)
    Ss, Ls = core.sigma_shift(L, SIGMA)
    Sa, La, Ss, Ls = (t.double().cpu().numpy() for t in (Sa, La, Ss, Ls))
    assert np.all(rows.cpu().numpy()[:, 0] == 0.0)
    for i in range(NL):
        check_structure(Sa[i].astype(np.float32), La[i].astype(np.float32), i)
        e_L = np.abs(La[i] - Ls[i]).max() / np.abs(Ls[i]).max()
        e_S = np.abs(Sa[i] - Ss[i]).max() / np.abs(Ss[i]).max()
        e_ld = abs(2.0 * np.log(np.diag(La[i])).sum() - 2.0 * N_A * np.log(SIGMA))
        assert e_L <= 2 * BAR_L and e_S <= 2 * BAR_SIGMA and e_ld <= BAR_LOGDET, (i, e_L, e_S, e_ld)


def test_in_place_and_run_to_run(core, inputs):
    L, Cs, _ = inputs
    Cb = Cs[(257, 0.05)]
    Sp, Lp, rows = core.sigma_adapt(L, Cb, 0.5, SIGMA)
    S2, L2, rows2 = core.sigma_adapt(L, Cb, 0.5, SIGMA)
    assert torch.equal(Sp, S2) and torch.equal(Lp, L2) and torch.equal(rows, rows2)  # run equals run
    Lio = L.clone()
    S3, L3, rows3 = core.sigma_adapt(Lio, Cb, 0.5, SIGMA, L_out=Lio)                 # in place, as the step does it
    assert L3 is Lio and torch.equal(Lio, Lp) and torch.equal(S3, Sp) and torch.equal(rows3, rows)


@pytest.mark.parametrize("bad", ["nan", "indefinite"])
def test_guard_falls_back_per_instance(core, inputs, bad):
    """A batch of 3 whose middle instance has a C the blend cannot take -- one NaN entry, or -10 Sigma (M = -4.5 S(Sigma) at
    gamma = 0.5) -- in place: that instance's output is its own gamma = 0 launch bit for bit with flag 1, its neighbours equal their
    single launches with flag 0.  Finite work throughout: the guard is arithmetic, the launch completes normally."""
    L, Cs, _ = inputs
    Lb = L[3:6].contiguous()
    Cb = Cs[(257, 0.5)][3:6].clone()
    if bad == "nan":
        Cb[1, 40, 17] = float("nan")
    else:
        Cb[1] = -10.0 * (Lb[1] @ Lb[1].T)
    Lio = Lb.clone()
    Sp, Lp, rows = core.sigma_adapt(Lio, Cb, 0.5, SIGMA, L_out=Lio)
    S0, L0, r0 = core.sigma_adapt(Lb[1].contiguous(), Cb[1].contiguous(), 0.0, SIGMA)
    assert torch.equal(Sp[1], S0) and torch.equal(Lp[1], L0)
    assert bool(torch.isfinite(Sp).all()) and bool(torch.isfinite(Lp).all())
    rh = rows.cpu().numpy()
    assert rh[1, 0] == 1.0 and np.array_equal(rh[1, 1:], r0.cpu().numpy()[1:]) and r0.cpu().numpy()[0] == 0.0
    for e in (0, 2):
        S1, L1, r1 = core.sigma_adapt(Lb[e].contiguous(), Cb[e].contiguous(), 0.5, SIGMA)
        assert torch.equal(Sp[e], S1) and torch.equal(Lp[e], L1) and torch.equal(rows[e], r1) and rh[e, 0] == 0.0, e
    assert core.device_status() == 0


def test_adapt_alone_refuses_bad_arguments(core):
    Lb = torch.eye(N_A, device=DEV).contiguous()
    out = torch.empty(3, N_A, N_A, device=DEV)
    call = lambda L, Cm, batch, gm, sig, S, Lo: core.lib.covo_sigma_adapt(core.h, _lib.ptr(L), _lib.ptr(Cm), batch, gm, sig, _lib.ptr(S),
                                                                        _lib.ptr(Lo), None, core.stream())
    for batch, gm, sig in ((0, 0.5, 0.5), (1, 1.0, 0.5), (1, -0.1, 0.5), (1, 0.5, 0.0)):
        assert call(Lb, out[2], batch, gm, sig, out[0], out[1]) != 0
    assert call(Lb, out[2], 1, 0.5, 0.5, Lb, out[1]) != 0 and b"Sigma_out must not be" in core.lib.covo_last_error()
    assert call(Lb, out[2], 1, 0.5, 0.5, out[0], out[2]) != 0 and b"L_out must not be C" in core.lib.covo_last_error()
    with pytest.raises(ValueError, match="sigma_adapt="):
        core.sigma_adapt(Lb, out[2], 1.0)
    assert core.device_status() == 0


# ---- the steps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_period_three_adapts_on_the_reuse_steps(graph, monkeypatch):
    """N = 256, m = 3, gamma = 0.2, seven steps.  Step 0 is the step of the same controller without adaptation.  A reuse step's a_cov,
    factor and scale are core.sigma_adapt of the factor read after the previous step and that step's info["post_cov"], bit for bit,
    and its a_cov is not what the plain shift of the same factor gives.  Refresh steps report fallback 0 and scale 1."""
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    N, gm = 256, 0.2
    env = quad_env(task="tracking_zigzag")
    ca, cpa, obs, info, state, params = single_controller(env, "covo-online", N, sigma_period=3, sigma_adapt=gm)
    cb, cpb = single_controller(env, "covo-online", N, sigma_period=3)[:2]
    assert ca.core.compute_post_cov and ca.core.sigma_adapt_gamma == gm
    key = cr.PRNGKey(7)
    L_prev = C_prev = None
    for step in range(7):
        key, k_act, k_step = cr.split(key, 3)
        ua, cpa2, ia = ca(obs, state, params, k_act, cpa, info)
        torch.cuda.synchronize()
        age = ia["sigma_age"]
        assert age == step % 3, (step, age)
        L_now = ca.core.sigma_factor()
        fb, scale = float(ia["sigma_adapt_fallback"]), float(ia["sigma_adapt_scale"])
        if step == 0:
            ub, cpb2, _ = cb(obs, state, params, k_act, cpb, info)
            torch.cuda.synchronize()
            assert torch.equal(ua, ub) and torch.equal(cpa2.a_mean, cpb2.a_mean) and torch.equal(cpa2.a_cov, cpb2.a_cov)
            assert torch.equal(ca.core.cost, cb.core.cost)
        if age == 0:
            assert (fb, scale) == (0.0, 1.0), step
        else:
            Sp, Lp, rows = ca.core.sigma_adapt(L_prev, C_prev, gm, cpa.sample_sigma)
            assert torch.equal(cpa2.a_cov, Sp) and torch.equal(L_now, Lp), step
            assert scale == float(rows[1]) and fb == float(rows[0]) == 0.0, step
            S_shift, _ = ca.core.sigma_shift(L_prev, cpa.sample_sigma)
            assert not torch.equal(cpa2.a_cov, S_shift), step  # the shift path would not pass this test
            assert bool(torch.isfinite(cpa2.a_mean).all())
        L_prev, C_prev, cpa = L_now, ia["post_cov"].clone(), cpa2
        obs, state, _, _, info = env.step(k_step, state, ua.cpu().numpy(), params)
    assert ca.core.device_status() == 0
    ca.core.close()
    cb.core.close()


def test_two_passes_of_a_reuse_step_adapt_once_from_the_last_pass(monkeypatch):
    """iters = 2, m = 2: a reuse step's a_cov and factor are the stand-alone call on the previous step's factor and on the C its
    last pass left; both passes sample from that one L'."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, "covo-online", 256, sigma_period=2, sigma_adapt=0.2, iters=2)
    key = cr.PRNGKey(13)
    L_prev = C_prev = None
    for step in range(4):
        key, k_act, k_step = cr.split(key, 3)
        u, cp2, ci = c(obs, state, params, k_act, cp, info)
        torch.cuda.synchronize()
        L_now = c.core.sigma_factor()
        assert ci["sigma_age"] == step % 2 and tuple(ci["iter_cost_min"].shape) == (2,)
        if step % 2 == 1:
            Sp, Lp, _ = c.core.sigma_adapt(L_prev, C_prev, 0.2, cp.sample_sigma)
            assert torch.equal(cp2.a_cov, Sp) and torch.equal(L_now, Lp), step
        L_prev, C_prev, cp = L_now, ci["post_cov"].clone(), cp2
        obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
    assert c.core.device_status() == 0
    c.core.close()


@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_run_episode_equals_the_python_loop(graph, monkeypatch):
    """Seven steps, m = 3, gamma = 0.2, in two segments: log (u among it), final mean and a_cov equal a Python loop of single steps
    bit for bit."""
    from covo_mpc_amd.envs.quadrotor import DeviceEpisode
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    m, N, T = 3, 256, 7
    out = {}
    for kind in ("episode", "steps"):
        c, cp, _, _, _, params = single_controller(env, "covo-online", N, sigma_period=m, sigma_adapt=0.2)
        c.alias_outputs = True
        ep = DeviceEpisode(env, cr.PRNGKey(21), params, (c.core.lib, c.core.h), c.core.device)
        cp = c.reset(ep.state0, params, cp, cr.PRNGKey(22))
        rng = cr.PRNGKey(23)
        if kind == "steps":
            for t in range(T):
                rng, rng_act, rng_step, _ = cr.split(rng, 4)
                u, cp, ci = c(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                assert ci["sigma_age"] == t % m
                ep.step(rng_step, u)
                rng, _ = cr.split(rng)
        else:
            cp, rng = c.run_episode(ep, params, cp, rng, 2)
            cp, rng = c.run_episode(ep, params, cp, rng, T - 2)
        log = ep.read_log()
        assert c.core._sigma_ages() == (T % m, (T - 1) % m), kind
        out[kind] = (log, cp.a_mean.clone().cpu().numpy(), cp.a_cov.clone().cpu().numpy(), np.asarray(rng).copy(),
                     c.core.sigma_adapt_rows.clone().cpu().numpy())
        assert c.core.device_status() == 0
        c.core.close()
    for x, y in zip(out["episode"], out["steps"]):
        assert np.array_equal(x, y)


def test_batched_online_equals_single():
    """E = 3, N = 256, m = 2, gamma = 0.2, four steps: row e of a_mean, a_cov, the factor and the adapt rows is torch.equal to the
    single controller on instance e alone."""
    E, N, m, gm = 3, 256, 2, 0.2
    env = quad_env(task="tracking", randomizer=True)
    inst = []
    for e in range(E):
        params = env.sample_params(cr.PRNGKey(100 + e))
        obs, info, state = env.reset(cr.PRNGKey(200 + e), params)
        c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False, sigma_period=m,
                                      sigma_adapt=gm)
        inst.append(dict(params=params, obs=obs, info=info, state=state, key=cr.PRNGKey(300 + e), c=c, cp=c.init_control_params))
    cp0 = inst[0]["cp"]
    b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, discount=cp0.discount, gamma_mean=cp0.gamma_mean,
                                             sample_sigma=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=DEV, sigma_period=m,
                                             sigma_adapt=gm)
    assert tuple(b.sigma_adapt_rows.shape) == (E, 4) and tuple(b.post_cov.shape) == (E, N_A, N_A)
    b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    for step in range(4):
        k_acts = []
        for i in inst:
            i["key"], k_act, i["k_step"] = cr.split(i["key"], 3)
            k_acts.append(np.asarray(k_act))
        b([i["info"]["noisy_state"] for i in inst], np.stack(k_acts))
        assert b.sigma_age == step % m
        Lb = b.core.sigma_factor(E)
        for e, i in enumerate(inst):
            u, i["cp"], sinfo = i["c"](i["obs"], i["state"], i["params"], k_acts[e], i["cp"], i["info"])
            where = (step, e)
            assert torch.equal(b._cost[e], i["c"].core.cost), where
            assert torch.equal(b.a_mean[e], i["cp"].a_mean.reshape(-1)), where
            assert torch.equal(b.a_cov[e], i["cp"].a_cov), where
            assert torch.equal(Lb[e], i["c"].core.sigma_factor()), where
            assert torch.equal(b.post_cov[e], i["c"].core.post_cov[0]), where
            assert torch.equal(b.sigma_adapt_rows[e], i["c"].core.sigma_adapt_rows[0]), where
            if step % m:
                assert float(b.sigma_adapt_rows[e, 0]) == 0.0 and float(b.sigma_adapt_rows[e, 1]) != 1.0, where
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u.cpu().numpy(), i["params"])
    assert b.core.device_status() == 0
    for i in inst:
        i["c"].core.close()
    b.core.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_adaptation_without_a_post_cov_target_is_refused_before_any_launch(monkeypatch):
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, "covo-online", 256, sigma_period=2)
    rows = torch.zeros((1, 4), device=DEV)
    lib, h = c.core.lib, c.core.h
    assert lib.covo_set_step_sigma_adapt(h, 1.0, _lib.ptr(rows), 1) != 0 and b"gamma=1" in lib.covo_last_error()
    assert lib.covo_set_step_sigma_adapt(h, 0.2, _lib.ptr(rows), 0) != 0 and b"n_inst=0" in lib.covo_last_error()
    _lib.check(lib.covo_set_step_sigma_adapt(h, 0.2, _lib.ptr(rows), 1), "covo_set_step_sigma_adapt")
    with pytest.raises(_lib.CovoError, match=r"Sigma adapt.*without a posterior covariance target"):
        c(obs, state, params, cr.PRNGKey(3), cp, info)
    _lib.check(lib.covo_set_step_sigma_period(h, 1), "covo_set_step_sigma_period")
    with pytest.raises(_lib.CovoError, match=r"Sigma adapt.*Sigma period of 1"):
        c(obs, state, params, cr.PRNGKey(3), cp, info)
    assert c.core.device_status() == 0
    _lib.check(lib.covo_set_step_sigma_adapt(h, 0.0, None, 0), "covo_set_step_sigma_adapt")  # off: the handle steps again
    u, cp2, _ = c(obs, state, params, cr.PRNGKey(3), cp, info)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(u).all()) and c.core.device_status() == 0
    c.core.close()


def test_adaptation_on_an_mppi_step_is_refused_before_any_launch(monkeypatch):
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, "mppi", 256)
    rows = torch.zeros((1, 4), device=DEV)
    _lib.check(c.core.lib.covo_set_step_sigma_adapt(c.core.h, 0.2, _lib.ptr(rows), 1), "covo_set_step_sigma_adapt")
    with pytest.raises(_lib.CovoError, match=r"Sigma adapt.*belongs to the reuse steps of covo-online.*MPPI"):
        c(obs, state, params, cr.PRNGKey(3), cp, info)
    assert c.core.device_status() == 0
    _lib.check(c.core.lib.covo_set_step_sigma_adapt(c.core.h, 0.0, None, 0), "covo_set_step_sigma_adapt")
    u, cp2, _ = c(obs, state, params, cr.PRNGKey(3), cp, info)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(cp2.a_mean).all()) and c.core.device_status() == 0
    c.core.close()


def test_kernel_by_kernel_path_refuses_adaptation():
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, "covo-online", 256, sigma_period=2, sigma_adapt=0.2)
    c.materialize_eps = True
    with pytest.raises(NotImplementedError, match="sigma_period=2|sigma_adapt=0.2"):
        c(obs, state, params, cr.PRNGKey(3), cp, info)
    c.core.close()
