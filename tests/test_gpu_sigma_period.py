"""GPU tests (-m gpu) of the Sigma period (covo_set_step_sigma_period / covo_sigma_shift; `sigma_period=m`): every m-th covo-online
step refreshes Sigma, the steps between sample from the previous step's factor moved one stage down the horizon (csrc/sigma_shift.hip).

The reference of the shift is the fp64 numpy restatement of tests/test_sigma_period_abi.py, fed the kernel's own fp32 input L.
Bars (test 1).  The kernel computes in fp64 and rounds every output to fp32 once, so what separates it from the reference is one fp32
rounding per entry:
  L'      max |L' - L'_ref| / max |L'_ref| <= 3e-6, the bar tests/test_gpu_parity.py::test_sigma_and_cholesky_vs_lapack holds L to
          against LAPACK; the inputs here (shifted Hessians of condition 6e2 .. 7e4, cond(Sigma) 24 .. 265) are of that
          test's kind
  Sigma'  max |Sigma' - L'_ref L'_ref^T| / max |Sigma'| <= 1e-6, DESIGN.md 2's bar for Sigma against LAPACK
  log det |2 sum log L'_ii - 2 n log sigma| <= 2 n 2^-24 = 1.53e-5: every diagonal entry of the fp32 L' is within 2^-24 relative of
          the fp64 one, whose log det is exact to fp64 rounding, and log(1 + e) ~ e
Everything else is equality of bits: a reuse step against core.sigma_shift and covo_noise_gemm_philox, a refresh step against a plain
controller, graph against eager, a batched row against the single controller, the device episode against the Python loop."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from tests.gpu_cases import _batched_period_case, _period_case, check_shift  # noqa: E402
from tests.gpu_support import DEV, quad_env, single_controller  # noqa: E402
from tests.sigma_shift_oracle import N_A, shift_factor_ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SIGMA = 0.5


# ---- 1. the stand-alone shift ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core():
    c = SamplingCore(256, 32, 0.01, 1.0, device=DEV, use_graph=False, compute_info=False)
    yield c
    c.close()


@pytest.fixture(scope="module")
def factors(core):
    """fp32 input factors: sigma I, and covo_sigma's factor of every matrix of tests/golden/hessians_r03.npz, with the fp64 reference
    (Sigma'_ref, L'_ref) of each -- computed once."""
    g = np.load(os.path.join(HERE, "golden", "hessians_r03.npz"))
    Rm = np.stack([np.ascontiguousarray(m) for k in g.files for m in g[k]])
    assert Rm.shape == (14, N_A, N_A)
    _, L = core.sigma(torch.from_numpy(Rm).to(DEV), SIGMA, batch=14)
    torch.cuda.synchronize()
    L = np.concatenate([(SIGMA * np.eye(N_A, dtype=np.float32))[None], L.cpu().numpy()])
    # Sigma = c (R + delta I)^(-1/2): cond(Sigma)^2 is the condition of the shifted Hessian, 6e2 .. 7e4 for these matrices
    conds = [np.linalg.cond(l.astype(np.float64) @ l.astype(np.float64).T) ** 2 for l in L[1:]]
    assert 5e2 < min(conds) and max(conds) < 1e5, conds
    return L, [shift_factor_ref(l, SIGMA) for l in L]


def test_shift_alone_against_the_fp64_restatement(core, factors):
    """Batch of 1 (every input on its own) and a batch of 14 (the golden factors in one launch); in place (L_out = L_in) gives the same
    bits; the identity input is a fixed point to fp32 rounding."""
    L, refs = factors
    singles = []
    for i in range(len(L)):
        Sp, Lp = core.sigma_shift(torch.from_numpy(L[i]).to(DEV), SIGMA)
        torch.cuda.synchronize()
        singles.append((Sp, Lp))
        check_shift(Sp.cpu().numpy(), Lp.cpu().numpy(), refs[i], ("single", i))
    assert np.abs(singles[0][0].cpu().numpy() - SIGMA ** 2 * np.eye(N_A)).max() < 1e-7
    Lb = torch.from_numpy(L[1:]).to(DEV).contiguous()
    Sp, Lp = core.sigma_shift(Lb, SIGMA)
    torch.cuda.synchronize()
    for e in range(14):
        check_shift(Sp[e].cpu().numpy(), Lp[e].cpu().numpy(), refs[1 + e], ("batch of 14", e))
        assert torch.equal(Sp[e], singles[1 + e][0]) and torch.equal(Lp[e], singles[1 + e][1]), e
    # in place, as the step does it
    So = torch.empty_like(Lb)
    _lib.check(core.lib.covo_sigma_shift(core.h, _lib.ptr(Lb), 14, SIGMA, _lib.ptr(So), _lib.ptr(Lb), core.stream()), "covo_sigma_shift")
    torch.cuda.synchronize()
    assert torch.equal(Lb, Lp) and torch.equal(So, Sp)


def test_shift_alone_refuses_bad_arguments(core):
    Lb = torch.eye(N_A, device=DEV).contiguous()
    out = torch.empty(2, N_A, N_A, device=DEV)
    for batch, sig in ((0, 0.5), (1, 0.0), (1, -1.0)):
        assert core.lib.covo_sigma_shift(core.h, _lib.ptr(Lb), batch, sig, _lib.ptr(out[0]), _lib.ptr(out[1]), core.stream()) != 0
    assert core.lib.covo_sigma_shift(core.h, _lib.ptr(Lb), 1, 0.5, _lib.ptr(Lb), _lib.ptr(out[1]), core.stream()) != 0
    assert b"Sigma_out must not be" in core.lib.covo_last_error()
    assert core.device_status() == 0


# ---- the steps ------------------------------------------------------------------------------------------------------------------
def test_period_one_equals_a_controller_without_the_argument(monkeypatch):
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    ca, cpa, obs, info, state, params = single_controller(env, "covo-online", 256, sigma_period=1)
    cb, cpb = single_controller(env, "covo-online", 256)[:2]
    key = cr.PRNGKey(5)
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        ua, cpa, ia = ca(obs, state, params, k_act, cpa, info)
        ub, cpb, ib = cb(obs, state, params, k_act, cpb, info)
        torch.cuda.synchronize()
        assert torch.equal(ua, ub) and torch.equal(cpa.a_mean, cpb.a_mean) and torch.equal(cpa.a_cov, cpb.a_cov), step
        assert "sigma_age" not in ia and "sigma_age" not in ib
        obs, state, _, _, info = env.step(k_step, state, ua.cpu().numpy(), params)
    assert ca.core.sigma_age == 0
    ca.core.close()
    cb.core.close()


def test_period_three_refresh_reuse_reuse_refresh(monkeypatch):
    """Step 0 is the plain step; step 1 and 2 shift the factor the step before left, report a_cov = Sigma' and sample clip(shifted mean
    + L' eps) with the step's act key; step 3 is a plain controller's step from the same mean, state and key."""
    _period_case(3, 4, "eager", monkeypatch)


def test_graph_equals_eager_over_three_periods(monkeypatch):
    """m = 2, six steps: the graph handle runs its refresh step eagerly, captured and replayed (steps 0, 2, 4) and its reuse step
    likewise (1, 3, 5).  (The graph cache exposes no capture counter: that each graph is captured once is not asserted.)"""
    N = 256
    env = quad_env(task="tracking_zigzag")
    monkeypatch.setenv("COVO_GRAPH", "1")
    cg, cpg, obs, info, state, params = single_controller(env, "covo-online", N, sigma_period=2)
    monkeypatch.delenv("COVO_GRAPH")
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    ce, cpe = single_controller(env, "covo-online", N, sigma_period=2)[:2]
    assert cg.core.uses_graph and not ce.core.uses_graph
    key = cr.PRNGKey(11)
    for step in range(6):
        key, k_act, k_step = cr.split(key, 3)
        ug, cpg, ig = cg(obs, state, params, k_act, cpg, info)
        ue, cpe, ie = ce(obs, state, params, k_act, cpe, info)
        torch.cuda.synchronize()
        assert ig["sigma_age"] == ie["sigma_age"] == step % 2
        assert torch.equal(ug, ue) and torch.equal(cpg.a_mean, cpe.a_mean) and torch.equal(cpg.a_cov, cpe.a_cov), step
        assert torch.equal(cg.core.cost, ce.core.cost) and torch.equal(cg.core.sigma_factor(), ce.core.sigma_factor()), step
        obs, state, _, _, info = env.step(k_step, state, ug.cpu().numpy(), params)
    assert cg.core.device_status() == 0 and ce.core.device_status() == 0
    cg.core.close()
    ce.core.close()


def test_batched_online_equals_single():
    """E = 2, N = 256, m = 2, four steps: row e of a_mean, a_cov, the costs and the factor is torch.equal to the single controller on
    instance e alone; the batch shares one age."""
    _batched_period_case(2, 256, 2, 4)


@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_two_passes_of_a_reuse_step_share_one_sigma(graph, monkeypatch):
    """iters = 2, m = 2: the reuse step shifts the refresh step's factor ONCE -- after both passes a_cov and the factor are
    core.sigma_shift of it -- and iter_cost_min has two finite entries, the last one the minimum of the last pass's costs."""
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, "covo-online", 256, sigma_period=2, iters=2)
    key = cr.PRNGKey(13)
    L_prev = None
    for step in range(6):
        key, k_act, k_step = cr.split(key, 3)
        u, cp2, ci = c(obs, state, params, k_act, cp, info)
        torch.cuda.synchronize()
        L_now = c.core.sigma_factor()
        assert ci["sigma_age"] == step % 2
        icm = ci["iter_cost_min"].cpu().numpy()
        assert icm.shape == (2,) and np.all(np.isfinite(icm)) and icm[1] == float(c.core.cost.min()), (step, icm)
        if step % 2 == 1:
            Sp, Lp = c.core.sigma_shift(L_prev, cp.sample_sigma)
            assert torch.equal(cp2.a_cov, Sp) and torch.equal(L_now, Lp), step
        L_prev, cp = L_now, cp2
        obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
    assert c.core.device_status() == 0
    c.core.close()


def test_reuse_step_next_to_the_other_options(monkeypatch):
    """update="guarded", elite = 32, compute_diag on a reuse step: it runs and every row is finite."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, "covo-online", 256, sigma_period=2, update="guarded", elite=32,
                                                        compute_diag=True)
    key = cr.PRNGKey(17)
    for step in range(2):
        key, k_act, k_step = cr.split(key, 3)
        u, cp, ci = c(obs, state, params, k_act, cp, info)
        torch.cuda.synchronize()
        obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
    assert ci["sigma_age"] == 1
    assert bool(torch.isfinite(c.core.diag).all()) and bool(torch.isfinite(c.core.arbiter[0, :4]).all())
    assert bool(torch.isfinite(c.core.elite_rows[0, 2:6]).all()) and float(ci["elite_count"]) == 32
    assert bool(torch.isfinite(cp.a_mean).all()) and bool(torch.isfinite(cp.a_cov).all()) and bool(torch.isfinite(u).all())
    assert c.core.device_status() == 0
    c.core.close()


@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_run_episode_equals_the_python_loop(graph, monkeypatch):
    """2 m steps, m = 3, in two segments: log, final mean, a_cov and key chain equal a Python loop of single steps bit for bit; the
    schedule has wrapped twice: the next step refreshes, the last one ran at age m - 1."""
    from covo_mpc_amd.envs.quadrotor import DeviceEpisode
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    m, N = 3, 256
    T = 2 * m
    out = {}
    for kind in ("episode", "steps"):
        c, cp, _, _, _, params = single_controller(env, "covo-online", N, sigma_period=m)
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
            assert c.core.sigma_age == 2
            cp, rng = c.run_episode(ep, params, cp, rng, T - 2)
        log = ep.read_log()
        assert c.core._sigma_ages() == (0, m - 1), kind
        out[kind] = (log, cp.a_mean.clone().cpu().numpy(), cp.a_cov.clone().cpu().numpy(), np.asarray(rng).copy())
        assert c.core.device_status() == 0
        c.core.close()
    for x, y in zip(out["episode"], out["steps"]):
        assert np.array_equal(x, y)


def test_reset_and_a_period_change_set_the_age_to_zero(monkeypatch):
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, "covo-online", 256, sigma_period=3)
    step = lambda cp: c(obs, state, params, cr.PRNGKey(3), cp, info)
    _, cp1, i0 = step(cp)
    assert i0["sigma_age"] == 0 and c.core.sigma_age == 1
    cp = c.reset(state, params, cp, cr.PRNGKey(2))
    assert c.core.sigma_age == 0
    _, cp1, i1 = step(cp)
    _, cp1, i2 = step(cp1)
    assert (i1["sigma_age"], i2["sigma_age"]) == (0, 1) and c.core.sigma_age == 2
    c.core.set_sigma_period(2)
    assert c.core.sigma_age == 0 and c.core.sigma_period == 2
    _, cp1, i3 = step(cp1)
    _, cp1, i4 = step(cp1)
    _, cp1, i5 = step(cp1)
    assert (i3["sigma_age"], i4["sigma_age"], i5["sigma_age"]) == (0, 1, 0)
    # another sample_sigma: the factor on the handle was built for the old one -- the step refreshes
    _, cp1, i6 = step(cp1.replace(sample_sigma=0.4))
    assert i6["sigma_age"] == 0 and c.core.sigma_age == 1
    torch.cuda.synchronize()
    ld = torch.linalg.slogdet(cp1.a_cov.double())[1].item()
    # (the fp32 rounding of Sigma moves log det by at most n cond(Sigma) 2^-24 ~ 2e-3; the old sigma would be off by 2 n log 1.25 = 57)
    assert abs(ld - 2 * N_A * np.log(0.4)) < 5e-3
    c.core.set_sigma_period(1)
    _, cp1, i7 = step(cp1)
    assert "sigma_age" not in i7 and c.core.sigma_age == 0
    assert c.core.device_status() == 0
    c.core.close()


def test_closed_loop_hovering_sixty_steps(monkeypatch):
    """N = 1 024, m = 4, 60 steps of the hovering task against the host env: every u finite, the instance never terminated, and the
    quadrotor stays near its target."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    env = quad_env(task="hovering")
    c, cp, obs, info, state, params = single_controller(env, "covo-online", 1024, sigma_period=4)
    cp = c.reset(state, params, cp, cr.PRNGKey(2))
    key = cr.PRNGKey(31)
    us = []
    for t in range(60):
        key, k_act, k_step = cr.split(key, 3)
        u, cp, ci = c(obs, state, params, k_act, cp, info)
        assert ci["sigma_age"] == t % 4
        us.append(u)
        obs, state, _, done, info = env.step(k_step, state, u.cpu().numpy(), params)
        assert not bool(done), t
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.stack(us)).all())
    assert float(np.linalg.norm(np.asarray(state.pos) - np.asarray(state.pos_tar))) < 1.0
    assert c.core.device_status() == 0
    c.core.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mppi", "covo-offline"])
def test_refusals_on_the_device(name, monkeypatch):
    """A period above 1 attached through the C entry to a handle that steps in the MPPI / covo-offline mode: CovoError naming it before
    any launch; detached, the same handle steps."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, name, 256, offline_table=False)
    if name == "covo-offline":
        cp = c.reset(state, params, cp, cr.PRNGKey(2))
    assert c.core.lib.covo_set_step_sigma_period(c.core.h, 0) != 0 and b"period=0" in c.core.lib.covo_last_error()
    assert c.core.lib.covo_set_step_sigma_period(c.core.h, 65) != 0 and b"period=65" in c.core.lib.covo_last_error()
    _lib.check(c.core.lib.covo_set_step_sigma_period(c.core.h, 2), "covo_set_step_sigma_period")
    with pytest.raises(_lib.CovoError, match=r"Sigma period.*belongs to covo-online"):
        c(obs, state, params, cr.PRNGKey(3), cp, info)
    assert c.core.device_status() == 0
    _lib.check(c.core.lib.covo_set_step_sigma_period(c.core.h, 1), "covo_set_step_sigma_period")
    u, cp2, _ = c(obs, state, params, cr.PRNGKey(3), cp, info)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(cp2.a_mean).all()) and c.core.device_status() == 0
    c.core.close()


def test_kernel_by_kernel_path_refuses_a_period():
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, "covo-online", 256, sigma_period=2)
    c.materialize_eps = True
    with pytest.raises(NotImplementedError, match="sigma_period=2"):
        c(obs, state, params, cr.PRNGKey(3), cp, info)
    c.core.close()
