"""GPU (-m gpu): the annealed MPPI step (covo_set_step_anneal / covo_cost_standardise; controllers/dial.py) against its
definition in tests/anneal_oracle.py.

Bars.  The solver's lam_eff and std: at most one fp32 ulp from the fp32 rounding of the oracle's fp64 value (the fp64 sums of <= 2^17
terms are exact to ~2^-36, so only the final rounding can flip); |F|, the fallback decision and entry 1 given entry 0: exact.  Sample
buffers, costs, a_cov and rows between two runs of the same launches: torch.equal.  A pass's new mean against fp64 on the device's own
costs at the device's own temperature: tests/update_oracle.py::check_update's 1e-5 as it stands.  The passes of a k-pass step are
chained through the fused controllers themselves, as tests/test_gpu_iters.py does: rows 0 .. j - 1 of the schedule do not depend on k, so
a controller built with iters = j returns the mean after pass j - 1."""
import ctypes as C
import functools

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
from tests import anneal_oracle as AO  # noqa: E402
from tests import update_oracle as UO  # noqa: E402
from tests.gpu_support import DEV, H, bits, instances, quad_env  # noqa: E402

LAM, TEMP = 0.01, 0.1


def _controller(env, name, N, **kw):
    c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam{LAM}", device=DEV, compute_info=False, **kw)
    return c


def _start(env, c, seed=4):
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(seed), params)
    cp = c.reset(state, params, c.init_control_params, cr.PRNGKey(seed + 1))
    return cp, obs, info, state, params


def _same(x, y, where):
    assert np.array_equal(bits(x.contiguous()), bits(y.contiguous())), where


@functools.lru_cache(maxsize=None)
def _core(N):
    return SamplingCore(N, 32, LAM, 1.0, device=DEV, compute_info=False)


# ------------------------------------------------------------------------------------------ 1: the solver against the oracle
@pytest.mark.parametrize("pattern", AO.SOLVER_PATTERNS)
@pytest.mark.parametrize("N", AO.SOLVER_SIZES)
def test_solver_against_the_oracle(N, pattern):
    """covo_cost_standardise on three instances with different costs: every row against standardise64 -- the fallback cases are cases,
    with their expected rows."""
    core = _core(256)
    cost = np.stack([AO.solver_costs(pattern, N, e) for e in range(3)])
    rows = core.cost_standardise(torch.from_numpy(cost).to(DEV), TEMP, LAM)
    torch.cuda.synchronize()
    assert core.device_status() == 0 and tuple(rows.shape) == (3, 4)
    rows = rows.cpu().numpy()
    for e in range(3):
        ref = AO.check_row(rows[e], cost[e], TEMP, LAM, where=f"{pattern} N={N} instance {e}")
        if pattern in ("equal", "one_finite") or N < 2:
            assert ref["fallback"] and np.array_equal(rows[e].view(np.uint32)[[0, 1, 3]], AO.row_words(ref)[[0, 1, 3]])
    # one instance alone gives the same row as inside the batch (a 1-d tensor)
    one = core.cost_standardise(torch.from_numpy(cost[1]).to(DEV), TEMP, LAM).cpu().numpy()
    assert np.array_equal(one.view(np.uint32), rows[1:2].view(np.uint32))


def test_solver_falls_back_on_a_temperature_that_is_no_normal_float():
    core = _core(256)
    for cost, temp in ((np.array([0, 1e-30] * 50, dtype=np.float32), 1e-10), (np.array([-3e38, 3e38] * 50, dtype=np.float32), 10.0)):
        row = core.cost_standardise(torch.from_numpy(cost).to(DEV), temp, LAM).cpu().numpy()[0]
        ref = AO.check_row(row, cost, temp, LAM, where=f"temp {temp}")
        assert ref["fallback"] and ref["n_finite"] == 100


# ------------------------------------------------------------------------------------------ 2: the neutral element
@pytest.mark.parametrize("N", [256, 20000])
@pytest.mark.parametrize("k", [1, 3])
def test_neutral_element_is_the_mppi_controller(k, N):
    """beta_pass = beta_stage = 1 with temp=None attaches nothing: MPPIController(iters=k), bit for bit (N = 20 000: beyond the one-launch
    small step's 16 384)."""
    env = quad_env(task="tracking_zigzag")
    d = _controller(env, "dial", N, iters=k, beta_pass=1.0, beta_stage=1.0, temp=None)
    m = _controller(env, "mppi", N, iters=k)
    assert d.anneal is None and d.core.anneal_rows is None and isinstance(d, cm.controllers.MPPIController)
    cp, obs, info, state, params = _start(env, m)
    cpd = cpm = cp
    key = cr.PRNGKey(6)
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        ud, cpd, idd = d(obs, state, params, k_act, cpd, info)
        um, cpm, im = m(obs, state, params, k_act, cpm, info)
        where = (k, N, step)
        assert "anneal_rows" not in idd and set(idd) == set(im)
        _same(cpd.a_mean, cpm.a_mean, where), _same(ud, um, where), _same(cpd.a_cov, cpm.a_cov, where)
        _same(d.core.a, m.core.a, where), _same(d.core.cost, m.core.cost, where)
        obs, state, _, _, info = env.step(k_step, state, ud.cpu().numpy(), params)
    assert d.core.device_status() == 0
    d.core.close(), m.core.close()


# ------------------------------------------------------------------------------------------ 3: the schedule
@pytest.mark.parametrize("k", [1, 3])
def test_schedule_step_equals_the_one_pass_compositions(k):
    """temp=None, beta_pass = 0.5, beta_stage = 0.9.  Pass j of the step: the kernel-by-kernel path's core.randn(act_key_j) +
    core.noise_blockdiag(sigma[j][h] I, mu_j) -- mu_0 the shifted input mean, mu_j the mean pass j - 1 committed, unshifted -- as words;
    the returned a_cov is row j squared; the committed mean against fp64 at the configured lam.  a_cov on input is ignored."""
    N = 1000
    env = quad_env(task="tracking_zigzag")
    cs = [_controller(env, "dial", N, iters=j, beta_pass=0.5, beta_stage=0.9, temp=None) for j in range(1, k + 1)]
    ref = _core(N)
    sigma = AO.schedule64(0.5, k, 0.5, 0.9)
    _same(cs[-1].core.anneal_sigma, torch.from_numpy(sigma), "the table")
    cp, obs, info, state, params = _start(env, cs[0])
    key = cr.PRNGKey(6)
    for step in range(3):  # call 1 eager, 2 and 3 as the handle pleases
        key, k_act, k_step = cr.split(key, 3)
        if step == 1:  # whatever a_cov holds on input
            cp = cp.replace(a_cov=(3.0 * torch.eye(4, device=DEV)).repeat(H, 1, 1).contiguous())
        outs = [c(obs, state, params, k_act, cp, info) for c in cs]
        torch.cuda.synchronize()
        start = ref.shift_mean(cp.a_mean.reshape(-1).contiguous())
        for j in range(k):
            where = f"k={k} step {step} pass {j}"
            _, act_key = AO.pass_keys(k_act, j)
            ref.randn(act_key)
            ref.noise_blockdiag(torch.from_numpy(AO.factor_blocks(sigma[j])).to(DEV).contiguous(), start)
            u, cpj, ij = outs[j]
            _same(cs[j].core.a, ref.a, where)
            _same(cpj.a_cov, torch.from_numpy(AO.cov_blocks(sigma[j])), where)
            UO.check_update(cs[j].core, start.view(H, 4), cpj.gamma_mean, LAM, cpj.a_mean, where=where, shifted=True)
            assert torch.equal(u, cpj.a_mean[0]), where
            # no solver runs: the rows say the configured lam, no fallback
            assert tuple(ij["anneal_rows"].shape) == (j + 1, 4) and tuple(ij["anneal_sigma"].shape) == (j + 1, 32)
            assert bool((ij["anneal_lam"] == float(np.float32(LAM))).all()) and not bool(ij["anneal_fallback"].any()) and "lam_eff" not in ij
            start = cpj.a_mean.reshape(-1).contiguous().clone()
        u, cp, _ = outs[k - 1]
        cp = cp.replace(a_mean=cp.a_mean.clone(), a_cov=cp.a_cov.clone())
        obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
    for c in cs:
        assert c.core.device_status() == 0
        c.core.close()


# ------------------------------------------------------------------------------------------ 4: the standardised update
def _problem_state(which):
    if which == "make_problem":
        from tests.conftest import make_problem
        return make_problem(seed=17, time=37)[0]
    from tests.state_atlas import atlas_state
    return atlas_state(which)[0]


@pytest.mark.parametrize("which", ["make_problem", "far_fast"])
@pytest.mark.parametrize("k", [1, 3])
def test_standardised_update(k, which):
    """temp = 0.1: the last pass's row against the oracle on the device's own cost buffer; its new mean against mean64 on those costs
    at the device's lam_eff; every pass's row finite, lam_eff > 0, no fallback."""
    N = 1024
    env = quad_env(task="tracking_zigzag")
    cs = [_controller(env, "dial", N, iters=j, temp=TEMP) for j in range(max(k - 1, 1), k + 1)]  # the last two prefixes (k = 1: one)
    c = cs[-1]
    cp, obs, info, state, params = _start(env, c)
    ns = AO.env_state_with(info["noisy_state"], _problem_state(which))
    k_act = cr.split(cr.PRNGKey(3), 3)[1]
    outs = [x(obs, state, params, k_act, cp, dict(info, noisy_state=ns)) for x in cs]
    torch.cuda.synchronize()
    u, cpk, ik = outs[-1]
    rows = ik["anneal_rows"].cpu().numpy()
    where = f"k={k} {which}"
    assert rows.shape == (k, 4) and np.isfinite(rows[:, :3]).all() and (rows[:, 0] > 0).all(), (where, rows)
    assert not bool(ik["anneal_fallback"].any()) and np.array_equal(ik["anneal_lam"].cpu().numpy(), rows[:, 0])
    assert np.array_equal(ik["anneal_std"].cpu().numpy(), rows[:, 2]) and float(ik["lam_eff"]) == rows[-1, 0]
    print(f"  {where}: lam_eff per pass {rows[:, 0].tolist()} std {rows[:, 2].tolist()}")
    ref = AO.check_row(rows[-1], c.core.cost.cpu().numpy(), TEMP, LAM, where=where)
    assert not ref["fallback"]
    if k == 1:
        before, shifted = cp.a_mean, False
    else:  # the mean pass k - 2 committed: the controller with one pass less returns it
        before, shifted = outs[0][1].a_mean, True
        _same(outs[0][2]["anneal_rows"], ik["anneal_rows"][:k - 1], where)  # the prefix's rows are this step's
    UO.check_update(c.core, before, cpk.gamma_mean, float(rows[-1, 0]), cpk.a_mean, where=where, shifted=shifted)
    _same(cpk.a_cov, torch.from_numpy(AO.cov_blocks(AO.schedule64(0.5, k, 0.5, 0.9)[k - 1])), where)
    for x in cs:
        assert x.core.device_status() == 0
        x.core.close()


# ------------------------------------------------------------------------------------------ 5: captured graph equals eager
def test_captured_graph_equals_eager(monkeypatch):
    N, k = 1024, 3
    env = quad_env(task="tracking_zigzag")
    monkeypatch.setenv("COVO_GRAPH", "1")
    g = _controller(env, "dial", N, iters=k, temp=TEMP)
    monkeypatch.delenv("COVO_GRAPH")
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    e = _controller(env, "dial", N, iters=k, temp=TEMP)
    assert g.core.uses_graph and not e.core.uses_graph
    cp, obs, info, state, params = _start(env, e)
    cpg = cpe = cp
    key = cr.PRNGKey(6)
    for step in range(4):  # the graph handle: eager, capture, replay, replay
        key, k_act, k_step = cr.split(key, 3)
        ug, cpg, ig = g(obs, state, params, k_act, cpg, info)
        ue, cpe, ie = e(obs, state, params, k_act, cpe, info)
        _same(g.core.a, e.core.a, step), _same(g.core.cost, e.core.cost, step), _same(cpg.a_mean, cpe.a_mean, step)
        _same(cpg.a_cov, cpe.a_cov, step), _same(ig["anneal_rows"], ie["anneal_rows"], step)
        _same(ig["iter_cost_min"], ie["iter_cost_min"], step)
        assert not bool(ie["anneal_fallback"].any())
        obs, state, _, _, info = env.step(k_step, state, ue.cpu().numpy(), params)
    assert g.core.device_status() == 0 and e.core.device_status() == 0
    g.core.close(), e.core.close()


# ------------------------------------------------------------------------------------------ 6, 7: batched, device episodes
def _batched(env, inst, E, N, k, **kw):
    cp0 = inst[0]["cp"]
    return cm.controllers.BatchedDialController(env, E, N, H, LAM, iters=k, sigmas=cp0.sample_sigma, discount=cp0.discount,
                                                gamma_mean=cp0.gamma_mean, a_mean_init=cp0.a_mean, device=DEV, **kw)


def test_batched_equals_single_controllers():
    E, N, k = 3, 256, 3
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "dial", N, str(LAM), E, iters=k)
    b = _batched(env, inst, E, N, k)
    assert b.staged and tuple(b.anneal_rows.shape) == (E, k, 4) and tuple(b.anneal_sigma.shape) == (k, 32)
    b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    for step in range(3):
        k_acts = []
        for i in inst:
            i["key"], k_act, i["k_step"] = cr.split(i["key"], 3)
            k_acts.append(np.asarray(k_act))
        u_b = b.step([i["info"]["noisy_state"] for i in inst], np.stack(k_acts)).clone()
        for e, i in enumerate(inst):
            u, i["cp"], info = i["c"](i["obs"], i["state"], i["params"], k_acts[e], i["cp"], i["info"])
            where = (step, e)
            _same(b.a_mean[e].view(H, 4), i["cp"].a_mean, where), _same(b._a[e], i["c"].core.a, where)
            _same(b._cost[e], i["c"].core.cost, where), _same(u_b[e], u, where), _same(b.a_cov[e], i["cp"].a_cov, where)
            _same(b.anneal_rows[e], info["anneal_rows"], where), _same(b.iter_cost_min[e], info["iter_cost_min"], where)
            assert not bool(info["anneal_fallback"].any()), where
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u.cpu().numpy(), i["params"])
    assert b.core.device_status() == 0 and torch.isfinite(b.a_mean).all()
    b.core.close()
    for i in inst:
        i["c"].core.close()


def test_run_episode_equals_the_python_loop():
    """covo_run_episode, 5 steps of the annealed controller (N = 256, k = 2), against the Python loop of __call__ / env step pairs with
    the same keys, as words; the episode's temperature log holds the last pass's row of every step."""
    n, N, k = 5, 256, 2
    env = quad_env(task="hovering")
    params = env.default_params
    outs = []
    for fused in (False, True):
        c = _controller(env, "dial", N, iters=k)
        c.alias_outputs = True
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (c.core.lib, c.core.h), DEV)
        cp = c.reset(ep.state0, params, c.init_control_params, cr.PRNGKey(42))
        rng = cr.PRNGKey(43)
        if fused:
            cp, rng = c.run_episode(ep, params, cp, rng, n)
            lam = ep.read_lam()
            rows = ep.lamlog[:n].cpu().numpy()
            assert np.array_equal(lam["lam_eff"], rows[:, 0]) and np.array_equal(lam["inv_lam_eff"], rows[:, 1])
        else:
            rows = []
            for _ in range(n):  # eval_env's run_one_step (quadrotor.py:520-538)
                rng, rng_act, rng_step, rng_control = cr.split(rng, 4)
                u, cp, info = c(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                rows.append(info["anneal_rows"][-1].clone())
                ep.step(rng_step, u)
                rng, rng_control = cr.split(rng)
            rows = torch.stack(rows).cpu().numpy()
        outs.append((ep.read_log().copy(), cp.a_mean.cpu().numpy().copy(), cp.a_cov.cpu().numpy().copy(), ep.true.cpu().numpy().copy(),
                     np.asarray(rng).copy(), rows.view(np.uint32).copy()))
        assert c.core.device_status() == 0
        c.core.close()
    for x, y in zip(outs[0], outs[1]):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    assert outs[0][0].shape == (n, 4) and outs[0][5].shape == (n, 4) and (outs[0][5][:, 3] >> 31 == 0).all()


def test_run_episode_batched_equals_per_instance_loops():
    E, n, N, k = 2, 5, 256, 2
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "dial", N, str(LAM), E, iters=k)
    params = [i["params"] for i in inst]
    b = _batched(env, inst, E, N, k)
    reset_keys = [cr.PRNGKey(150 + e) for e in range(E)]
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    rngs0 = np.stack([np.asarray(cr.PRNGKey(160 + e)) for e in range(E)])
    rngs = b.run_episode(ep, rngs0, n)
    log = ep.read_log()
    lam = ep.read_lam()
    lamlog = ep.lamlog[:, :n].cpu().numpy()
    assert log.shape == (E, n, 4) and lam["lam_eff"].shape == (E, n) and np.array_equal(lam["lam_eff"], lamlog[:, :, 0])
    for e, i in enumerate(inst):
        c = i["c"]
        c.alias_outputs = True
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        cp = c.reset(se.state0, params[e], c.init_control_params, cr.PRNGKey(250 + e))
        rng, rows = rngs0[e], []
        for _ in range(n):
            rng, rng_act, rng_step, rng_control = cr.split(rng, 4)
            u, cp, info = c(None, None, params[e], rng_act, cp, {"noisy_state": se.noisy_state})
            rows.append(info["anneal_rows"][-1].clone())
            se.step(rng_step, u)
            rng, rng_control = cr.split(rng)
        assert np.array_equal(se.read_log().view(np.uint32), log[e].view(np.uint32)), e
        _same(cp.a_mean.reshape(-1), b.a_mean[e], e), _same(se.true, ep.true[e], e), _same(cp.a_cov, b.a_cov[e], e)
        assert np.array_equal(np.asarray(rng, dtype=np.uint32), rngs[e]), e
        assert np.array_equal(torch.stack(rows).cpu().numpy().view(np.uint32), lamlog[e].view(np.uint32)), e
        c.core.close()
    assert b.core.device_status() == 0
    b.core.close()


# ------------------------------------------------------------------------------------------ 8: options alongside
def test_options_alongside():
    """compute_diag=True with update="guarded": the arbiter never commits a mean dearer than the pass's starting mean; the diagnostics
    describe the last pass at its own temperature."""
    N, k = 512, 2
    env = quad_env(task="tracking_zigzag")
    c = _controller(env, "dial", N, iters=k, compute_diag=True, update="guarded", compute_plan=True)
    cp, obs, info, state, params = _start(env, c)
    key = cr.PRNGKey(6)
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        u, cp, i = c(obs, state, params, k_act, cp, info)
        torch.cuda.synchronize()
        arb = i["arb_cost"].cpu().numpy()
        print(f"  step {step}: arb_cost {arb.tolist()} chosen {float(i['arb_cost_chosen']):.6g} ess {float(i['ess']):.4g} "
              f"lam_eff {float(i['lam_eff']):.6g}")
        assert float(i["arb_cost_chosen"]) <= float(arb[1]), step
        assert torch.equal(i["cost_min"], c.core.cost.min()) and 1.0 <= float(i["ess"]) <= N
        assert np.isfinite(i["pos_plan"].cpu().numpy()).all() and not bool(i["anneal_fallback"].any())
        cp = cp.replace(a_mean=cp.a_mean.clone(), a_cov=cp.a_cov.clone())
        obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
    assert c.core.device_status() == 0
    c.core.close()


# ------------------------------------------------------------------------------------------ 9: refusals at the C boundary
def _refused(core, pc, args, message):
    rc = core.lib.covo_mpc_step(core.h, C.byref(pc), C.byref(args), 1, 2, None, core.stream())
    err = core.lib.covo_last_error()
    assert rc != 0 and message in err, (message, err)


def test_refusals_name_the_condition_and_leave_the_handle_usable():
    env = quad_env(task="hovering")
    c = _controller(env, "dial", 256, iters=2)
    core = c.core
    lib, h = core.lib, core.h
    cp, obs, info, state, params = _start(env, c)
    c(obs, state, params, cr.PRNGKey(9), cp, info)
    pc, args = core._last_step
    # the setter's own ranges
    tab = (C.c_float * 64)(*([0.5] * 64))
    for bad in (0, 17):
        assert lib.covo_set_step_anneal(h, tab, bad, 0.1, None, 0) != 0 and b"n_pass=" in lib.covo_last_error()
    assert lib.covo_set_step_anneal(h, tab, 2, -1.0, None, 0) != 0 and b"temp=-1" in lib.covo_last_error()
    tab[40] = 0.0
    assert lib.covo_set_step_anneal(h, tab, 2, 0.1, None, 0) != 0 and b"sigma_table[1][8]=0" in lib.covo_last_error()
    # at the step, before any launch
    args.mode = _lib.MODE_COVO_ONLINE
    _refused(core, pc, args, b"belongs to MPPI steps")
    args.mode = _lib.MODE_MPPI
    log3 = torch.zeros((1, 3), dtype=torch.float32, device=DEV)
    assert lib.covo_set_step_iters(h, 3, _lib.ptr(log3), 1) == 0
    _refused(core, pc, args, b"was set for n_pass=2 passes, this step runs iters=3")
    assert lib.covo_set_step_iters(h, 2, _lib.ptr(core.iter_cost_min), 1) == 0
    args.gamma_sigma = 0.25
    _refused(core, pc, args, b"together with gamma_sigma=0.25: the schedule owns a_cov")
    args.gamma_sigma = 0.0
    assert lib.covo_set_step_ess_floor(h, 8.0, None, 0) == 0
    _refused(core, pc, args, b"standardised temperature (covo_set_step_anneal, temp=0.1) together with the ESS floor")
    assert lib.covo_set_step_ess_floor(h, 0.0, None, 0) == 0
    assert lib.covo_set_step_elite(h, 8, None, 0) == 0
    _refused(core, pc, args, b"standardised temperature (covo_set_step_anneal, temp=0.1) together with the elite-set update")
    assert lib.covo_set_step_elite(h, 0, None, 0) == 0
    assert lib.covo_mpc_step(h, C.byref(pc), C.byref(args), 1, 2, None, core.stream()) == 0  # as it was: it steps
    # off: a null table with temp = 0; the handle steps on as MPPI with two passes
    assert lib.covo_set_step_anneal(h, None, 0, 0.0, None, 0) == 0
    assert lib.covo_mpc_step(h, C.byref(pc), C.byref(args), 1, 2, None, core.stream()) == 0
    torch.cuda.synchronize()
    assert core.device_status() == 0 and bool(torch.isfinite(core._bufs["a_mean"]).all())
    core.close()
    # a sample-sharded step (one pass: iterations have their own refusal there)
    c = _controller(env, "dial", 256, iters=1)
    core = c.core
    c(obs, state, params, cr.PRNGKey(9), cp, info)
    pc, args = core._last_step
    args.partial_out = core.partial.data_ptr()
    _refused(core, pc, args, b"the annealed step (covo_set_step_anneal) is not available for sample-sharded steps")
    args.partial_out = None
    assert core.lib.covo_mpc_step(core.h, C.byref(pc), C.byref(args), 1, 2, None, core.stream()) == 0
    torch.cuda.synchronize()
    assert core.device_status() == 0
    core.close()


def test_fused_batch_is_refused_by_the_library():
    E, N, k = 2, 256, 2
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "dial", N, str(LAM), E, controllers=False)
    c0 = _controller(env, "dial", N, iters=k)
    for i in inst:
        i["cp"] = c0.init_control_params
    b = _batched(env, inst, E, N, k)
    b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    keys = np.stack([np.asarray(cr.PRNGKey(70 + e)) for e in range(E)])
    assert b.core.lib.covo_set_step_batched_staged(b.core.h, 0) == 0
    with pytest.raises(_lib.CovoError, match="not available for the env-batched step's one fused launch"):
        b.step([i["info"]["noisy_state"] for i in inst], keys)
    assert b.core.lib.covo_set_step_batched_staged(b.core.h, 1) == 0
    b.step([i["info"]["noisy_state"] for i in inst], keys)
    torch.cuda.synchronize()
    assert b.core.device_status() == 0 and torch.isfinite(b.a_mean).all()
    b.core.close(), c0.core.close()
