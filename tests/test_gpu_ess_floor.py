"""GPU tests (-m gpu) of the ESS floor (covo_set_step_ess_floor / covo_ess_lambda; `ess_min`): the per-step temperature lam_eff solved
on the device from the step's costs so that ESS(lam_eff) >= ess_min (csrc/ess_lambda.hip), and the staged update that reads it
from device memory (csrc/reduce_lam.hip).

The reference is numpy fp64 on the device's own fp32 costs, with 1 / lambda the float the kernels multiply by (as
tests/test_gpu_diag.py).  Bars:
  active floor     |ESS64(lam_eff) / ess_min - 1| <= 1e-4.  The project's bar for a device ESS against fp64 is 3e-5; the solver
                   evaluates the same fp32 expression, the rest covers the bracket's one-ulp resolution (6e-8 .. 1.2e-7 relative in
                   lambda) times the sensitivity d ln ESS / d ln lambda, which the tests compute in fp64 and require to be <= 50
                   (so the bar cannot be met by an insensitive case alone: 50 x 1.2e-7 = 6e-6).
  inactive floor   lam_eff == lam0 bit for bit, one evaluation.
  ESS(lam0) (row [2]) and the diagnostics' ess: 3e-5; new mean and MPPI's adapted covariance at lam_eff: 1e-5 (the softmax bar).
Relative errors as everywhere in this suite: |x - ref| / max(|ref|, 1).
Measured on the MI355X: see DESIGN 4.7 "ESS floor"."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from tests.gpu_support import DEV, finite_step, quad_env, single_controller  # noqa: E402
from tests.oracle_support import rel_err_scalar  # noqa: E402

BAR_ROOT, BAR_ESS, BAR_MEAN, MAX_SENS = 1e-4, 3e-5, 1e-5, 50.0


def ess64(cost_f32, lam, exact_inverse=False):
    """ESS in fp64 on fp32 costs; 1 / lambda is the fp32 quotient the kernels multiply by (exact_inverse: the fp64 one)."""
    inv = 1.0 / np.float64(lam) if exact_inverse else np.float64(np.float32(1.0) / np.float32(lam))
    c = cost_f32.astype(np.float64)
    w = np.exp(-(c - c.min()) * inv)
    s = w.sum()
    return s * s / (w * w).sum()


def sensitivity(cost_f32, lam):
    """d ln ESS / d ln lambda at lam in fp64 (central difference over +-1e-4)."""
    h = 1e-4
    up, dn = ess64(cost_f32, lam * (1 + h), True), ess64(cost_f32, lam * (1 - h), True)
    return (np.log(up) - np.log(dn)) / (np.log1p(h) - np.log1p(-h))


def check_row(row, cost, lam0, ess_min, where):
    """One solver row {lam_eff, 1 / lam_eff, ESS(lam0), evaluations} against fp64 on `cost` (fp32 numpy).  -> active?"""
    lam0 = np.float32(lam0)
    lam_eff, inv, e0, evals = (np.float32(v) for v in row)
    ref0 = ess64(cost, lam0)
    assert 1.0 <= evals <= 64.0, (where, evals)
    assert rel_err_scalar(e0, ref0) <= BAR_ESS, (where, e0, ref0)
    assert inv == np.float32(1.0) / lam_eff, (where, inv, lam_eff)
    active = lam_eff != lam0
    # the fp32 decision may differ from the fp64 one only within the ESS bar of the threshold
    if ref0 >= ess_min * (1 + BAR_ESS):
        assert not active, (where, "inactive by fp64", ref0, ess_min, lam_eff)
    if ref0 <= ess_min * (1 - BAR_ESS):
        assert active, (where, "active by fp64", ref0, ess_min, lam_eff)
    if not active:
        assert evals == 1.0, (where, evals)
        print(f"  {where}: inactive, ESS(lam0) {e0:.6g} (fp64 {ref0:.6g}) >= {ess_min:g}")
        return False
    assert lam_eff > lam0, (where, lam_eff, lam0)
    got = ess64(cost, lam_eff)
    sens = sensitivity(cost, lam_eff)
    print(f"  {where}: lam_eff {lam_eff:.8g} after {int(evals)} evaluations, ESS64(lam_eff) / ess_min - 1 = {got / ess_min - 1:+.2e}, "
          f"sensitivity {sens:.2f}, ESS(lam0) {e0:.6g} (fp64 {ref0:.6g})")
    assert sens <= MAX_SENS, (where, sens)
    assert abs(got / ess_min - 1.0) <= BAR_ROOT, (where, got, ess_min)
    return True


# ---- 1. the solver alone --------------------------------------------------------------------------------------------------------
def _family(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "gauss4096":
        c = 10.0 + 3.0 * rng.standard_normal(4096)
    elif name == "lognormal1000":
        c = np.exp(rng.standard_normal(1000))
    elif name.startswith("cubic"):
        c = 1.0 + 100.0 * rng.random(int(name[5:])) ** 3
    elif name == "gauss40":
        c = 10.0 + 3.0 * rng.standard_normal(40)
    elif name in ("ties257", "manyties257"):  # rounded to 0.1, 7 / 16 samples share the minimum
        c = np.round(5.0 + rng.standard_normal(257), 1)
        c[rng.permutation(257)[:7 if name == "ties257" else 16]] = c.min()
    elif name == "equal1000":
        c = np.full(1000, 3.25)
    elif name == "two":
        c = np.array([1.0, 2.0])
    else:
        raise KeyError(name)
    return c.astype(np.float32)


FAMILIES = ["gauss4096", "lognormal1000", "cubic65536", "cubic65537", "cubic300000", "gauss40", "ties257", "manyties257", "equal1000",
            "two"]
SETTINGS = [(0.01, 1 / 20), (0.01, 1 / 2), (5.0, 1 / 4)]


def _ess_min(frac, N):
    return float(min(max(1.0, frac * N), N / 2))  # the valid range is [1, N / 2]


@pytest.fixture(scope="module")
def core():
    from covo_mpc_amd.controllers._core import SamplingCore
    c = SamplingCore(64, 32, 0.01, 1.0, device=DEV, use_graph=False)
    yield c
    c.close()


def _solve(core, cost, lam0, ess_min):
    """covo_ess_lambda on cost [E, N] (numpy fp32) -> rows [E, 4] numpy."""
    E, N = cost.shape
    d = torch.from_numpy(np.ascontiguousarray(cost)).to(DEV)
    out = torch.full((E, 4), -1.0, device=DEV)
    _lib.check(core.lib.covo_ess_lambda(core.h, _lib.ptr(d), N, E, float(lam0), float(ess_min), _lib.ptr(out), core.stream()),
               "covo_ess_lambda")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("lam0,frac", SETTINGS)
@pytest.mark.parametrize("name", FAMILIES)
def test_solver_alone(core, name, lam0, frac):
    cost = _family(name)
    N = cost.size
    ess_min = _ess_min(frac, N)
    row = _solve(core, cost[None], lam0, ess_min)[0]
    active = check_row(row, cost, lam0, ess_min, (name, lam0, ess_min))
    ties = int((cost == cost.min()).sum())
    if ties >= ess_min:  # the minimum's ties alone carry ESS >= their count at any temperature
        assert not active, (name, ties, ess_min)
    if name in ("equal1000", "two"):
        assert not active and row[0] == np.float32(lam0)
    assert core.device_status() == 0


def test_solver_three_instances_in_one_call(core):
    """E = 3 instances with different costs in one launch: row e is the row of instance e alone, and holds against fp64."""
    N = 4096
    rng = np.random.default_rng(17)
    cost = np.stack([10.0 + 3.0 * rng.standard_normal(N), np.exp(rng.standard_normal(N)), np.full(N, 2.5)]).astype(np.float32)
    for lam0, frac in SETTINGS:
        ess_min = _ess_min(frac, N)
        rows = _solve(core, cost, lam0, ess_min)
        for e in range(3):
            check_row(rows[e], cost[e], lam0, ess_min, ("E3", e, lam0, ess_min))
            assert np.array_equal(rows[e], _solve(core, cost[e:e + 1], lam0, ess_min)[0]), (e, lam0)
        assert rows[2, 0] == np.float32(lam0)  # equal costs: ESS = N


def test_solver_nonfinite_costs_terminate_at_lam0(core):
    """All-inf and NaN costs: the launch ends, lam0 stays."""
    for fill in (np.inf, np.nan):
        cost = np.full((1, 300), fill, dtype=np.float32)
        row = _solve(core, cost, 0.01, 8.0)[0]
        assert row[0] == np.float32(0.01) and row[3] == 1.0, (fill, row)
    cost = _family("gauss4096").copy()
    cost[5] = np.nan
    row = _solve(core, cost[None], 0.01, 8.0)[0]
    assert row[0] == np.float32(0.01) and 1.0 <= row[3] <= 64.0, row


def test_solver_refuses_ess_min_outside_its_range(core):
    d = torch.zeros(64, device=DEV)
    out = torch.zeros(4, device=DEV)
    for bad in (0.5, 33.0):
        rc = core.lib.covo_ess_lambda(core.h, _lib.ptr(d), 64, 1, 0.01, bad, _lib.ptr(out), core.stream())
        assert rc != 0 and b"ess_min" in core.lib.covo_last_error()


# ---- the steps ------------------------------------------------------------------------------------------------------------------
def _mean_ref(c, cp_before, lam, gamma_sigma=0.0):
    """The fp64 update on the step's own fp32 costs and actions at temperature `lam` -> (mean [32, 4], a_cov or None)."""
    a = c.core.a.permute(1, 0, 2).contiguous().cpu().numpy().astype(np.float64)  # (N, H, 4)
    cost = c.core.cost.cpu().numpy().astype(np.float64)
    shift = R.shift_mean(cp_before.a_mean.cpu().numpy().astype(np.float64))
    mean, w = R.softmax_update(cost, a, np.float64(1.0) / np.float64(np.float32(1.0) / np.float32(lam)), cp_before.gamma_mean, shift)
    cov = None
    if gamma_sigma != 0.0:
        cov_shift = R.shift_mean(cp_before.a_cov.cpu().numpy().astype(np.float64))
        cov = R.mppi_cov_update(w, a, mean, cov_shift, gamma_sigma)
    return mean, cov


@pytest.mark.parametrize("N", [257, 1024, 4096])
@pytest.mark.parametrize("name", ["mppi", "covo-offline", "covo-online"])
def test_one_step_three_modes(name, N, monkeypatch):
    """lam0 = 0.01, ess_min = N / 8: sampling is untouched (actions and costs torch.equal to a handle without the floor), ESS64 at the
    solved temperature meets the floor, the new mean is the fp64 update at lam_eff, the diagnostics' ess is the floor."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    lam0, ess_min = "0.01", N / 8
    env = quad_env(task="tracking_zigzag")
    ca, cpa, obs, info, state, params = single_controller(env, name, N, lam=lam0, ess_min=ess_min, compute_diag=True)
    cb, cpb = single_controller(env, name, N, lam=lam0)[:2]
    k_act = cr.PRNGKey(3)
    ua, cpa2, ia = ca(obs, state, params, k_act, cpa, info)
    ub, cpb2, ib = cb(obs, state, params, k_act, cpb, info)
    torch.cuda.synchronize()
    assert torch.equal(ca.core.a, cb.core.a) and torch.equal(ca.core.cost, cb.core.cost)
    assert ia["lam_eff"].dim() == 0 and ia["lam_eff"].data_ptr() == ca.core.lam_eff.data_ptr()  # views: no copy, no sync
    assert ia["ess_lam0"].data_ptr() == ca.core.lam_eff[0, 2:].data_ptr() and "lam_eff" not in ib
    cost = ca.core.cost.cpu().numpy()
    row = ca.core.lam_eff[0].cpu().numpy()
    active = check_row(row, cost, lam0, ess_min, (name, N))
    mean, _ = _mean_ref(ca, cpa, row[0])
    err = np.abs(cpa2.a_mean.cpu().numpy() - mean).max()
    d = ca.core.diag[0].cpu().numpy()
    print(f"  {name} N={N}: mean err {err:.2e}, diag ess {d[0]:.6g} (floor {ess_min:g})")
    assert err <= BAR_MEAN, (name, N, err)
    if active:
        assert rel_err_scalar(d[0], ess_min) <= BAR_ESS, (name, N, d[0], ess_min)
        assert not torch.equal(cpa2.a_mean, cpb2.a_mean)
    assert rel_err_scalar(d[0], ess64(cost, row[0])) <= BAR_ESS
    assert ca.core.device_status() == 0
    ca.core.close()
    cb.core.close()


def test_one_step_mppi_covariance_adaptation(monkeypatch):
    """MPPI with gamma_sigma = 0.3: mean and a_cov against the fp64 update at lam_eff."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    N, lam0, ess_min = 1024, "0.01", 128.0
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, "mppi", N, lam=lam0, ess_min=ess_min, compute_diag=True)
    cp = cp.replace(gamma_sigma=0.3)
    _, cp2, _ = c(obs, state, params, cr.PRNGKey(3), cp, info)
    torch.cuda.synchronize()
    cost = c.core.cost.cpu().numpy()
    row = c.core.lam_eff[0].cpu().numpy()
    active = check_row(row, cost, lam0, ess_min, "mppi gamma_sigma")
    mean, cov = _mean_ref(c, cp, row[0], gamma_sigma=0.3)
    e_mean = np.abs(cp2.a_mean.cpu().numpy() - mean).max()
    e_cov = np.abs(cp2.a_cov.cpu().numpy() - cov).max()
    print(f"  mppi gamma_sigma=0.3: mean err {e_mean:.2e}, a_cov err {e_cov:.2e}")
    assert e_mean <= BAR_MEAN and e_cov <= BAR_MEAN, (e_mean, e_cov)
    if active:
        assert rel_err_scalar(c.core.diag[0, 0].item(), ess_min) <= BAR_ESS
    c.core.close()


@pytest.mark.parametrize("name", ["mppi", "covo-offline", "covo-online"])
def test_inactive_floor(name, monkeypatch):
    """lam0 = 5: ESS(lam0) is far above the floor (checked in fp64), lam_eff == lam0 and the mean is the fp64 update at lam0."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    N, lam0 = 1024, "5.0"
    ess_min = N / 64
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, name, N, lam=lam0, ess_min=ess_min)
    _, cp2, ci = c(obs, state, params, cr.PRNGKey(3), cp, info)
    torch.cuda.synchronize()
    cost = c.core.cost.cpu().numpy()
    assert ess64(cost, 5.0) >= 2 * ess_min  # the case is what it claims to be
    row = c.core.lam_eff[0].cpu().numpy()
    assert not check_row(row, cost, lam0, ess_min, (name, "inactive"))
    assert row[0] == np.float32(5.0) and float(ci["lam_eff"]) == 5.0
    mean, _ = _mean_ref(c, cp, 5.0)
    err = np.abs(cp2.a_mean.cpu().numpy() - mean).max()
    assert err <= BAR_MEAN, (name, err)
    c.core.close()


@pytest.mark.parametrize("name", ["mppi", "covo-offline", "covo-online"])
def test_graph_equals_eager(name, monkeypatch):
    """Three closed-loop steps (the graph handle: eager call, capture, replay): mean, solver row and diagnostics bit-identical."""
    N, lam0, ess_min = 1024, "0.01", 128.0
    env = quad_env(task="tracking_zigzag")
    monkeypatch.setenv("COVO_GRAPH", "1")
    cg, cpg, obs, info, state, params = single_controller(env, name, N, lam=lam0, ess_min=ess_min, compute_diag=True)
    monkeypatch.delenv("COVO_GRAPH")
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    ce, cpe = single_controller(env, name, N, lam=lam0, ess_min=ess_min, compute_diag=True)[:2]
    assert cg.core.uses_graph and not ce.core.uses_graph
    key = cr.PRNGKey(11)
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        ug, cpg, _ = cg(obs, state, params, k_act, cpg, info)
        ue, cpe, _ = ce(obs, state, params, k_act, cpe, info)
        torch.cuda.synchronize()
        assert torch.equal(cpg.a_mean, cpe.a_mean) and torch.equal(cg.core.cost, ce.core.cost), (name, step)
        assert torch.equal(cg.core.lam_eff, ce.core.lam_eff) and torch.equal(cg.core.diag, ce.core.diag), (name, step)
        check_row(cg.core.lam_eff[0].cpu().numpy(), cg.core.cost.cpu().numpy(), lam0, ess_min, (name, "graph", step))
        obs, state, _, _, info = env.step(k_step, state, ug.cpu().numpy(), params)
    assert cg.core.device_status() == 0 and ce.core.device_status() == 0
    cg.core.close()
    ce.core.close()


# ---- 5. env-batched covo-online ---------------------------------------------------------------------------------------------------
def test_batched_online_equals_single():
    """E = 3, N = 256, instance 1 near the episode end (time = 285: its rollouts freeze after 15 steps, its costs discriminate
    least).  ess_min is placed between the largest and the second largest ESS64(lam0) of the instances' costs -- which the floor does
    not touch; taken from handles without a floor -- so that by the fp64 reference at least one row is inactive and at least one
    active.  Row e of lam_eff, a_mean and a_cov is torch.equal to the single controller with the same floor on instance e, over
    three steps (eager call, capture, replay)."""
    import covo_mpc_amd as cm
    E, N, lam0 = 3, 256, "1.0"  # (at lam0 = 0.01 every instance's ESS is 1.00..: no floor would separate them)
    env = quad_env(task="tracking", randomizer=True)
    inst = []
    for e in range(E):
        params = env.sample_params(cr.PRNGKey(100 + e))
        obs, info, state = env.reset(cr.PRNGKey(200 + e), params)
        if e == 1:
            state = state.replace(time=285)
            info = dict(info, noisy_state=info["noisy_state"].replace(time=285))
        inst.append(dict(params=params, obs=obs, info=info, state=state, key=cr.PRNGKey(300 + e)))
    k0 = [np.asarray(cr.split(i["key"], 3)[1]) for i in inst]
    ess0 = []
    for e, i in enumerate(inst):  # the instances' costs of the first step, from handles without a floor
        c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam{lam0}", device=DEV, compute_info=False)
        c(i["obs"], i["state"], i["params"], k0[e], c.init_control_params, i["info"])
        torch.cuda.synchronize()
        ess0.append(ess64(c.core.cost.cpu().numpy(), np.float32(lam0)))
        c.core.close()
    top = sorted(ess0)
    ess_min = float(min(max(np.sqrt(top[-1] * top[-2]), 1.0), N / 2))
    print(f"  ESS64(lam0) per instance {['%.4g' % v for v in ess0]} -> ess_min {ess_min:.4g}")
    assert top[-1] >= ess_min * (1 + BAR_ESS) and top[-2] <= ess_min * (1 - BAR_ESS), (ess0, ess_min)
    for i in inst:
        i["c"], _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam{lam0}", device=DEV, compute_info=False, ess_min=ess_min)
        i["cp"] = i["c"].init_control_params
    cp0 = inst[0]["cp"]
    b = cm.controllers.BatchedCoVOController(env, E, N, 32, float(lam0), discount=cp0.discount, gamma_mean=cp0.gamma_mean,
                                             sample_sigma=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=DEV, ess_min=ess_min)
    b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    assert tuple(b.lam_eff.shape) == (E, 4)
    for step in range(3):
        k_acts = []
        for i in inst:
            i["key"], k_act, i["k_step"] = cr.split(i["key"], 3)
            k_acts.append(np.asarray(k_act))
        b([i["info"]["noisy_state"] for i in inst], np.stack(k_acts))
        for e, i in enumerate(inst):
            u, i["cp"], _ = i["c"](i["obs"], i["state"], i["params"], k_acts[e], i["cp"], i["info"])
            where = (step, e)
            assert torch.equal(b._cost[e], i["c"].core.cost), where
            assert torch.equal(b.lam_eff[e], i["c"].core.lam_eff[0]), (where, b.lam_eff[e], i["c"].core.lam_eff[0])
            assert torch.equal(b.a_mean[e], i["cp"].a_mean.reshape(-1)), where
            assert torch.equal(b.a_cov[e], i["cp"].a_cov), where
            check_row(b.lam_eff[e].cpu().numpy(), b._cost[e].cpu().numpy(), lam0, ess_min, ("batched",) + where)
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u.cpu().numpy(), i["params"])
        if step == 0:
            act = (b.lam_eff[:, 0] != float(np.float32(lam0))).cpu().numpy()
            assert act.any() and not act.all(), act
    assert b.core.device_status() == 0
    for i in inst:
        i["c"].core.close()
    b.core.close()


# ---- 6. device closed loop ------------------------------------------------------------------------------------------------------
def test_closed_loop_run_episode(monkeypatch):
    """run_episode, MPPI, N = 1 024, lam0 = 0.01, ess_min = 32, 40 steps in two segments with the diagnostic log: every row's ess
    holds the floor; log, diagnostics, final mean and key chain equal a Python loop of single steps bit for bit."""
    from covo_mpc_amd.envs.quadrotor import DeviceEpisode
    monkeypatch.setenv("COVO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    T, N, ess_min = 40, 1024, 32.0
    out = {}
    for kind in ("episode", "steps"):
        c, cp, _, _, _, params = single_controller(env, "mppi", N, ess_min=ess_min, compute_diag=True)
        c.alias_outputs = True
        ep = DeviceEpisode(env, cr.PRNGKey(21), params, (c.core.lib, c.core.h), c.core.device)
        cp = c.reset(ep.state0, params, cp, cr.PRNGKey(22))
        rng = cr.PRNGKey(23)
        if kind == "steps":
            rows = []
            for _ in range(T):
                rng, rng_act, rng_step, _ = cr.split(rng, 4)
                u, cp, _ = c(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                rows.append(c.core.diag[0].clone())
                ep.step(rng_step, u)
                rng, _ = cr.split(rng)
            diag = torch.stack(rows).cpu().numpy()
        else:
            cp, rng = c.run_episode(ep, params, cp, rng, 15)
            cp, rng = c.run_episode(ep, params, cp, rng, T - 15)
            diag = None
        log = ep.read_log()
        if kind == "episode":
            diag = ep.read_diag()
        out[kind] = (diag, log, cp.a_mean.clone().cpu().numpy(), np.asarray(rng).copy())
        assert c.core.device_status() == 0
        c.core.close()
    d_ep, log_ep, mean_ep, rng_ep = out["episode"]
    d_st, log_st, mean_st, rng_st = out["steps"]
    assert d_ep.shape == (T, 8)
    print("  ess rows: " + " ".join(f"{v:.2f}" for v in d_ep[:, 0]))
    assert (d_ep[:, 0] >= ess_min * (1 - BAR_ROOT)).all(), d_ep[:, 0]
    assert np.array_equal(d_ep, d_st) and np.array_equal(log_ep, log_st)
    assert np.array_equal(mean_ep, mean_st) and np.array_equal(rng_ep, rng_st)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_single_step():
    """A sharded step, ess_min > N / 2 and ess_min < 1: CovoError naming the condition, nothing launched, the handle works after."""
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.dynamics.dataclass import as_device_state
    N = 4096
    core = SamplingCore(N, 32, 0.01, 1.0, device=DEV, use_graph=False, ess_min=64.0)
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(3), params)
    dstate = as_device_state(info["noisy_state"], DEV)
    pc = params.to_c()
    g = torch.Generator().manual_seed(0)
    A = torch.randn(3, 128, 128, generator=g, dtype=torch.float64)
    L = torch.linalg.cholesky(0.05 * A @ A.transpose(1, 2) + 0.2 * torch.eye(128, dtype=torch.float64)).float().to(DEV).contiguous()
    a_mean = (0.1 * torch.randn(128, generator=g)).to(DEV)
    args, am, am_shift, _ = core._prepare_step(_lib.MODE_COVO_OFFLINE, dstate, a_mean, L_table=L, derive_keys=True)
    step = lambda: _lib.check(core.lib.covo_mpc_step(core.h, C.byref(pc), C.byref(args), 7, 9, None, core.stream()), "covo_mpc_step")
    rec = torch.zeros(_lib.COVO_PARTIAL_FLOATS, device=DEV)
    args.partial_out = rec.data_ptr()
    with pytest.raises(_lib.CovoError, match=r"ESS floor.*sample-sharded"):
        step()
    args.partial_out = None
    assert core.device_status() == 0
    finite_step(core, pc, args)
    for bad, pat in ((N / 2 + 1, r"ess_min=2049 .*outside \[1, n_samples / 2"), (0.5, r"ess_min=0\.5 .*outside \[1, n_samples / 2")):
        _lib.check(core.lib.covo_set_step_ess_floor(core.h, bad, _lib.ptr(core.lam_eff), 1), "covo_set_step_ess_floor")
        with pytest.raises(_lib.CovoError, match=pat):
            step()
        assert core.device_status() == 0
        _lib.check(core.lib.covo_set_step_ess_floor(core.h, 64.0, _lib.ptr(core.lam_eff), 1), "covo_set_step_ess_floor")
        finite_step(core, pc, args)
    assert core.lam_eff[0, 0].item() >= float(np.float32(0.01))
    # a negative or non-finite floor is refused by the setter itself
    for bad in (-1.0, float("nan"), float("inf")):
        assert core.lib.covo_set_step_ess_floor(core.h, bad, None, 0) != 0 and b"ess_min" in core.lib.covo_last_error()
    core.close()


def test_refusal_batched_mode():
    """covo_mpc_step_batched_mode (env-batched MPPI: one fused launch) with a floor attached to the handle: CovoError naming it;
    detached, the same controller steps."""
    import covo_mpc_amd as cm
    E, N = 2, 256
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "mppi", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    b = cm.controllers.BatchedMPPIController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=DEV)
    c0.core.close()
    b.set_instances([s[2] for s in states], params)
    noisy = [s[1]["noisy_state"] for s in states]
    keys = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    _lib.check(b.core.lib.covo_set_step_ess_floor(b.core.h, 32.0, None, 0), "covo_set_step_ess_floor")
    with pytest.raises(_lib.CovoError, match=r"covo_mpc_step_batched_mode.*ESS floor"):
        b(noisy, keys)
    assert b.core.device_status() == 0
    _lib.check(b.core.lib.covo_set_step_ess_floor(b.core.h, 0.0, None, 0), "covo_set_step_ess_floor")
    b(noisy, keys)
    torch.cuda.synchronize()
    assert b.core.device_status() == 0 and bool(torch.isfinite(b.a_mean).all())
    b.core.close()
