"""GPU (-m gpu): covo-online in spline-node space (covo_set_step_sigma_nodes / covo_sigma_nodes / covo_noise_factor_philox;
csrc/sigma_nodes.hip) against its definition in tests/sigma_nodes_oracle.py.

Bars.  Sigma_M (fp64) against numpy's eigh, max-abs over the spectral norm: 5e-11, measured 1.4e-12 at worst over the real Hessians,
the indefinite and the repeated-eigenvalue matrices; 1e-6 for the spectrum graded over 10 decades, measured 2.6e-8 at worst (d = 64)
-- the kernel recovers eigenvalues from the column norms of R_M + shift I, so an eigenvalue carries an absolute error of a few
d 2^-53 shift (shift ~ 1e6 there), which the spectrum map divides by o >= 1e-2.  Both bars stand ~40 times over their measured value,
as the project's Sigma bar (1e-6) stands over its own (2.5e-8); every measured value: DESIGN 4.30.  R_M is no output of the C ABI:
its extreme eigenvalues in the side row (fp32) against the oracle's at 1e-6 of the larger one.  Sigma_stage (fp32) against the oracle at the project's Sigma bar, 1e-6 relative;
||G G^T - Sigma_stage|| <= 2e-7 ||Sigma_stage||, the Sigma chain's factor bar.  The sampler against oracle/c_oracle.py's
explicit fmaf chain: as words.  Two runs of the same arithmetic (launch shapes, batched / single, graph / eager, episode driver /
loop, the step / its parts, off / never on): as words or torch.equal.  The new mean against fp64 on the step's own costs:
tests/update_oracle.py::check_update's 1e-5 as it stands."""
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
from covo_mpc_amd.controllers._options import node_basis  # noqa: E402
from covo_mpc_amd.dynamics.dataclass import as_device_state  # noqa: E402
from tests import anneal_oracle as AO  # noqa: E402
from tests import sigma_nodes_oracle as SO  # noqa: E402
from tests import update_oracle as UO  # noqa: E402
from tests.gpu_support import DEV, H, bits, dev_state, instances, params_c, perturbed_hover_mean, quad_env  # noqa: E402

LAM, SIGMA = 0.01, 0.5
SIGMA_M_BAR, SIGMA_M_BAR_GRADED = 5e-11, 1e-6  # Sigma_M against eigh, max-abs over the spectral norm (see the header)
REAL = ("make_problem", "far_fast", "roll_120_spin", "yaw_cross")


def _same(x, y, where):
    assert np.array_equal(bits(x.contiguous()), bits(y.contiguous())), where


@functools.lru_cache(maxsize=None)
def _core(N, nan=None):
    return SamplingCore(N, 32, LAM, 1.0, device=DEV, compute_info=False, propagate_nan=nan)


def _dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(DEV)


@functools.lru_cache(maxsize=None)
def _real_hessian(which):
    """The Hessian of the step's objective at a perturbed hover mean, from core.hessian -> fp64 numpy [128, 128] (computed once)"""
    if which == "make_problem":
        from tests.conftest import make_problem
        s, p, rng = make_problem(seed=17, time=37)
    else:
        from tests.state_atlas import atlas_state
        s, p, rng = atlas_state(which)
    a = perturbed_hover_mean(p, rng, 0.1)
    ds = dev_state(s)
    R = _core(256).hessian(ds.packed, ds, params_c(p), _dev(a))[0]
    torch.cuda.synchronize()
    return R.cpu().numpy().copy()


def _matrices(W):
    out = [(w, _real_hessian(w)) for w in REAL]
    return out + [(k, SO.crafted(k, W)) for k in ("indefinite", "graded", "repeated", "zero")]


def _solve(R, M, interp, sigma=SIGMA):
    """core.sigma_nodes on a numpy R [128, 128] or [B, 128, 128] -> numpy (Sigma_M, G, Sigma_stage, rows)"""
    out = _core(256).sigma_nodes(_dev(R, np.float64), M, interp, sample_sigma=sigma)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in out)


def _check_against_oracle(SM, G, Sst, row, R, W, where, sigma=SIGMA):
    d = W.shape[1] * 4
    ref = SO.solve(R, W, sigma)
    e_sm = SO.rel(SM, ref["SigmaM"])
    e_st = float(np.linalg.norm(Sst.astype(np.float64) - ref["Sigma_stage"]) / np.linalg.norm(ref["Sigma_stage"]))
    G64 = G.astype(np.float64)
    e_g = float(np.linalg.norm(G64 @ G64.T - Sst.astype(np.float64), 2) / np.linalg.norm(Sst.astype(np.float64), 2))
    lam_scale = max(abs(ref["lam"][0]), abs(ref["lam"][-1]), 1e-30)
    e_lam = max(abs(row[0] - ref["lam"][0]), abs(row[1] - ref["lam"][-1])) / lam_scale
    print(f"  {where}: Sigma_M {e_sm:.2e} Sigma_stage {e_st:.2e} GG^T {e_g:.2e} lam {e_lam:.2e} sweeps {int(row[5])} "
          f"cond(Sigma_M) {ref['s'].max() / ref['s'].min():.1e}")
    assert int(row[6]) == 0 and int(row[7]) == d and 1 <= int(row[5]) <= 16, (where, row)
    assert np.array_equal(SM, SM.T) and np.array_equal(Sst.view(np.uint32), Sst.T.copy().view(np.uint32)), where  # bit for bit
    assert e_sm <= (SIGMA_M_BAR_GRADED if "graded" in where else SIGMA_M_BAR), (where, e_sm)
    assert e_st <= 1e-6, (where, e_st)
    assert e_g <= 2e-7, (where, e_g)
    assert e_lam <= 1e-6 or ref["lam"][-1] - ref["lam"][0] == 0.0, (where, e_lam)
    # the side row against the matrices it reports on
    ev = np.linalg.eigvalsh(SM)
    assert abs(row[2] - ev[-1]) <= 1e-6 * ev[-1] and abs(row[3] - ev[0]) <= 1e-6 * ev[-1], (where, row, ev[0], ev[-1])
    sign, logdet = np.linalg.slogdet(SM)
    want = 2 * d * np.log(sigma)
    assert sign == 1.0 and abs(logdet - want) <= 1e-6 * d and abs(row[4] - want) <= 1e-5 * abs(want) + 1e-5, (where, logdet, row[4], want)
    assert np.all(np.isfinite(G)) and np.all(np.isfinite(Sst))
    return e_sm


# ------------------------------------------------------------------------------------------ 1: kernel 1 against the oracle
@pytest.mark.parametrize("interp", SO.INTERPS)
@pytest.mark.parametrize("M", SO.MS)
def test_sigma_nodes_against_the_oracle(M, interp):
    W = node_basis(M, interp)
    worst = 0.0
    for name, R in _matrices(W):
        worst = max(worst, _check_against_oracle(*_solve(R, M, interp), R, W, f"M={M} {interp} {name}"))
    z = _solve(SO.crafted("zero"), M, interp)
    assert np.abs(z[0] - SIGMA * SIGMA * np.eye(4 * M)).max() <= 1e-15  # R = 0: Sigma_M = sigma^2 I, and not by the fallback
    print(f"  M={M} {interp}: worst Sigma_M error / norm {worst:.2e}")
    assert _core(256).device_status() == 0


@pytest.mark.parametrize("M,interp", [(3, "cubic"), (16, "linear")])
def test_sigma_nodes_batch_of_five_equals_single_calls(M, interp):
    W = node_basis(M, interp)
    mats = [R for _, R in _matrices(W)][:5]
    SMb, Gb, Sb, rb = _solve(np.stack(mats), M, interp, 0.25)
    for b, R in enumerate(mats):
        SM, G, Sst, row = _solve(R, M, interp, 0.25)
        assert np.array_equal(SMb[b], SM) and np.array_equal(Gb[b].view(np.uint32), G.view(np.uint32)), (M, b)
        assert np.array_equal(Sb[b].view(np.uint32), Sst.view(np.uint32)) and np.array_equal(rb[b].view(np.uint32), row.view(np.uint32)), (M, b)
        _check_against_oracle(SMb[b], Gb[b], Sb[b], rb[b], R, W, f"batch M={M} {interp} #{b}", sigma=0.25)


# ------------------------------------------------------------------------------------------ 2: the fallback
@pytest.mark.parametrize("M", [3, 8])
def test_one_nan_entry_falls_back_and_leaves_the_neighbours_alone(M):
    """Plain arithmetic on a NaN value: that instance's R_M is not finite, its flag is set, it samples from sigma^2 I; the neighbours
    are the matrices of a batch without it, as words."""
    W = node_basis(M, "linear")
    good = [_real_hessian("make_problem"), SO.crafted("indefinite")]
    bad = _real_hessian("far_fast").copy()
    bad[40, 9] = np.nan
    SMb, Gb, Sb, rb = _solve(np.stack([good[0], bad, good[1]]), M, "linear")
    SMg, Gg, Sg, rg = _solve(np.stack(good), M, "linear")
    for i, j in ((0, 0), (2, 1)):
        assert np.array_equal(SMb[i], SMg[j]) and np.array_equal(Gb[i].view(np.uint32), Gg[j].view(np.uint32)), i
        assert np.array_equal(Sb[i].view(np.uint32), Sg[j].view(np.uint32)) and np.array_equal(rb[i].view(np.uint32), rg[j].view(np.uint32)), i
        assert int(rb[i][6]) == 0
    fb = SO.fallback(W, SIGMA)
    assert int(rb[1][6]) == _lib.SIGMA_NODES_NONFINITE and int(rb[1][7]) == 4 * M and int(rb[1][5]) == 0, rb[1]
    assert np.array_equal(SMb[1], fb["SigmaM"]) and np.isfinite(Gb[1]).all() and np.isfinite(Sb[1]).all()
    assert np.array_equal(Gb[1].view(np.uint32), fb["G"].view(np.uint32))
    assert np.abs(Sb[1] - fb["Sigma_stage"]).max() <= 2.0 ** -23 * SIGMA * SIGMA and np.array_equal(Sb[1], Sb[1].T)
    assert rb[1][2] == rb[1][3] == np.float32(SIGMA * SIGMA) and abs(rb[1][4] - 2 * 4 * M * np.log(SIGMA)) <= 1e-5 * 4 * M
    assert _core(256).device_status() == 0


# ------------------------------------------------------------------------------------------ 3: kernel 2, bit-exact
def _draw(core, G, mu, key):
    a = core.noise_factor(_dev(G), _dev(mu), key)
    torch.cuda.synchronize()
    return UO.stripes(a).copy()


@pytest.mark.parametrize("N", [1, 63, 257, 1000])
def test_sampler_is_the_fmaf_chain(N, monkeypatch):
    core = _core(N)
    mu = SO.clip_live_mean(N)  # +-0.999: the clip is live
    for d in (8, 12, 64):
        for inst in range(3):  # three instances' factors, means and keys
            key = cr.PRNGKey(100 + N + inst)
            eps = core.randn(key).reshape(N, 32, 4).cpu().numpy().copy()
            G = SO.random_factor(d, inst)
            where = f"N={N} d={d} #{inst}"
            a = _draw(core, G, mu, key)
            assert np.array_equal(a.view(np.uint32), SO.sample_words(G, mu, eps).view(np.uint32)), where
            ref, _, mag = SO.sample64(G, mu, eps)
            bound = SO.chain_bound(d, mag) + 2 * SO.U * (np.abs(mu.reshape(1, 32, 4).astype(np.float64)) + mag)
            assert np.all(np.abs(a.astype(np.float64) - ref) <= bound), where
            if N >= 257:
                assert a.min() == -1.0 and a.max() == 1.0 and ((a > -1.0) & (a < 1.0)).any(), where
            if inst == 0:  # two forced launch shapes: the same words
                for split in ("1", "8"):
                    monkeypatch.setenv("COVO_FACTOR_SPLIT", split)
                    assert np.array_equal(_draw(core, G, mu, key).view(np.uint32), a.view(np.uint32)), (where, split)
                monkeypatch.delenv("COVO_FACTOR_SPLIT")
    assert core.device_status() == 0


@pytest.mark.parametrize("flag", [False, True])
def test_sampler_nan_in_the_mean_follows_the_flag(flag):
    N, d = 257, 12
    core, plain = _core(N, flag), _core(N)
    assert core.propagate_nan == flag
    key = cr.PRNGKey(8)
    mu = SO.clip_live_mean(1)
    mun = mu.copy()
    mun[4 * 13 + 2] = np.nan
    G = SO.random_factor(d, 1)
    a = _draw(core, G, mun, key)
    col = a[:, 13, 2]
    assert np.isnan(col).all() if flag else np.all(col == -1.0)
    ref = _draw(plain, G, mu, key)
    a[:, 13, 2] = ref[:, 13, 2]
    assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), ref.view(np.uint32))


def test_sampler_does_not_depend_on_the_launch_size():
    key = cr.PRNGKey(77)
    mu = SO.clip_live_mean(3)
    for d in (8, 20, 64):
        G = SO.random_factor(d, 2)
        big, small = _draw(_core(1000), G, mu, key), _draw(_core(257), G, mu, key)
        assert np.array_equal(big[:257].view(np.uint32), small.view(np.uint32)), d


# ------------------------------------------------------------------------------------------ 4: the subspace
@pytest.mark.parametrize("interp", SO.INTERPS)
@pytest.mark.parametrize("M", [2, 3, 8])
def test_samples_lie_in_the_node_subspace(M, interp):
    """sigma = 0.02, mu = 0: no clip is live, a - mu = G eps up to the chain's rounding, and G = fp32(P L_M): the part of a - mu
    outside range(P) is at most the chain's d 2^-24 (|G| |eps|) plus the one rounding of G's entries (2^-24 |G| |eps|), pushed
    through I - P P^+ (entry-wise: |I - P P^+| applied to the bound).  Linear nodes: a stage between two nodes is their
    interpolation within the same bound."""
    N, sigma = 1000, 0.02
    W = node_basis(M, interp)
    d = 4 * M
    P = SO.projector(W)
    _, G, _, row = _solve(_real_hessian("make_problem"), M, interp, sigma)
    assert int(row[6]) == 0
    core = _core(N)
    key = cr.PRNGKey(5)
    eps = core.randn(key).reshape(N, 32, 4).cpu().numpy().copy()
    mu = np.zeros(128, np.float32)
    a = _draw(core, G, mu, key).astype(np.float64).reshape(N, 128)
    assert np.abs(a).max() < 1.0
    _, _, mag = SO.sample64(G, mu, eps)
    entry = (d + 1) * SO.U * mag.reshape(N, 128)
    Q = np.eye(128) - P @ np.linalg.pinv(P)
    out = a @ Q.T
    bound = entry @ np.abs(Q).T
    print(f"  M={M} {interp}: worst out-of-subspace / bound {float((np.abs(out) / bound).max()):.3f}, |a| max {np.abs(a).max():.3f}")
    assert np.all(np.abs(out) <= bound)
    if interp == "linear":
        a3, e3 = a.reshape(N, 32, 4), entry.reshape(N, 32, 4)
        checked = 0
        for h in range(32):
            nz = np.flatnonzero(W[h])
            if len(nz) != 2:
                continue
            # the two nodes' own stages, where they are stages (t_m integer): a[h] = W[h][m] a[t_m] + W[h][m+1] a[t_m+1]
            t = [(m * 31) / (M - 1) for m in nz]
            if any(x != int(x) for x in t):
                continue
            lo, hi = int(t[0]), int(t[1])
            want = W[h, nz[0]] * a3[:, lo] + W[h, nz[1]] * a3[:, hi]
            assert np.all(np.abs(a3[:, h] - want) <= e3[:, h] + W[h, nz[0]] * e3[:, lo] + W[h, nz[1]] * e3[:, hi]), h
            checked += 1
        assert checked == (30 if M == 2 else 0)  # (M = 2: both nodes are stages, every stage between them is checked)


# ------------------------------------------------------------------------------------------ 5: the step is its parts
def _online(env, N, cp=None, **kw):
    """(CoVOController(mode="online", **kw), its control params): the factory's parameters, the controller built directly -- the
    factory's own nodes= keyword stays dial's"""
    if cp is None:
        c0, cp = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam{LAM}", device=DEV, compute_info=False)
        c0.core.close()
    return cm.controllers.CoVOController(env, cp, N, H, LAM, "online", device=DEV, compute_info=False, **kw), cp


def _start(env, c, cp, seed=4):
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(seed), params)
    cp = c.reset(state, params, cp, cr.PRNGKey(seed + 1))
    return cp, obs, info, state, params


@pytest.mark.parametrize("M,interp", [(8, "linear"), (5, "cubic")])
def test_the_step_is_its_parts(M, interp):
    N = 256
    env = quad_env(task="tracking_zigzag")
    c, cp = _online(env, N, sigma_nodes=M, node_interp=interp)
    ref = _core(N)
    cp, obs, info, state, params = _start(env, c, cp)
    k_act = cr.split(cr.PRNGKey(3), 3)[1]
    u, cp1, inf = c(obs, state, params, k_act, cp, info)
    torch.cuda.synchronize()
    assert inf["sigma_nodes"] == M and tuple(inf["sigma_node_cov"].shape) == (4 * M, 4 * M) and inf["sigma_node_cov"].dtype == torch.float64
    row = inf["sigma_node_rows"].cpu().numpy()
    assert int(row[6]) == 0 and int(row[7]) == 4 * M, row
    # the parts: Hessian at the shifted mean -> node-space Sigma -> dense-factor sampler with the pass's act key
    ds = as_device_state(info["noisy_state"], DEV)
    start = ref.shift_mean(cp.a_mean.reshape(-1).contiguous())
    R = ref.hessian(ds.packed, ds, c._params_c(params), start)
    SM, G, Sst, rows = ref.sigma_nodes(R[0], M, interp, sample_sigma=cp.sample_sigma)
    _, act_key = AO.pass_keys(k_act, 0)
    ref.noise_factor(G, start, act_key)
    _same(c.core.a, ref.a, "a")
    _same(cp1.a_cov, Sst, "a_cov")
    assert torch.equal(inf["sigma_node_cov"], SM) and torch.equal(inf["sigma_node_rows"], rows)
    assert torch.linalg.matrix_rank(cp1.a_cov.double(), rtol=1e-6).item() == 4 * M  # (above the fp32 rounding of the entries)
    # everything behind the sampler is untouched: the new mean against fp64 on the step's own costs
    UO.check_update(c.core, start.view(H, 4), cp.gamma_mean, LAM, cp1.a_mean, where=f"sigma_nodes={M}", shifted=True)
    assert torch.equal(u, cp1.a_mean[0]) and c.core.device_status() == 0
    c.core.close()


def test_captured_graph_equals_eager(monkeypatch):
    N = 256
    env = quad_env(task="tracking_zigzag")
    monkeypatch.setenv("COVO_GRAPH", "1")
    g, cp = _online(env, N, sigma_nodes=8)
    monkeypatch.delenv("COVO_GRAPH")
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    e, _ = _online(env, N, cp, sigma_nodes=8)
    assert g.core.uses_graph and not e.core.uses_graph
    cp, obs, info, state, params = _start(env, e, cp)
    cpg = cpe = cp
    key = cr.PRNGKey(6)
    for step in range(4):  # the graph handle: eager, capture, replay, replay -- three consecutive steps through the graph among them
        key, k_act, k_step = cr.split(key, 3)
        ug, cpg, ig = g(obs, state, params, k_act, cpg, info)
        ue, cpe, ie = e(obs, state, params, k_act, cpe, info)
        _same(g.core.a, e.core.a, step), _same(g.core.cost, e.core.cost, step), _same(cpg.a_mean, cpe.a_mean, step)
        _same(cpg.a_cov, cpe.a_cov, step), _same(ig["sigma_node_rows"], ie["sigma_node_rows"], step)
        assert torch.equal(ig["sigma_node_cov"], ie["sigma_node_cov"]), step
        obs, state, _, _, info = env.step(k_step, state, ue.cpu().numpy(), params)
    assert g.core.device_status() == 0 and e.core.device_status() == 0
    g.core.close(), e.core.close()


@pytest.mark.parametrize("kw", [dict(iters=2), dict(riccati=True), dict(compute_diag=True, compute_plan=True, compute_post_cov=True, elite=32),
                                dict(compute_fan=8, update="guarded", ess_min=16.0),
                                dict(riccati=True, riccati_feedback=True, riccati_box=True, plan_hold=2)])
def test_it_goes_with_the_options_behind_the_sampler(kw):
    N = 256
    env = quad_env(task="tracking_zigzag")
    c, cp = _online(env, N, sigma_nodes=8, **kw)
    cp, obs, info, state, params = _start(env, c, cp)
    key = cr.PRNGKey(9)
    for step in range(2):
        key, k_act, k_step = cr.split(key, 3)
        u, cp, inf = c(obs, state, params, k_act, cp, info)
        obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
    torch.cuda.synchronize()
    assert torch.isfinite(cp.a_mean).all() and torch.isfinite(cp.a_cov).all() and int(inf["sigma_node_rows"][6]) == 0
    if "iters" in kw:
        assert tuple(inf["iter_cost_min"].shape) == (2,) and torch.isfinite(inf["iter_cost_min"]).all()
    if "riccati" in kw:
        assert "riccati_cost" in inf
    assert c.core.device_status() == 0
    c.core.close()


# ------------------------------------------------------------------------------------------ 6: batched equals single
def _batched(env, cp0, E, N, **kw):
    return cm.controllers.BatchedCoVOController(env, E, N, H, LAM, discount=cp0.discount, gamma_mean=cp0.gamma_mean,
                                                sample_sigma=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=DEV, **kw)


def test_batched_equals_single_controllers():
    E, N, M = 3, 256, 4
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "covo-online", N, str(LAM), E, controllers=False)
    for i in inst:
        i["c"], i["cp"] = _online(env, N, sigma_nodes=M)
    b = _batched(env, inst[0]["cp"], E, N, sigma_nodes=M)
    assert tuple(b.sigma_nodes_rows.shape) == (E, 8)
    b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    for step in range(3):
        k_acts = []
        for i in inst:
            i["key"], k_act, i["k_step"] = cr.split(i["key"], 3)
            k_acts.append(np.asarray(k_act))
        u_b = b([i["info"]["noisy_state"] for i in inst], np.stack(k_acts)).clone()
        covs = b.core.read_sigma_node_cov().clone()
        for e, i in enumerate(inst):
            u, i["cp"], info = i["c"](i["obs"], i["state"], i["params"], k_acts[e], i["cp"], i["info"])
            where = (step, e)
            _same(b.a_mean[e].view(H, 4), i["cp"].a_mean, where), _same(b._a[e], i["c"].core.a, where)
            _same(b._cost[e], i["c"].core.cost, where), _same(u_b[e], u, where), _same(b.a_cov[e], i["cp"].a_cov, where)
            _same(b.sigma_nodes_rows[e], info["sigma_node_rows"], where)
            assert torch.equal(covs[e], info["sigma_node_cov"]) and int(b.sigma_nodes_rows[e][6]) == 0, where
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u.cpu().numpy(), i["params"])
    assert b.core.device_status() == 0 and torch.isfinite(b.a_mean).all()
    b.core.close()
    for i in inst:
        i["c"].core.close()


def test_run_episode_batched_equals_step_calls():
    """One covo_run_episode_batched of 5 steps against 5 step calls with the env step between them (BatchedDeviceEpisode.step), on two
    controllers with the same instances and keys: as words."""
    E, n, N, M = 3, 5, 256, 4
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "covo-online", N, str(LAM), E, controllers=False)
    c0, cp0 = _online(env, N)
    c0.core.close()
    params = [i["params"] for i in inst]
    reset_keys = [cr.PRNGKey(150 + e) for e in range(E)]
    rngs0 = np.stack([np.asarray(cr.PRNGKey(160 + e)) for e in range(E)])
    outs = []
    for fused in (True, False):
        b = _batched(env, cp0, E, N, sigma_nodes=M)
        ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
        if fused:
            rngs = b.run_episode(ep, rngs0, n)
        else:
            b.bind_episode(ep)
            rngs = rngs0.copy()
            for _ in range(n):  # eval_env's run_one_step per instance (quadrotor.py:520-538)
                acts, steps = [], []
                for e in range(E):
                    r, rng_act, rng_step, _ = cr.split(rngs[e], 4)
                    rngs[e] = cr.split(r)[0]
                    acts.append(np.asarray(rng_act)), steps.append(np.asarray(rng_step))
                b(None, np.stack(acts))
                ep.step(np.stack(steps), b.a_mean)
        torch.cuda.synchronize()
        outs.append((ep.read_log().copy(), b.a_mean.cpu().numpy().copy(), b.a_cov.cpu().numpy().copy(), ep.true.cpu().numpy().copy(),
                     np.asarray(rngs, dtype=np.uint32).copy(), b.sigma_nodes_rows.cpu().numpy().copy()))
        assert b.core.device_status() == 0
        b.core.close()
    for k, (x, y) in enumerate(zip(outs[0], outs[1])):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), k


# ------------------------------------------------------------------------------------------ 7: off is off, and the refusals at the C boundary
def test_sigma_nodes_none_is_the_controller_without_the_keyword():
    N = 256
    env = quad_env(task="tracking_zigzag")
    a, cp = _online(env, N, sigma_nodes=None)
    b, _ = _online(env, N, cp)
    assert a.core.sigma_nodes_M is None and a.core.sigma_nodes_rows is None
    cp, obs, info, state, params = _start(env, a, cp)
    k_act = cr.PRNGKey(12)
    ua, cpa, ia = a(obs, state, params, k_act, cp, info)
    ub, cpb, ib = b(obs, state, params, k_act, cp, info)
    assert "sigma_nodes" not in ia and "sigma_node_cov" not in ia
    assert torch.equal(ua, ub) and torch.equal(cpa.a_mean, cpb.a_mean) and torch.equal(cpa.a_cov, cpb.a_cov)
    assert torch.equal(a.core.a, b.core.a) and torch.equal(a.core.cost, b.core.cost)
    assert torch.linalg.matrix_rank(cpa.a_cov.double(), rtol=1e-6).item() == 128  # the full-rank Sigma of the chain
    a.core.close(), b.core.close()


def test_refusals_at_the_c_boundary_leave_the_handle_usable():
    import ctypes as C
    env = quad_env(task="hovering")
    c, cp = _online(env, 256, sigma_nodes=8)
    core = c.core
    lib, h = core.lib, core.h
    cp, obs, info, state, params = _start(env, c, cp)
    c(obs, state, params, cr.PRNGKey(9), cp, info)
    pc, args = core._last_step
    W = np.ascontiguousarray(core.sigma_nodes_weights)
    Wp = W.ctypes.data_as(C.POINTER(C.c_double))
    rows = core.sigma_nodes_rows

    def refused(message):
        rc = lib.covo_mpc_step(h, C.byref(pc), C.byref(args), 1, 2, None, core.stream())
        err = lib.covo_last_error()
        assert rc != 0 and message in err, (message, err)

    for bad in (1, 17, 32):
        assert lib.covo_set_step_sigma_nodes(h, Wp, bad, _lib.ptr(rows), 1) != 0 and b"M=" in lib.covo_last_error()
    assert lib.covo_set_step_sigma_nodes(h, Wp, 8, _lib.ptr(rows), 0) != 0 and b"n_inst=0" in lib.covo_last_error()
    poisoned = W.copy()
    poisoned[3, 5] = np.inf
    assert lib.covo_set_step_sigma_nodes(h, poisoned.ctypes.data_as(C.POINTER(C.c_double)), 8, _lib.ptr(rows), 1) != 0
    assert b"W[3][5]=inf is not a finite number" in lib.covo_last_error()
    M = C.c_int32(-1)
    assert lib.covo_step_sigma_nodes(h, C.byref(M), None, None, 0, None) == 0 and M.value == 8  # a refused call changes nothing
    # at the step, before any launch
    args.mode = _lib.MODE_MPPI
    refused(b"belongs to covo-online steps")
    args.mode = _lib.MODE_COVO_ONLINE
    assert lib.covo_set_step_sigma_period(h, 3) == 0
    refused(b"together with a Sigma period")
    assert lib.covo_set_step_sigma_period(h, 1) == 0
    refine_rows = torch.zeros((1, _lib.COVO_REFINE_FLOATS), dtype=torch.float32, device=DEV)
    assert lib.covo_set_step_refine(h, _lib.ptr(refine_rows), 1) == 0
    refused(b"together with the Newton refinement")
    assert lib.covo_set_step_refine(h, None, 0) == 0
    assert lib.covo_mpc_step(h, C.byref(pc), C.byref(args), 1, 2, None, core.stream()) == 0  # as it was: it steps
    # the stand-alone entries' own ranges
    ref = _core(256)
    R = _dev(_real_hessian("make_problem"), np.float64)
    for bad in (1, 17):
        with pytest.raises(ValueError, match="sigma_nodes="):
            ref.sigma_nodes(R, bad)
    G = _dev(SO.random_factor(8, 0))
    assert lib.covo_noise_factor_philox(h, _lib.ptr(G), 10, _lib.ptr(G), 1, 2, 0, 256, _lib.ptr(core.a), core.stream()) != 0
    assert b"d=10 is no multiple of 4" in lib.covo_last_error()
    # off: a null W; the handle steps on as plain covo-online
    assert lib.covo_set_step_sigma_nodes(h, None, 0, None, 0) == 0
    assert lib.covo_step_sigma_nodes(h, C.byref(M), None, None, 0, None) == 0 and M.value == 0
    assert lib.covo_mpc_step(h, C.byref(pc), C.byref(args), 1, 2, None, core.stream()) == 0
    torch.cuda.synchronize()
    assert core.device_status() == 0 and bool(torch.isfinite(core._bufs["a_mean"]).all())
    assert torch.linalg.matrix_rank(core._bufs["a_cov"].double(), rtol=1e-6).item() == 128
    core.close()
