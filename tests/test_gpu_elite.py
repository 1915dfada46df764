"""GPU tests (-m gpu) of the elite-set update (covo_set_step_elite / covo_elite_select; `elite=K`): the exact top-K selection on the
device (csrc/elite_select.hip) and the update with 0/1 weights that reads its threshold (csrc/reduce_elite.hip).

The reference is numpy on the device's own fp32 costs and actions: np.argsort of the uint64 keys (u(c_n) << 32) | n, fp64 averages.
Bars.  The selector is integer work: threshold words, cost_min, cost_kth, K and the tie count are compared exactly.  The mean, MPPI's
adapted a_cov and cost_weighted are the softmax update's fp32 accumulation with weights of 1: the project's softmax-update bar,
|x - ref| / max(|ref|, 1) <= 1e-5.  ess and weight_sum are sums of ones and K^2 / K with K^2 < 2^24 here: exactly K.  Graph against
eager and a batched row against the single controller: torch.equal."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from tests.gpu_support import DEV, finite_step, quad_env, single_controller  # noqa: E402

BAR = 1e-5


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def words(cost):
    """u(c): the order-preserving unsigned form of the fp32 bits; -0 -> +0; NaN -> 0xFFFFFFFF."""
    c = np.array(cost, dtype=np.float32)
    c[c == 0] = 0.0
    b = c.view(np.uint32)
    u = np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    u[np.isnan(c)] = 0xFFFFFFFF
    return u


def word_bits(u):
    """fp32 bits of the cost a word stands for."""
    u = np.uint32(u)
    return np.uint32(u & np.uint32(0x7FFFFFFF)) if u >> 31 else np.uint32(~u)


def keys(cost):
    return (words(cost).astype(np.uint64) << np.uint64(32)) | np.arange(len(cost), dtype=np.uint64)


def ref_row(cost, K):
    """-> (threshold cost word, threshold index word, bits(cost_min), bits(cost_kth), K, ties, elite indices in key order)."""
    k = keys(cost)
    order = np.argsort(k, kind="stable")
    kth = int(k[order[K - 1]])
    U, I = kth >> 32, kth & 0xFFFFFFFF
    u = words(cost)
    elites = order[:K]
    return U, I, word_bits(u.min()), word_bits(U), K, int((u[elites] == U).sum()), elites


def check_row(row_f32, cost, K, where):
    bits = row_f32.view(np.uint32)
    U, I, bmin, bkth, _, ties, elites = ref_row(cost, K)
    assert (int(bits[0]), int(bits[1])) == (U, I), (where, hex(int(bits[0])), int(bits[1]), hex(U), I)
    assert int(bits[2]) == int(bmin) and int(bits[3]) == int(bkth), (where, bits[2:4], bmin, bkth)
    assert row_f32[4] == K and row_f32[5] == ties and row_f32[6] == 0 and row_f32[7] == 0, (where, row_f32, ties)
    thr = (np.uint64(bits[0]) << np.uint64(32)) | np.uint64(bits[1])
    assert int((keys(cost) <= thr).sum()) == K, where
    return elites


def rel(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(x - ref) / np.maximum(np.abs(ref), 1.0)).max())


# ---- 1. the selector alone ---------------------------------------------------------------------------------------------------------
FAMILIES = ("gauss", "cubic", "rounded", "equal", "zeros", "negative", "infnan", "allnan")


def family(name, N, rng):
    if name == "gauss":
        c = rng.standard_normal(N)
    elif name == "cubic":
        c = 1.0 + 100.0 * rng.random(N) ** 3
    elif name == "rounded":  # costs on a 0.1 grid: the cut falls inside a tie group
        c = np.round(rng.standard_normal(N), 1)
    elif name == "equal":
        c = np.full(N, 3.5)
    elif name == "zeros":
        c = np.where(rng.random(N) < 0.5, -0.0, 0.0)
    elif name == "negative":
        c = -10.0 * np.abs(rng.standard_normal(N)) - 1.0
    elif name == "infnan":
        c = rng.standard_normal(N) * 5.0
        r = rng.random(N)
        c[r < 0.15] = np.inf
        c[r < 0.07] = np.nan
    else:
        c = np.full(N, np.nan)
    return c.astype(np.float32)


@pytest.fixture(scope="module")
def core():
    from covo_mpc_amd.controllers._core import SamplingCore
    c = SamplingCore(64, 32, 0.01, 1.0, device=DEV, use_graph=False, compute_info=False)
    yield c
    c.close()


@pytest.mark.parametrize("N", [1, 2, 40, 63, 64, 65, 257, 1000, 1023, 1024, 1025, 65536, 65537, 300000])
def test_selector_is_exact(core, N):
    """All cost families as the instances of one call (different costs per instance), the cost buffer at a 4-byte offset, K = 1, 2,
    N / 20, N / 2, N - 1 and N: every row equals numpy's K-th key and statistics exactly, and the set {n : key(n) <= threshold} has K
    members.  N = 65 536 / 65 537 / 300 000 cross from the register-resident path to the re-reading one."""
    rng = np.random.default_rng(1000 + N)
    cost = np.stack([family(f, N, rng) for f in FAMILIES])
    E = len(FAMILIES)
    buf = torch.empty(E * N + 1, dtype=torch.float32, device=DEV)
    d = buf[1:].view(E, N)
    d.copy_(torch.from_numpy(cost))
    assert d.data_ptr() % 16 == 4 and d.is_contiguous()
    inside = False
    for K in sorted({k for k in (1, 2, N // 20, N // 2, N - 1, N) if 1 <= k <= N}):
        rows = core.elite_select(d, K).cpu().numpy()
        for e, f in enumerate(FAMILIES):
            check_row(rows[e], cost[e], K, (f, N, K))
        if K == N // 2:
            u = words(cost[2])
            inside = 0 < rows[2][5] < int((u == rows[2].view(np.uint32)[0]).sum())
    if N >= 1000:
        assert inside, "rounded family: the K = N / 2 cut should fall strictly inside a tie group"
    # a row of the batched call equals the single call, bit for bit
    K = max(1, N // 2)
    one = torch.empty(N, dtype=torch.float32, device=DEV)
    one.copy_(d[6])
    assert torch.equal(core.elite_select(one, K)[0].view(torch.int32), core.elite_select(d, K)[6].view(torch.int32))


def test_selector_refuses_bad_arguments(core):
    d = torch.zeros(64, device=DEV)
    out = torch.zeros(8, device=DEV)
    for K in (0, -1, 65):
        rc = core.lib.covo_elite_select(core.h, _lib.ptr(d), 64, 1, K, _lib.ptr(out), core.stream())
        assert rc != 0 and b"K=" in core.lib.covo_last_error() and b"outside [1, n_samples" in core.lib.covo_last_error()
    rc = core.lib.covo_elite_select(core.h, _lib.ptr(d), 64, 0, 4, _lib.ptr(out), core.stream())
    assert rc != 0 and b"n_inst" in core.lib.covo_last_error()


# ---- the steps ------------------------------------------------------------------------------------------------------------------
def elite_mean_ref(core, K, start, gamma_mean):
    """The fp64 elite update on the core's own fp32 costs and actions around `start` [32, 4] (fp64) -> (mean, elites, a [N, H, 4])."""
    a = core.a.permute(1, 0, 2).contiguous().cpu().numpy().astype(np.float64)
    cost = core.cost.cpu().numpy()
    elites = check_row(core.elite_rows[0].cpu().numpy(), cost, K, "step")
    return gamma_mean * a[elites].mean(axis=0) + (1.0 - gamma_mean) * start, elites, a


_MODES = ("mppi", "covo-offline", "covo-online")


@pytest.mark.parametrize("name,N,gamma_mean", [(m, n, 1.0) for m in _MODES for n in (257, 1024, 4096)] + [(m, 1024, 0.7) for m in _MODES])
def test_one_step_three_modes(name, N, gamma_mean, monkeypatch):
    """K = N / 8: sampling is untouched (actions and costs torch.equal to a handle without elite), the selector's row is numpy's, the
    new mean is the fp64 elite average (gamma_mean = 0.7: blended with the shifted old mean), the diagnostics count K."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    K = N // 8
    env = quad_env(task="tracking_zigzag")
    ca, cpa, obs, info, state, params = single_controller(env, name, N, elite=K, compute_diag=True)
    cb, cpb = single_controller(env, name, N)[:2]
    cpa, cpb = cpa.replace(gamma_mean=gamma_mean), cpb.replace(gamma_mean=gamma_mean)
    k_act = cr.PRNGKey(3)
    ua, cpa2, ia = ca(obs, state, params, k_act, cpa, info)
    ub, cpb2, ib = cb(obs, state, params, k_act, cpb, info)
    torch.cuda.synchronize()
    assert torch.equal(ca.core.a, cb.core.a) and torch.equal(ca.core.cost, cb.core.cost)
    assert torch.equal(cpa2.a_cov, cpb2.a_cov)
    assert ia["elite_count"].dim() == 0 and ia["elite_count"].data_ptr() == ca.core.elite_rows[0, 4:].data_ptr()  # views: no copy
    assert float(ia["elite_count"]) == K and "elite_count" not in ib
    shift = R.shift_mean(cpa.a_mean.cpu().numpy().astype(np.float64))
    mean, elites, _ = elite_mean_ref(ca.core, K, shift, gamma_mean)
    cost = ca.core.cost.cpu().numpy()
    assert float(ia["elite_cost_max"]) == cost[elites].max() and float(ia["elite_cost_min"]) == cost.min()
    err = rel(cpa2.a_mean.cpu().numpy(), mean)
    d = ca.core.diag[0].cpu().numpy()
    cw = rel(d[2], cost[elites].astype(np.float64).mean())
    print(f"  {name} N={N} gamma_mean={gamma_mean}: mean err {err:.2e}, ess {d[0]!r}, weight_sum {d[4]!r}, cost_weighted err {cw:.2e}")
    assert err <= BAR, (name, N, err)
    assert d[0] == K and d[4] == K and d[5] == N, d
    assert cw <= BAR and d[1] == cost.min(), d
    assert rel(d[3], cost.astype(np.float64).mean()) <= BAR
    assert not torch.equal(cpa2.a_mean, cpb2.a_mean)
    assert ca.core.device_status() == 0
    ca.core.close()
    cb.core.close()


def test_one_step_mppi_covariance_refit(monkeypatch):
    """MPPI with gamma_sigma = 0.3, N = 1 024, K = 128: mean and a_cov against the fp64 refit to the elites."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    N, K = 1024, 128
    env = quad_env(task="tracking_zigzag")
    for diag in (False, True):
        c, cp, obs, info, state, params = single_controller(env, "mppi", N, elite=K, compute_diag=diag)
        cp = cp.replace(gamma_sigma=0.3)
        _, cp2, _ = c(obs, state, params, cr.PRNGKey(3), cp, info)
        torch.cuda.synchronize()
        shift = R.shift_mean(cp.a_mean.cpu().numpy().astype(np.float64))
        mean, elites, a = elite_mean_ref(c.core, K, shift, cp.gamma_mean)
        w = np.zeros(N)
        w[elites] = 1.0 / K
        cov = R.mppi_cov_update(w, a, mean, R.shift_mean(cp.a_cov.cpu().numpy().astype(np.float64)), 0.3)
        e_mean, e_cov = rel(cp2.a_mean.cpu().numpy(), mean), rel(cp2.a_cov.cpu().numpy(), cov)
        print(f"  mppi gamma_sigma=0.3 diag={diag}: mean err {e_mean:.2e}, a_cov err {e_cov:.2e}")
        assert e_mean <= BAR and e_cov <= BAR, (e_mean, e_cov)
        if diag:
            d = c.core.diag[0].cpu().numpy()
            assert d[0] == K and d[4] == K, d
        c.core.close()


@pytest.mark.parametrize("N,K,gamma_sigma", [(65, 8, 0.0), (65600, 4000, 0.0), (65600, 4000, 0.3)])
def test_stage1_sample_tail_and_second_grid_trip(N, K, gamma_sigma, monkeypatch):
    """The shapes at which the stage 1 shared with the softmax update walks its stripes differently, MPPI with diagnostics, one step.
    N = 65: one full 64-sample group and a one-sample tail (the sample clamp is live in the second group, two waves have no group).
    N = 65 600: 1 025 groups on the 256 x 4 waves of the capped grid -- one wave takes a second trip, over a full group; once more
    with gamma_sigma = 0.3 for the second-moment records.  Mean, a_cov and diagnostics against the fp64 elite update (K^2 < 2^24)."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, "mppi", N, elite=K, compute_diag=True)
    cp = cp.replace(gamma_sigma=gamma_sigma)
    _, cp2, _ = c(obs, state, params, cr.PRNGKey(3), cp, info)
    torch.cuda.synchronize()
    shift = R.shift_mean(cp.a_mean.cpu().numpy().astype(np.float64))
    mean, elites, a = elite_mean_ref(c.core, K, shift, cp.gamma_mean)
    cov = R.mppi_cov_update(np.full(K, 1.0 / K), a[elites], mean, R.shift_mean(cp.a_cov.cpu().numpy().astype(np.float64)), gamma_sigma)
    cost = c.core.cost.cpu().numpy()
    d = c.core.diag[0].cpu().numpy()
    e_mean, e_cov = rel(cp2.a_mean.cpu().numpy(), mean), rel(cp2.a_cov.cpu().numpy(), cov)
    cw, cm = rel(d[2], cost[elites].astype(np.float64).mean()), rel(d[3], cost.astype(np.float64).mean())
    print(f"  mppi N={N} K={K} gamma_sigma={gamma_sigma}: mean err {e_mean:.2e}, a_cov err {e_cov:.2e}, ess {d[0]!r}, weight_sum {d[4]!r}, "
          f"cost_weighted err {cw:.2e}, cost_mean err {cm:.2e}, elites in the last group {int((elites >= 64 * ((N - 1) // 64)).sum())}")
    assert e_mean <= BAR and e_cov <= BAR, (N, gamma_sigma, e_mean, e_cov)
    assert d[0] == K and d[4] == K and d[5] == N, d
    assert cw <= BAR and cm <= BAR and d[1] == cost.min(), d
    assert c.core.device_status() == 0
    c.core.close()


@pytest.mark.parametrize("name", ["mppi", "covo-offline", "covo-online"])
def test_one_elite_is_the_best_sample_and_all_elites_the_plain_average(name, monkeypatch):
    """K = 1, gamma_mean = 1: a_mean is a[:, n*, :] bit for bit, n* the arbiter's arb_best on the same step.  K = N: the plain average."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    N = 1024
    env = quad_env(task="tracking_zigzag")
    c1, cp, obs, info, state, params = single_controller(env, name, N, elite=1)
    cn = single_controller(env, name, N, elite=N)[0]
    cg = single_controller(env, name, N, update="guarded")[0]
    k_act = cr.PRNGKey(3)
    _, cp1, _ = c1(obs, state, params, k_act, cp, info)
    _, cpn, _ = cn(obs, state, params, k_act, cp, info)
    _, _, ig = cg(obs, state, params, k_act, cp, info)
    torch.cuda.synchronize()
    best = int(ig["arb_best"])
    assert torch.equal(c1.core.cost, cg.core.cost) and best == int(c1.core.elite_rows[0, 1:2].view(torch.int32))
    assert torch.equal(cp1.a_mean, c1.core.a[:, best, :]), name
    avg = cn.core.a.cpu().numpy().astype(np.float64).mean(axis=1)
    err = rel(cpn.a_mean.cpu().numpy(), avg)
    print(f"  {name}: K = N mean err {err:.2e}")
    assert err <= BAR
    for c in (c1, cn, cg):
        c.core.close()


# ---- 3. graph and batched ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mppi", "covo-offline", "covo-online"])
def test_graph_equals_eager(name, monkeypatch):
    """Three closed-loop steps (the graph handle: eager call, capture, replay): mean, selector row and diagnostics bit-identical."""
    N, K = 1024, 128
    env = quad_env(task="tracking_zigzag")
    monkeypatch.setenv("COVO_GRAPH", "1")
    cg, cpg, obs, info, state, params = single_controller(env, name, N, elite=K, compute_diag=True)
    monkeypatch.delenv("COVO_GRAPH")
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    ce, cpe = single_controller(env, name, N, elite=K, compute_diag=True)[:2]
    assert cg.core.uses_graph and not ce.core.uses_graph
    key = cr.PRNGKey(11)
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        ug, cpg, _ = cg(obs, state, params, k_act, cpg, info)
        ue, cpe, _ = ce(obs, state, params, k_act, cpe, info)
        torch.cuda.synchronize()
        assert torch.equal(cpg.a_mean, cpe.a_mean) and torch.equal(cg.core.cost, ce.core.cost), (name, step)
        assert torch.equal(cg.core.elite_rows.view(torch.int32), ce.core.elite_rows.view(torch.int32)), (name, step)
        assert torch.equal(cg.core.diag, ce.core.diag), (name, step)
        check_row(cg.core.elite_rows[0].cpu().numpy(), cg.core.cost.cpu().numpy(), K, (name, "graph", step))
        obs, state, _, _, info = env.step(k_step, state, ug.cpu().numpy(), params)
    assert cg.core.device_status() == 0 and ce.core.device_status() == 0
    cg.core.close()
    ce.core.close()


def test_batched_online_equals_single():
    """E = 3, N = 256, K = 32: row e of the selector rows, a_mean and a_cov is torch.equal to the single controller on instance e, over
    three steps (eager call, capture, replay)."""
    E, N, K = 3, 256, 32
    env = quad_env(task="tracking", randomizer=True)
    inst = []
    for e in range(E):
        params = env.sample_params(cr.PRNGKey(100 + e))
        obs, info, state = env.reset(cr.PRNGKey(200 + e), params)
        c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False, elite=K)
        inst.append(dict(params=params, obs=obs, info=info, state=state, key=cr.PRNGKey(300 + e), c=c, cp=c.init_control_params))
    cp0 = inst[0]["cp"]
    b = cm.controllers.BatchedCoVOController(env, E, N, 32, 0.01, discount=cp0.discount, gamma_mean=cp0.gamma_mean,
                                             sample_sigma=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=DEV, elite=K)
    b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    assert tuple(b.elite.shape) == (E, 8)
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
            assert torch.equal(b.elite[e].view(torch.int32), i["c"].core.elite_rows[0].view(torch.int32)), where
            assert torch.equal(b.a_mean[e], i["cp"].a_mean.reshape(-1)), where
            assert torch.equal(b.a_cov[e], i["cp"].a_cov), where
            check_row(b.elite[e].cpu().numpy(), b._cost[e].cpu().numpy(), K, ("batched",) + where)
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u.cpu().numpy(), i["params"])
    assert b.core.device_status() == 0
    for i in inst:
        i["c"].core.close()
    b.core.close()


# ---- 4. iterated and closed loop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["graph", "eager"])
@pytest.mark.parametrize("name", ["mppi", "covo-online"])
def test_three_passes_select_again_in_every_pass(name, graph, monkeypatch):
    """iters = 3, N = 256, K = 32, gamma_mean = 0.7 (the blend shows each pass's starting mean): twins with iters = 1 and 2 stop after
    pass 0 and 1 -- their a, cost and mean are those passes' -- and every pass's mean is the fp64 elite update of that pass's own
    costs around the mean the pass before committed; iter_cost_min holds every pass's true minimum."""
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    N, K = 256, 32
    env = quad_env(task="tracking_zigzag")
    cs = []
    for j in (1, 2, 3):
        c, cp, obs, info, state, params = single_controller(env, name, N, elite=K, iters=j)
        cs.append(c)
    cp = cp.replace(gamma_mean=0.7)
    key = cr.PRNGKey(6)
    for step in range(3):  # call 1 eager, call 2 captures, call 3 replays
        key, k_act, k_step = cr.split(key, 3)
        outs = [c(obs, state, params, k_act, cp, info) for c in cs]
        torch.cuda.synchronize()
        start = R.shift_mean(cp.a_mean.cpu().numpy().astype(np.float64))
        for j in range(3):
            mean, _, _ = elite_mean_ref(cs[j].core, K, start, 0.7)
            got = outs[j][1].a_mean.cpu().numpy()
            err = rel(got, mean)
            print(f"  {name} {graph} step {step} pass {j}: mean err {err:.2e}")
            assert err <= BAR, (name, graph, step, j, err)
            assert torch.equal(outs[2][2]["iter_cost_min"][j], cs[j].core.cost.min()), (name, graph, step, j)
            start = got.astype(np.float64)  # teacher-forced: the next pass starts from the mean the device committed
        u, cp, _ = outs[2]
        cp = cp.replace(a_mean=cp.a_mean.clone(), a_cov=cp.a_cov.clone())
        obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
    for c in cs:
        assert c.core.device_status() == 0
        c.core.close()


def test_guarded_arbiter_sees_the_elite_mean(monkeypatch):
    """update="guarded" next to elite: candidate 0 is the elite mean -- arb_cost[0] is the cost covo_arbitrate gives the mean of a twin
    without the arbiter."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    N, K = 1024, 128
    env = quad_env(task="tracking_zigzag")
    cg, cp, obs, info, state, params = single_controller(env, "covo-online", N, elite=K, update="guarded", compute_plan=True)
    ct = single_controller(env, "covo-online", N, elite=K, compute_plan=True)[0]
    k_act = cr.PRNGKey(3)
    _, cpg, ig = cg(obs, state, params, k_act, cp, info)
    _, cpt, it = ct(obs, state, params, k_act, cp, info)
    torch.cuda.synchronize()
    # the twin's plan cost is the rollout cost of the (clipped) elite mean with the step's own inputs: the arbiter's candidate 0
    assert torch.equal(ig["arb_cost"][0], it["cost_plan"]), (ig["arb_cost"], it["cost_plan"])
    if int(ig["arb_choice"]) == 0:
        assert torch.equal(cpg.a_mean, cpt.a_mean)
    cg.core.close()
    ct.core.close()


def test_closed_loop_run_episode(monkeypatch):
    """run_episode, MPPI, N = 1 024, K = 64, 12 steps in two segments with the diagnostic log: log, diagnostics, final mean and key
    chain equal a Python loop of single steps bit for bit; every row's ess is K."""
    from covo_mpc_amd.envs.quadrotor import DeviceEpisode
    monkeypatch.setenv("COVO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    T, N, K = 12, 1024, 64
    out = {}
    for kind in ("episode", "steps"):
        c, cp, _, _, _, params = single_controller(env, "mppi", N, elite=K, compute_diag=True)
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
            cp, rng = c.run_episode(ep, params, cp, rng, 5)
            cp, rng = c.run_episode(ep, params, cp, rng, T - 5)
            diag = None
        log = ep.read_log()
        if kind == "episode":
            diag = ep.read_diag()
        out[kind] = (diag, log, cp.a_mean.clone().cpu().numpy(), np.asarray(rng).copy())
        assert c.core.device_status() == 0
        c.core.close()
    d_ep, log_ep, mean_ep, rng_ep = out["episode"]
    d_st, log_st, mean_st, rng_st = out["steps"]
    assert d_ep.shape == (T, 8) and (d_ep[:, 0] == K).all() and (d_ep[:, 4] == K).all(), d_ep[:, :5]
    assert np.array_equal(d_ep, d_st) and np.array_equal(log_ep, log_st)
    assert np.array_equal(mean_ep, mean_st) and np.array_equal(rng_ep, rng_st)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_single_step():
    """A sharded step, K > N, elite next to an ESS floor, n_inst outside (0, 64], K < 0: an error naming the condition, nothing
    launched, the handle works after."""
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.dynamics.dataclass import as_device_state
    N = 4096
    core = SamplingCore(N, 32, 0.01, 1.0, device=DEV, use_graph=False, elite=64)
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
    attach = lambda K: _lib.check(core.lib.covo_set_step_elite(core.h, K, _lib.ptr(core.elite_rows), 1), "covo_set_step_elite")
    rec = torch.zeros(_lib.COVO_PARTIAL_FLOATS, device=DEV)
    args.partial_out = rec.data_ptr()
    with pytest.raises(_lib.CovoError, match=r"elite-set update.*sample-sharded"):
        step()
    args.partial_out = None
    assert core.device_status() == 0
    finite_step(core, pc, args)
    attach(N + 1)
    with pytest.raises(_lib.CovoError, match=r"K=4097 .*outside \[1, n_samples = 4096\]"):
        step()
    attach(64)
    finite_step(core, pc, args)
    lam = torch.zeros(_lib.COVO_LAM_FLOATS, device=DEV)
    _lib.check(core.lib.covo_set_step_ess_floor(core.h, 32.0, _lib.ptr(lam), 1), "covo_set_step_ess_floor")
    with pytest.raises(_lib.CovoError, match=r"elite-set update.*together with the ESS floor"):
        step()
    _lib.check(core.lib.covo_set_step_ess_floor(core.h, 0.0, None, 0), "covo_set_step_ess_floor")
    finite_step(core, pc, args)
    for n_inst in (0, 65):
        assert core.lib.covo_set_step_elite(core.h, 64, _lib.ptr(core.elite_rows), n_inst) != 0
        assert b"n_inst" in core.lib.covo_last_error()
    assert core.lib.covo_set_step_elite(core.h, -1, None, 0) != 0 and b"K=-1" in core.lib.covo_last_error()
    finite_step(core, pc, args)  # (the refused setters changed nothing)
    check_row(core.elite_rows[0].cpu().numpy(), core.cost.cpu().numpy(), 64, "after the refusals")
    # detached: the same handle steps with the softmax update again
    attach(0)
    core.elite_rows.zero_()
    finite_step(core, pc, args)
    assert not bool(core.elite_rows.any())
    core.close()


def test_refusal_batched_mode():
    """covo_mpc_step_batched_mode (env-batched MPPI: one fused launch) with elite attached to the handle: CovoError naming it;
    detached, the same controller steps."""
    E, N = 2, 256
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(100 + e)) for e in range(E)]
    states = [env.reset(cr.PRNGKey(200 + e), p) for e, p in enumerate(params)]
    c0, cp0 = cm.envs.get_controller(env, "mppi", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    b = cm.controllers.BatchedMPPIController(env, E, N, 32, 0.01, a_mean_init=cp0.a_mean, device=DEV)
    c0.core.close()
    b.set_instances([s[2] for s in states], params)
    noisy = [s[1]["noisy_state"] for s in states]
    keys_ = np.stack([np.asarray(cr.PRNGKey(300 + e)) for e in range(E)])
    _lib.check(b.core.lib.covo_set_step_elite(b.core.h, 32, None, 0), "covo_set_step_elite")
    with pytest.raises(_lib.CovoError, match=r"covo_mpc_step_batched_mode.*elite-set update"):
        b(noisy, keys_)
    assert b.core.device_status() == 0
    _lib.check(b.core.lib.covo_set_step_elite(b.core.h, 0, None, 0), "covo_set_step_elite")
    b(noisy, keys_)
    torch.cuda.synchronize()
    assert b.core.device_status() == 0 and bool(torch.isfinite(b.a_mean).all())
    b.core.close()


def test_python_refusals_on_the_device():
    """The kernel-by-kernel path raises NotImplementedError with elite attached."""
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, "covo-offline", 256, elite=32)
    c.materialize_eps = True
    with pytest.raises(NotImplementedError, match="elite=32"):
        c(obs, state, params, cr.PRNGKey(3), cp, info)
    c.core.close()
