"""GPU (-m gpu): the annealed step's spline-node sampler (covo_set_step_nodes / covo_noise_nodes_philox; csrc/noise_nodes.hip; DESIGN
4.29) against its definition in tests/nodes_oracle.py.

Bars.  A sampled entry against fp64: (M + 2) 2^-24 (|mu| + sum_m |B e_m|), the forward bound of an M-term fp32 fmaf chain plus one add
(clip is 1-Lipschitz); against oracle/c_oracle.py's explicit fmaf chain: as words.  Two runs of the same arithmetic (launch shapes,
batched / single, graph / eager, episode driver / loop, nodes=32 / nodes=None): as words or torch.equal.  A pass's new mean against
fp64 on the device's own costs at the device's own temperature: tests/update_oracle.py::check_update's 1e-5 as it stands.  The passes
of a k-pass step are chained through the fused controllers themselves, as tests/test_gpu_anneal.py does: slices 0 .. j - 1 of the tables
do not depend on k, so a controller built with iters = j returns the mean after pass j - 1."""
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
from covo_mpc_amd.controllers._options import anneal_schedule, node_schedule  # noqa: E402
from tests import anneal_oracle as AO  # noqa: E402
from tests import nodes_oracle as NO  # noqa: E402
from tests import update_oracle as UO  # noqa: E402
from tests.gpu_support import DEV, H, bits, instances, quad_env  # noqa: E402

LAM, TEMP = 0.01, 0.1
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)


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
def _core(N, nan=None):
    return SamplingCore(N, 32, LAM, 1.0, device=DEV, compute_info=False, propagate_nan=nan)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def _bases(M):
    """the bases a case runs: a pass of the schedule under both interpolations, and a dense random one"""
    out = [(interp, node_schedule(0.5, 1, 0.5, 0.9, M, interp)[1][0]) for interp in NO.INTERPS]
    return out + [("random", NO.random_basis(M, 0))]


def _draw(core, B, mu, key):
    """the stand-alone sampler -> a [N, 32, 4] numpy (a copy)"""
    a = core.noise_nodes(_dev(B), _dev(mu), key)
    torch.cuda.synchronize()
    return UO.stripes(a).copy()


# ------------------------------------------------------------------------------------------ 5: the sampler against the oracle
@pytest.mark.parametrize("N", SIZES)
def test_sampler_against_the_oracle(N):
    core = _core(N)
    key = cr.PRNGKey(100 + N)
    eps = core.randn(key).reshape(N, 32, 4).cpu().numpy().copy()
    mu = NO.clip_live_mean(N)
    worst = 0.0
    for M in NO.MS:
        for kind, B in _bases(M):
            where = f"N={N} M={M} {kind}"
            a = _draw(core, B, mu, key)
            ref, mag = NO.sample64(B, mu, eps)
            err = np.abs(a.astype(np.float64) - ref)
            worst = max(worst, float((err / NO.bound(M, mag)).max()))
            assert np.all(err <= NO.bound(M, mag)), (where, float((err / NO.bound(M, mag)).max()))
            assert np.array_equal(a.view(np.uint32), NO.sample_words(B, mu, eps).view(np.uint32)), where
            if N >= 255:  # the clip is live on both sides, and not everywhere
                assert a.min() == -1.0 and a.max() == 1.0 and ((a > -1.0) & (a < 1.0)).any(), where
    print(f"  N={N}: worst error / bound {worst:.3f}")
    assert core.device_status() == 0


@pytest.mark.parametrize("flag", [False, True])
def test_sampler_nan_in_the_mean_follows_the_flag(flag):
    """COVO_FLAG_PROPAGATE_NAN as in noise_blockdiag_kernel: a NaN entry of mu is -1 in every sample by default and stays a NaN under
    the flag; every other entry is the flagless core's, as words."""
    N, M = 257, 5
    core, plain = _core(N, flag), _core(N)
    assert core.propagate_nan == flag
    key = cr.PRNGKey(8)
    mu = NO.clip_live_mean(1)
    mun = mu.copy()
    mun[4 * 13 + 2] = np.nan
    for kind, B in _bases(M):
        a = _draw(core, B, mun, key)
        col = a[:, 13, 2]
        assert np.isnan(col).all() if flag else np.all(col == -1.0), kind
        ref = _draw(plain, B, mu, key)
        a[:, 13, 2] = ref[:, 13, 2]
        assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), ref.view(np.uint32)), kind


# ------------------------------------------------------------------------------------------ 6: the neutral element
@pytest.mark.parametrize("N", [257, 1000])
def test_sampler_at_32_nodes_with_a_diagonal_basis_is_the_block_kernel(N):
    core = _core(N)
    key = cr.PRNGKey(31)
    mu = _dev(NO.clip_live_mean(2))
    for i, s in enumerate(anneal_schedule(0.5, 2, 0.5, 0.9)):
        a = core.noise_nodes(_dev(np.diag(s)), mu, key).clone()
        b = core.noise_blockdiag_philox(_dev(AO.factor_blocks(s)), mu, key).clone()
        assert torch.equal(a, b), (N, i)
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ 7: shape independence
def test_sampler_does_not_depend_on_the_launch_shape():
    key = cr.PRNGKey(77)
    mu = NO.clip_live_mean(3)
    for M in (3, 8, 32):
        for kind, B in _bases(M):
            big, small = _draw(_core(1000), B, mu, key), _draw(_core(257), B, mu, key)
            assert np.array_equal(big[:257].view(np.uint32), small.view(np.uint32)), (M, kind)


@pytest.mark.parametrize("N", [16384, 32768, 65536])
def test_sampler_does_not_depend_on_the_stage_split(N):
    """The launch splits the 32 stages into S groups by the number of sample blocks (csrc/noise_nodes.hip: noise_nodes_split): 8 up to
    N = 16 384, 4 at 32 768, 2 from 65 536 on -- each its own instantiation.  The first 1 000 samples are the N = 1 000 launch's and the
    launch's last 300 the explicit fmaf chain's (oracle/c_oracle.py), both as words."""
    key = cr.PRNGKey(78)
    mu = NO.clip_live_mean(4)
    core = _core(N)
    eps = core.randn(key).reshape(N, 32, 4)[-300:].cpu().numpy().copy()
    for M in (5, 32):
        B = node_schedule(0.5, 1, 0.5, 0.9, M, "cubic")[1][0]
        small = _draw(_core(1000), B, mu, key)
        a = core.noise_nodes(_dev(B), _dev(mu), key)
        torch.cuda.synchronize()
        head, tail = UO.stripes(a[:, :1000]).copy(), UO.stripes(a[:, -300:]).copy()
        assert np.array_equal(head.view(np.uint32), small.view(np.uint32)), (N, M)
        assert np.array_equal(tail.view(np.uint32), NO.sample_words(B, mu, eps).view(np.uint32)), (N, M)
    assert core.device_status() == 0


@pytest.mark.parametrize("N", [257, 22016])
def test_batched_sampler_equals_three_single_launches(N):
    """The instance form (blockIdx.z) runs in the staged batch only: one pass of BatchedDialController(E = 3, nodes=8) leaves in
    instance e's stripes what the stand-alone sampler gives for e's shifted mean and act key, as words.  N = 22 016: the batch's 258
    sample blocks run the split S = 2, a single launch's 86 run S = 4."""
    E, M = 3, 8
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "dial", N, str(LAM), E, controllers=False)
    b = cm.controllers.BatchedDialController(env, E, N, H, LAM, iters=1, nodes=M, node_interp="cubic", device=DEV)
    rng = np.random.default_rng(5)
    b.a_mean.copy_(_dev(np.clip(0.5 * rng.normal(size=(E, 128)), -1, 1)))
    means = b.a_mean.clone()
    b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    k_acts = np.stack([np.asarray(cr.PRNGKey(500 + e)) for e in range(E)])
    b.step([i["info"]["noisy_state"] for i in inst], k_acts)
    torch.cuda.synchronize()
    ref = _core(N)
    basis = _dev(b.anneal.basis[0])
    for e in range(E):
        _, act_key = AO.pass_keys(k_acts[e], 0)
        a = ref.noise_nodes(basis, ref.shift_mean(means[e].contiguous()), act_key)
        _same(b._a[e], a, e)
    assert b.core.device_status() == 0
    b.core.close()


# ------------------------------------------------------------------------------------------ 8: the rank
@pytest.mark.parametrize("interp", NO.INTERPS)
def test_sample_matrix_has_rank_4M(interp):
    """mu = 0, sigma0 = 0.05 (no clip), N = 1 000, M = 5: the sample matrix [N, 128] is the exact rank-20 product up to the sampler's
    rounding -- singular value number 21 under the bar, number 20 more than 100 times above it (tests/test_nodes_abi.py holds the CPU
    check of the gap for this key)."""
    N, M = NO.RANK_N, NO.RANK_M
    _, B, _, _ = node_schedule(NO.RANK_SIGMA, 1, 0.5, 0.9, M, interp)
    a = _draw(_core(N), B[0], np.zeros(128, np.float32), cr.PRNGKey(NO.RANK_KEY_SEED))
    amax = float(np.abs(a).max())
    assert amax < 1.0
    sv = np.linalg.svd(a.reshape(N, 128).astype(np.float64), compute_uv=False)
    bar = NO.rank_bar(N, M, amax)
    print(f"  {interp}: sv[4M-1] {sv[4 * M - 1]:.4g} sv[4M] {sv[4 * M]:.4g} bar {bar:.4g}")
    assert sv[4 * M] <= bar and sv[4 * M - 1] > 100.0 * bar


# ------------------------------------------------------------------------------------------ 9: the controller
def _problem_state(which):
    if which == "make_problem":
        from tests.conftest import make_problem
        return make_problem(seed=17, time=37)[0]
    from tests.state_atlas import atlas_state
    return atlas_state(which)[0]


@pytest.mark.parametrize("which", ["make_problem", "far_fast"])
@pytest.mark.parametrize("M,interp", [(4, "linear"), (8, "cubic")])
@pytest.mark.parametrize("k", [1, 3])
def test_controller_passes_against_the_sampler_and_the_oracle(k, M, interp, which):
    """temp = 0.1, the defaults 0.5 / 0.9.  Pass j of the step: the stand-alone sampler with act_key_j, basis[j] and mu_j -- mu_0 the
    shifted input mean, mu_j the mean pass j - 1 committed -- as words; the returned a_cov is sigma_e[j]^2 I as words; the committed mean
    against fp64 on the device's own costs at the device's lam_eff."""
    N = 256
    env = quad_env(task="tracking_zigzag")
    cs = [_controller(env, "dial", N, iters=j, temp=TEMP, nodes=M, node_interp=interp) for j in range(1, k + 1)]
    ref = _core(N)
    sn, basis, sigma_e, _ = node_schedule(0.5, k, 0.5, 0.9, M, interp)
    _same(cs[-1].core.anneal_sigma, torch.from_numpy(sigma_e), "the schedule is fed the marginals")
    assert cs[-1].core.step_nodes() == (k, M)
    cp, obs, info, state, params = _start(env, cs[0])
    ns = AO.env_state_with(info["noisy_state"], _problem_state(which))
    k_act = cr.split(cr.PRNGKey(3), 3)[1]
    outs = [c(obs, state, params, k_act, cp, dict(info, noisy_state=ns)) for c in cs]
    torch.cuda.synchronize()
    start = ref.shift_mean(cp.a_mean.reshape(-1).contiguous())
    for j in range(k):
        where = f"k={k} M={M} {interp} {which} pass {j}"
        _, act_key = AO.pass_keys(k_act, j)
        ref.noise_nodes(_dev(basis[j]), start, act_key)
        u, cpj, ij = outs[j]
        _same(cs[j].core.a, ref.a, where)
        _same(cpj.a_cov, torch.from_numpy(NO.cov_blocks(sigma_e[j])), where)
        rows = ij["anneal_rows"].cpu().numpy()
        assert rows.shape == (j + 1, 4) and np.isfinite(rows[:, :3]).all() and (rows[:, 0] > 0).all(), (where, rows)
        assert not bool(ij["anneal_fallback"].any()), where
        AO.check_row(rows[-1], cs[j].core.cost.cpu().numpy(), TEMP, LAM, where=where)
        UO.check_update(cs[j].core, start.view(H, 4), cpj.gamma_mean, float(rows[-1, 0]), cpj.a_mean, where=where, shifted=True)
        assert torch.equal(u, cpj.a_mean[0]), where
        assert ij["anneal_nodes"] == M and tuple(ij["anneal_node_sigma"].shape) == (j + 1, M)
        _same(ij["anneal_node_sigma"], torch.from_numpy(sn[:j + 1].astype(np.float32)), where)
        _same(ij["anneal_sigma"], torch.from_numpy(sigma_e[:j + 1]), where)
        start = cpj.a_mean.reshape(-1).contiguous().clone()
    for c in cs:
        assert c.core.device_status() == 0
        c.core.close()


@pytest.mark.parametrize("k", [1, 3])
def test_controller_at_32_nodes_is_the_controller_without(k):
    """DialController(nodes=32) and DialController() with the same other arguments: torch.equal in u, a_mean, a_cov, anneal_rows (and
    the sample buffers), over three steps."""
    N = 256
    env = quad_env(task="tracking_zigzag")
    d = _controller(env, "dial", N, iters=k, temp=TEMP, nodes=32)
    m = _controller(env, "dial", N, iters=k, temp=TEMP)
    assert d.core.step_nodes() == (k, 32) and m.core.step_nodes() == (0, 0)
    cp, obs, info, state, params = _start(env, m)
    cpd = cpm = cp
    key = cr.PRNGKey(6)
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        ud, cpd, idd = d(obs, state, params, k_act, cpd, info)
        um, cpm, im = m(obs, state, params, k_act, cpm, info)
        where = (k, step)
        assert torch.equal(ud, um) and torch.equal(cpd.a_mean, cpm.a_mean) and torch.equal(cpd.a_cov, cpm.a_cov), where
        assert torch.equal(idd["anneal_rows"], im["anneal_rows"]) and torch.equal(idd["anneal_sigma"], im["anneal_sigma"]), where
        assert torch.equal(d.core.a, m.core.a) and torch.equal(d.core.cost, m.core.cost), where
        obs, state, _, _, info = env.step(k_step, state, ud.cpu().numpy(), params)
    assert d.core.device_status() == 0
    d.core.close(), m.core.close()


# ------------------------------------------------------------------------------------------ 10: paths
def test_captured_graph_equals_eager(monkeypatch):
    N, k = 1024, 3
    env = quad_env(task="tracking_zigzag")
    monkeypatch.setenv("COVO_GRAPH", "1")
    g = _controller(env, "dial", N, iters=k, temp=TEMP, nodes=8)
    monkeypatch.delenv("COVO_GRAPH")
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    e = _controller(env, "dial", N, iters=k, temp=TEMP, nodes=8)
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
        obs, state, _, _, info = env.step(k_step, state, ue.cpu().numpy(), params)
    assert g.core.device_status() == 0 and e.core.device_status() == 0
    g.core.close(), e.core.close()


def _batched(env, inst, E, N, k, **kw):
    cp0 = inst[0]["cp"]
    return cm.controllers.BatchedDialController(env, E, N, H, LAM, iters=k, sigmas=cp0.sample_sigma, discount=cp0.discount,
                                                gamma_mean=cp0.gamma_mean, a_mean_init=cp0.a_mean, device=DEV, **kw)


def test_batched_equals_single_controllers():
    E, N, k = 3, 256, 3
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "dial", N, str(LAM), E, iters=k, nodes=8)
    b = _batched(env, inst, E, N, k, nodes=8)
    assert b.staged and tuple(b.anneal_rows.shape) == (E, k, 4) and b.core.step_nodes() == (k, 8)
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
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u.cpu().numpy(), i["params"])
    assert b.core.device_status() == 0 and torch.isfinite(b.a_mean).all()
    b.core.close()
    for i in inst:
        i["c"].core.close()


def test_run_episode_equals_the_python_loop():
    """covo_run_episode, 5 steps of the controller under nodes=8 (N = 256, k = 2), against the Python loop of __call__ / env step pairs
    with the same keys, as words, the temperature rows included."""
    n, N, k = 5, 256, 2
    env = quad_env(task="hovering")
    params = env.default_params
    outs = []
    for fused in (False, True):
        c = _controller(env, "dial", N, iters=k, nodes=8, node_interp="cubic")
        c.alias_outputs = True
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (c.core.lib, c.core.h), DEV)
        cp = c.reset(ep.state0, params, c.init_control_params, cr.PRNGKey(42))
        rng = cr.PRNGKey(43)
        if fused:
            cp, rng = c.run_episode(ep, params, cp, rng, n)
            rows = ep.lamlog[:n].cpu().numpy()
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
    assert outs[0][0].shape == (n, 4) and outs[0][5].shape == (n, 4)


def test_run_episode_batched_equals_per_instance_loops():
    E, n, N, k = 2, 5, 256, 2
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "dial", N, str(LAM), E, iters=k, nodes=8)
    params = [i["params"] for i in inst]
    b = _batched(env, inst, E, N, k, nodes=8)
    reset_keys = [cr.PRNGKey(150 + e) for e in range(E)]
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    rngs0 = np.stack([np.asarray(cr.PRNGKey(160 + e)) for e in range(E)])
    rngs = b.run_episode(ep, rngs0, n)
    log = ep.read_log()
    lamlog = ep.lamlog[:, :n].cpu().numpy()
    assert log.shape == (E, n, 4)
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


# ------------------------------------------------------------------------------------------ 11: off, and the refusals at the C boundary
def test_nodes_none_leaves_no_table_on_the_handle():
    env = quad_env(task="hovering")
    c = _controller(env, "dial", 256, iters=2)
    assert c.anneal is not None and c.anneal.nodes is None and c.core.step_nodes() == (0, 0) and c.core.anneal_node_sigma is None
    cp, obs, info, state, params = _start(env, c)
    _, _, i = c(obs, state, params, cr.PRNGKey(9), cp, info)
    assert "anneal_nodes" not in i and "anneal_node_sigma" not in i and c.core.step_nodes() == (0, 0)
    c.core.close()
    n = _controller(env, "dial", 256, iters=2, beta_pass=1.0, beta_stage=1.0, temp=None)  # the schedule's neutral element
    assert n.anneal is None and n.core.step_nodes() == (0, 0)
    n.core.close()


def _refused(core, pc, args, message):
    rc = core.lib.covo_mpc_step(core.h, C.byref(pc), C.byref(args), 1, 2, None, core.stream())
    err = core.lib.covo_last_error()
    assert rc != 0 and message in err, (message, err)


def test_refusals_name_the_condition_and_leave_the_handle_usable():
    env = quad_env(task="hovering")
    c = _controller(env, "dial", 256, iters=2, nodes=8)
    core = c.core
    lib, h = core.lib, core.h
    cp, obs, info, state, params = _start(env, c)
    c(obs, state, params, cr.PRNGKey(9), cp, info)
    pc, args = core._last_step
    basis = np.ascontiguousarray(c.anneal.basis, dtype=np.float32)
    tab = basis.ctypes.data_as(C.POINTER(C.c_float))
    # the setter's own ranges
    for bad in (0, 17):
        assert lib.covo_set_step_nodes(h, tab, bad, 8) != 0 and b"n_pass=" in lib.covo_last_error()
    for bad in (1, 33):
        assert lib.covo_set_step_nodes(h, tab, 2, bad) != 0 and b"n_nodes=" in lib.covo_last_error()
    poisoned = basis.copy()
    poisoned[1, 3, 5] = np.inf
    assert lib.covo_set_step_nodes(h, poisoned.ctypes.data_as(C.POINTER(C.c_float)), 2, 8) != 0
    assert b"basis_table[1][3][5]=inf is not a finite number" in lib.covo_last_error()
    assert core.step_nodes() == (2, 8)  # a refused call changes nothing
    # at the step, before any launch
    assert lib.covo_set_step_nodes(h, tab, 1, 8) == 0
    _refused(core, pc, args, b"were set for n_pass=1 passes, the schedule (covo_set_step_anneal) for n_pass=2")
    assert lib.covo_set_step_nodes(h, tab, 2, 8) == 0
    args.mode = _lib.MODE_COVO_ONLINE  # whatever the schedule refuses
    _refused(core, pc, args, b"belongs to MPPI steps")
    args.mode = _lib.MODE_MPPI
    assert lib.covo_mpc_step(h, C.byref(pc), C.byref(args), 1, 2, None, core.stream()) == 0  # as it was: it steps
    assert lib.covo_set_step_anneal(h, None, 0, 0.0, None, 0) == 0  # the schedule off, the nodes still on
    _refused(core, pc, args, b"the spline nodes (covo_set_step_nodes, n_nodes=8) without an attached schedule")
    # off: a null table; the handle steps on as MPPI with two passes
    assert lib.covo_set_step_nodes(h, None, 0, 0) == 0 and core.step_nodes() == (0, 0)
    assert lib.covo_mpc_step(h, C.byref(pc), C.byref(args), 1, 2, None, core.stream()) == 0
    torch.cuda.synchronize()
    assert core.device_status() == 0 and bool(torch.isfinite(core._bufs["a_mean"]).all())
    core.close()
