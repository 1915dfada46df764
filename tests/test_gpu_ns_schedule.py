"""GPU tests (-m gpu) of the Sigma chain's tile-block schedule (sigma_ns.hip: block_load / block_mma_reduce).  The operand loads of
a phase go out tile-major behind the phase's flag loads and every tile's MFMA chain starts on a counted wait for its own operands: a
change of ORDER only -- every tile is still 8 MFMAs on its own accumulator, kk ascending, K-quarters summed (0 + 1) + (2 + 3) -- so
every launch plan must still give the same bits as every other, and the same Sigma as the eigh oracle to the chain's 1e-6.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from tests.gpu_support import DEV  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N_A = 128
SC_COUNT = 3712  # doubles of per-matrix scalars behind the chain's 11 matrix buffers (sigma_ns.hip: enum SC_*)
SC_ITERS, SC_KWIN, SC_BARFAIL = 6, 7, 26


def golden_hessians():
    g = np.load(os.path.join(HERE, "golden", "hessians_r03.npz"))
    return [np.ascontiguousarray(m) for k in g.files for m in g[k]]


def cheap_matrices():
    """spectrum in [1, 4] with an isolated bottom, {1} and [3.5, 4]: with the bottom pair deflated B's interval is [~1.8, ~3], so the
    Newton-Schulz chain needs only its first few iterations (the counts are printed, not asserted: they are the chain's business)"""
    w = np.concatenate([[1.0], np.linspace(3.5, 4.0, N_A - 1)])
    Q, _ = np.linalg.qr(np.random.default_rng(17).standard_normal((N_A, N_A)))
    rot = (Q * w) @ Q.T
    return [np.diag(w), 0.5 * (rot + rot.T)]


def chain_scalars(core, batch):
    """(SC_ITERS, SC_KWIN) of every matrix of the last covo_sigma call on `batch` matrices; no barrier of the chain timed out"""
    out = torch.zeros(32, dtype=torch.float64, device=DEV)
    res = []
    for b in range(batch):
        _lib.check(core.lib.covo_debug_sigma_workspace(core.h, _lib.ptr(out), 11 * batch * N_A * N_A + b * SC_COUNT, 32, core.stream()))
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert o[SC_BARFAIL] == 0.0, b
        res.append((int(o[SC_ITERS]), int(o[SC_KWIN])))
    return res


@pytest.fixture(scope="module")
def cores():
    persistent = SamplingCore(256, 32, 0.01, 1.0, device=DEV)                  # batch 1: two persistent launches; batches: batched tail
    phased = SamplingCore(256, 32, 0.01, 1.0, device=DEV, shared_device=True)  # every phase its own launch
    yield persistent, phased
    persistent.close()
    phased.close()


@pytest.fixture(scope="module")
def oracle_sigmas():
    """eigh-based optimize_sigma of the matrices the tests below use, computed once"""
    return [R.optimize_sigma(m, 0.5, 32, 4) for m in golden_hessians()[:9]], [R.optimize_sigma(m, 0.5, 32, 4) for m in cheap_matrices()]


@pytest.mark.parametrize("batch", [1, 3, 9])
def test_chain_plans_agree_on_golden_hessians(cores, oracle_sigmas, batch):
    """covo_sigma on closed-loop Hessians, batch 1, 3 and 9 (9: not a multiple of 8, the batched tail's last XCD round is ragged):
    Sigma, L, SC_ITERS and SC_KWIN bit-equal between the persistent plan (two launches for one matrix, the batched tail for more) and
    the phased plan; a matrix of a batch equals the same matrix alone; Sigma within 1e-6 of the eigh oracle."""
    persistent, phased = cores
    mats = golden_hessians()[:batch]
    R_d = torch.from_numpy(np.stack(mats)).to(DEV)
    outs = []
    for c in (phased, persistent):
        Sig, L = c.sigma(R_d, 0.5, batch=batch)
        outs.append((Sig.clone(), L.clone(), chain_scalars(c, batch)))
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][2] == outs[1][2], outs
    Sig1, L1 = persistent.sigma(R_d[batch - 1:batch].contiguous(), 0.5)
    assert torch.equal(Sig1[0], outs[0][0][batch - 1]) and torch.equal(L1[0], outs[0][1][batch - 1])
    assert chain_scalars(persistent, 1)[0] == outs[0][2][batch - 1]
    for i in range(batch):
        ref = oracle_sigmas[0][i]
        err = np.linalg.norm(outs[1][0][i].cpu().numpy() - ref) / np.linalg.norm(ref)
        print(f"batch {batch} matrix {i}: Sigma rel err {err:.3e}, (iters, kwin) {outs[1][2][i]}")
        assert err < 1e-6, (i, err)


def test_chain_cheap_convergence_plans_agree(cores, oracle_sigmas):
    """Matrices whose chain converges within its first iterations (cheap_matrices): the phases that find the iteration
    converged and leave -- behind operand loads that were already issued -- are the same on every plan."""
    persistent, phased = cores
    mats = cheap_matrices()
    for i, Rm in enumerate(mats):
        R_d = torch.from_numpy(Rm[None].copy()).to(DEV)
        outs = []
        for c in (phased, persistent):
            Sig, L = c.sigma(R_d, 0.5)
            outs.append((Sig.clone(), L.clone(), chain_scalars(c, 1)))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert outs[0][2] == outs[1][2], outs
        ref = oracle_sigmas[1][i]
        err = np.linalg.norm(outs[1][0][0].cpu().numpy() - ref) / np.linalg.norm(ref)
        print(f"cheap matrix {i}: Sigma rel err {err:.3e}, (iters, kwin) {outs[1][2][0]}")
        assert err < 1e-6, (i, err)
    # and as a batch (batched tail: the last NS_BATCH_TAIL_ITERS iterations find nothing left to do)
    R_b = torch.from_numpy(np.stack(mats)).to(DEV)
    Sp, Lp = phased.sigma(R_b, 0.5, batch=2)
    Sb, Lb = persistent.sigma(R_b, 0.5, batch=2)
    assert torch.equal(Sp, Sb) and torch.equal(Lp, Lb)
    assert torch.equal(Sb[1], outs[1][0][0]) and torch.equal(Lb[1], outs[1][1][0])


@pytest.mark.parametrize("graph", ["graph", "eager"])
@pytest.mark.parametrize("N", [1000, 4096])
def test_full_step_plans_agree_ragged_samples(N, graph, monkeypatch):
    """Closed-loop covo-online steps at N = 1000 (ragged: no multiple of the GEMM's and the rollout's tiles) and N = 4096, eager
    and as a captured graph: actions, costs, a_cov, the new mean and u bit-equal between covo_debug_set_stream_gemm(h, 0 / 1)
    (plain / streamed finalize: the 8-wave factorisation without / with its hook) and between covo_debug_set_ns_merged(h, 0 / 1)
    (two launches / the merged chain launch)."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    lib = _lib.load_library()
    params = env.default_params
    ctrls = []
    for stream_gemm, merged in ((1, 1), (0, 1), (1, 0)):
        c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
        _lib.check(lib.covo_debug_set_stream_gemm(c.core.h, stream_gemm), "stream_gemm")
        _lib.check(lib.covo_debug_set_ns_merged(c.core.h, merged), "ns_merged")
        ctrls.append(c)
    obs, info, state = env.reset(cr.PRNGKey(61), params)
    cps = [c.reset(state, params, c.init_control_params, cr.PRNGKey(5)) for c in ctrls]
    key = cr.PRNGKey(62)
    for step in range(5):
        key, k_act, k_step = cr.split(key, 3)
        outs = []
        for i, c in enumerate(ctrls):
            u, cps[i], _ = c(obs, state, params, k_act, cps[i], info)
            outs.append((cps[i].a_mean.clone(), c.core.a.clone(), c.core.cost.clone(), cps[i].a_cov.clone(), u.clone()))
        for j in (1, 2):
            for what, x, y in zip(("a_mean", "a", "cost", "a_cov", "u"), outs[0], outs[j]):
                assert torch.equal(x, y), (N, graph, step, j, what, (x - y).abs().max().item())
        obs, state, reward, done, info = env.step(k_step, state, outs[0][4].cpu().numpy(), params)
    assert all(c.core.device_status() == 0 for c in ctrls) and torch.isfinite(outs[0][0]).all()
    for c in ctrls:
        c.core.close()
