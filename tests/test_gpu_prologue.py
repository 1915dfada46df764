"""GPU tests (-m gpu) of the finalize launches' prologues (sigma_ns.hip: ns_finalize_stream_kernel, ns_finalize_kernel).  The
factoring workgroup asks for every scalar slot in one round trip, sends the Z loads out as soon as SC_ZBUF is back (column panel 0's
tiles first), waits for log det B under them and forms cz in a wave that waits anyway: a change of ORDER and of who computes what,
not of one arithmetic operation -- so every output must still equal, bit for bit, the in-tree path that computes the same thing
with other code:

  * the streamed finalize (factoring workgroup + GEMM workers) against the plain finalize launch with the noise GEMM as a launch
    of its own (covo_debug_set_stream_gemm(h, 1 / 0)) over closed-loop covo-online steps, N = 4096 and the ragged N = 1000, with and
    without deflation (zc != 0 / zc == 0 in the fill), on Sigma (a_cov), L, the actions, the costs and the new mean;
  * the plain finalize launch of covo_sigma on the golden Hessians and on the w01 family of test_sigma_deflation_on_real_hessians
    (degenerate and isolated ends): merged chain launch == two launches == phased plan, batch 3 == single.

  * the Hessian's adjoint launches (KB / KC / KD) against the per-pair twin covo_hessian_pairs, and merge_kernel against the
    one-launch small step's in-kernel merge (further down: these launches' entries were stamped with this change, not altered).

Both Z buffers must be read (SC_ZBUF = 0 and 1: an even and an odd Newton-Schulz count).  The fused step takes its Hessian from
the state -- there is no entry point that feeds it a matrix -- so for the streamed launch the two parities come from the steps of
the closed loop and for covo_sigma from the golden matrices; each test ASSERTS that it has seen both.
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
from tests.gpu_support import DEV, DP, dev_state, params_c, perturbed_hover_mean  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N_A = 128
SC_COUNT = 3712  # doubles of per-matrix scalars behind the chain's 11 matrix buffers (sigma_ns.hip: enum SC_*)
SC_ZBUF, SC_ITERS, SC_BARFAIL, SC_ZCOEF = 5, 6, 26, 30


def chain_slots(core, batch=1):
    """(SC_ZBUF, SC_ITERS, SC_ZCOEF != 0) of every matrix of the handle's last Sigma chain; no barrier of the chain timed out"""
    out = torch.zeros(32, dtype=torch.float64, device=DEV)
    res = []
    for b in range(batch):
        _lib.check(core.lib.covo_debug_sigma_workspace(core.h, _lib.ptr(out), 11 * batch * N_A * N_A + b * SC_COUNT, 32, core.stream()))
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert o[SC_BARFAIL] == 0.0, b
        res.append((int(o[SC_ZBUF]), int(o[SC_ITERS]), bool(o[SC_ZCOEF] != 0.0)))
    return res


# closed-loop steps per case: enough for both Z buffers to occur (the count falls by one or two once the plan has settled);
# which steps read which buffer is printed
STEPS = 8


@pytest.mark.parametrize("deflate", [1, 0])
@pytest.mark.parametrize("N", [4096, 1000])
def test_streamed_finalize_equals_plain_finalize_both_z_buffers(N, deflate):
    """covo_debug_set_stream_gemm(h, 1) against (h, 0) on two handles driven through the same closed loop: a_cov, tril(L), actions,
    costs, new mean and u bit-equal at every step, SC_ZBUF / SC_ITERS / deflated-or-not equal, and over the steps the chain
    ends in EACH of the two Z buffers; deflation on: steps are deflated (zc != 0), off: none is (zc == 0)."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    lib = _lib.load_library()
    params = env.default_params
    ctrls = []
    for stream_gemm in (1, 0):
        c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
        _lib.check(lib.covo_debug_set_stream_gemm(c.core.h, stream_gemm), "stream_gemm")
        _lib.check(lib.covo_debug_set_ns_deflate(c.core.h, deflate), "ns_deflate")
        ctrls.append(c)
    try:
        obs, info, state = env.reset(cr.PRNGKey(61), params)
        cps = [c.reset(state, params, c.init_control_params, cr.PRNGKey(5)) for c in ctrls]
        key = cr.PRNGKey(62)
        seen = []
        for step in range(STEPS):
            key, k_act, k_step = cr.split(key, 3)
            outs, slots = [], []
            for i, c in enumerate(ctrls):
                u, cps[i], _ = c(obs, state, params, k_act, cps[i], info)
                # (the lower triangle of L: the streamed launch sends exactly that and its readers mask by column <= row; what lies
                # above the diagonal of the handle's buffer is whatever the allocation held)
                outs.append((cps[i].a_cov.clone(), torch.tril(c.core.sigma_factor()), c.core.a.clone(), c.core.cost.clone(),
                             cps[i].a_mean.clone(), u.clone()))
                slots.append(chain_slots(c.core)[0])
            print(f"N {N} deflate {deflate} step {step}: (zbuf, iters, deflated) streamed {slots[0]} plain {slots[1]}")
            assert slots[0] == slots[1], (step, slots)
            assert deflate or not slots[0][2], (step, slots)  # (switched off: zc == 0 on every step)
            for what, x, y in zip(("a_cov", "L", "a", "cost", "a_mean", "u"), *outs):
                assert torch.equal(x, y), (N, deflate, step, what, (x - y).abs().max().item())
            assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all() and torch.isfinite(outs[0][4]).all()
            seen.append(slots[0])
            obs, state, reward, done, info = env.step(k_step, state, outs[0][5].cpu().numpy(), params)
        assert all(c.core.device_status() == 0 for c in ctrls)
        assert {z for z, _, _ in seen} == {0, 1}, seen  # the Z loads were aimed at each of the two buffers
        assert not deflate or any(d for _, _, d in seen), seen  # (switched on: zc != 0 was exercised)
    finally:
        for c in ctrls:
            c.core.close()


def golden_hessians():
    g = np.load(os.path.join(HERE, "golden", "hessians_r03.npz"))
    return [np.ascontiguousarray(m) for k in g.files for m in g[k]]


def w01_matrices():
    """test_sigma_deflation_on_real_hessians's family at its two ends: bottom gap 1e-9 (degenerate: deflation declines, zc == 0)
    and 3.0 (isolated)"""
    rng = np.random.default_rng(4)
    A = rng.normal(size=(128, 128))
    w, U = np.linalg.eigh(0.05 * (A + A.T))
    mats = []
    for w01 in (1e-9, 3.0):
        ww = w.copy()
        ww[0] = ww[1] - w01
        mats.append(np.ascontiguousarray((U * ww) @ U.T))
    return mats


@pytest.fixture(scope="module")
def sigma_cores():
    merged = SamplingCore(256, 32, 0.01, 1.0, device=DEV)                      # one matrix: the merged chain launch
    two = SamplingCore(256, 32, 0.01, 1.0, device=DEV)                         # ... its two launches
    _lib.check(two.lib.covo_debug_set_ns_merged(two.h, 0), "ns_merged")
    phased = SamplingCore(256, 32, 0.01, 1.0, device=DEV, shared_device=True)  # every phase its own launch
    yield merged, two, phased
    for c in (merged, two, phased):
        c.close()


def test_plain_finalize_plans_agree_both_z_buffers(sigma_cores):
    """covo_sigma (ns_finalize_kernel) on the golden Hessians and, with deflation on and off, on the two w01 ends: Sigma, L and the
    chain's slots bit-equal between the merged chain launch, the two-launch plan and the phased plan; a batch of 3 equals its
    matrices alone; both Z buffers and both zc == 0 and zc != 0 occur."""
    gold, w01 = golden_hessians(), w01_matrices()
    cases = [(m, 1) for m in gold] + [(m, d) for m in w01 for d in (1, 0)]
    singles = []
    try:
        for i, (Rm, deflate) in enumerate(cases):
            R_d = torch.from_numpy(Rm[None].copy()).to(DEV)
            outs = []
            for c in sigma_cores:
                _lib.check(c.lib.covo_debug_set_ns_deflate(c.h, deflate), "ns_deflate")
                Sig, L = c.sigma(R_d, 0.5)
                outs.append((Sig[0].clone(), L[0].clone(), chain_slots(c)[0]))
            print(f"case {i} (deflation {'on' if deflate else 'off'}): (zbuf, iters, deflated) {outs[0][2]}")
            assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all(), i
            assert deflate or not outs[0][2][2], (i, outs[0][2])
            for j in (1, 2):
                assert torch.equal(outs[0][0], outs[j][0]) and torch.equal(outs[0][1], outs[j][1]), (i, j)
                assert outs[0][2] == outs[j][2], (i, j, outs[0][2], outs[j][2])
            singles.append(outs[0])
    finally:
        for c in sigma_cores:
            _lib.check(c.lib.covo_debug_set_ns_deflate(c.h, 1), "ns_deflate")
    assert {s[2][0] for s in singles} == {0, 1}, [s[2] for s in singles]
    assert {s[2][2] for s in singles} == {False, True}, [s[2] for s in singles]
    # batches of 3 (the batched tail + the finalize launch's sibling log det workgroups): golden, and both w01 ends with a golden one
    ng = len(gold)
    for idx in ((0, 1, 2), (ng, ng + 2, ng - 1)):  # (cases ng and ng + 2: the w01 ends with deflation on)
        R_b = torch.from_numpy(np.stack([cases[k][0] for k in idx])).to(DEV)
        for c in (sigma_cores[0], sigma_cores[2]):
            Sb, Lb = c.sigma(R_b, 0.5, batch=3)
            slots = chain_slots(c, 3)
            for k, src in enumerate(idx):
                assert torch.equal(Sb[k], singles[src][0]) and torch.equal(Lb[k], singles[src][1]), (idx, k)
                assert slots[k] == singles[src][2], (idx, k)


# ------------------------------------------------------------------------------------------ Hessian (KB / KC / KD)
# The adjoint launches against their per-pair twin (covo_hessian_pairs: hyper-dual arithmetic, no chains, no KD) at the 1e-9 bar of
# tests/test_gpu_parity.py / test_gpu_state_atlas.py, batch-of-2 == single calls bit for bit, R exactly symmetric: adj13 without
# and with a force table, adj16 (drag: the force is part of the differentiated state), at two entries of tests/state_atlas.py.
HESS_MODELS = {"adj13": None, "adj13_table": ("periodic", "realworld"), "adj16": ("drag", "penyaw")}
HESS_ENTRIES = ("far_fast", "yaw_cross")


@pytest.mark.parametrize("model", list(HESS_MODELS))
def test_hessian_adjoint_equals_pairs_batch_equals_single(model):
    from covo_mpc_amd import random as cr
    from covo_mpc_amd.dynamics.dataclass import EnvParams3D
    from tests.state_atlas import atlas_state
    core = SamplingCore(256, 32, 0.01, 1.0, device=DEV)
    try:
        states, means, tabs, singles = [], [], [], []
        for e, name in enumerate(HESS_ENTRIES):
            s, p, rng = atlas_state(name)
            if HESS_MODELS[model] is None:
                pc = EnvParams3D().to_c()
            else:
                p = p.replace(disturb_params=DP)
                pc = params_c(p, *HESS_MODELS[model])
            a = torch.from_numpy(perturbed_hover_mean(p, rng, 0.1)).to(DEV)
            ds = dev_state(s)
            tab = None
            if HESS_MODELS[model] is not None:
                tab = core.disturb_table(pc, ds.packed, key=cr.PRNGKey(21 + e), key_mode=_lib.DISTURB_KEYS_HESSIAN, deterministic=True)
            res = {m: core.hessian(ds.packed, ds, pc, a, method=m, f_steps=tab)[0].clone() for m in ("adjoint", "pairs")}
            Ra, Rp = res["adjoint"].cpu().numpy(), res["pairs"].cpu().numpy()
            err, big = np.abs(Ra - Rp).max(), np.abs(Rp).max()
            print(f"{model} {name}: |adjoint - pairs| {err:.2e}, max|R| {big:.3g}, relative {err / max(1.0, big):.2e}")
            assert np.all(np.isfinite(Ra)) and np.abs(Ra).max() > 0
            assert np.array_equal(Ra, Ra.T), (model, name)
            assert err < 1e-9 * max(1.0, big), (model, name, err, big)
            states.append(ds)
            means.append(a)
            tabs.append(tab)
            singles.append(res["adjoint"])
        packed = torch.stack([d.packed for d in states])
        tab2 = None if tabs[0] is None else torch.cat(tabs).contiguous()
        Rb = core.hessian(packed, states[0], pc, torch.stack(means), batch=2, f_steps=tab2)
        for e, name in enumerate(HESS_ENTRIES):
            assert torch.equal(Rb[e], singles[e]), (model, name, (Rb[e] - singles[e]).abs().max().item())
        assert core.device_status() == 0
    finally:
        core.close()


# ------------------------------------------------------------------------------------------ merge_kernel
# merge_kernel (the staged step's last launch; covo_debug_set_fuse_small(h, 0)) against the one-launch small step's in-kernel merge
# (softmax_merge.hpp: merge_body on 192 ... 1 024 threads) on the same 2, 17 and 256 records: covo-offline at N = 128, 1 088 and
# 16 384 (64 samples per record), bit for bit; `late`: the state's clock at 299, so that time + k >= 300 for every k >= 1 -- the
# costs (nearly) coincide and every sample carries weight.
@pytest.mark.parametrize("late", [False, True])
@pytest.mark.parametrize("N", [128, 1088, 16384])
def test_merge_kernel_equals_in_kernel_merge(N, late, monkeypatch):
    import covo_mpc_amd as cm
    from covo_mpc_amd import random as cr
    env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                         generate_noisy_state=True, device=DEV)
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    lib = _lib.load_library()
    params = env.default_params
    lam = 0.01
    res = []
    for fuse in (1, 0):
        c, _ = cm.envs.get_controller(env, "covo-offline", f"N{N}_H32_lam{lam}", device=DEV, compute_info=False)
        try:
            _lib.check(lib.covo_debug_set_fuse_small(c.core.h, fuse), "fuse_small")
            obs, info, state = env.reset(cr.PRNGKey(14), params)
            cp = c.reset(state, params, c.init_control_params, cr.PRNGKey(5))
            key = cr.PRNGKey(16)
            out = []
            for step in range(3):
                key, k_act, k_step = cr.split(key, 3)
                st, inf = state, info
                if late and step == 2:  # the last step plans from the episode's end
                    st = state.replace(time=299)
                    inf = dict(info, noisy_state=info["noisy_state"].replace(time=299))
                u, cp, _ = c(obs, st, params, k_act, cp, inf)
                out.append((cp.a_mean.clone(), c.core.a.clone(), c.core.cost.clone(), u.clone()))
                obs, state, reward, done, info = env.step(k_step, state, u.cpu().numpy(), params)
            assert c.core.device_status() == 0
            res.append(out)
        finally:
            c.core.close()
    for step, (f, s) in enumerate(zip(*res)):
        for what, x, y in zip(("a_mean", "a", "cost", "u"), f, s):
            assert torch.equal(x, y), (N, late, step, what, (x - y).abs().max().item())
    cost = res[0][-1][2].double()
    wmin = torch.exp(-(cost.max() - cost.min()) / lam).item()
    print(f"N {N} late {late}: cost spread {(cost.max() - cost.min()).item():.3e}, smallest weight {wmin:.3e}")
    assert torch.isfinite(res[0][-1][0]).all()
    if late:
        assert wmin > 1e-30, (N, wmin)  # every sample's fp32 weight exp(-(c - min) / lam) is a normal number: all of them count
