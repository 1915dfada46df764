"""GPU tests (-m gpu) of the two linear recursions of the adjoint Hessian's chain launch (csrc/hessian_adj_body.hpp:
adj_chain_kernel), which runs each of them as four horizon segments on the four waves of a workgroup and joins the segments:
    S_0 = 0,  S_{k+1} = A_k S_k + B_k E_k          lam_31 = g_31,  lam_k = g_k + A_k^T lam_{k+1}
read back from the workspace (covo_debug_hess_workspace) next to the A_k, B_k, g_k the launch before left there.

Bars.  (1) The recursions against their sequential restatement in numpy fp64 on the read-back operands: the a-priori forward error
bound of a product of n = 31 factors of dimension d = 16 in ANY association (Higham, Accuracy and Stability, (3.12) with
gamma_{n d}), doubled for the restatement's own rounding: |S_k - S_k^ref| <= 2 H 16 2^-53 Shat_k entry-wise, Shat_k the same
recursion on |A_k|, |B_k E_k|; likewise lam with |g_k|.  What the layout pads is exactly zero, and so is tile w of S_k for k <= 4w.
(2) Launch shapes: batch 3 (one launch), batch 9 and batch 40 (chains and hyper-dual workgroups as two launches; at 40 chain
workgroups share CUs, which moves the waves of a workgroup against each other) bit-equal to the single calls.  (3) A NaN
(norm'(0) at a state that sits on its target) reaches the rows of lam the sequential restatement gives and the entries of R the
oracle's AD gives.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from covo_mpc_amd.dynamics.dataclass import EnvParams3D  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from tests.conftest import make_problem  # noqa: E402
from tests.gpu_support import DEV, DP, dev_state, params_c, perturbed_hover_mean  # noqa: E402
from tests.state_atlas import atlas_state  # noqa: E402

H, NA = 32, 128
STATES = ("far_fast", "roll_120_spin")
VARIANTS = {"adj13": ("none", 13), "adj13_table": ("periodic", 13), "adj16": ("drag", 16)}
BAR = 2 * H * 16 * 2.0 ** -53


def layout(nx):
    """offsets (doubles) of one matrix's workspace, csrc/hessian_adj_body.hpp WS_*"""
    nz = nx + 4
    o = dict(X=0)
    o["JF"] = o["X"] + 32 * 16
    o["GL"] = o["JF"] + 32 * nx * nz
    o["LAM"] = o["GL"] + 32 * 16
    o["MXX"] = o["LAM"] + 33 * 16
    o["MXU"] = o["MXX"] + 32 * 256
    o["MUU"] = o["MXU"] + 32 * 64
    o["S"] = o["MUU"] + 32 * 16
    o["COUNT"] = o["S"] + 32 * 16 * NA + 2
    return o


def read_workspace(core, nx, b=0):
    """-> A [31, nx, nx], B [31, nx, 4], g [32, 16], lam [33, 16], S [32, 16, 128] of batch entry b of the last Hessian call"""
    o = layout(nx)
    out = torch.zeros(o["COUNT"], dtype=torch.float64)
    _lib.check(core.lib.covo_debug_hess_workspace(core.h, _lib.ptr(out), C.c_int64(b * o["COUNT"]), C.c_int64(o["COUNT"]),
                                                  core.stream()), "covo_debug_hess_workspace")
    torch.cuda.synchronize()
    w = out.numpy()
    jf = w[o["JF"]:o["GL"]].reshape(32, nx, nx + 4)[:31]
    return dict(A=jf[:, :, :nx].copy(), B=jf[:, :, nx:].copy(), g=w[o["GL"]:o["LAM"]].reshape(32, 16).copy(),
                lam=w[o["LAM"]:o["MXX"]].reshape(33, 16).copy(), S=w[o["S"]:o["S"] + 32 * 16 * NA].reshape(32, 16, NA).copy())


def sequential(A, B, g, nx):
    """both recursions step by step in fp64 -> S [32, nx, 128], lam [32, nx] (row 0 unused: the launch stores rows 1 .. 31)"""
    S = np.zeros((H, nx, NA))
    for k in range(H - 1):
        S[k + 1] = A[k] @ S[k]
        S[k + 1][:, 4 * k:4 * k + 4] += B[k]
    lam = np.zeros((H, nx))
    lam[H - 1] = g[H - 1, :nx]
    for k in range(H - 2, 0, -1):
        lam[k] = g[k, :nx] + A[k].T @ lam[k + 1]
    return S, lam


@functools.lru_cache(maxsize=None)
def _core():
    return SamplingCore(256, 32, 0.01, 1.0, device=DEV)


@functools.lru_cache(maxsize=None)
def _inputs(name, variant):
    kind, nx = VARIANTS[variant]
    s, p, rng = atlas_state(name)
    a = perturbed_hover_mean(p, rng, 0.5)
    core, ds = _core(), dev_state(s)
    if kind == "none":
        return ds, EnvParams3D().to_c(), torch.from_numpy(a).to(DEV), None, nx
    pc = params_c(p.replace(disturb_params=DP), kind, "penyaw")
    tab = core.disturb_table(pc, ds.packed, key=cr.PRNGKey(21), key_mode=_lib.DISTURB_KEYS_HESSIAN, deterministic=True)
    return ds, pc, torch.from_numpy(a).to(DEV), tab, nx


@functools.lru_cache(maxsize=None)
def _single(name, variant):
    """one core.hessian call -> its R and the workspace behind it; computed once, shared, left unchanged"""
    ds, pc, a, tab, nx = _inputs(name, variant)
    core = _core()
    Rm = core.hessian(ds.packed, ds, pc, a, f_steps=tab)[0].cpu().numpy()
    ws = read_workspace(core, nx)
    assert core.device_status() == 0
    return Rm, ws


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", STATES)
def test_recursions_against_their_sequential_restatement(name, variant):
    nx = VARIANTS[variant][1]
    Rm, ws = _single(name, variant)
    A, B, g, lam, S = ws["A"], ws["B"], ws["g"], ws["lam"], ws["S"]
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(B)) and np.all(np.isfinite(g))
    Sref, lref = sequential(A, B, g, nx)
    Shat, lhat = sequential(np.abs(A), np.abs(B), np.abs(g), nx)
    eS, el = np.abs(S[:, :nx] - Sref), np.abs(lam[1:H, :nx] - lref[1:])  # (row 0 of lam: never stored)
    lhat = lhat[1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        rS, rl = np.max(np.where(Shat > 0, eS / Shat, 0.0)), np.max(np.where(lhat > 0, el / lhat, 0.0))
    print(f"  {name} {variant}: max |S - ref| / Shat {rS:.2e}, max |lam - ref| / lamhat {rl:.2e}, bar {BAR:.2e}")
    assert np.all(eS <= BAR * Shat), (name, variant, rS)
    assert np.all(el <= BAR * lhat), (name, variant, rl)
    # every tile of S and every segment of both chains is live
    for w in range(8):
        assert np.all(np.abs(S[4 * w + 1:, :nx, 16 * w:16 * w + 16]).max(axis=(1, 2)) > 0), (name, variant, w)
        assert np.all(S[:4 * w + 1, :, 16 * w:16 * w + 16] == 0.0), (name, variant, w)
    assert np.all(np.abs(lam[1:H, :nx]).max(axis=1) > 0)
    # what the layout pads
    assert np.all(S[:, nx:] == 0.0) and np.all(lam[1:H, nx:] == 0.0) and np.all(lam[H] == 0.0)
    assert np.all(Rm[124:] == 0.0) and np.all(Rm[:, 124:] == 0.0) and np.array_equal(Rm, Rm.T)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("batch", [3, 9, 40])  # 40: more chain workgroups than CUs to take one each
def test_launch_shapes_equal_the_single_calls(batch, variant):
    nx = VARIANTS[variant][1]
    names = [STATES[i % len(STATES)] for i in range(batch)]
    single = [_single(n, variant) for n in names]
    ins = [_inputs(n, variant) for n in names]
    core = _core()
    packed = torch.stack([i[0].packed for i in ins])
    am = torch.stack([i[2] for i in ins])
    tab = None if ins[0][3] is None else torch.cat([i[3] for i in ins])
    Rb = core.hessian(packed, ins[0][0], ins[0][1], am, batch=batch, f_steps=tab).cpu().numpy()
    for b in range(batch):
        ws = read_workspace(core, nx, b)
        assert np.array_equal(Rb[b], single[b][0]), (variant, batch, b, np.abs(Rb[b] - single[b][0]).max())
        assert np.array_equal(ws["S"], single[b][1]["S"]), (variant, batch, b)
        assert np.array_equal(ws["lam"][1:], single[b][1]["lam"][1:]), (variant, batch, b)
    assert core.device_status() == 0


@functools.lru_cache(maxsize=None)
def _nan_case():
    """the reset state of a fixed target: position and velocity sit exactly on their targets, and (the position moves with the
    PRE-step velocity) so does the position of step 1 -- norm'(0) is NaN there (tests/test_gpu_models.py:313)"""
    s, p, rng = make_problem(0, 0, task="fixed")
    s = s.replace(pos=s.pos_tar.copy(), vel=s.vel_tar.copy())
    a = perturbed_hover_mean(p, rng, 0.5)
    core, ds = _core(), dev_state(s)
    Rm = core.hessian(ds.packed, ds, EnvParams3D().to_c(), torch.from_numpy(a).to(DEV))[0].cpu().numpy()
    ws = read_workspace(core, 13)
    assert core.device_status() == 0
    return s, p, a, Rm, ws


def test_nan_reaches_the_rows_of_the_costate_it_reaches_sequentially():
    s, p, a, Rm, ws = _nan_case()
    assert np.isnan(ws["g"]).any()
    A16, g = np.zeros((31, 16, 16)), ws["g"]
    A16[:, :13, :13] = ws["A"]
    lam = np.zeros((H, 16))  # the sequential chain on the zero-padded operands: 0 x NaN = NaN, as on the matrix cores
    lam[H - 1] = g[H - 1]
    with np.errstate(invalid="ignore"):
        for k in range(H - 2, 0, -1):
            lam[k] = g[k] + np.einsum("ij,i->j", A16[k], lam[k + 1])
    got, want = np.isnan(ws["lam"][1:H]), np.isnan(lam[1:])
    print(f"  NaN rows of lam: device {np.argwhere(got).tolist()}, sequential {np.argwhere(want).tolist()}")
    assert want.any()
    assert np.array_equal(got, want)


def test_nan_reaches_the_entries_of_the_hessian_it_reaches_in_the_oracle():
    """The oracle's AD holds a NaN in all 16 384 entries here: every pair's rollout passes step 1, whose position sits on its target
    (the position moves with the pre-step velocity), and multiplies norm'(0) by a zero.  The kernels' tiles skip the steps whose
    sensitivity is zero and would keep the NaN to the tile R[0:16, 0:16] (256 entries: what they gave before the chain launch was
    segmented, too); adj_gemm_kernel lays a NaN of the costate over every tile."""
    s, p, a, Rm, ws = _nan_case()
    ref = CO.hessian(s, p, a.astype(np.float64), 32)
    got, want = np.isnan(Rm), np.isnan(ref)
    print(f"  NaN entries of R: device {int(got.sum())}, oracle {int(want.sum())}, in one only {int((got != want).sum())}")
    assert want.any()
    assert np.array_equal(got, want)
