"""GPU (-m gpu): covo_cholesky at every size and dispatch path, and the factor inside covo_sigma_jacobi, against LAPACK to one fp32 ulp.

launch_cholesky / cholesky_kernel (csrc/sigma.hip) pick between the scalar body (cholesky_lds; 64 threads for n < 8, 256 for the other
n that are no multiple of 8) and the panel body (chol_lds_fast, csrc/chol_lds.hpp; one wave at n = 8, four otherwise, rows split over
two register slots); covo_sigma_jacobi runs the panel body with 512 threads.  The kernel symmetrises the fp32 input in fp64, factors in
fp64 and rounds once, so against tests/chol_cases.py: chol_ref (the same on the host with LAPACK) every lower-triangle entry must obey

    |L_dev - L_ref| <= ulp32(L_ref[i][j]) + 16 FWD64 max|L_ref|

(the floor pays for the kernel's operation order, its FMAs and rsqrt + Newton in place of sqrt and a division; FWD64 is the distance
of two host factorisations before rounding, tests/test_chol_cases.py), and pooled over a test's matrices >= 99.9 % of the entries
must equal chol_ref bit for bit -- ten times the miss rate the two host references show against each other.  The output buffer is
pre-filled with NaN, so an entry the kernel forgets shows.

Measured on the MI355X (printed by the tests with -s):
    covo_cholesky, 104 family cases      217 300 entries, 0 differ: share 1.0000000, largest distance 0 ulp
    covo_cholesky, batch 300 x 128     2 476 800 entries, 1 differs: share 0.9999996, largest distance 1 ulp
    covo_cholesky, batch 1000 x 5         15 000 entries, 0 differ: share 1.0000000, largest distance 0 ulp
    covo_cholesky, batch 600 x 16         81 600 entries, 0 differ: share 1.0000000, largest distance 0 ulp
    covo_sigma_jacobi, 18 matrices       148 608 entries, 0 differ: share 1.0000000, largest distance 0 ulp

What the bar sees that 1e-6 absolute did not (scratch builds of the kernel, not kept): the panel body's trailing update accumulated
in float moves most entries by 2-3 ulp and fails every multiple of 8 from n = 16 on (first: spectrum cond 1e1 at n = 16, L[9][8]),
the batches 300 x 128 and 600 x 16 and covo_sigma_jacobi; the pivot slot sj forced to 0 gives non-finite factors at n = 72, 120, 128
and in covo_sigma_jacobi.  Two edits change no value the kernel ever reads and so pass, as they must: the guard lane + 64 <= n only
adds row n, the padding element of the column stride ld = n + 1 (and at n = 128 there is no lane 64), and the scalar
body without its i >= c test only updates the strict upper triangle of the LDS image, which is neither read nor written out.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd._lib import ptr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from tests import chol_cases as CC  # noqa: E402
from tests.conftest import make_problem  # noqa: E402
from tests.gpu_support import DEV  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SHARE = 0.999


@pytest.fixture(scope="module")
def core():
    return SamplingCore(256, 32, 0.01, 1.0, device=DEV)


def factor(core, A, n=None, batch=None, null_in=False, null_out=False):
    """covo_cholesky through the C ABI on fp32 [batch, n, n] -> (status, L with NaN wherever nothing was written, A as the device
    holds it afterwards)."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    n = A.shape[-1] if n is None else n
    batch = A.shape[0] if batch is None else batch
    a = torch.from_numpy(A).to(DEV)
    out = torch.full_like(a, float("nan"))
    rc = core.lib.covo_cholesky(core.h, None if null_in else ptr(a), n, batch, None if null_out else ptr(out), core.stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), a.cpu().numpy()


def bar(Lref):
    return CC.ulp32(Lref) + 16 * CC.FWD64 * np.abs(Lref).max()


def check_factor(L, Lref, tag, cols=None):
    """the bars of one matrix (columns < cols only, if given) -> the ulp distances of its lower-triangle entries"""
    n = Lref.shape[0]
    low = np.tril(np.ones((n, n), dtype=bool))
    if cols is not None:
        low[:, cols:] = False
    else:
        assert np.all(np.isfinite(L)), (tag, "non-finite")
        assert not L[np.triu_indices(n, 1)].view(np.uint32).any(), (tag, "strict upper triangle is not +0.0f")
        assert np.all(np.diag(L) > 0), (tag, "diagonal")
    err = np.abs(L.astype(np.float64) - Lref.astype(np.float64))
    assert np.all(np.isfinite(L[low])), (tag, "non-finite")
    over = low & ~(err <= bar(Lref))
    if over.any():
        i, j = np.argwhere(over)[0]
        raise AssertionError(f"{tag}: {int(over.sum())} entries over the bar, first L[{i}][{j}] = {L[i, j]!r} vs {Lref[i, j]!r} "
                             f"({CC.ulp_distance(L[i, j], Lref[i, j])} ulp), max |L| = {np.abs(Lref).max():.3e}")
    return CC.ulp_distance(L[low], Lref[low])


def pooled(dists, what):
    d = np.concatenate(dists)
    share, worst = float(np.mean(d == 0)), int(d.max())
    print(f"{what}: {d.size} lower-triangle entries, {int((d != 0).sum())} differ from chol_ref, bit-identical share {share:.7f}, "
          f"largest distance {worst} ulp")
    return share, d.size


# ------------------------------------------------------------------------------------------ every size, every family
@pytest.fixture(scope="module")
def family(core):
    """one launch per n with that n's cases as the batch -> {n: (names, A, status, L, A afterwards, references)}"""
    out = {}
    for n in CC.NS:
        names, mats = zip(*CC.family_cases(n))
        A = np.stack(mats)
        rc, L, A_after = factor(core, A)
        out[n] = (names, A, rc, L, A_after, [CC.chol_ref(m) for m in mats])
    return out


@pytest.mark.parametrize("n", CC.NS)
def test_every_size_every_family(family, n):
    names, A, rc, L, A_after, refs = family[n]
    assert rc == 0
    assert np.array_equal(A_after.view(np.uint32), A.view(np.uint32)), "the input buffer changed"
    for b, name in enumerate(names):
        check_factor(L[b], refs[b], (n, name))


def test_bit_identity_share_of_the_families(family):
    dists = [check_factor(L[b], refs[b], (n, names[b])) for n, (names, A, rc, L, A_after, refs) in family.items()
             for b in range(len(names))]
    share, count = pooled(dists, "covo_cholesky, family cases")
    assert count > 100000
    assert share >= SHARE, share


# ------------------------------------------------------------------------------------------ batches beyond residency
@pytest.mark.parametrize("n,batch", [(128, 300), (5, 1000), (16, 600)])
def test_batch_beyond_residency(core, n, batch):
    """More workgroups than the device holds at once (n = 128: 129 KiB of LDS, one workgroup per CU): every factor meets the bars, and
    a dozen spread over the batch equal the factor of a batch-1 launch of the same matrix bit for bit."""
    A = CC.batch_cases(n, batch)
    assert len({m.tobytes() for m in A}) == batch
    rc, L, A_after = factor(core, A)
    assert rc == 0 and np.array_equal(A_after.view(np.uint32), A.view(np.uint32))
    dists = [check_factor(L[b], CC.chol_ref(A[b]), (n, batch, b)) for b in range(batch)]
    share, _ = pooled(dists, f"covo_cholesky, batch {batch} x {n}")
    assert share >= SHARE, share
    for b in sorted({int(x) for x in np.linspace(0, batch - 1, 12)}):
        rc1, L1, _ = factor(core, A[b:b + 1])
        assert rc1 == 0 and np.array_equal(L1[0].view(np.uint32), L[b].view(np.uint32)), (n, batch, b)


# ------------------------------------------------------------------------------------------ indefinite input
@pytest.mark.parametrize("n", [5, 8, 72])
def test_indefinite_matrix_stays_in_its_own_workgroup(core, n):
    """A matrix that is not positive definite is not detected: status 0, NaN from the failing pivot on, in that matrix only."""
    clean, bad, p = CC.indefinite(n)
    assert CC.first_bad_pivot(CC._sym64(bad)) == p
    left, right = CC.spectrum(n, 1e3), CC.spectrum(n, 1e5)
    rc, L, A_after = factor(core, np.stack([left, bad, right]))
    assert rc == 0
    assert np.array_equal(A_after[1].view(np.uint32), bad.view(np.uint32))
    rc2, L2, _ = factor(core, np.stack([left, right]))
    assert rc2 == 0
    assert np.array_equal(L[0].view(np.uint32), L2[0].view(np.uint32)) and np.array_equal(L[2].view(np.uint32), L2[1].view(np.uint32))
    check_factor(L[0], CC.chol_ref(left), (n, "left"))
    check_factor(L[2], CC.chol_ref(right), (n, "right"))
    check_factor(L[1], CC.chol_ref(clean), (n, "bad, columns before p"), cols=p)
    assert np.isnan(L[1][p, p])
    rc3, L3, _ = factor(core, clean[None])  # the handle afterwards
    assert rc3 == 0
    check_factor(L3[0], CC.chol_ref(clean), (n, "clean afterwards"))


# ------------------------------------------------------------------------------------------ covo_sigma_jacobi
def sigma_inputs():
    """the four matrices of test_gpu_parity.py: test_sigma_and_cholesky_vs_lapack, and tests/golden/hessians_r03.npz"""
    _, _, rng = make_problem(seed=0, time=37)
    A = rng.normal(size=(128, 128))
    S = 0.05 * (A + A.T)
    B = S.copy()
    B[124:, :] = 0
    B[:, 124:] = 0
    w, U = np.linalg.eigh(S)
    w[1] = w[0] + 1e-7
    w[-1] = w[0] + 40.0
    g = np.load(os.path.join(HERE, "golden", "hessians_r03.npz"))
    return np.stack([S, B, np.eye(128) * 3.0, (U * w) @ U.T] + [m for k in g.files for m in g[k]])


def test_sigma_jacobi_factor_is_the_factor_of_its_sigma(core):
    """chol_lds_fast at 512 threads: the returned L[i] is the factor of the returned fp32 Sigma[i]."""
    Rb = sigma_inputs()
    batch = len(Rb)
    r = torch.from_numpy(np.ascontiguousarray(Rb, dtype=np.float64)).to(DEV)
    Sigma = torch.full((batch, 128, 128), float("nan"), dtype=torch.float32, device=DEV)
    L = torch.full_like(Sigma, float("nan"))
    rc = core.lib.covo_sigma_jacobi(core.h, ptr(r), batch, 0.5, ptr(Sigma), ptr(L), core.stream())
    torch.cuda.synchronize()
    assert rc == 0
    Sigma, L = Sigma.cpu().numpy(), L.cpu().numpy()
    assert np.all(np.isfinite(Sigma))
    dists = []
    for i in range(batch):
        assert np.array_equal(Sigma[i], Sigma[i].T), i
        dists.append(check_factor(L[i], CC.chol_ref(Sigma[i]), ("sigma_jacobi", i)))
    share, count = pooled(dists, "covo_sigma_jacobi")
    assert count > 100000
    assert share >= SHARE, share


# ------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what", ["n=0", "n=129", "batch=0", "null A", "null L_out"])
def test_refusals(core, what):
    """Refused with a non-zero status and a message that names the entry point; nothing is launched (the output keeps its NaN fill),
    and the handle factors correctly afterwards."""
    A = np.stack([CC.spectrum(129, 1e3)])  # large enough for whatever a wrongly accepted call would touch
    kw = {"n=0": dict(n=0), "n=129": dict(n=129), "batch=0": dict(n=8, batch=0), "null A": dict(n=8, null_in=True),
          "null L_out": dict(n=8, null_out=True)}[what]
    rc, L, A_after = factor(core, A, **kw)
    assert rc != 0, what
    msg = core.lib.covo_last_error()
    assert msg and b"covo_cholesky" in msg, (what, msg)
    assert np.all(np.isnan(L)) and np.array_equal(A_after, A), what
    good = CC.spectrum(8, 1e3)
    rc, L, _ = factor(core, good[None])
    assert rc == 0
    check_factor(L[0], CC.chol_ref(good), (what, "afterwards"))
