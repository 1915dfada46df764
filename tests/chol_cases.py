"""Deterministic cases and host references for the batched Cholesky (covo_cholesky, csrc/sigma.hip: cholesky_kernel; and the factor
inside covo_sigma_jacobi): shared by tests/test_chol_cases.py (CPU: the two references against each other) and
tests/test_gpu_cholesky.py (the device against chol_ref).  numpy only, no device, no pytest.

What the kernel computes: the fp32 input is symmetrised as (A + A^T)/2 in fp64, factored in fp64 and rounded once to fp32.  Two host
restatements of that:

    chol_ref   LAPACK dpotrf on the fp64 image, rounded to fp32                  (the reference of the GPU test)
    chol_ld    the same factorisation column by column in np.longdouble          (independent; CPU test only)

The bar of the GPU test is one fp32 ulp of the reference entry plus a floor of 16 FWD64 max|L|, where FWD64 bounds the distance of the
two references' unrounded factors over every positive-definite case below (tests/test_chol_cases.py measures it on every run).
"""
import numpy as np

# Every n in [1, 128] is promised (include/covo_hip.h); the dispatch of launch_cholesky / cholesky_kernel and the bookkeeping of
# chol_lds_fast decide which sizes can go wrong independently:
#   1, 2, 3, 4, 5, 7   scalar body (cholesky_lds), 64 threads; 1: no trailing update at all, 7: the last size before the panel body
#   8                  panel body (chol_lds_fast) in ONE wave: wave 0 factors the panel, no worker wave, no trailing column
#   9, 15, 17, 63,     scalar body at 256 threads (the m * m trailing loop spread over four waves); 9: the first 256-thread size,
#   65, 127            63 / 65: either side of the wave width, 127: the largest, dynamic LDS above 64 KiB
#   16, 24, 56, 64     panel body, second register slot (rows lane + 64) empty; 16: the first size with a trailing update,
#                      64: slot 0 exactly full
#   72, 120            panel body, second slot ragged (8 and 56 rows); the panel at j0 = 64 takes its pivots from slot 1 with n < 128;
#                      120 (like 127, 128) needs the dynamic-LDS opt-in (n (n + 1) 8 B > 64 KiB from n = 91 on)
#   128                panel body, both slots full (the size the suite always had)
NS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 56, 63, 64, 65, 72, 120, 127, 128)
NS_EDGE = (5, 8, 24, 72, 127, 128)  # scaled / graded / asym / indefinite: each body, 64 and 256 threads, slot 1 empty, ragged and full
CONDS = (1e1, 1e3, 1e5, 1e6)

# max |L64 - L_ld| / max |L64| over the positive-definite cases: measured 7.9e-14 (the worst: spectrum, cond 1e6, n = 128; about
# cond x 2^-53 / 1400).  The constant is that figure with a factor 2.5 for another LAPACK build's operation order, and
# test_chol_cases.py fails if a case ever exceeds it.  16 FWD64 = 3.2e-12 is still four orders below one fp32 ulp of max|L| (6e-8).
FWD64 = 2e-13


def _sym64(A32):
    A64 = np.asarray(A32).astype(np.float64)
    return 0.5 * (A64 + A64.T)


def chol_ref(A32):
    """cholesky_kernel restated: symmetrise the fp32 input in fp64, factor in fp64 (LAPACK), round once to fp32.  This is also what
    jax.lax.linalg.cholesky does with its default symmetrize_input=True (there in the input's own precision)."""
    return np.linalg.cholesky(_sym64(A32)).astype(np.float32)


def chol_ld(A64):
    """The lower factor of the symmetric matrix A64 column by column (left-looking) in np.longdouble -> longdouble [n, n].  Only the
    lower triangle of A64 is read."""
    A = np.asarray(A64).astype(np.longdouble)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        d = np.sqrt(v[0])
        L[j, j] = d
        L[j + 1:, j] = v[1:] / d
    return L


def pivots(A64):
    """The pivots d_j = A[j][j] - sum_{k<j} L[j][k]^2 of the fp64 right-looking elimination, up to and including the first one
    that is <= 0 (the elimination stops there)."""
    S = np.array(A64, dtype=np.float64)
    n = S.shape[0]
    out = []
    for j in range(n):
        out.append(S[j, j])
        if not S[j, j] > 0.0:
            break
        l = S[j + 1:, j] / np.sqrt(S[j, j])
        S[j + 1:, j + 1:] -= np.outer(l, l)
    return np.array(out)


def first_bad_pivot(A64):
    """The first column at which the fp64 right-looking elimination meets a pivot <= 0, or None."""
    d = pivots(A64)
    return None if d[-1] > 0.0 else len(d) - 1


def ulp32(x):
    """The spacing of fp32 at |x| (x as fp32)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def ulp_distance(a, b):
    """|a - b| in units in the last place for fp32 arrays of equal sign pattern or not: the distance of their ordered integer images."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---------------------------------------------------------------------------------------------- generators
def _seed(*parts):
    return np.random.default_rng([0xC401] + [int(p) for p in parts])


def _spectrum64(n, cond, rng):
    """Q diag(w) Q^T in fp64, exactly symmetric: Q a random orthogonal basis, w log-spaced over [s / cond, s], s a seeded scale in
    [0.5, 2) so that no size is a matrix of round numbers."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    w = rng.uniform(0.5, 2.0) * np.logspace(0.0, -np.log10(cond), n)
    A = (Q * w) @ Q.T
    return 0.5 * (A + A.T)


def _assert_pd(A32, equilibrate=False):
    S = _sym64(A32)
    if equilibrate:  # D^-1 S D^-1 with unit diagonal has the inertia of S (Sylvester) and a spectrum eigvalsh can resolve
        d = np.sqrt(np.diag(S))
        S = S / np.outer(d, d)
    w = np.linalg.eigvalsh(S)
    assert np.all(np.diag(S) > 0) and w[0] > 0.0, w[0]


def spectrum(n, cond, tag=0):
    A32 = _spectrum64(n, cond, _seed(1, n, np.log10(cond) * 10, tag)).astype(np.float32)
    _assert_pd(A32)
    return A32


def scaled(n, e):
    """cond 1e4 times 2^e (exact in fp32)."""
    A32 = np.ldexp(_spectrum64(n, 1e4, _seed(2, n)).astype(np.float32), e).astype(np.float32)
    _assert_pd(A32)
    return A32


def graded(n):
    """cond 1e4, then D A D with D log-spaced over 1e-3 ... 1e3 and shuffled.  The positive-definiteness check runs on the
    unit-diagonal scaling of the fp32 image: the raw image's spectrum spans more than fp64's eigvalsh resolves."""
    rng = _seed(3, n)
    A = _spectrum64(n, 1e4, rng)
    D = rng.permutation(np.logspace(-3.0, 3.0, n))
    A32 = (A * np.outer(D, D)).astype(np.float32)
    _assert_pd(A32, equilibrate=True)
    return A32


def asym(n):
    """A spectrum matrix (cond 1e4) whose strict upper triangle is moved by -2 ... 2 fp32 ulps."""
    rng = _seed(4, n)
    A32 = _spectrum64(n, 1e4, rng).astype(np.float32)
    k = np.triu(rng.integers(-2, 3, size=(n, n)), 1).astype(np.int32)
    i = A32.view(np.int32)
    out = np.where(i < 0, i - k, i + k).astype(np.int32).view(np.float32)  # k ulps up (k > 0) or down, whatever the sign
    assert np.all(np.isfinite(out)) and np.array_equal(np.tril(out), np.tril(A32))
    if n > 2:
        assert np.mean(out[np.triu_indices(n, 1)] != out.T[np.triu_indices(n, 1)]) > 0.5
    _assert_pd(out)
    return out


def bad_column(n):
    """The column the indefinite case breaks at: about the middle, never the first column of an 8-column panel."""
    p = n // 2
    return p + 1 if p % 8 == 0 else p


def indefinite(n):
    """-> (clean, bad, p): a spectrum matrix (cond 1e4) and its copy with A[p][p] lowered so far that the pivot at column p is
    <= -0.1 max|A|; every pivot before p is untouched (and positive)."""
    clean = _spectrum64(n, 1e4, _seed(5, n)).astype(np.float32)
    _assert_pd(clean)
    p = bad_column(n)
    S = _sym64(clean)
    amax = np.abs(S).max()
    piv = pivots(S)[p]
    bad = clean.copy()
    bad[p, p] = np.float32(S[p, p] - piv - 0.25 * amax)
    Sb = _sym64(bad)
    d = pivots(Sb)
    assert len(d) == p + 1 and d[-1] <= -0.1 * np.abs(Sb).max(), (n, p, d[-1])
    return clean, bad, p


def family_cases(n):
    """The positive-definite cases of size n -> list of (name, fp32 matrix)."""
    out = [(f"spectrum-{c:.0e}", spectrum(n, c)) for c in CONDS]
    if n in NS_EDGE:
        out += [("scaled-2^-60", scaled(n, -60)), ("scaled-2^60", scaled(n, 60)), ("graded", graded(n)), ("asym", asym(n))]
    return out


def batch_cases(n, batch):
    """`batch` distinct spectrum matrices of size n, cond cycling through 1e1 ... 1e5 -> fp32 [batch, n, n]."""
    conds = (1e1, 1e2, 1e3, 1e4, 1e5)
    return np.stack([spectrum(n, conds[b % len(conds)], tag=1 + b) for b in range(batch)])
