"""CPU: the two host references of tests/chol_cases.py against each other, so that the bars of tests/test_gpu_cholesky.py are met
by the references alone: LAPACK fp64 (chol_ref) and the long-double restatement (chol_ld) of every positive-definite case agree to one
fp32 ulp after rounding, bit for bit in >= 99.99 % of the entries, and within FWD64 before rounding; the indefinite cases break at
the intended column and nowhere before it.  (An x87 long double is assumed only in so far as chol_ld must not be LESS accurate than
fp64; where np.longdouble is fp64 the two references are merely two operation orders.)"""
import numpy as np
import pytest

from tests import chol_cases as CC


@pytest.fixture(scope="module")
def refs():
    """per positive-definite case: (n, name, L64 = LAPACK fp64 factor, L_ld = long-double factor)"""
    out = []
    for n in CC.NS:
        for name, A32 in CC.family_cases(n):
            S = CC._sym64(A32)
            out.append((n, name, np.linalg.cholesky(S), CC.chol_ld(S), A32))
    return out


def test_references_agree_to_one_ulp_and_mostly_bit_for_bit(refs):
    same = total = 0
    worst = 0
    for n, name, L64, Lld, A32 in refs:
        a, b = CC.chol_ref(A32), Lld.astype(np.float64).astype(np.float32)
        assert np.array_equal(a, L64.astype(np.float32))
        lo = np.tril_indices(n)
        assert np.all(np.abs(a[lo].astype(np.float64) - b[lo].astype(np.float64)) <= CC.ulp32(a[lo])), (n, name)
        d = CC.ulp_distance(a[lo], b[lo])
        worst = max(worst, int(d.max()))
        same += int((d == 0).sum())
        total += d.size
    share = same / total
    print(f"host references: {total} lower-triangle entries, bit-identical share {share:.6f}, largest distance {worst} ulp")
    assert total > 100000 and worst <= 1
    assert share >= 0.9999, share


def test_fp64_distance_of_the_references_is_within_FWD64(refs):
    worst, where = 0.0, None
    for n, name, L64, Lld, _ in refs:
        d = float(np.abs(L64.astype(np.longdouble) - Lld).max() / np.abs(L64).max())
        if d > worst:
            worst, where = d, (n, name)
    print(f"host references: max |L64 - L_ld| / max |L64| = {worst:.3e} at {where} (FWD64 = {CC.FWD64:.1e})")
    assert worst <= CC.FWD64, (worst, where)
    assert 16 * CC.FWD64 < 2.0 ** -24 * 1e-4  # the GPU test's floor stays orders below one fp32 ulp of max|L|


@pytest.mark.parametrize("n", CC.NS_EDGE)
def test_indefinite_cases_break_at_the_intended_column(n):
    clean, bad, p = CC.indefinite(n)
    assert p == CC.bad_column(n) and p % 8 != 0 and 0 < p < n - 1
    assert CC.first_bad_pivot(CC._sym64(clean)) is None
    Sb = CC._sym64(bad)
    assert CC.first_bad_pivot(Sb) == p
    assert CC.pivots(Sb)[-1] <= -0.1 * np.abs(Sb).max()
    # the columns before p do not see A[p][p]: the elimination of the bad matrix up to the break gives the very columns the same
    # elimination gives on the clean matrix, and those are LAPACK's factor of the clean matrix
    def eliminate(S, cols):
        S = S.copy()
        for j in range(cols):
            S[j:, j] /= np.sqrt(S[j, j])
            S[j + 1:, j + 1:] -= np.outer(S[j + 1:, j], S[j + 1:, j])
        return S[:, :cols]
    low = np.tril(np.ones((n, n), dtype=bool))[:, :p]
    Eb, Ec = eliminate(Sb, p), eliminate(CC._sym64(clean), p)
    assert np.array_equal(Eb[low], Ec[low])
    Lc = np.linalg.cholesky(CC._sym64(clean))
    assert np.abs(Eb - Lc[:, :p])[low].max() <= CC.FWD64 * np.abs(Lc).max()
    assert CC.ulp_distance(Eb.astype(np.float32)[low], CC.chol_ref(clean)[:, :p][low]).max() <= 1


def test_generators_are_deterministic_and_distinct():
    a, b = CC.batch_cases(5, 12), CC.batch_cases(5, 12)
    assert np.array_equal(a, b)
    assert len({m.tobytes() for m in a}) == 12
    for n in (1, 8):
        assert np.array_equal(CC.asym(8), CC.asym(8)) and np.array_equal(CC.spectrum(n, 1e3), CC.spectrum(n, 1e3))
