"""CPU tests of tests/update_oracle.py: the fp64 reference of the weighted update against oracle/ref_np.py, the merge rule against
the unsharded update, and the crafted inputs of tests/test_gpu_update_edges.py for the properties the GPU tests rely on.

lambda reaches update_oracle's functions as the fp32 quotient 1 / lam, ref_np's as a division by lam: the comparisons to 1e-12 use
temperatures whose reciprocal is exact in fp32 (powers of two), where the two agree."""
import numpy as np
import pytest

from oracle import ref_np as R
from tests import update_oracle as U

LAMS = (2.0 ** -7, 0.5, 4.0)  # 1 / lam exact in fp32


def _problem(N, seed, lam):
    rng = np.random.default_rng(seed)
    cost = 5.0 + 6.0 * lam * rng.normal(size=N)
    a = np.clip(0.6 * rng.normal(size=(N, 32, 4)), -1, 1)
    mean = 0.1 * rng.normal(size=(32, 4))
    B = rng.normal(size=(32, 4, 4))
    return cost, a, mean, 0.05 * B @ B.transpose(0, 2, 1) + 0.1 * np.eye(4)


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("gamma", [1.0, 0.7])
def test_mean_and_cov_equal_ref_np(lam, gamma):
    cost, a, mean, cov = _problem(777, 1, lam)
    new, w = U.mean64(cost, a, lam, gamma, mean)
    ref, w_ref = R.softmax_update(cost, a, lam, gamma, mean)
    assert np.abs(new - ref).max() < 1e-12 and np.abs(w - w_ref).max() < 1e-12
    assert np.abs(U.cov64(w, a, new, cov, 0.3) - R.mppi_cov_update(w_ref, a, ref, cov, 0.3)).max() < 1e-12


@pytest.mark.parametrize("lam", LAMS)
def test_record_equals_ref_np(lam):
    cost, a, mean, _ = _problem(300, 2, lam)
    rec = U.record64(cost, a, lam, mu=mean)
    m, s, v = R.softmax_partial(cost, a.reshape(300, 128), lam)
    assert rec["m"] == m and abs(rec["s"] - s) < 1e-12 * s and np.abs(rec["v"] - v).max() < 1e-12 * s
    m2, s2, v2, S2 = R.softmax_partial_cov(cost, a, lam, mean)
    assert np.abs(rec["S2"] - S2).max() < 1e-12 * s and np.abs(rec["v"] - v2).max() < 1e-12 * s
    assert np.array_equal(U.unpack_pairs(rec["s2"]), rec["S2"]) or np.abs(U.unpack_pairs(rec["s2"]) - rec["S2"]).max() < 1e-15
    assert "S2" not in U.record64(cost, a, lam)
    empty = U.record64(cost[:0], a[:0], lam, mu=mean)
    assert empty["m"] == np.inf and empty["s"] == 0 and not empty["v"].any() and not empty["S2"].any()


def _splits(N, G, rng, with_empty):
    cuts = np.sort(rng.integers(0, N + 1, size=G - 1))
    if with_empty and G > 1:
        cuts[0 if G == 2 else 1] = cuts[0]  # two equal cuts: an empty shard (G = 2: the first shard is empty)
        if G == 2:
            cuts[0] = 0
    edges = np.concatenate([[0], np.sort(cuts), [N]])
    return [slice(int(edges[g]), int(edges[g + 1])) for g in range(G)]


@pytest.mark.parametrize("G", [1, 3, 8])
@pytest.mark.parametrize("with_empty", [False, True])
@pytest.mark.parametrize("lam", LAMS + (0.01,))
def test_merge_of_any_split_equals_the_whole(G, with_empty, lam):
    """merge64 of the record64s of a split of the samples == mean64 (and cov64) of the whole, to 1e-12 -- in fp64 rows, so that the
    records are not rounded."""
    N = 500
    cost, a, mean, cov = _problem(N, 3 + G, lam)
    cost, a, mean = cost.astype(np.float32), a.astype(np.float32), mean.astype(np.float32)
    rng = np.random.default_rng(G)
    parts = _splits(N, G, rng, with_empty)
    assert not with_empty or G == 1 or any(p.stop == p.start for p in parts)
    rows = np.zeros((G, U.PARTIAL_FLOATS + U.COV_FLOATS))
    for g, p in enumerate(parts):
        r = U.record64(cost[p], a[p], lam, mu=mean)
        rows[g, 0], rows[g, 1], rows[g, 2:130], rows[g, 132:452] = r["m"], r["s"], r["v"], r["s2"]
    for gamma in (1.0, 0.7):
        out = U.merge64(rows, lam, gamma, mean, cov, 0.3)
        ref, w = U.mean64(cost, a, lam, gamma, mean)
        assert np.abs(out["mean"] - ref).max() < 1e-12
        assert np.abs(out["cov"] - U.cov64(w, a, ref, cov, 0.3)).max() < 1e-12
    whole = U.record64(cost, a, lam)
    assert out["m"] == whole["m"] and abs(out["s"] - whole["s"]) < 1e-12 * whole["s"]
    assert np.abs(out["v"] - whole["v"]).max() < 1e-12 * whole["s"]


def test_merge_ignores_what_an_empty_record_holds():
    rows, _ = U.shard_records(9, 0.01, "empty")
    dirty, _ = U.shard_records(9, 0.01, "empty_garbage")
    assert (dirty[1::3, 2:130] == np.float32(1e30)).all() and (rows[1::3, 1] == 0).all() and np.isinf(rows[1::3, 0]).all()
    a, b = U.merge64(rows, 0.01, 0.7, np.zeros((32, 4))), U.merge64(dirty, 0.01, 0.7, np.zeros((32, 4)))
    assert np.array_equal(a["mean"], b["mean"]) and np.isfinite(a["mean"]).all()
    padded = U.merge64(U.pad_rows(rows, 64), 0.01, 0.7, np.zeros((32, 4)))
    assert np.array_equal(a["mean"], padded["mean"])


def test_stripes_round_trip():
    a = np.random.default_rng(0).normal(size=(70, 32, 4)).astype(np.float32)
    s = U.from_stripes(a)
    assert s.shape == (32, 70, 4) and s.flags.c_contiguous and np.array_equal(U.stripes(s), a) and s[5, 9, 2] == a[9, 5, 2]


# ------------------------------------------------------------------------------------------ the crafted inputs
@pytest.mark.parametrize("N", U.EDGE_SIZES)
@pytest.mark.parametrize("lam", U.EDGE_LAMS)
def test_cost_patterns_have_the_properties_the_gpu_tests_rely_on(N, lam):
    for pattern in U.PATTERNS:
        c = U.cost_pattern(pattern, N, lam)
        assert c.dtype == np.float32 and c.shape == (N,) and np.isfinite(c).all(), pattern
        assert np.array_equal(c, U.cost_pattern(pattern, N, lam)), pattern  # reproducible
        w = U.weights_f32(c, lam)
        if pattern == "equal":
            assert (c == c[0]).all() and (w == 1.0).all()
        if pattern in ("winner", "winner_last"):
            i = U.winner_index(pattern, N)
            assert int(np.argmin(c)) == i and (pattern != "winner_last" or i == N - 1)
            assert N == 1 or np.delete(c, i).min() - c[i] >= 49.99
            if lam == 0.01:  # every other weight is exactly 0 in fp32: the new mean is that sample's actions, bit for bit
                assert w[i] == 1.0 and w.sum() == 1.0 and U.n_live(c, lam) == 1
        if pattern == "tied":
            i, j = U.tied_positions(N)
            assert c[i] == c[j] == c.min() and (c == c.min()).sum() == (2 if N > 1 else 1)
            assert N <= 64 or i // 64 != j // 64          # different waves
            assert N <= 256 or i // 256 != j // 256       # different stage-1 workgroups ...
            assert N <= 256 or (i // 64) % 1024 // 4 != (j // 64) % 1024 // 4  # ... also where the capped grid's waves stride
        if pattern == "offset":
            c64 = c.astype(np.float64)
            k = (c64 - 1e6) / 0.0625
            assert (k == np.round(k)).all() and (k >= 0).all() and (k < 4096).all() and c.min() >= 1e6
            assert ((c - c.min()).astype(np.float64) == c64 - c64.min()).all()  # c - m is exact in fp32
        if pattern == "lanes":
            live = U.lanes_live_mask(N)
            assert live.any() and c[live].min() == c.min() == 5.0
            assert (w[live] > 0).all() and (w[~live] == 0).all(), (N, lam)
            assert (c[live] - 5.0 <= 0.5 * lam * (1 + 1e-6) + 1e-6 * 5).all() and (c[~live] - 5.0 >= 199.0 * lam).all()
            counts = np.add.reduceat(live, np.arange(0, N, 64))
            sizes = np.minimum(64, N - np.arange(0, N, 64))
            assert all(k in U.LANE_COUNTS or k == s for k, s in zip(counts, sizes)) or N < 64
            if N >= 1025:
                assert set(U.LANE_COUNTS) <= set(counts.tolist())


def test_edge_sizes_reach_the_striding_grid():
    """65 600 samples are 1 025 full groups of 64: one more than the capped grid (256 workgroups x 4 waves) holds, so one wave
    strides to a second group; 65 570 are the same 1 025 groups with the strided one partial."""
    assert (65600 + 63) // 64 == 1025 and 65600 % 64 == 0 and max(U.EDGE_SIZES) == 65600
    assert (65570 + 63) // 64 == 1025 and 65570 % 64 == 34 and {65600, 65570} <= set(U.EDGE_SIZES)


@pytest.mark.parametrize("variant", U.MERGE_VARIANTS)
def test_merge_records_have_the_properties_the_gpu_tests_rely_on(variant):
    lam = 0.01
    G = 65
    rows, mu = U.shard_records(G, lam, variant, floats=836, with_cov=True)
    assert rows.dtype == np.float32 and rows.shape == (G, 836) and not rows[:, 452:].any()
    assert np.array_equal(rows, U.shard_records(G, lam, variant, floats=836, with_cov=True)[0])  # reproducible
    narrow, _ = U.shard_records(G, lam, variant)
    assert np.array_equal(narrow[:, :130], rows[:, :130])  # the same records at every stride
    empty = rows[:, 1] == 0
    if variant in ("empty", "empty_garbage", "empty_stale"):
        assert np.array_equal(np.flatnonzero(empty), np.arange(1, G, 3))
        if variant == "empty_stale":  # a finite minimum, not below the live ones: only s = 0 marks the record
            assert np.array_equal(rows[empty, 0], rows[np.flatnonzero(empty) - 1, 0]) and np.isfinite(rows[empty, 0]).all()
            assert rows[empty, 0].min() >= rows[~empty, 0].min()
            with np.errstate(under="ignore"):
                assert np.exp(((rows[~empty, 0].min() - rows[empty, 0]) * (np.float32(1) / np.float32(lam))).astype(np.float32)).max() > 0
        else:
            assert np.isinf(rows[empty, 0]).all()
        assert (rows[empty, 2:130] == (0 if variant == "empty" else 1e30)).all()
        clean, _ = U.shard_records(G, lam, "empty", floats=836, with_cov=True)
        for k in ("mean", "cov", "s"):
            assert np.array_equal(U.merge64(rows, lam, 0.7, mu, np.zeros((32, 4, 4)), 0.3)[k],
                                  U.merge64(clean, lam, 0.7, mu, np.zeros((32, 4, 4)), 0.3)[k])
    else:
        assert not empty.any()
    assert (rows[~empty, 1] >= 1.0).all() and np.isfinite(rows[~empty]).all()
    m = rows[~empty, 0].min()
    assert m == rows[:, 0].min()
    inv = np.float32(1.0) / np.float32(lam)
    with np.errstate(under="ignore"):
        scale32 = np.exp(((m - rows[~empty, 0]) * inv).astype(np.float32))
    if variant == "underflow":
        gaps = np.sort(rows[:, 0]) - m
        assert np.array_equal(gaps, 0.5 * np.arange(G))  # minima 0.5 apart
        top = np.sort(scale32)[::-1]  # exp(-50) = 2e-22 is still a normal fp32 number, exp(-100) a denormal, exp(-150) is 0
        assert top[0] == 1.0 and 0 < top[1] < 3e-22 and top[2] < 1e-43 and (top[3:] == 0).all()
        assert int(np.argmin(rows[:, 0])) != 0  # not the first record
    elif variant == "equal_m":
        assert (rows[:, 0] == m).all() and (scale32 == 1.0).all()
    else:
        assert (scale32 > 0).all() and len(np.unique(rows[~empty, 0])) == (~empty).sum() and scale32.min() < 0.5
    padded = U.pad_rows(rows, 257)
    assert padded.shape == (257, 836) and np.array_equal(padded[:G], rows, equal_nan=True) and np.isinf(padded[G:, 0]).all() and not padded[G:, 1:].any()
