"""tests/cma_oracle.py on synthetic inputs: the properties of the step-size formulas that the CMA controller relies on,
checked on the CPU before anything is held against that oracle."""
import numpy as np

from tests import cma_oracle as CO

N = 256  # samples per step: the cap of mu_eff


def test_constants_at_the_ends_of_the_ess_range():
    n = float(CO.N_A)
    mu, cs, ds = CO.constants(0.3, N)  # below 1: clamped
    assert mu == 1.0 and cs == 3.0 / (n + 6.0) and ds == 1.0 + cs
    mu, cs, ds = CO.constants(1e9, N)  # above N: clamped; sqrt((N - 1) / (n + 1)) > 1 adds to the damping
    assert mu == N and cs == (N + 2.0) / (n + N + 5.0)
    assert np.isclose(ds, 1.0 + 2.0 * (np.sqrt((N - 1.0) / (n + 1.0)) - 1.0) + cs, rtol=1e-15)
    assert CO.constants(7.3, N, damping=2.0)[2] == 2.0 * CO.constants(7.3, N)[2]
    assert np.isclose(CO.CHI_N, np.sqrt(n) * (1.0 - 1.0 / (4.0 * n) + 1.0 / (21.0 * n * n)), rtol=1e-15)


def test_no_displacement_shrinks_to_s_min_monotonically():
    """d = 0 for ever: |p| decays geometrically and s falls, never rises, until it sits on s_min."""
    L = 0.5 * np.eye(CO.N_A)
    p, ls = np.random.default_rng(0).normal(size=CO.N_A) * 0.05, 0.0
    lo = np.log(float(np.float32(0.1)))
    norms, scales = [np.linalg.norm(p)], [1.0]
    for _ in range(400):
        p, ls, row = CO.step_size(L, np.zeros(CO.N_A), 1.0, 7.3, p, ls, N)
        norms.append(row[2]), scales.append(row[0])
    assert all(b < a for a, b in zip(norms, norms[1:])) and norms[-1] < 1e-12
    assert all(b <= a for a, b in zip(scales, scales[1:]))
    assert ls == lo and int(row[7]) == CO.FLAG_CLAMP and np.isclose(scales[-1], 0.1, rtol=1e-7)


def test_a_persistent_long_displacement_grows_to_s_max():
    """z held at a fixed vector of norm 2 chi_n: |p| tends to sqrt(mu_eff (2 - c) / c) |z| > chi_n and exceeds chi_n from the first
    step on (sqrt(c (2 - c) mu_eff) 2 > 1 at ess = 7.3), so s never falls and climbs to s_max."""
    mu, cs, ds = CO.constants(7.3, N)
    z = np.zeros(CO.N_A)
    z[3] = 2.0 * CO.CHI_N
    p, ls, hi = np.zeros(CO.N_A), 0.0, np.log(float(np.float32(4.0)))
    seen = []
    for _ in range(200):
        p, ls, hit = CO.path_update(p, ls, z, mu, cs, ds, np.log(0.1), hi)
        seen.append(ls)
    assert all(b >= a for a, b in zip(seen, seen[1:])) and ls == hi and hit
    # the same through step_size: d = L z
    L = np.tril(np.random.default_rng(1).normal(size=(CO.N_A, CO.N_A)) * 0.01) + 0.5 * np.eye(CO.N_A)
    p2, ls2, row = CO.step_size(L, L @ z, 1.0, 7.3, np.zeros(CO.N_A), 0.0, N)
    assert np.isclose(row[3], 2.0 * CO.CHI_N, rtol=1e-10) and ls2 > 0.0 and int(row[7]) == 0


def test_random_selection_leaves_log_s_without_drift():
    """z ~ N(0, I / mu_eff) redrawn every step -- what the weighted mean of mu_eff equally weighted standard normal draws is under
    random selection: the path is then N(0, I) in the stationary state and |p| / chi_n - 1 has mean ~ 0.  Mean drift of log s per
    step below 0.02 over 500 steps, for each ess of the GPU cases."""
    for ess, seed in ((1.0, 0), (7.3, 1), (float(N), 2)):
        rng = np.random.default_rng(seed)
        mu, cs, ds = CO.constants(ess, N)
        p, ls = np.zeros(CO.N_A), 0.0  # (the reset state)
        for _ in range(500):
            z = rng.normal(size=CO.N_A) / np.sqrt(mu)
            p, ls, hit = CO.path_update(p, ls, z, mu, cs, ds, -np.inf, np.inf)
        assert abs(ls) / 500.0 < 0.02, (ess, ls / 500.0)


def test_whiten_is_the_inverse_of_the_lower_triangle():
    rng = np.random.default_rng(3)
    L = np.tril(rng.normal(size=(CO.N_A, CO.N_A))) * 0.1 + np.eye(CO.N_A)
    d = rng.normal(size=CO.N_A)
    assert np.allclose(CO.whiten(L, d), np.linalg.solve(L, d), rtol=1e-9, atol=1e-12)
    assert np.allclose(CO.whiten(L + np.triu(np.ones_like(L), 1), d), np.linalg.solve(L, d), rtol=1e-9, atol=1e-12)  # (upper: not read)


def test_fall_backs_keep_the_state_and_name_themselves():
    L = 0.5 * np.eye(CO.N_A)
    p0, d = np.arange(CO.N_A) * 1e-3, np.ones(CO.N_A) * 0.01
    bad_d = d.copy()
    bad_d[17] = np.nan
    bad_L = L.copy()
    bad_L[40, 40] = 0.0
    for kw in (dict(W=0.0), dict(d=bad_d), dict(L=bad_L), dict(ess=np.inf), dict(W=np.nan)):
        a = dict(L=L, d=d, W=1.0, ess=7.3)
        a.update(kw)
        p, ls, row = CO.step_size(a["L"], a["d"], a["W"], a["ess"], p0, 0.25, N)
        assert np.array_equal(p, p0) and ls == 0.25 and int(row[7]) == CO.FLAG_KEPT, kw
        assert np.isclose(row[0], np.exp(0.25)) and row[1] == 0.25 and np.isclose(row[2], np.linalg.norm(p0)) and not row[3:7].any()
    p, ls, row = CO.step_size(L, d, 1.0, 7.3, p0, 0.25, N, shape_fallback=True)
    assert int(row[7]) == CO.FLAG_SHAPE and ls != 0.25


def test_a_broken_state_is_mended_on_entry():
    """log s is held inside its bounds before anything uses it -- on a fall-back too, which scales by exp(log s) --, a log s or a path
    that is not finite counts as 0."""
    L = 0.5 * np.eye(CO.N_A)
    d, p0 = np.ones(CO.N_A) * 0.01, np.arange(CO.N_A) * 1e-3
    hi, lo = np.log(float(np.float32(4.0))), np.log(float(np.float32(0.1)))
    p, ls, row = CO.step_size(L, d, 0.0, 7.3, p0, 800.0, N)  # a fall-back with a log s far outside
    assert ls == hi and row[0] == np.exp(hi) and int(row[7]) == CO.FLAG_KEPT and np.array_equal(p, p0)
    p, ls, row = CO.step_size(L, d, 0.0, 7.3, p0, -800.0, N)
    assert ls == lo and np.isclose(row[0], 0.1, rtol=1e-7)
    bad = p0.copy()
    bad[9] = np.nan
    for a, b in ((CO.step_size(L, d, 1.0, 7.3, bad, 0.25, N), CO.step_size(L, d, 1.0, 7.3, np.zeros(CO.N_A), 0.25, N)),
                 (CO.step_size(L, d, 1.0, 7.3, p0, np.nan, N), CO.step_size(L, d, 1.0, 7.3, p0, 0.0, N)),
                 (CO.step_size(L, d, 1.0, 7.3, p0, np.inf, N), CO.step_size(L, d, 1.0, 7.3, p0, 0.0, N))):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.isfinite(a[2]).all()
    p, ls, row = CO.step_size(L, d, 0.0, 7.3, bad, 0.25, N)  # mended and kept
    assert not p.any() and ls == 0.25 and row[2] == 0.0 and int(row[7]) == CO.FLAG_KEPT


def test_scale_rounds_once_and_keeps_the_structure():
    rng = np.random.default_rng(4)
    Lh = np.tril(rng.normal(size=(CO.N_A, CO.N_A))).astype(np.float32)
    Sh = (Lh.astype(np.float64) @ Lh.astype(np.float64).T).astype(np.float32)
    Sh = np.maximum(Sh, Sh.T)  # exactly symmetric
    Lp, Sp = CO.scale(1.2345678901, Lh, Sh)
    assert Lp.dtype == Sp.dtype == np.float32 and not np.triu(Lp, 1).any() and np.array_equal(Sp, Sp.T)
    assert np.array_equal(Lp, (1.2345678901 * Lh.astype(np.float64)).astype(np.float32))
    L1, S1 = CO.scale(1.0, Lh, Sh)
    assert np.array_equal(L1, Lh) and np.array_equal(S1, Sh)


def test_adapt_step_without_step_size_is_the_shape_alone():
    from tests.sigma_shift_oracle import adapt_ref
    L = (0.5 * np.eye(CO.N_A)).astype(np.float32)
    C = 0.3 * np.eye(CO.N_A)
    Lp, Sp, p, ls, row = CO.adapt_step(L, C, np.ones(CO.N_A), 1.0, 7.3, np.zeros(CO.N_A), 0.0, N, 0.5, gamma=0.2, step_size_on=False)
    Sr, Lr = adapt_ref(L, C, 0.2, 0.5)[:2]
    assert np.array_equal(Lp, Lr) and np.array_equal(Sp, Sr) and ls == 0.0 and not p.any() and np.array_equal(row, CO.NEUTRAL_ROW)
    # sigma0 I is a fixed point of the shape at gamma = 0, and log det is held
    Lp, Sp, _, _, _ = CO.adapt_step(L, C, np.zeros(CO.N_A), 1.0, 7.3, np.zeros(CO.N_A), 0.0, N, 0.5, gamma=0.0, step_size_on=False)
    assert np.allclose(Sp, 0.25 * np.eye(CO.N_A), atol=1e-14)
