"""The fp64 numpy restatement of the CMA controller's adaptation, written from the definition: the shape (Sigma
adapt's blend, tests/sigma_shift_oracle.py), the cumulative step-size adaptation in Cholesky-whitened coordinates, and the scaling.
tests/test_cma_oracle.py checks its formulas on synthetic inputs; tests/test_gpu_cma.py holds csrc/cma_path.hip and the step against it."""
import numpy as np

from tests import sigma_shift_oracle as SO

N_A = 128
FLAG_KEPT, FLAG_CLAMP, FLAG_SHAPE = 1, 2, 4
CHI_N = np.sqrt(N_A) * (1.0 - 1.0 / (4.0 * N_A) + 1.0 / (21.0 * N_A * N_A))
NEUTRAL_ROW = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])


def constants(ess, n_samples, damping=1.0):
    """(mu_eff, c_sigma, d_sigma) of a step whose previous one had effective sample size ess."""
    n = float(N_A)
    mu = min(max(float(ess), 1.0), float(n_samples))
    cs = (mu + 2.0) / (n + mu + 5.0)
    ds = float(damping) * (1.0 + 2.0 * max(0.0, np.sqrt((mu - 1.0) / (n + 1.0)) - 1.0) + cs)
    return mu, cs, ds


def path_update(p, log_s, z, mu, cs, ds, log_s_min, log_s_max):
    """One update of (p, log s) from the whitened displacement z -> (p', log s', clamp hit)."""
    p = (1.0 - cs) * np.asarray(p, dtype=np.float64) + np.sqrt(cs * (2.0 - cs) * mu) * np.asarray(z, dtype=np.float64)
    raw = float(log_s) + (cs / ds) * (np.linalg.norm(p) / CHI_N - 1.0)
    new = min(max(raw, float(log_s_min)), float(log_s_max))
    return p, new, new != raw


def whiten(L, d):
    """z = L^-1 d by forward substitution on the lower triangle of L, row by row in fp64."""
    L = np.asarray(L, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    z = np.zeros(N_A)
    with np.errstate(all="ignore"):
        for i in range(N_A):
            z[i] = (d[i] - L[i, :i] @ z[:i]) / L[i, i]
    return z


def step_size(L_prev, d, W, ess, p, log_s, n_samples, *, damping=1.0, s_min=0.1, s_max=4.0, shape_fallback=False):
    """Step 2 of the definition on one instance -> (p', log s', row [8] in fp64).  L_prev: the factor the previous step sampled from
    (as stored: fp32 values); d, W, ess: that step's displacement, weight sum and effective sample size; s_min / s_max are rounded
    to fp32 first, as the C boundary takes them."""
    L = np.asarray(L_prev, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    W, ess, log_s = float(W), float(ess), float(log_s)
    lo, hi = np.log(float(np.float32(s_min))), np.log(float(np.float32(s_max)))
    # the state is mended on entry: a path or a log s that is not finite counts as 0, and log s is held inside its bounds
    if not np.all(np.isfinite(p)):
        p = np.zeros(N_A)
    log_s = min(max(log_s if np.isfinite(log_s) else 0.0, lo), hi)
    flags = FLAG_SHAPE if shape_fallback else 0
    diag = np.diag(L)
    good = W > 0.0 and np.isfinite(W) and np.isfinite(ess) and bool(np.all(np.isfinite(d))) and bool(np.all(np.isfinite(diag) & (diag > 0.0)))
    z = whiten(L, d) if good else None
    good = good and bool(np.all(np.isfinite(z)))
    if not good:
        s = np.exp(log_s)
        return p, log_s, np.array([s, log_s, np.linalg.norm(p), 0.0, 0.0, 0.0, 0.0, float(flags | FLAG_KEPT)])
    mu, cs, ds = constants(ess, n_samples, damping)
    p, log_s, hit = path_update(p, log_s, z, mu, cs, ds, lo, hi)
    flags |= FLAG_CLAMP if hit else 0
    return p, log_s, np.array([np.exp(log_s), log_s, np.linalg.norm(p), np.linalg.norm(z), mu, cs, ds, float(flags)])


def scale(s, L_hat, Sigma_hat):
    """Step 3: (L', Sigma') = (fp32(s L_hat), fp32(s^2 Sigma_hat)), each rounded once from fp64."""
    s = float(s)
    return ((s * np.asarray(L_hat, dtype=np.float64)).astype(np.float32),
            ((s * s) * np.asarray(Sigma_hat, dtype=np.float64)).astype(np.float32))


def adapt_step(L_prev, C, d, W, ess, p, log_s, n_samples, sample_sigma, *, gamma=0.2, step_size_on=True, damping=1.0, s_min=0.1,
               s_max=4.0):
    """Steps 1-3 on one instance, all in fp64 -> (L' fp64, Sigma' fp64, p', log s', row).  The shape is Sigma adapt's definition
    (sigma_shift_oracle.adapt_ref) on L_prev and C."""
    Sigma_hat, L_hat, fallback, _, _ = SO.adapt_ref(L_prev, C, gamma, sample_sigma)
    if not step_size_on:
        row = NEUTRAL_ROW.copy()
        row[7] = FLAG_SHAPE if fallback else 0
        return L_hat, Sigma_hat, np.asarray(p, dtype=np.float64), float(log_s), row
    p, log_s, row = step_size(L_prev, d, W, ess, p, log_s, n_samples, damping=damping, s_min=s_min, s_max=s_max,
                              shape_fallback=bool(fallback))
    s = np.exp(log_s)
    return s * L_hat, (s * s) * Sigma_hat, p, log_s, row
