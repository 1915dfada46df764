"""The fp64 numpy restatement of a reuse step's covariance: the Sigma period's shift and Sigma adapt's blend
(DESIGN.md 4.18), written from the definitions.  tests/test_sigma_period_abi.py and tests/test_sigma_adapt_abi.py check it against
known answers; the GPU tests hold the kernels against it."""
import numpy as np

N_A, DU = 128, 4


# ---------------------------------------------------------------------------------------------- the Sigma period's shift
def shift_S(Sigma):
    """S(Sigma): the trailing 124 x 124 block moved up, the old last stage's 4 x 4 marginal as the new last stage, no cross terms."""
    S = np.zeros_like(Sigma, dtype=np.float64)
    S[:N_A - DU, :N_A - DU] = Sigma[DU:, DU:]
    S[N_A - DU:, N_A - DU:] = Sigma[N_A - DU:, N_A - DU:]
    return S


def volume_scalar(S, sample_sigma):
    """c with log det (c S) = 2 n log sample_sigma."""
    sign, logdet = np.linalg.slogdet(S)
    assert sign > 0
    return float(np.exp((2.0 * N_A * np.log(float(sample_sigma)) - logdet) / N_A))


def shift_sigma_ref(Sigma, sample_sigma):
    """Sigma' = c S(Sigma) from the covariance itself."""
    S = shift_S(np.asarray(Sigma, dtype=np.float64))
    return volume_scalar(S, sample_sigma) * S


def rank_update(Lmat, X):
    """The lower factor of Lmat Lmat^T + X X^T by one rotation per column and update vector (the issue's recurrence):
    r = sqrt(L_kk^2 + x_k^2), c = r / L_kk, s = x_k / L_kk, L_ik <- (L_ik + s x_i) / c, x_i <- c x_i - s L_ik."""
    Lw = np.array(Lmat, dtype=np.float64)
    n = Lw.shape[0]
    for j in range(X.shape[1]):
        x = np.array(X[:, j], dtype=np.float64)
        for k in range(n):
            r = np.hypot(Lw[k, k], x[k])
            c, s = r / Lw[k, k], x[k] / Lw[k, k]
            Lw[k, k] = r
            if k + 1 < n:
                Lw[k + 1:, k] = (Lw[k + 1:, k] + s * x[k + 1:]) / c
                x[k + 1:] = c * x[k + 1:] - s * Lw[k + 1:, k]
    return Lw


def shift_factor_ref(L, sample_sigma):
    """(Sigma', L') from the factor alone, as the kernel forms them: the rank-4 update of L22 by the columns of L21, the factor of
    L[124:, :] L[124:, :]^T, c from the diagonal."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    Lp = np.zeros((N_A, N_A))
    Lp[:N_A - DU, :N_A - DU] = rank_update(L[DU:, DU:], L[DU:, :DU])
    Lp[N_A - DU:, N_A - DU:] = np.linalg.cholesky(L[N_A - DU:, :] @ L[N_A - DU:, :].T)
    logdet = 2.0 * np.log(np.diag(Lp)).sum()
    c = np.exp((2.0 * N_A * np.log(float(sample_sigma)) - logdet) / N_A)
    Lp *= np.sqrt(c)
    return Lp @ Lp.T, Lp


def shift_power_ref(Sigma, k, sample_sigma):
    """c_k S^k(Sigma) written down directly: k shifts leave the trailing 128 - 4 k rows and columns of Sigma in the corner and k
    copies of its last stage's 4 x 4 marginal B = Sigma[124:, 124:] below them, no cross terms; from k = 31 on that is 32 copies of
    B, whatever k."""
    Sigma = np.asarray(Sigma, dtype=np.float64)
    j = min(int(k), N_A // DU - 1)
    m = N_A - DU * j
    S = np.zeros((N_A, N_A))
    S[:m, :m] = Sigma[DU * j:, DU * j:]
    for t in range(j):
        S[m + DU * t:m + DU * t + DU, m + DU * t:m + DU * t + DU] = Sigma[N_A - DU:, N_A - DU:]
    return volume_scalar(S, sample_sigma) * S


def shift_chain_ref(L, k, sample_sigma, rounded=True, every=False):
    """(Sigma', L') after k reuse steps in a row: shift_factor_ref applied k times, each step fed the previous one's L' rounded to
    fp32 -- what the device keeps between steps (rounded=False: the fp64 L' as it is).  every=True: the list of all k results."""
    out = []
    for _ in range(int(k)):
        Sp, Lp = shift_factor_ref(L, sample_sigma)
        out.append((Sp, Lp))
        L = Lp.astype(np.float32) if rounded else Lp
    return out if every else out[-1]


def decoupled_rows(k):
    """After k shifts the rows from here on hold decoupled 4 x 4 stages only."""
    return N_A - DU * min(int(k), N_A // DU - 1)


BAR_L, BAR_SIGMA, BAR_LOGDET = 3e-6, 1e-6, 2 * N_A * 2.0 ** -24  # one reuse step's bars (tests/test_gpu_sigma_period.py)


def off_structure(k):
    """True where Sigma' and L' are exactly zero after k shifts: everything outside the leading corner and the decoupled 4 x 4 stages."""
    m = decoupled_rows(k)
    off = np.ones((N_A, N_A), dtype=bool)
    off[:m, :m] = False
    for t in range(m, N_A, DU):
        off[t:t + DU, t:t + DU] = False
    return off


def chain_ratios(Sp, Lp, Sref, Lref, sample_sigma):
    """(log det, L', Sigma') errors of an fp32 (Sigma', L') against a reference, each over its one-step bar."""
    Sp64, Lp64 = np.asarray(Sp, dtype=np.float64), np.asarray(Lp, dtype=np.float64)
    e_ld = abs(2.0 * np.log(np.diag(Lp64)).sum() - 2.0 * N_A * np.log(float(sample_sigma)))
    e_L = np.abs(Lp64 - Lref).max() / np.abs(Lref).max()
    e_S = np.abs(Sp64 - Sref).max() / np.abs(Sref).max()
    return np.array([e_ld / BAR_LOGDET, e_L / BAR_L, e_S / BAR_SIGMA])


def random_spd(rng, cond=1e3):
    w = np.exp(np.linspace(0.0, np.log(cond), N_A)) * 1e-2
    U, _ = np.linalg.qr(rng.normal(size=(N_A, N_A)))
    A = (U * w) @ U.T
    return 0.5 * (A + A.T)  # exactly symmetric


def random_spd_factors():
    """The fp32 factors of random_spd at cond 6e2 and 7e4 (the matrices of test_rank4_update_equals_the_cholesky_of_the_trailing_block)."""
    rng = np.random.default_rng(12)
    return [np.linalg.cholesky(random_spd(rng, cond)).astype(np.float32) for cond in (6e2, 7e4)]


# ---------------------------------------------------------------------------------------------- Sigma adapt (uses post_cov's C)
def blend_M(Sigma, Cmat, gamma):
    """M = (1 - gamma) S(Sigma) + gamma S(C); the lower triangle of C is what counts (the kernel reads nothing else)."""
    Cl = np.tril(np.asarray(Cmat, dtype=np.float64))
    Cs = Cl + np.tril(Cl, -1).T
    g = float(gamma)
    return (1.0 - g) * shift_S(np.asarray(Sigma, dtype=np.float64)) + g * shift_S(Cs)


def guarded_factor(M):
    """The lower Cholesky factor of M, or None when the guard fires: a pivot that is not finite or not positive, or a log det that
    is not finite."""
    if not np.all(np.isfinite(M)):
        return None
    try:
        Lf = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return None
    d = np.diag(Lf)
    if not (np.all(np.isfinite(d)) and np.all(d > 0.0) and np.isfinite(np.log(d).sum())):
        return None
    return Lf


def adapt_ref(L, Cmat, gamma, sample_sigma):
    """(Sigma', L', fallback, c, log det M) of the definition from the factor L the previous step sampled from (its lower triangle)
    and that step's posterior covariance C: Sigma' = c M, M = (1 - gamma) S(L L^T) + gamma S(C); a blend the guard refuses gives the
    gamma = 0 answer with fallback = 1."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    Sigma = L @ L.T
    fallback = 0
    M = blend_M(Sigma, Cmat, gamma) if float(gamma) != 0.0 else shift_S(Sigma)
    Lf = guarded_factor(M)
    if Lf is None:
        fallback, M = 1, shift_S(Sigma)
        Lf = np.linalg.cholesky(M)
    logdet = 2.0 * np.log(np.diag(Lf)).sum()
    c = float(np.exp((2.0 * N_A * np.log(float(sample_sigma)) - logdet) / N_A))
    return c * M, np.sqrt(c) * Lf, fallback, c, logdet
