"""The definition of covo-online in spline-node space (controllers/_options.py: check_sigma_nodes; csrc/sigma_nodes.hip) in
plain fp64 numpy -- a support module, not collected by pytest, shared by tests/test_sigma_nodes_abi.py (CPU) and
tests/test_gpu_sigma_nodes.py.  Nothing of csrc/ is in it: numpy.linalg.eigh and numpy.linalg.cholesky stand where the kernel has its
Jacobi sweeps and its LDS factorisation.

    P        = W (x) I_4 [128, d], d = 4 M, W [32, M] the interpolation weights (node_basis)
    R_M      = P^T ((R + R^T) / 2) P
    Sigma_M  = optimize_sigma(R_M) with element_num = d (oracle/ref_np.py's expression, restated for d): log det Sigma_M = 2 d log sigma
    L_M      = cholesky(Sigma_M),  G = fp32(P L_M) [128, d],  Sigma_stage = P Sigma_M P^T [128, 128]
    sampler  a[n][h][i] = clip(mu[h][i] + sum_{c < d} G[(h, i)][c] eps[n][c div 4][c mod 4]); the device forms the sum as ONE ascending-c
             fp32 fmaf chain from 0 and adds mu in fp32 (oracle/c_oracle.py's explicit chain: sample_words)
"""
import numpy as np

H = 32
NA = 128
MS = (2, 3, 5, 8, 16)        # an odd block count twice, the smallest and the largest d
INTERPS = ("linear", "cubic")
U = 2.0 ** -24


def projector(W):
    """P = W (x) I_4: [128, 4 M] fp64"""
    return np.kron(np.asarray(W, dtype=np.float64), np.eye(4))


def project(R, W):
    """R_M = P^T sym(R) P, symmetrised once more so that it is symmetric bit for bit"""
    P = projector(W)
    Rs = 0.5 * (np.asarray(R, dtype=np.float64) + np.asarray(R, dtype=np.float64).T)
    RM = P.T @ Rs @ P
    return 0.5 * (RM + RM.T)


def optimize_sigma_d(RM, sample_sigma):
    """covo.py:116-132 in d = len(RM) dimensions -> (Sigma_M, eigenvalues of R_M ascending, eigenvalues of Sigma_M in that order)"""
    RM = 0.5 * (RM + RM.T)
    lam, u = np.linalg.eigh(RM)
    d = RM.shape[0]
    log_o = np.log(lam - lam.min() + 1e-2)
    log_const = (d * (np.log(float(sample_sigma)) * 2.0) * 2.0 + log_o.sum()) / d
    log_s = 0.5 * log_const - 0.5 * log_o
    S = (u * np.exp(log_s)[None, :]) @ u.T
    return 0.5 * (S + S.T), lam, np.exp(log_s)


def solve(R, W, sample_sigma):
    """Steps 1-5 and 7 of the definition -> dict(RM, SigmaM, L, G64 (fp64 [128, d]), G (float32), Sigma_stage (fp64 [128, 128]), lam, s)"""
    P = projector(W)
    RM = project(R, W)
    SM, lam, s = optimize_sigma_d(RM, sample_sigma)
    L = np.linalg.cholesky(SM)
    G64 = P @ L
    Sst = P @ SM @ P.T
    return dict(RM=RM, SigmaM=SM, L=L, G64=G64, G=G64.astype(np.float32), Sigma_stage=0.5 * (Sst + Sst.T), lam=lam, s=s)


def fallback(W, sample_sigma):
    """What an instance that fell back samples from: Sigma_M = sigma^2 I_d"""
    M = np.asarray(W).shape[1]
    P = projector(W)
    sg = float(sample_sigma)
    return dict(SigmaM=sg * sg * np.eye(4 * M), G=(sg * P).astype(np.float32), Sigma_stage=sg * sg * (P @ P.T))


def rel(a, b):
    """max-abs of a - b over the spectral norm of b"""
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.linalg.norm(b, 2))


# ------------------------------------------------------------------------------------------ the sampler
def sample64(G, mu, eps):
    """G float32 [128, d], mu float32 [128], eps float32 [N, >= d / 4, 4] -> (a fp64 [N, 32, 4] = clip(mu + G eps), the unclipped value,
    the bound's magnitude |G| |eps| [N, 32, 4])"""
    G64 = np.asarray(G, dtype=np.float64)
    d = G64.shape[1]
    e = np.asarray(eps, dtype=np.float64)[:, :d // 4, :].reshape(-1, d)
    pert = (e @ G64.T).reshape(-1, H, 4)
    mag = (np.abs(e) @ np.abs(G64).T).reshape(-1, H, 4)
    pre = np.asarray(mu, dtype=np.float64).reshape(1, H, 4) + pert
    return np.clip(pre, -1.0, 1.0), pre, mag


def sample_words(G, mu, eps):
    """The device's own arithmetic through oracle/c_oracle.py's explicit fmaf chain: the sampler is the 128 x 128 product whose first d
    columns are G -- a zero column contributes fmaf(0, e, acc) = acc exactly (finite e) -- -> float32 [N, 32, 4].  mu must be free of
    NaN (the C clip compares)."""
    from oracle import c_oracle
    G = np.asarray(G, dtype=np.float32)
    d = G.shape[1]
    L = np.zeros((NA, NA), dtype=np.float32)
    L[:, :d] = G
    e = np.zeros((eps.shape[0], H, 4), dtype=np.float32)
    e[:, :d // 4] = np.asarray(eps, dtype=np.float32)[:, :d // 4]
    return c_oracle.noise_gemm(L, np.asarray(mu, dtype=np.float32), e.reshape(-1, NA)).reshape(-1, H, 4)


def chain_bound(d, mag):
    """forward bound of a d-term fp32 fmaf chain: d 2^-24 (|G| |eps|)"""
    return d * U * mag


def random_factor(d, seed, scale=0.3):
    """A dense G [128, d] float32 with entries of both signs, rows of norm ~scale"""
    rng = np.random.default_rng(900 + 7 * d + seed)
    return (scale / np.sqrt(d) * rng.normal(size=(NA, d))).astype(np.float32)


def clip_live_mean(seed):
    """mu [128] float32 at +-0.999 in alternation with moderate entries: the clip is live on both sides"""
    rng = np.random.default_rng(300 + seed)
    mu = (0.2 * rng.normal(size=(H, 4))).astype(np.float32)
    mu[::3, 0] = 0.999
    mu[1::3, 1] = -0.999
    mu[2::5, 2] = 0.999
    mu[3::5, 3] = -0.999
    return mu.reshape(-1)


# ------------------------------------------------------------------------------------------ crafted Hessians
def _orth(seed, n=NA):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(n, n)))
    return q


def crafted(kind, W=None):
    """A 128 x 128 fp64 matrix of one crafted kind:
    "indefinite"  eigenvalues of both signs, -300 .. 500
    "graded"      a positive spectrum graded over 10 decades, 1e-4 .. 1e6
    "repeated"    P0 A P0^T with P0 the orthonormalised P of `W` and A = Q diag(3, 3, 3, 7, 7, 1 ..) Q^T: R_M has repeated eigenvalues
                  whenever P^T P is well conditioned (and a repeated PAIR exactly for the matrix itself at M = 32 linear)
    "zero"        R = 0: Sigma_M = sigma^2 I
    Not symmetric to rounding on purpose ("indefinite" carries a skew part the symmetrisation must remove)."""
    if kind == "zero":
        return np.zeros((NA, NA))
    if kind == "indefinite":
        q = _orth(11)
        R = (q * np.linspace(-300.0, 500.0, NA)[None, :]) @ q.T
        K = np.random.default_rng(12).normal(size=(NA, NA))
        return R + 5.0 * (K - K.T)
    if kind == "graded":
        q = _orth(13)
        return (q * np.logspace(-4.0, 6.0, NA)[None, :]) @ q.T
    if kind == "repeated":
        P = projector(W)
        d = P.shape[1]
        p0, r = np.linalg.qr(P)            # P = p0 r
        ev = np.ones(d)
        ev[:3], ev[3:5] = 3.0, 7.0
        q = _orth(17, d)
        A = (q * ev[None, :]) @ q.T
        rinv = np.linalg.inv(r)
        return p0 @ (rinv.T @ A @ rinv) @ p0.T   # P^T R P = r^T (rinv^T A rinv) r = A
    raise ValueError(kind)
