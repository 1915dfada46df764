"""The definition of the annealed step's spline-node sampler (controllers/_options.py: node_basis, node_schedule; csrc/noise_nodes.hip;
DESIGN 4.29) in plain fp64 numpy -- a support module, not collected by pytest, shared by tests/test_nodes_abi.py (CPU) and
tests/test_gpu_nodes.py.  Nothing of csrc/ is in it.

    nodes      t_m = (m * 31) / (M - 1), m < M
    weights    W[h][m] = phi_m(h): "linear" the hat function max(0, 1 - |h - t_m| / (31 / (M - 1))); "cubic" the natural cubic spline
               through the unit vector e_m (second derivatives from the FULL (M x M) system, end rows z = 0, textbook evaluation)
    tables     sigma_n[i][m] = sigma0 beta_pass^i beta_stage^(M - 1 - m) (fp64);  B[i][h][m] = fp32(sigma_n[i][m] W[h][m]);
               sigma_e[i][h] = fp32(sqrt(sum_m fp64(B[i][h][m])^2))
    sampler    a[n][h][c] = clip(mu[h][c] + sum_{m < M} B[h][m] eps[n][m][c]); the device forms the sum as an ascending-m fp32 fmaf
               chain from 0 and adds mu in fp32: forward bound (M + 2) 2^-24 (|mu| + sum_m |B eps|), clip is 1-Lipschitz
"""
import numpy as np

H = 32
MS = (2, 3, 5, 8, 16, 32)
INTERPS = ("linear", "cubic")
U = 2.0 ** -24


def node_times(M):
    return np.array([(m * (H - 1)) / (M - 1) for m in range(M)], dtype=np.float64)


def basis64(M, interp):
    """W [32, M] fp64, by the formulas of the header (not by the package's interval form: the two agree to rounding)."""
    t = node_times(M)
    hs = np.arange(H, dtype=np.float64)
    if interp == "linear":
        return np.maximum(0.0, 1.0 - np.abs(hs[:, None] - t[None, :]) / ((H - 1) / (M - 1)))
    d = np.diff(t)
    A = np.zeros((M, M))
    A[0, 0] = A[M - 1, M - 1] = 1.0
    for j in range(1, M - 1):
        A[j, j - 1], A[j, j], A[j, j + 1] = d[j - 1], 2.0 * (d[j - 1] + d[j]), d[j]
    Y = np.eye(M)
    rhs = np.zeros((M, M))
    for j in range(1, M - 1):
        rhs[j] = 6.0 * ((Y[j + 1] - Y[j]) / d[j] - (Y[j] - Y[j - 1]) / d[j - 1])
    z = np.linalg.solve(A, rhs)
    W = np.zeros((H, M))
    for h in range(H):
        j = min(max(int(np.searchsorted(t, h, side="right")) - 1, 0), M - 2)
        a, b = t[j + 1] - h, h - t[j]
        W[h] = (z[j] * a ** 3 + z[j + 1] * b ** 3) / (6.0 * d[j]) + (Y[j] / d[j] - z[j] * d[j] / 6.0) * a + \
            (Y[j + 1] / d[j] - z[j + 1] * d[j] / 6.0) * b
    return W


def tables64(sigma0, k, beta_pass, beta_stage, M, W):
    """(sigma_n fp64 [k, M], B float32 [k, 32, M], sigma_e float32 [k, 32]) from the weights W [32, M]"""
    sn = np.array([[float(sigma0) * float(beta_pass) ** i * float(beta_stage) ** (M - 1 - m) for m in range(M)] for i in range(k)])
    B = np.empty((k, H, M), dtype=np.float32)
    for i in range(k):
        for h in range(H):
            for m in range(M):
                B[i, h, m] = np.float32(sn[i, m] * W[h, m])
    se = np.sqrt((B.astype(np.float64) ** 2).sum(axis=2)).astype(np.float32)
    return sn, B, se


def cov_blocks(sigma_row):
    """a_cov as a pass leaves it: [32, 4, 4] float32, fp32(sigma_e[h]^2) I"""
    s = np.asarray(sigma_row, dtype=np.float32)
    return ((s * s).astype(np.float32)[:, None, None] * np.eye(4, dtype=np.float32)[None]).astype(np.float32)


def sample64(B, mu, eps):
    """B float32 [32, M], mu float32 [128], eps float32 [N, >= M, 4] -> (a fp64 [N, 32, 4] = clip(mu + B eps), the bound's magnitude
    |mu| + sum_m |B eps| [N, 32, 4]).  A NaN in mu stays a NaN here (np.clip propagates)."""
    B64, M = np.asarray(B, dtype=np.float64), B.shape[1]
    e = np.asarray(eps, dtype=np.float64)[:, :M, :]
    mu64 = np.asarray(mu, dtype=np.float64).reshape(1, H, 4)
    pre = mu64 + np.einsum("hm,nmc->nhc", B64, e)
    mag = np.abs(mu64) + np.einsum("hm,nmc->nhc", np.abs(B64), np.abs(e))
    return np.clip(pre, -1.0, 1.0), mag


def bound(M, mag):
    return (M + 2) * U * mag


def sample_words(B, mu, eps):
    """The device's own arithmetic through oracle/c_oracle.py's explicit fmaf chain: the sampler is the 128 x 128 product with
    L[(h, c)][(m, c')] = B[h][m] [c == c'] -- the terms with c != c' are fmaf(0, e, acc) = acc exactly (finite e) -- -> float32
    [N, 32, 4].  mu must be free of NaN (the C clip compares)."""
    from oracle import c_oracle
    M = B.shape[1]
    L = np.zeros((H, 4, H, 4), dtype=np.float32)
    for c in range(4):
        L[:, c, :M, c] = B
    e = np.zeros((eps.shape[0], H, 4), dtype=np.float32)
    e[:, :M] = np.asarray(eps, dtype=np.float32)[:, :M]
    return c_oracle.noise_gemm(L.reshape(128, 128), mu, e.reshape(-1, 128)).reshape(-1, H, 4)


def random_basis(M, seed):
    """A dense B [32, M] float32 with entries of both signs, rows of norm ~0.3"""
    rng = np.random.default_rng(70 + 13 * M + seed)
    return (0.3 / np.sqrt(M) * rng.normal(size=(H, M))).astype(np.float32)


def clip_live_mean(seed):
    """mu [128] float32 near +-1 in alternation with moderate entries: the clip is live on both sides"""
    rng = np.random.default_rng(300 + seed)
    mu = (0.2 * rng.normal(size=(H, 4))).astype(np.float32)
    mu[::3, 0] = 0.98
    mu[1::3, 1] = -0.98
    mu[2::5, 2] = 1.0
    mu[3::5, 3] = -1.0
    return mu.reshape(-1)


def normal4_host(key, N, M):
    """The device stream core.randn(key)[:N, :M, :] restated on the host in fp64 (csrc/rng_device.hpp: counter (m, n, 0, 0), Box-Muller
    pairs) -- the same bits, the transcendentals in fp64, so equal to the device's values to ~1e-6: for CPU checks of PROPERTIES
    of a draw (the rank test's gap), not for comparisons."""
    from covo_mpc_amd.random import _philox
    n, m = np.meshgrid(np.arange(N, dtype=np.uint32), np.arange(M, dtype=np.uint32), indexing="ij")
    z = np.zeros_like(n)
    r = _philox(m, n, z, z, int(key[0]), int(key[1]))
    u = [((x >> np.uint32(8)).astype(np.float64) + 0.5) / 16777216.0 for x in r]
    ra, rb = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    return np.stack([ra * np.cos(2 * np.pi * u[1]), ra * np.sin(2 * np.pi * u[1]), rb * np.cos(2 * np.pi * u[3]),
                     rb * np.sin(2 * np.pi * u[3])], axis=-1)


# the rank test's case (tests/test_gpu_nodes.py; checked on the CPU in tests/test_nodes_abi.py)
RANK_N, RANK_M, RANK_SIGMA, RANK_KEY_SEED = 1000, 5, 0.05, 21


def rank_bar(N, M, amax):
    """singular value number 4 M + 1 of the sample matrix [N, 128] of a rank-4 M draw: every entry is off the exact product by at
    most (M + 2) 2^-24 max|a|, the spectral norm of such an error matrix at most sqrt(128 N) times that"""
    return np.sqrt(128.0 * N) * (M + 2) * U * amax
