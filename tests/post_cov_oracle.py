"""`ref_weighted_cov`: the fp64 restatement of the posterior covariance's definition (covo_weighted_cov).
tests/test_post_cov_abi.py checks it against hand-derived answers; the GPU tests compare the kernels against it."""
import numpy as np

NA = 128


def ref_weights(cost, lam=None, elite=None):
    """The weights of the definition, fp64: softmax exp(-(c - c_min) / lam) over the finite costs, or 1 on the `elite` samples of
    smallest key (cost, index) -- a NaN cost sorts last, +inf is a large cost -- and 0 elsewhere; a cost that is not finite weighs 0."""
    c = np.asarray(cost, dtype=np.float64).reshape(-1)
    fin = np.isfinite(c)
    w = np.zeros_like(c)
    if elite:
        key = np.where(np.isnan(c), np.inf, c)
        order = np.lexsort((np.arange(c.size), np.isnan(c), key))  # cost, then NaN last, then the lowest index
        w[order[:int(elite)]] = 1.0
        w[~fin] = 0.0
    elif fin.any():
        w[fin] = np.exp(-(c[fin] - c[fin].min()) / float(lam))
    return w


def ref_weighted_cov(a, cost, mu, lam=None, elite=None):
    """a [H, N, 4], cost [N], mu [128] (any float dtype, taken as they are) -> (C [128, 128], d [128], W, absS [128, 128]) in fp64:
    x_i[4 t + j] = a[t, i, j], y_i = x_i - mu, W = sum w, d = sum w y / W, C = sum w y y^T / W - d d^T;
    absS = sum w |y| |y|^T / W, the scale of the GPU tests' bar.  W = 0: zeros."""
    a = np.asarray(a, dtype=np.float64)
    N = a.shape[1]
    x = a.transpose(1, 0, 2).reshape(N, NA)
    y = x - np.asarray(mu, dtype=np.float64).reshape(1, NA)
    w = ref_weights(cost, lam, elite)
    W = w.sum()
    if not W > 0.0:
        z = np.zeros((NA, NA))
        return z, np.zeros(NA), 0.0, z
    live = w > 0.0  # a sample of weight 0 is dropped whatever it holds
    y, w = y[live], w[live]
    d = (w[:, None] * y).sum(axis=0) / W
    C_ = (y * w[:, None]).T @ y / W - np.outer(d, d)
    absS = (np.abs(y) * w[:, None]).T @ np.abs(y) / W
    return C_, d, W, absS
