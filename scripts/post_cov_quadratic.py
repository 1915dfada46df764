"""The posterior covariance on a problem with a known answer: samples x_i ~ N(mu, Sigma) in R^128, a synthetic quadratic cost
J(x) = (x - mu)^T H (x - mu) / 2 with H symmetric positive definite, weights exp(-J / lam).  The weighted cloud is then Gaussian with
covariance (Sigma^-1 + H / lam)^-1; the script feeds core.weighted_cov the samples and prints ||C - (Sigma^-1 + H / lam)^-1||_F
relative to the norm of the answer against N.  A statistical illustration (the error falls like 1 / sqrt(ESS)), not a test.
    python scripts/post_cov_quadratic.py [--lam 4.0] [--N 1024 4096 16384 65536 262144]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402

NA, H = 128, 32

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lam", type=float, default=4.0)
    ap.add_argument("--N", type=int, nargs="+", default=[1024, 4096, 16384, 65536, 262144])
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    Q, _ = np.linalg.qr(rng.normal(size=(NA, NA)))
    Sigma = (Q * np.geomspace(0.01, 0.09, NA)) @ Q.T  # unclipped: standard deviations 0.1 .. 0.3 about mu = 0
    Q2, _ = np.linalg.qr(rng.normal(size=(NA, NA)))
    Hm = (Q2 * np.geomspace(1.0, 100.0, NA)) @ Q2.T
    want = np.linalg.inv(np.linalg.inv(Sigma) + Hm / a.lam)
    L = np.linalg.cholesky(Sigma)
    mu = np.zeros(NA, dtype=np.float32)
    core = SamplingCore(max(a.N), H, a.lam, 1.0, device="cuda:0")
    print(f"lam = {a.lam}: ||Sigma||_F = {np.linalg.norm(Sigma):.4f}, ||(Sigma^-1 + H / lam)^-1||_F = {np.linalg.norm(want):.4f}")
    for N in a.N:
        x = (rng.normal(size=(N, NA)) @ L.T).astype(np.float32)
        J = 0.5 * np.einsum("ij,jk,ik->i", x.astype(np.float64), Hm, x.astype(np.float64)).astype(np.float32)
        stripes = torch.from_numpy(np.ascontiguousarray(x.reshape(N, H, 4).transpose(1, 0, 2))).to("cuda:0")
        C, d, W = core.weighted_cov(stripes, torch.from_numpy(J).to("cuda:0"), torch.from_numpy(mu).to("cuda:0"), lam=a.lam)
        torch.cuda.synchronize()
        w = np.exp(-(J - J.min()).astype(np.float64) / a.lam)
        ess = w.sum() ** 2 / (w ** 2).sum()
        err = np.linalg.norm(C.cpu().numpy().astype(np.float64) - want) / np.linalg.norm(want)
        print(f"N = {N:7d}  ESS = {ess:10.1f}  ||C - (Sigma^-1 + H / lam)^-1|| / ||.|| = {err:.4f}  |d|_max = {float(d.abs().max()):.2e}")
    assert core.device_status() == 0
    core.close()
