"""fp64 oracle of the state estimator (csrc/state_estimator.hip), a plain helper module like tests/riccati_oracle.py:
the extended Kalman filter on oracle/ref_torch.py's dyn, its Jacobian by torch.func.jacfwd, the linear algebra in numpy.

Per instance the filter keeps x (13: pos, vel, quat, omega), P (13 x 13), the force f_prev and the time word t_prev of the row it last
saw, and a valid bit.  A call with the measured row z (32 packed floats) and the applied action u (4):
    not all 13 measured coordinates finite   flag 4: the row is untouched, the filter is invalidated
    no valid state / time(z) != t_prev + 1   flag 1 / 2: x = z, P = R, the row is untouched
    else  x- = dyn(x, clip(u), f_prev),  A = d dyn / d x at x,  P- = A P A^T + Q
          S = P- + R = C C^T (unpivoted),  nu = z - x-,  K = (S^-1 P-)^T,  x = x- + K nu
          P = (I - K) P- (I - K)^T + K R K^T, the lower triangle mirrored
          a pivot of S not positive and finite, or a non-finite entry of x or P: flag 8, x = z, P = R, the row is untouched
    row[0:13] = fp32(x); f_prev = z.f_disturb; t_prev = time(z)
side row [8] = {flags, nu^T S^-1 nu, |nu_pos|, |x - z|_pos, P00 + P11 + P22, P33 + P44 + P55, smallest pivot of S (C_kk^2), time}
(an initialisation reports 0 for the innovation entries and the pivot; an invalidation reports 0 everywhere but flags and time).
"""
import numpy as np
import torch

from oracle import ref_torch as RT
from tests.riccati_oracle import model_params

NX = 13
ST_FDIST, ST_TIME = 13, 25
GROUP = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3])
OBS_GROUP_SCALE = np.array([0.25, 0.5, 0.02, 0.5])  # the env step's noise per unit obs_noise_scale: pos, vel, quat, omega
FLAG_INIT, FLAG_TIME, FLAG_NONFINITE, FLAG_FAILED = 1, 2, 4, 8


def _t(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=torch.float64)


def constants(p, obs_std=None, proc_std=None, force_std=None, obs_noise_scale=0.05):
    """(R [13], Q [13]): the diagonals from the four group standard deviations; the defaults of the issue: obs_noise_scale (.25, .5,
    .02, .5) and (0, dt force_std / m, 0, 0) with force_std = dyn_noise_scale.  A negative proc_std[1] means "derive"."""
    obs = obs_noise_scale * OBS_GROUP_SCALE if obs_std is None else np.asarray(obs_std, dtype=np.float64)
    proc = np.array([0.0, -1.0, 0.0, 0.0]) if proc_std is None else np.array(proc_std, dtype=np.float64)
    if proc[1] < 0:
        fs = float(p.dyn_noise_scale) if force_std is None else float(force_std)
        proc[1] = float(p.dt) * fs / float(p.m)
    return (obs ** 2)[GROUP], (proc ** 2)[GROUP]


def model(p):
    """x [13], u [4], f [3] (numpy fp64) -> (x' [13], A [13, 13]) of one model step"""
    prm = model_params(p)

    def step(x, u, f):
        pos, vel, quat, om = RT.dyn(x[0:3], x[3:6], x[6:10], x[10:13], f, u, prm)
        return torch.cat([pos, vel, quat, om])

    def both(x, u, f):
        x, u, f = _t(x), _t(u), _t(f)
        return step(x, u, f).numpy(), torch.func.jacfwd(lambda y: step(y, u, f))(x).numpy()

    return both


class Filter:
    """One instance's state; call(row, u) -> (row_out [32] float32, side [8] float64 with the two words as integers)"""

    def __init__(self, p, obs_std=None, proc_std=None, force_std=None, obs_noise_scale=0.05):
        self.R, self.Q = constants(p, obs_std, proc_std, force_std, obs_noise_scale)
        self.f = model(p)
        self.valid = False
        self.x, self.P, self.f_prev, self.t_prev = np.zeros(NX), np.zeros((NX, NX)), np.zeros(3), 0

    def _init(self, z, f, t):
        self.x, self.P, self.f_prev, self.t_prev, self.valid = z.copy(), np.diag(self.R), f.copy(), t, True

    def call(self, row, u):
        row = np.asarray(row, dtype=np.float32)
        z = row[:NX].astype(np.float64)
        fz = row[ST_FDIST:ST_FDIST + 3].astype(np.float64)
        t = int(row.view(np.int32)[ST_TIME])
        out = row.copy()
        if not np.isfinite(z).all():
            self.valid = False
            return out, np.array([FLAG_NONFINITE, 0, 0, 0, 0, 0, 0, t], dtype=np.float64)
        flags = 0 if self.valid else FLAG_INIT
        if self.valid and t != self.t_prev + 1:
            flags = FLAG_TIME
        stats = None
        if flags == 0:
            stats = self._update(z, np.clip(np.asarray(u, dtype=np.float32).astype(np.float64), -1.0, 1.0))
            if stats is None:
                flags = FLAG_FAILED
        if stats is None:
            self._init(z, fz, t)
            return out, np.array([flags, 0, 0, 0, self.R[0:3].sum(), self.R[3:6].sum(), 0, t], dtype=np.float64)
        self.f_prev, self.t_prev = fz.copy(), t
        out[:NX] = self.x.astype(np.float32)
        nis, innov, pivot = stats
        P = self.P
        return out, np.array([0, nis, innov, np.linalg.norm(self.x[0:3] - z[0:3]), P[0, 0] + P[1, 1] + P[2, 2], P[3, 3] + P[4, 4] + P[5, 5],
                              pivot, t], dtype=np.float64)

    def _update(self, z, u):
        with np.errstate(all="ignore"):
            xm, A = self.f(self.x, u, self.f_prev)
            Pm = A @ self.P @ A.T + np.diag(self.Q)
            S = Pm + np.diag(self.R)
            try:
                C = np.linalg.cholesky(S)
            except np.linalg.LinAlgError:
                return None
            piv = np.diag(C) ** 2
            if not (np.isfinite(piv).all() and (piv > 0).all()):
                return None
            nu = z - xm
            K = np.linalg.solve(S, Pm).T
            x = xm + K @ nu
            G = np.eye(NX) - K
            P = G @ Pm @ G.T + (K * self.R) @ K.T
            P = np.tril(P) + np.tril(P, -1).T
            if not (np.isfinite(x).all() and np.isfinite(P).all()):
                return None
            self.x, self.P = x, P
            return float(nu @ np.linalg.solve(S, nu)), float(np.linalg.norm(nu[0:3])), float(piv.min())


def measure(rng, x, obs_std):
    """The env step's noisy copy of the true state x [13]: x + obs_std (by group) normal, as fp32"""
    return (x + np.asarray(obs_std)[GROUP] * rng.normal(size=NX)).astype(np.float32)


def pack_row(z13, f, t, base=None):
    """A packed row [32] float32 with the 13 coordinates, the force and the time word (the rest from base, or 0)"""
    row = np.zeros(32, dtype=np.float32) if base is None else np.array(base, dtype=np.float32)
    row[:NX] = z13
    row[ST_FDIST:ST_FDIST + 3] = f
    row.view(np.int32)[ST_TIME] = t
    return row


def open_loop(s, p, seed, n_steps=200, obs_noise_scale=0.05, **kw):
    """The issue's CPU experiment: n_steps from the oracle state s, open-loop actions around hover (0.1 normal), the plant under a
    gaussian force of dyn_noise_scale, measurements at the reference's noise scales -> (truth, measured, estimate [n_steps, 13],
    sides [n_steps, 8])"""
    rng = np.random.default_rng(seed)
    f = model(p)
    filt = Filter(p, obs_noise_scale=obs_noise_scale, **kw)
    obs = obs_noise_scale * OBS_GROUP_SCALE
    hover = np.array([float(p.m) * float(p.g) / float(p.max_thrust) * 2.0 - 1.0, 0.0, 0.0, 0.0])
    x = np.concatenate([s.pos, s.vel, s.quat / np.linalg.norm(s.quat), s.omega]).astype(np.float64)
    force = np.zeros(3)
    u = hover.astype(np.float32)
    truth, meas, est, sides = [], [], [], []
    for k in range(n_steps):
        row = pack_row(measure(rng, x, obs), force.astype(np.float32), int(s.time) + k)
        out, side = filt.call(row, u)
        truth.append(x.copy())
        meas.append(row[:NX].astype(np.float64))
        est.append(out[:NX].astype(np.float64))
        sides.append(side)
        u = (hover + 0.1 * rng.normal(size=4)).astype(np.float32)
        x = f(x, np.clip(u.astype(np.float64), -1, 1), row[ST_FDIST:ST_FDIST + 3].astype(np.float64))[0]
        force = float(p.dyn_noise_scale) * rng.normal(size=3)
    return np.array(truth), np.array(meas), np.array(est), np.array(sides)
