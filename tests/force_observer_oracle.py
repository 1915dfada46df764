"""fp64 oracle of the force observer (csrc/force_observer.hip), a plain helper module like tests/estimator_oracle.py:
the 16-state extended Kalman filter on oracle/ref_torch.py's dyn, its Jacobian by torch.func.jacfwd, the linear algebra in numpy.

Per instance the filter keeps xi = (x [13]: pos, vel, quat, omega; f [3]: the disturbance force), P (16 x 16), the time word t_prev of
the row it last saw, and a valid bit.  A call with the measured row z (32 packed floats) and the applied action u (4); the row's force
slots are never read:
    not all 13 measured coordinates finite   flag 4: the row is untouched, the filter is invalidated
    no valid state / time(z) != t_prev + 1   flag 1 / 2: x = z, f = 0, P = diag(R, force_init_std^2 I3); row[13:16] = 0
    else  x- = dyn(x, clip(u), f), f- = f,  A16 = d (x-, f-) / d (x, f) at xi,  P- = A16 P A16^T + Q
          H = [I13 0],  S = P-[0:13, 0:13] + R = C C^T (unpivoted),  nu = z - x-,  K = (S^-1 P-[0:13, :])^T,  xi = xi- + K nu
          P = (I - K H) P- (I - K H)^T + K R K^T, the lower triangle mirrored
          a pivot of S not positive and finite, or a non-finite entry of xi or P: flag 8, as an initialisation
    row[0:16] = fp32(xi); t_prev = time(z)
side row [8] = {flags, nu^T S^-1 nu, |nu_pos|, |f^|, P00 + P11 + P22, P13,13 + P14,14 + P15,15, smallest pivot of S (C_kk^2), time}
(an initialisation reports 0 for the innovation entries, |f^| and the pivot; an invalidation reports 0 everywhere but flags and time).

algebra_longdouble re-runs a call's filter algebra in np.longdouble from the same x- and A16 (a hand-written Cholesky: numpy's LAPACK
has no extended type); FP64_LOSS below is the largest deviation of the fp64 filter from it on the chains the GPU test runs, measured by
tests/test_force_observer_oracle.py, and the number the GPU test's bar is built from.
"""
import numpy as np
import torch

from oracle import ref_torch as RT
from tests.estimator_oracle import GROUP, OBS_GROUP_SCALE, ST_TIME, measure  # noqa: F401  (one convention for both filters)
from tests.riccati_oracle import model_params

NX, NF, N = 13, 3, 16
ST_FDIST = 13
FLAG_INIT, FLAG_TIME, FLAG_NONFINITE, FLAG_FAILED = 1, 2, 4, 8
GROUP16 = np.concatenate([GROUP, [4, 4, 4]])  # the force: a fifth group

# The fp64 filter's largest deviation from its np.longdouble re-run over the GPU test's chains (5 start states x 3 masses x 8 calls, each
# filter on its own state): deviation() below, measured and held to this value by tests/test_force_observer_oracle.py.
FP64_LOSS = 4.4e-15  # (measured 4.35e-15, at far_fast, mass 0.021, call 5)

# The open-loop experiment's ratio under the periodic plant (force_ratio, mean of seeds 0, 1, 2: 0.444, 0.304, 0.290), measured and held
# to this value by tests/test_force_observer_oracle.py; the GPU test's closed-loop episode is held to 1.5 x this.
OPEN_LOOP_PERIODIC_RATIO = 0.346


def _t(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=torch.float64)


def constants(p, obs_std=None, proc_std=None, force_walk_std=None, force_init_std=None, obs_noise_scale=0.05):
    """(R [13], Q [16], P0 [16]): the diagonals; the defaults of the issue: obs_noise_scale (.25, .5, .02, .5), proc_std 0,
    force_walk_std = dyn_noise_scale, force_init_std = disturb_scale / sqrt(3)."""
    obs = obs_noise_scale * OBS_GROUP_SCALE if obs_std is None else np.asarray(obs_std, dtype=np.float64)
    proc = np.zeros(4) if proc_std is None else np.asarray(proc_std, dtype=np.float64)
    fw = float(p.dyn_noise_scale) if force_walk_std is None else float(force_walk_std)
    fi = abs(float(p.disturb_scale)) / np.sqrt(3.0) if force_init_std is None else float(force_init_std)
    R = (obs ** 2)[GROUP]
    return R, np.concatenate([(proc ** 2)[GROUP], np.full(NF, fw * fw)]), np.concatenate([R, np.full(NF, fi * fi)])


def model(p):
    """xi [16], u [4] (numpy fp64) -> (xi- [16], A16 [16, 16]) of one model step with the force as a state"""
    prm = model_params(p)

    def step(xi, u):
        pos, vel, quat, om = RT.dyn(xi[0:3], xi[3:6], xi[6:10], xi[10:13], xi[13:16], u, prm)
        return torch.cat([pos, vel, quat, om, xi[13:16]])

    def both(xi, u):
        xi, u = _t(xi), _t(u)
        return step(xi, u).numpy(), torch.func.jacfwd(lambda y: step(y, u))(xi).numpy()

    return both


def algebra(xm, A, P, Q, R, z):
    """The filter algebra of one update in fp64 -> (xi, P, nis, |nu_pos|, smallest pivot), or None (flag 8)"""
    with np.errstate(all="ignore"):
        Pm = A @ P @ A.T + np.diag(Q)
        S = Pm[:NX, :NX] + np.diag(R)
        try:
            C = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            return None
        piv = np.diag(C) ** 2
        if not (np.isfinite(piv).all() and (piv > 0).all()):
            return None
        nu = z - xm[:NX]
        K = np.linalg.solve(S, Pm[:NX, :]).T  # 16 x 13
        xi = xm + K @ nu
        G = np.eye(N)
        G[:, :NX] -= K
        Pn = G @ Pm @ G.T + (K * R) @ K.T
        Pn = np.tril(Pn) + np.tril(Pn, -1).T
        if not (np.isfinite(xi).all() and np.isfinite(Pn).all()):
            return None
        return xi, Pn, float(nu @ np.linalg.solve(S, nu)), float(np.linalg.norm(nu[0:3])), float(piv.min())


def algebra_longdouble(xm, A, P, Q, R, z):
    """algebra() in np.longdouble from the same xm and A -> (xi, P) as longdouble"""
    L = np.longdouble
    xm, A, P, Q, R, z = (np.asarray(v, dtype=L) for v in (xm, A, P, Q, R, z))
    Pm = A @ P @ A.T + np.diag(Q)
    S = Pm[:NX, :NX] + np.diag(R)
    C = np.zeros((NX, NX), dtype=L)
    for j in range(NX):
        C[j, j] = np.sqrt(S[j, j] - C[j, :j] @ C[j, :j])
        for i in range(j + 1, NX):
            C[i, j] = (S[i, j] - C[i, :j] @ C[j, :j]) / C[j, j]

    def solve(B):  # S^-1 B
        Y = np.array(B, dtype=L)
        for i in range(NX):
            Y[i] = (Y[i] - C[i, :i] @ Y[:i]) / C[i, i]
        for i in range(NX - 1, -1, -1):
            Y[i] = (Y[i] - C[i + 1:, i] @ Y[i + 1:]) / C[i, i]
        return Y
    K = solve(Pm[:NX, :]).T
    xi = xm + K @ (z - xm[:NX])
    G = np.eye(N, dtype=L)
    G[:, :NX] -= K
    Pn = G @ Pm @ G.T + (K * R) @ K.T
    return xi, np.tril(Pn) + np.tril(Pn, -1).T


def deviation(xi, P, xi_ref, P_ref):
    """How far (xi, P) is from (xi_ref, P_ref), the measure of the GPU test's bar: xi per coordinate group, max |d xi_g| / max |xi_g|
    -- the force group on the scale max(max |f|, sqrt(max P_ff)): an estimate near 0 N is as good as its own standard deviation --,
    P on the scale of its own diagonal, max |dP_ij| / sqrt(P_ii P_jj), as tests/test_gpu_estimator.py scales it."""
    xi, P = np.asarray(xi, dtype=np.longdouble), np.asarray(P, dtype=np.longdouble)
    ex = 0.0
    for g in range(5):
        m = GROUP16 == g
        scale = np.abs(xi_ref[m]).max()
        if g == 4:
            scale = max(scale, np.sqrt(np.diag(P_ref)[m].max()))
        ex = max(ex, float(np.abs(xi[m] - xi_ref[m]).max() / scale))
    d = np.sqrt(np.diag(P_ref))
    return max(ex, float((np.abs(P - P_ref) / np.outer(d, d)).max()))


class Filter:
    """One instance's state; call(row, u) -> (row_out [32] float32, side [8] float64 with the two words as integers).  shadow=True: a
    second filter in np.longdouble rides along on its own state (self.xi_ld, self.P_ld), fed the same x- and A16 (moved to its own
    state by A16 (xi_ld - xi): exact to first order)."""

    def __init__(self, p, obs_std=None, proc_std=None, force_walk_std=None, force_init_std=None, obs_noise_scale=0.05, shadow=False):
        self.R, self.Q, self.P0 = constants(p, obs_std, proc_std, force_walk_std, force_init_std, obs_noise_scale)
        self.f = model(p)
        self.valid, self.shadow = False, shadow
        self.xi, self.P, self.t_prev = np.zeros(N), np.zeros((N, N)), 0
        self.xi_ld = self.P_ld = None

    @property
    def x(self):
        return self.xi[:NX]

    @property
    def force(self):
        return self.xi[NX:]

    def _init(self, z, t):
        self.xi, self.P, self.t_prev, self.valid = np.concatenate([z, np.zeros(NF)]), np.diag(self.P0), t, True
        if self.shadow:
            self.xi_ld, self.P_ld = self.xi.astype(np.longdouble), self.P.astype(np.longdouble)

    def call(self, row, u):
        row = np.asarray(row, dtype=np.float32)
        z = row[:NX].astype(np.float64)
        t = int(row.view(np.int32)[ST_TIME])
        out = row.copy()
        if not np.isfinite(z).all():
            self.valid = False
            return out, np.array([FLAG_NONFINITE, 0, 0, 0, 0, 0, 0, t], dtype=np.float64)
        flags = 0 if self.valid else FLAG_INIT
        if self.valid and t != self.t_prev + 1:
            flags = FLAG_TIME
        res = None
        if flags == 0:
            xm, A = self.f(self.xi, np.clip(np.asarray(u, dtype=np.float32).astype(np.float64), -1.0, 1.0))
            res = algebra(xm, A, self.P, self.Q, self.R, z)
            if res is None:
                flags = FLAG_FAILED
            elif self.shadow:
                xm_ld = xm.astype(np.longdouble) + A.astype(np.longdouble) @ (self.xi_ld - self.xi.astype(np.longdouble))
                self.xi_ld, self.P_ld = algebra_longdouble(xm_ld, A, self.P_ld, self.Q, self.R, z)
        if res is None:
            self._init(z, t)
            out[ST_FDIST:ST_FDIST + NF] = 0.0
            return out, np.array([flags, 0, 0, 0, self.R[0:3].sum(), self.P0[NX:].sum(), 0, t], dtype=np.float64)
        self.xi, self.P, nis, innov, pivot = res
        self.t_prev = t
        out[:N] = self.xi.astype(np.float32)
        P = self.P
        return out, np.array([0, nis, innov, np.linalg.norm(self.xi[NX:]), P[0, 0] + P[1, 1] + P[2, 2],
                              P[13, 13] + P[14, 14] + P[15, 15], pivot, t], dtype=np.float64)


def pack_row(z13, f, t, base=None):
    """A packed row [32] float32 with the 13 coordinates, the (true) force and the time word (the rest from base, or 0)"""
    row = np.zeros(32, dtype=np.float32) if base is None else np.array(base, dtype=np.float32)
    row[:NX] = z13
    row[ST_FDIST:ST_FDIST + NF] = f
    row.view(np.int32)[ST_TIME] = t
    return row


def build_chain(s, p, seed, obs_std, n_calls=8, shadow=False, **kw):
    """The chain of the GPU test for start state s and model p: n_calls measured rows with their actions -- fresh fixed-seed
    measurements of a truth the oracle's model steps under a TRUE force of 0.1 N on one axis (which axis: the seed), the row's force
    slots holding that true force, one action beyond the clip -- and the oracle's answer to every call -> list of dicts."""
    rng = np.random.default_rng(seed)
    filt = Filter(p, obs_std=obs_std, shadow=shadow, **kw)
    hover = np.array([float(p.m) * float(p.g) / float(p.max_thrust) * 2.0 - 1.0, 0.0, 0.0, 0.0])
    xi = np.concatenate([s.pos, s.vel, s.quat, s.omega, np.zeros(NF)])
    xi[NX + seed % 3] = 0.1
    base = np.zeros(32, dtype=np.float32)
    base[16:25] = rng.normal(size=9)
    base[26:32] = rng.normal(size=6)  # (the row's unused tail: must survive)
    u = hover.astype(np.float32)
    calls = []
    for k in range(n_calls):
        row = pack_row(measure(rng, xi[:NX], obs_std), xi[NX:].astype(np.float32), int(s.time) + k, base)
        ref_row, ref_side = filt.call(row, u)
        call = dict(row=row, u=u, ref_row=ref_row, ref_side=ref_side, xi=filt.xi.copy(), P=filt.P.copy(), t_prev=filt.t_prev)
        if shadow:
            call.update(xi_ld=filt.xi_ld.copy(), P_ld=filt.P_ld.copy())
        calls.append(call)
        xi = filt.f(xi, np.clip(u.astype(np.float64), -1, 1))[0]
        u = (hover + 0.3 * rng.normal(size=4)).astype(np.float32)
        if k == 4:
            u[1] = 1.5  # (clipped by the model)
    return calls


def open_loop(s, p, seed, plant="periodic", n_steps=200, obs_noise_scale=0.05, **kw):
    """The issue's CPU experiment: n_steps from the oracle state s, open-loop actions around hover (0.1 normal), measurements at the
    reference's noise scales; the plant's force: "periodic" -- U(-disturb_scale, disturb_scale)^3 redrawn every disturb_period steps
    (defaults 0.2 N, 50), "gaussian" -- dyn_noise_scale normal redrawn every step.  Row t carries force[t], the force plant step t -> t
    + 1 integrates: the filter's estimate at call t is a prediction of it.
    -> (force [n_steps, 3], estimate [n_steps, 3], sides [n_steps, 8])"""
    rng = np.random.default_rng(seed)
    f = model(p)
    filt = Filter(p, obs_noise_scale=obs_noise_scale, **kw)
    obs = obs_noise_scale * OBS_GROUP_SCALE
    hover = np.array([float(p.m) * float(p.g) / float(p.max_thrust) * 2.0 - 1.0, 0.0, 0.0, 0.0])
    xi = np.concatenate([s.pos, s.vel, s.quat / np.linalg.norm(s.quat), s.omega, np.zeros(NF)]).astype(np.float64)
    scale, period = abs(float(p.disturb_scale)), max(int(p.disturb_period), 1)
    u = hover.astype(np.float32)
    forces, est, sides = [], [], []
    for k in range(n_steps):
        if plant == "gaussian":
            xi[NX:] = float(p.dyn_noise_scale) * rng.normal(size=NF)
        elif k % period == 0:
            xi[NX:] = rng.uniform(-scale, scale, size=NF)
        row = pack_row(measure(rng, xi[:NX], obs), xi[NX:].astype(np.float32), int(s.time) + k)
        out, side = filt.call(row, u)
        forces.append(xi[NX:].copy())
        est.append(out[ST_FDIST:ST_FDIST + NF].astype(np.float64))
        sides.append(side)
        u = (hover + 0.1 * rng.normal(size=4)).astype(np.float32)
        xi = f(xi, np.clip(u.astype(np.float64), -1, 1))[0]
    return np.array(forces), np.array(est), np.array(sides)


def force_ratio(forces, est, start=20):
    """RMS |f^_t - f_{t+1}| / RMS |f_{t+1}| from step `start`: the estimate written at call t against the true force of the NEXT row"""
    e = est[start:-1] - forces[start + 1:]
    return float(np.sqrt((e ** 2).sum(axis=1).mean()) / np.sqrt((forces[start + 1:] ** 2).sum(axis=1).mean()))
