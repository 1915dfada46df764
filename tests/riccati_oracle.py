"""fp64 oracle of the Riccati refinement (csrc/riccati.hip), a plain helper module like tests/sigma_shift_oracle.py: the stage blocks
of the Hessian's objective by torch.func on oracle/ref_torch.py's dyn / reward, and the sweep, the ladder and the forward pass in numpy.

In cost sign, with c_k = -r_k on the PRE-step state x_k (k = 0 .. 31), x_{k+1} = f_k(x_k, u_k) = dyn(x_k, force_k, u_k):
    costate   lam_32 = 0,  lam_k = grad c_k + A_k^T lam_{k+1}
    gradient  g_k = B_k^T lam_{k+1}
    blocks    M_k = Hess_z( c_k(x) + lam_{k+1} . f_k(z) ),  z = (x, u)
The force of step k is a constant of that step (kinds none / periodic), formed as oracle/ref_torch.py::make_objective forms it: step 0
runs under the state's own force, and under kind "none" every later step under zero.
"""
import numpy as np
import torch

from oracle import ref_torch as RT

NX, NU, H = 13, 4, 32
RUNGS = 8


def _t(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=torch.float64)


def model_params(p):
    """oracle/ref_torch.py::make_objective's parameter dict"""
    return dict(max_thrust=float(p.max_thrust), max_torque=_t(p.max_torque), max_omega=_t(p.max_omega), dt=float(p.dt), g=float(p.g),
                m=float(p.m), action_scale=float(p.action_scale), alpha_bodyrate=float(p.alpha_bodyrate),
                disturb_period=int(p.disturb_period), disturb_scale=float(p.disturb_scale), disturb_params=_t(p.disturb_params))


def step_forces(s, p, kind, draws=None):
    """[H, 3]: the force step k integrates (kinds none / periodic: no function of the state), as make_objective threads it"""
    prm = model_params(p)
    f = _t(s.f_disturb)
    out = [f]
    for k in range(H - 1):
        f = RT.disturb_next(kind, prm, int(s.time) + k, torch.zeros(3, dtype=torch.float64), f, None if draws is None else draws[k])
        out.append(f)
    return torch.stack(out).numpy()


def forces_from_table(s, tab):
    """[H, 3] from the device's Hessian table (csrc/disturb.hip): row k >= 1 holds the force of step k, step 0 runs under the state's"""
    f = np.array(tab[:, :3], dtype=np.float64)
    f[0] = np.asarray(s.f_disturb, dtype=np.float64)
    return f


def _stage_functions(s, p, reward_kind, forces):
    prm = model_params(p)
    pt, vt = _t(s.pos_traj), _t(s.vel_traj)
    T = pt.shape[0]
    tars = [(_t(s.pos_tar), _t(s.vel_tar))]
    for k in range(1, H):
        idx = min(max(int(s.time) + k, 0), T - 1)
        tars.append((pt[idx], vt[idx]))
    fd = _t(forces)

    def f(k, z):
        pos, vel, quat, om = RT.dyn(z[0:3], z[3:6], z[6:10], z[10:13], fd[k], z[13:17], prm)
        return torch.cat([pos, vel, quat, om])

    def c(k, x):
        if reward_kind == "penyaw":
            return -RT.reward(x[0:3], x[3:6], x[6:10], tars[k][0], tars[k][1])
        return -RT.reward_realworld(x[0:3], x[6:10], tars[k][0])

    return f, c


def stage_blocks(s, p, a, reward_kind="penyaw", forces=None):
    """dict of numpy fp64: x [H, 13] the nominal states, A [H, 13, 13], B [H, 13, 4], lam [H + 1, 13], g [128], Mxx [H, 13, 13],
    Mxu [H, 13, 4], Muu [H, 4, 4] at the plan a [128]"""
    if forces is None:
        forces = step_forces(s, p, "none")
    f, c = _stage_functions(s, p, reward_kind, forces)
    u = _t(a).reshape(H, NU)
    x = torch.cat([_t(s.pos), _t(s.vel), _t(s.quat), _t(s.omega)])
    xs, J, gc = [], [], []
    for k in range(H):
        z = torch.cat([x, u[k]])
        xs.append(x)
        J.append(torch.func.jacfwd(lambda zz, k=k: f(k, zz))(z))
        gc.append(torch.func.jacfwd(lambda xx, k=k: c(k, xx))(x))
        x = f(k, z)
    lam = [None] * H + [torch.zeros(NX, dtype=torch.float64)]
    M, g = [None] * H, [None] * H
    for k in range(H - 1, -1, -1):
        lk1 = lam[k + 1]
        lam[k] = gc[k] + J[k][:, :NX].T @ lk1
        g[k] = J[k][:, NX:].T @ lk1
        z = torch.cat([xs[k], u[k]])
        ham = lambda zz, k=k, lk1=lk1: c(k, zz[:NX]) + lk1 @ f(k, zz)
        M[k] = torch.func.jacfwd(torch.func.jacfwd(ham))(z)
    J, M = torch.stack(J).numpy(), torch.stack(M).numpy()
    return dict(x=torch.stack(xs).numpy(), A=J[:, :, :NX], B=J[:, :, NX:], lam=torch.stack(lam).numpy(), g=torch.stack(g).numpy().reshape(-1),
                Mxx=M[:, :NX, :NX], Mxu=M[:, :NX, NX:], Muu=M[:, NX:, NX:])


def _chol4(Q):
    """unpivoted lower Cholesky of a 4 x 4 matrix -> (L, the four pivots before the square root) or (None, pivots so far)"""
    L = np.zeros((NU, NU))
    piv = []
    for j in range(NU):
        s = Q[j, j] - L[j, :j] @ L[j, :j]
        piv.append(s)
        if not (np.isfinite(s) and s > 0.0):
            return None, piv
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, NU):
            L[i, j] = (Q[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L, piv


def sweep(blk, mu):
    """The backward sweep with Quu + mu I and the linear forward pass -> dict: ok (all 32 factorisations succeeded), pivots (list),
    and, when ok, K [H, 4, 13], kff [H, 4], d [128], dx [H, 13]"""
    A, B = blk["A"], blk["B"]
    P, pv = np.zeros((NX, NX)), np.zeros(NX)
    K, kff = np.zeros((H, NU, NX)), np.zeros((H, NU))
    pivots = []
    for k in range(H - 1, -1, -1):
        Ak, Bk = (A[k], B[k]) if k < H - 1 else (np.zeros((NX, NX)), np.zeros((NX, NU)))  # (P_32 = 0: stage 31 has no A, B)
        Qxx = blk["Mxx"][k] + Ak.T @ P @ Ak
        Qux = blk["Mxu"][k].T + Bk.T @ P @ Ak
        Quu = blk["Muu"][k] + Bk.T @ P @ Bk + mu * np.eye(NU)
        Qu = blk["g"][4 * k:4 * k + 4] + Bk.T @ pv
        L, piv = _chol4(Quu)
        pivots += piv
        if L is None:
            return dict(ok=False, pivots=pivots)
        solve = lambda rhs: np.linalg.solve(L.T, np.linalg.solve(L, rhs))
        kff[k] = -solve(Qu)
        K[k] = -solve(Qux)
        P = Qxx + Qux.T @ K[k]
        P = 0.5 * (P + P.T)
        pv = Ak.T @ pv + Qux.T @ kff[k]
    d, dx = forward(A, B, K, kff)
    return dict(ok=True, pivots=pivots, K=K, kff=kff, d=d, dx=dx)


def forward(A, B, K, kff):
    """dx_0 = 0, du_k = k_k + K_k dx_k, dx_{k+1} = A_k dx_k + B_k du_k -> (d [128], dx [H, 13])"""
    x = np.zeros(NX)
    d, dx = np.zeros((H, NU)), np.zeros((H, NX))
    for k in range(H):
        dx[k] = x
        d[k] = kff[k] + K[k] @ x
        if k < H - 1:
            x = A[k] @ x + B[k] @ d[k]
    return d.reshape(-1), dx


def ladder(blk, reg0=1e-2):
    """(rung, mu, sweep result) of the lowest rung mu_j = reg0 4^j, j < 8, whose sweep succeeds; (8, 0.0, None) when none does"""
    for j in range(RUNGS):
        mu = reg0 * 4.0 ** j
        r = sweep(blk, mu)
        if r["ok"]:
            return j, mu, r
    return RUNGS, 0.0, None


def tail_gain(s, p, a, reward_kind, forces, k, mu, xk):
    """The first four rows of -(R_tail + mu I)^-1 d^2 C_tail / da dx_k: the tail problem from the nominal state xk of stage k, whose
    cost is sum_{j >= k} c_j along the plan's tail a[4k:] -- what K_k of the sweep at the same mu equals"""
    f, c = _stage_functions(s, p, reward_kind, forces)

    def tail(x, at):
        u = at.reshape(H - k, NU)
        total = torch.zeros((), dtype=torch.float64)
        for j in range(k, H):
            total = total + c(j, x)
            x = f(j, torch.cat([x, u[j - k]]))
        return total

    x0, at = _t(xk), _t(a).reshape(-1)[4 * k:]
    Raa = torch.func.jacfwd(torch.func.jacfwd(tail, argnums=1), argnums=1)(x0, at).numpy()
    Rax = torch.func.jacfwd(torch.func.jacfwd(tail, argnums=1), argnums=0)(x0, at).numpy()
    return -np.linalg.solve(Raa + mu * np.eye(Raa.shape[0]), Rax)[:NU]


def candidates(b, d):
    """[17, 128] fp64 holding fp32 numbers: clip(b), then fp32(clip(b + 2^(3 - j) d)), j = 1 .. 16"""
    alpha = 2.0 ** (3 - np.arange(1, 17))
    b64 = np.asarray(b, dtype=np.float64)
    c = np.clip(b64[None] + alpha[:, None] * d[None], -1.0, 1.0).astype(np.float32).astype(np.float64)
    return np.concatenate([np.clip(b64, -1.0, 1.0)[None], c])
