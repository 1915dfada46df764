"""Oracle of the closed-loop generator (csrc/feedback_rollout.hip), a plain helper module like tests/riccati_oracle.py: the forward pass
of DDP / iLQR under the Riccati sweep's gains, the nonlinear plant of oracle/ref_np.py::raw_step in the loop, all step sizes at once.

    for k = 0 .. 31:
        dx   = (double)x_k - xb_k                                   (13 raw coordinates: pos, vel, quat, omega)
        v_i  = alpha kff_k[i] + b_k[i];  v_i += K_k[i][j] dx_j,  j ascending   (fp64)
        u_k  = clip(v, -1, 1)                                        (rounded to float32 when the state is float32)
        x_{k+1} = raw_step(x_k, u_k) under forces[k]
A v that is not finite makes the sequence invalid from that k on: its actions are clip(b) from there.

dtype=np.float64: the exact loop, actions unrounded.  dtype=np.float32: the restatement of the kernel -- state and plant in float32, the
feedback law in fp64 on the float32 state, actions rounded to float32: what it loses against the fp64 loop is the measure of what
fp32 arithmetic costs on a case (the device's 1-ulp hardware reciprocals may lose twice that: tests/test_gpu_state_atlas.py).
"""
import numpy as np

from oracle import ref_np as R

NX, NU, H = 13, 4, 32
LADDER = 2.0 ** (3 - np.arange(1, 17))


def _stack(s, n, dtype, x0=None):
    """the state with a leading axis of n step sizes; x0 [13] replaces (pos, vel, quat, omega)"""
    s = s.astype(dtype)
    if x0 is not None:
        x0 = np.asarray(x0, dtype=dtype)
        s = s.replace(pos=x0[0:3], vel=x0[3:6], quat=x0[6:10], omega=x0[10:13])
    tile = lambda a: np.broadcast_to(np.asarray(a, dtype=dtype), (n,) + np.shape(a)).copy()
    return s.replace(pos=tile(s.pos), vel=tile(s.vel), quat=tile(s.quat), omega=tile(s.omega))


def closed_loop(s, p, b, K, kff, xbar, forces, alphas=LADDER, dtype=np.float64, x0=None):
    """s, p: the State / Params of tests.conftest.make_problem; b [128] the plan; K [H, 4, >=13], kff [H, 4], xbar [H, >=13] the
    sweep's outputs; forces [H, 3] the force step k integrates; alphas [n]; x0: an optional start state [13] (default: s's own).
    -> dict: u [n, H, 4] float64 (holding float32 numbers when dtype is float32), v [n, H, 4] the unclipped fp64 commands,
    gain [n] = max over k, i of |v_i - (alpha kff_i + b_i)|, clipped [n] = number of components with |v| > 1, bad [n] = first k with a v
    that is not finite (-1: none); gain and clipped over the stages before `bad`."""
    dtype = np.dtype(dtype)
    alphas = np.asarray(alphas, dtype=np.float64).reshape(-1)
    n = alphas.size
    b64 = np.asarray(b, dtype=np.float64).reshape(H, NU)
    K = np.asarray(K, dtype=np.float64)[:, :, :NX]
    kff = np.asarray(kff, dtype=np.float64)
    xbar = np.asarray(xbar, dtype=np.float64)[:, :NX]
    forces = np.asarray(forces, dtype=np.float64)
    p = p.fp32() if dtype == np.float32 and hasattr(p, "fp32") else p
    st = _stack(s, n, dtype, x0)
    u_all, v_all = np.zeros((n, H, NU)), np.zeros((n, H, NU))
    gain, clipped, bad = np.zeros(n), np.zeros(n, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    for k in range(H):
        x = np.concatenate([st.pos, st.vel, st.quat, st.omega], axis=-1).astype(np.float64)
        dx = x - xbar[k][None]
        v0 = alphas[:, None] * kff[k][None] + b64[k][None]
        v = v0.copy()
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(NX):
                v = v + K[k][None, :, j] * dx[:, j:j + 1]
        fin = np.isfinite(v).all(axis=1)
        bad = np.where((bad < 0) & ~fin, k, bad)
        ok = bad < 0
        with np.errstate(invalid="ignore"):
            gain = np.where(ok, np.maximum(gain, np.nan_to_num(np.abs(v - v0)).max(axis=1)), gain)
            clipped = clipped + np.where(ok, (np.abs(v) > 1.0).sum(axis=1), 0)
            u = np.where(ok[:, None], np.clip(v, -1.0, 1.0), np.clip(b64[k], -1.0, 1.0)[None])
        if dtype == np.float32:
            u = u.astype(np.float32).astype(np.float64)
        u_all[:, k], v_all[:, k] = u, v
        st = st.replace(f_disturb=np.asarray(forces[k], dtype=dtype))
        st = R.raw_step(st, u.astype(dtype), p, np.zeros(3, dtype=dtype))
    return dict(u=u_all, v=v_all, gain=gain, clipped=clipped, bad=bad)


def open_loop(b, kff, alphas=LADDER):
    """[n, H, 4] fp64: clip(b + alpha kff), unrounded -- the closed loop's K = 0 twin"""
    alphas = np.asarray(alphas, dtype=np.float64).reshape(-1)
    b64 = np.asarray(b, dtype=np.float64).reshape(1, H, NU)
    return np.clip(b64 + alphas[:, None, None] * np.asarray(kff, dtype=np.float64)[None], -1.0, 1.0)
