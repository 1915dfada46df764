"""Oracle of the hold step (csrc/plan_hold.hip), a plain helper module like tests/feedback_oracle.py: one stage of the generator's law
in numpy fp64 on the measured state, the three fall-backs, and the shift of the controller state.

    dx   = (double)x - xb_j                                      (13 raw coordinates: pos, vel, quat, omega)
    v0_i = alpha kff_j[i] + b_j[i];  v_i = v0_i, v_i += K_j[i][c] dx_c, c ascending      (fp64, unfused)
    u    = clip(v, -1, 1)                                         (rounded to float32 when dtype is float32)
flags, in the kernel's order of precedence:
    1  the sweep is flagged (`flagged`: its side row says so): u = clip(b_j)
    2  (bit 0 clear) a component of the command that is not finite: u = clip(b_j)
    4  t_plan is given and the state's time is not t_plan + j: the feedback term is dropped, the command is v0
row: age j, alpha, gain = max |v - v0| (0 when the feedback term is not applied), clipped = number of components whose applied
command (v, v0 or b_j) exceeds 1 in magnitude, flags, dpos = |dx_pos|_2, time.
"""
import numpy as np

NX, NU, H = 13, 4, 32
FLAG_SWEEP, FLAG_NOT_FINITE, FLAG_TIME = 1, 2, 4


def hold_step(x, b, K, kff, xbar, alpha, stage, time=0, t_plan=None, flagged=False, dtype=np.float32):
    """x [>= 13]: the measured state's (pos, vel, quat, omega); b [128] the latched mean; K [H, 4, >= 13], kff [H, 4], xbar [H, >= 13]
    the sweep's outputs; alpha: the committed step size; stage j; time: the state's time word; t_plan: the latched time or None.
    -> dict: u [4] float64 (holding float32 numbers when dtype is float32), v, v0 [4] fp64, and the row's entries."""
    j = int(stage)
    x = np.asarray(x, dtype=np.float64)[:NX]
    bj32 = np.asarray(b, dtype=np.float32).reshape(H, NU)[j]
    bj = bj32.astype(np.float64)
    Kj = np.asarray(K, dtype=np.float64)[j, :, :NX]
    kj = np.asarray(kff, dtype=np.float64)[j]
    dx = x - np.asarray(xbar, dtype=np.float64)[j, :NX]
    v0 = float(alpha) * kj + bj
    v = v0.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(NX):
            v = v + Kj[:, c] * dx[c]
    sweep = bool(flagged)
    mismatch = t_plan is not None and int(time) != int(t_plan) + j
    cmd = v0 if mismatch else v
    fin = bool(np.isfinite(cmd).all())
    plan_only = sweep or not fin
    applied = bj if plan_only else cmd
    u = np.clip(applied, -1.0, 1.0)
    if np.dtype(dtype) == np.float32:
        u = u.astype(np.float32).astype(np.float64)
    flags = (FLAG_SWEEP if sweep else 0) | (FLAG_NOT_FINITE if (not sweep and not fin) else 0) | (FLAG_TIME if mismatch else 0)
    gain = 0.0 if (plan_only or mismatch) else float(np.abs(v - v0).max())
    with np.errstate(invalid="ignore"):
        clipped = int((np.abs(applied) > 1.0).sum())
        dpos = float(np.sqrt((dx[:3] ** 2).sum()))
    return dict(u=u, v=v, v0=v0, age=j, alpha=float(alpha), gain=gain, clipped=clipped, flags=flags, dpos=dpos, time=int(time))


def shift(a_mean, u, a_cov=None):
    """What a hold step leaves of the controller state: a_mean [128] -> [a_mean[1:], a_mean[31]] with u in front; a_cov [H, 4, 4]
    (MPPI) -> [a_cov[1:], a_cov[31]].  Copies, dtype kept."""
    m = np.asarray(a_mean).reshape(H, NU)
    out = np.concatenate([m[1:], m[-1:]], axis=0)
    out[0] = np.asarray(u, dtype=out.dtype)
    if a_cov is None:
        return out.reshape(-1)
    c = np.asarray(a_cov).reshape(H, NU, NU)
    return out.reshape(-1), np.concatenate([c[1:], c[-1:]], axis=0)
