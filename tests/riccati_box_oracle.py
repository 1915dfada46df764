"""fp64 oracle of the box form of the Riccati sweep (csrc/riccati.hip, BOX; covo_riccati_box), a plain helper module next to
tests/riccati_oracle.py, whose stage blocks, Cholesky and forward pass it uses.

At stage k of rung mu, with bc = clip(b_k, -1, 1), lo = -1 - bc, hi = 1 - bc (an entry of the plan that is not finite: lo = hi = 0):
    k_k = argmin 1/2 du^T Quu du + Qu^T du   on   lo <= du <= hi               (Quu includes mu I)
Coordinate i is CLAMPED when k_k[i] sits on a bound and the multiplier (Quu k_k + Qu)[i] pushes strictly outward (> 0 at lo, < 0 at hi);
every other coordinate is FREE.  k_k[i] is the bound itself on the clamped set c, K_k[c] = 0, and on the free set f
    k_f = -Quu_ff^-1 (Qu_f + Quu_fc k_c),   K_k[f] = -Quu_ff^-1 Qux_f.
The recurrences of P and p are RO.sweep's.  The rung is judged by the unpivoted Cholesky of the FULL Quu, as there.
"""
import itertools

import numpy as np

from tests import riccati_oracle as RO

NX, NU, H, RUNGS = RO.NX, RO.NU, RO.H, RO.RUNGS
FREE, AT_LO, AT_HI = 0, 1, 2
PATTERNS = tuple(tuple(reversed(t)) for t in itertools.product((FREE, AT_LO, AT_HI), repeat=NU))  # index = sum_i t_i 3^i


def mask_word(t):
    """the device's word of a pattern: bits 0-3 coordinate i clamped at lo, bits 4-7 at hi"""
    return sum((1 << i) if ti == AT_LO else (16 << i) if ti == AT_HI else 0 for i, ti in enumerate(t))


def solve_pattern(Q, q, lo, hi, t):
    """the stationary point of the QP with the coordinates t names held at their bounds -> (k, multipliers Q k + q)"""
    t = np.asarray(t)
    c, f = t != FREE, t == FREE
    k = np.where(t == AT_LO, lo, hi).astype(np.float64)
    k[f] = 0.0
    if f.any():
        k[f] = -np.linalg.solve(Q[np.ix_(f, f)], q[f] + Q[np.ix_(f, c)] @ k[c])
    return k, Q @ k + q


def box_qp(Q, q, lo, hi):
    """The box QP by enumeration of the 3^4 = 81 active sets -> (k, t, margin): the lowest pattern whose free coordinates are feasible
    and whose clamped coordinates' multipliers point strictly outward (Q positive definite: exactly one pattern does, up to ties of a
    multiplier that is exactly 0, which the definition calls free); margin = the smallest distance of a free coordinate to its
    bounds and the smallest |multiplier| of a clamped one"""
    for t in PATTERNS:
        k, m = solve_pattern(Q, q, lo, hi, t)
        ok, margin = True, np.inf
        for i, ti in enumerate(t):
            if ti == FREE:
                ok = ok and lo[i] <= k[i] <= hi[i]
                margin = min(margin, k[i] - lo[i], hi[i] - k[i])
            else:
                ok = ok and (m[i] > 0.0 if ti == AT_LO else m[i] < 0.0)
                margin = min(margin, abs(m[i]))
        if ok:
            return k, t, margin
    raise ArithmeticError("box_qp: no active set satisfies the KKT conditions (Q not positive definite?)")


def bounds(b):
    """(lo, hi) [H, 4] of the plan b [128]"""
    b = np.asarray(b, dtype=np.float64).reshape(H, NU)
    fin = np.isfinite(b)
    bc = np.clip(np.where(fin, b, 0.0), -1.0, 1.0)
    return np.where(fin, -1.0 - bc, 0.0), np.where(fin, 1.0 - bc, 0.0)


def sweep_box(blk, mu, b, lo=None, hi=None):
    """RO.sweep with the box QP at every stage -> its dict plus masks [H] (the device's words), sets [H] (the patterns) and margin [H].
    lo / hi [H, 4]: the bounds, default bounds(b) (+-inf: the unconstrained sweep)"""
    A, B = blk["A"], blk["B"]
    if lo is None:
        lo, hi = bounds(b)
    P, pv = np.zeros((NX, NX)), np.zeros(NX)
    K, kff = np.zeros((H, NU, NX)), np.zeros((H, NU))
    masks, sets, margin = np.zeros(H, dtype=np.int32), [None] * H, np.full(H, np.inf)
    pivots = []
    for k in range(H - 1, -1, -1):
        Ak, Bk = (A[k], B[k]) if k < H - 1 else (np.zeros((NX, NX)), np.zeros((NX, NU)))
        Qxx = blk["Mxx"][k] + Ak.T @ P @ Ak
        Qux = blk["Mxu"][k].T + Bk.T @ P @ Ak
        Quu = blk["Muu"][k] + Bk.T @ P @ Bk + mu * np.eye(NU)
        Qu = blk["g"][4 * k:4 * k + 4] + Bk.T @ pv
        L, piv = RO._chol4(Quu)
        pivots += piv
        if L is None:
            return dict(ok=False, pivots=pivots)
        kff[k], t, margin[k] = box_qp(Quu, Qu, lo[k], hi[k])
        f = np.asarray(t) == FREE
        if f.any():
            K[k][f] = -np.linalg.solve(Quu[np.ix_(f, f)], Qux[f])
        masks[k], sets[k] = mask_word(t), t
        P = Qxx + Qux.T @ K[k]
        P = 0.5 * (P + P.T)
        pv = Ak.T @ pv + Qux.T @ kff[k]
    d, dx = RO.forward(A, B, K, kff)
    return dict(ok=True, pivots=pivots, K=K, kff=kff, d=d, dx=dx, masks=masks, sets=sets, margin=margin)


def ladder_box(blk, b, reg0=1e-2):
    """(rung, mu, sweep_box result) of the lowest rung mu_j = reg0 4^j, j < 8, whose box sweep succeeds; (8, 0.0, None) when none does"""
    for j in range(RUNGS):
        mu = reg0 * 4.0 ** j
        r = sweep_box(blk, mu, b)
        if r["ok"]:
            return j, mu, r
    return RUNGS, 0.0, None


def clamp_count(masks):
    return int(sum(bin(int(m) & 0xFF).count("1") for m in np.asarray(masks).reshape(-1)))


def named_case(name):
    """The inputs the box tests are held on -> (s, p, b float32 [128], reg0), each with the hover plan: A yaw_quarter (4 clamped
    coordinates at stages 0-2, stage 0 with a lower and an upper clamp, rung 4 like the unconstrained ladder), B make_problem(17, 37)
    at reg0 = 1e-4 (48 clamped coordinates; the box ladder wins at rung 6, the unconstrained one at 7), C double_cover (no clamp,
    margin 0.18).  far_fast does not serve as the no-clamp case: its box ladder wins at rung 3, two rungs below the unconstrained
    one -- with clamped rows of K zero the pivots pass earlier -- and there 58 coordinates are clamped at a margin of 1.1e-3"""
    from oracle import ref_np as R
    from tests.conftest import make_problem
    from tests.state_atlas import atlas_state
    if name == "A":
        s, p, _ = atlas_state("yaw_quarter")
        reg0 = 1e-2
    elif name == "B":
        s, p, _ = make_problem(seed=17, time=37)
        reg0 = 1e-4
    elif name == "C":
        s, p, _ = atlas_state("double_cover")
        reg0 = 1e-2
    else:
        raise KeyError(name)
    b = R.hover_action(p, 32, np.float64).astype(np.float32).reshape(-1)
    return s, p, b, reg0
