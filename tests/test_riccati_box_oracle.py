"""CPU: the fp64 oracle of the box form of the Riccati sweep (tests/riccati_box_oracle.py) against itself.

1. the box QP by enumeration against an independent method -- projected Gauss-Seidel run to its fixed point -- on 200 random positive
   definite 4 x 4 problems, to 1e-12, with the KKT conditions checked on the result;
2. sweep_box with bounds +-inf is RO.sweep;
3. the named inputs the GPU tests are held on (riccati_box_oracle.named_case) show what those tests need, by the oracle alone and under
   ladder_box: A >= 3 clamped coordinates, a stage with a lower and an upper clamp together, margin >= 1e-3; B >= 3 clamped
   coordinates, margin >= 1e-3; C no clamp, margin >= 0.1.  Measured: A rung 4, 4 clamps, margin 2.6e-2; B rung 6 (the unconstrained
   ladder: 7), 48 clamps, margin 2.2e-2; C (double_cover) rung 4, margin 0.18.
"""
import functools

import numpy as np
import pytest

from tests import riccati_box_oracle as BO
from tests import riccati_oracle as RO


def projected_gauss_seidel(Q, q, lo, hi, sweeps=20000):
    """argmin 1/2 k^T Q k + q^T k on [lo, hi] by exact coordinate minimisation, clipped, until a sweep moves nothing"""
    k = np.clip(np.zeros(4), lo, hi)
    for _ in range(sweeps):
        moved = 0.0
        for i in range(4):
            new = min(max(-(q[i] + Q[i] @ k - Q[i, i] * k[i]) / Q[i, i], lo[i]), hi[i])
            moved = max(moved, abs(new - k[i]))
            k[i] = new
        if moved == 0.0:
            break
    return k


def test_enumeration_against_projected_gauss_seidel():
    rng = np.random.default_rng(2014)
    sets, worst = set(), 0.0
    for n in range(200):
        M = rng.normal(size=(4, 4))
        Q = M @ M.T + 0.5 * np.eye(4)
        q = 3.0 * rng.normal(size=4)
        bc = rng.uniform(-1.0, 1.0, size=4)
        lo, hi = -1.0 - bc, 1.0 - bc
        k, t, margin = BO.box_qp(Q, q, lo, hi)
        ref = projected_gauss_seidel(Q, q, lo, hi)
        worst = max(worst, np.abs(k - ref).max())
        assert np.abs(k - ref).max() <= 1e-12, (n, k, ref)
        # KKT: feasible; a clamped coordinate is the bound itself and its multiplier points outward; a free one is stationary
        m = Q @ k + q
        assert np.all(k >= lo) and np.all(k <= hi), n
        for i, ti in enumerate(t):
            if ti == BO.FREE:
                assert abs(m[i]) <= 1e-12 * max(1.0, np.abs(q).max()), (n, i, m)
            elif ti == BO.AT_LO:
                assert k[i] == lo[i] and m[i] > 0.0, (n, i)
            else:
                assert k[i] == hi[i] and m[i] < 0.0, (n, i)
        assert margin > 0.0
        sets.add(t)
    print(f"200 problems, {len(sets)} different active sets, worst |k - k_pgs| {worst:.2e}")
    assert len(sets) >= 20 and (BO.FREE,) * 4 in sets  # the enumeration was exercised, the all-free set included


@functools.lru_cache(maxsize=None)
def _case(name):
    s, p, b, reg0 = BO.named_case(name)
    blk = RO.stage_blocks(s, p, b.astype(np.float64), "penyaw", RO.step_forces(s, p, "none"))
    return b, reg0, blk


def test_sweep_box_without_bounds_is_the_sweep():
    b, reg0, blk = _case("A")
    inf = np.full((RO.H, RO.NU), np.inf)
    for mu in (2.56, 10.24):
        want = RO.sweep(blk, mu)
        got = BO.sweep_box(blk, mu, b, lo=-inf, hi=inf)
        assert want["ok"] and got["ok"] and not got["masks"].any()
        assert np.allclose(got["pivots"], want["pivots"], rtol=1e-10, atol=0.0)
        for name in ("K", "kff", "d", "dx"):
            err = np.abs(got[name] - want[name]).max()
            assert err <= 1e-12 * max(1.0, np.abs(want[name]).max()), (mu, name, err)
    # a rung the unconstrained sweep fails fails here at the same pivot
    bad, got = RO.sweep(blk, 1e-2), BO.sweep_box(blk, 1e-2, b, lo=-inf, hi=inf)
    assert not bad["ok"] and not got["ok"] and len(got["pivots"]) == len(bad["pivots"])


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_named_inputs_show_what_the_gpu_tests_need(name):
    b, reg0, blk = _case(name)
    assert np.abs(b).max() < 1.0  # the hover plan: the bounds are +-1 - b, none degenerate
    j, mu, r = BO.ladder_box(blk, b, reg0)
    ju, muu, ru = RO.ladder(blk, reg0)
    assert j < RO.RUNGS and mu == reg0 * 4.0 ** j
    n, margin = BO.clamp_count(r["masks"]), r["margin"].min()
    lo, hi = BO.bounds(b)
    print(f"case {name}: box rung {j} (unconstrained {ju}), {n} clamped coordinates at stages {np.flatnonzero(r['masks']).tolist()}, "
          f"margin {margin:.3e}, unconstrained max |b + k| {np.abs(b.reshape(32, 4) + ru['kff']).max():.3f}, "
          f"g.d {blk['g'] @ ru['d']:.2f} -> {blk['g'] @ r['d']:.2f}")
    assert np.all(r["kff"] >= lo) and np.all(r["kff"] <= hi)
    assert np.all(np.abs(np.clip(b.astype(np.float64), -1, 1).reshape(32, 4) + r["kff"]) <= 1.0)
    assert blk["g"] @ r["d"] < 0.0
    if name == "C":
        assert n == 0 and margin >= 0.1, (n, margin)
        assert j == ju and np.array_equal(r["d"], ru["d"]) or np.abs(r["d"] - ru["d"]).max() <= 1e-12 * np.abs(ru["d"]).max()
        return
    assert n >= 3 and margin >= 1e-3, (n, margin)
    assert np.abs(b.reshape(32, 4) + ru["kff"]).max() > 1.0  # the unconstrained step of the same inputs leaves the box
    for k in np.flatnonzero(r["masks"]):  # clamped: the bound itself, a zero row of K
        for i, ti in enumerate(r["sets"][k]):
            if ti != BO.FREE:
                assert r["kff"][k, i] == (lo if ti == BO.AT_LO else hi)[k, i] and not r["K"][k, i].any()
    if name == "A":
        both = [k for k in range(32) if (r["masks"][k] & 0x0F) and (r["masks"][k] & 0xF0)]
        assert both, r["masks"]
