"""CPU tests of the closed-loop generator's oracle (tests/feedback_oracle.py) on the fp64 Riccati oracle's own sweep
(tests/riccati_oracle.py): make_problem(seed=17, time=37), hover + 0.1 noise, no disturbance, penyaw reward -- rung 4 (mu = 2.56),
|K|max about 1.04, no component saturates for alpha <= 1.

1. K = 0 reduces the closed loop to the open-loop candidates riccati_oracle.candidates(b, kff)[1:], bit for bit.
2. it is the DDP / iLQR forward pass and nothing else: closed(alpha) - open(alpha) is the second-order remainder of the plant along
   the step, so it is there at alpha = 1 (>= 1e-3) and falls by a factor in [3, 5] per halving of alpha from 1/2 to 2^-3.
3. the bookkeeping: a start state off the nominal one moves the first action by K_0 dx_0 at alpha = 0; a NaN gain invalidates the
   sequence from its stage on and leaves clip(b) there.
"""
import functools

import numpy as np

from oracle import ref_np as R
from tests import feedback_oracle as FO
from tests import riccati_oracle as RO
from tests.conftest import make_problem


@functools.lru_cache(maxsize=None)
def _case():
    s, p, rng = make_problem(seed=17, time=37)
    b = (R.hover_action(p, 32, np.float64) + 0.1 * rng.normal(size=(32, 4))).astype(np.float32).reshape(-1)
    forces = RO.step_forces(s, p, "none")
    blk = RO.stage_blocks(s, p, b.astype(np.float64), "penyaw", forces)
    rung, mu, r = RO.ladder(blk)
    return s, p, b, forces, blk, rung, mu, r


def test_the_case_is_the_probed_one():
    s, p, b, forces, blk, rung, mu, r = _case()
    print(f"  rung {rung} mu {mu} |K|max {np.abs(r['K']).max():.4f} |kff|max {np.abs(r['kff']).max():.4f}")
    assert rung == 4 and mu == 2.56
    assert 0.5 < np.abs(r["K"]).max() < 2.0
    v = FO.closed_loop(s, p, b, r["K"], r["kff"], blk["x"], forces, alphas=[1.0, 0.5, 0.25, 0.125])["v"]
    assert np.abs(v).max() < 1.0  # no component saturates for alpha <= 1: the differences below are the plant's, not the clip's


def test_zero_gains_are_the_open_loop_candidates_bit_for_bit():
    s, p, b, forces, blk, rung, mu, r = _case()
    want = RO.candidates(b, r["kff"].reshape(-1))[1:]
    got = FO.closed_loop(s, p, b, np.zeros_like(r["K"]), r["kff"], blk["x"], forces, dtype=np.float32)
    assert got["u"].reshape(16, 128).tobytes() == want.tobytes()
    assert not got["gain"].any() and np.all(got["bad"] == -1)
    # ... from any start state: with K = 0 the state never enters
    x0 = np.concatenate([s.pos + 0.05, s.vel + 0.1, s.quat, s.omega])
    moved = FO.closed_loop(s, p, b, np.zeros_like(r["K"]), r["kff"], blk["x"], forces, dtype=np.float32, x0=x0)
    assert moved["u"].tobytes() == got["u"].tobytes()


def test_second_order_agreement_with_the_open_loop_step():
    s, p, b, forces, blk, rung, mu, r = _case()
    alphas = [1.0, 0.5, 0.25, 0.125]
    closed = FO.closed_loop(s, p, b, r["K"], r["kff"], blk["x"], forces, alphas=alphas)["u"]
    # the open-loop step of the line search: d = the linear forward pass, which is what riccati_oracle.sweep returns
    opened = np.clip(b.astype(np.float64)[None] + np.asarray(alphas)[:, None] * r["d"][None], -1.0, 1.0).reshape(4, 32, 4)
    diff = np.abs(closed - opened).reshape(4, -1).max(axis=1)
    ratios = diff[:-1] / diff[1:]
    print(f"  max |closed - open| at alpha = 1, 1/2, 1/4, 1/8: {diff}; ratios {ratios}")
    assert diff[0] >= 1e-3
    assert np.all((ratios >= 3.0) & (ratios <= 5.0)), ratios  # (the halvings from 1/2 to 2^-3, and the one from 1 too)
    # alpha = 0 from the nominal start: dx = 0 at every stage, the plan itself
    zero = FO.closed_loop(s, p, b, r["K"], r["kff"], blk["x"], forces, alphas=[0.0])
    assert np.abs(zero["u"].reshape(-1) - np.clip(b.astype(np.float64), -1, 1)).max() <= 1e-12 and zero["gain"][0] <= 1e-12


def test_start_state_and_invalid_gains():
    s, p, b, forces, blk, rung, mu, r = _case()
    x0 = np.concatenate([s.pos + 0.05, s.vel + 0.1, s.quat, s.omega])
    moved = FO.closed_loop(s, p, b, r["K"], r["kff"], blk["x"], forces, alphas=[0.0], x0=x0)
    want0 = b.astype(np.float64)[:4] + r["K"][0] @ (x0 - blk["x"][0])
    assert np.abs(moved["v"][0, 0] - want0).max() <= 1e-12
    assert moved["gain"][0] >= np.abs(r["K"][0] @ (x0 - blk["x"][0])).max() - 1e-12
    Kn = r["K"].copy()
    Kn[5, 2, 3] = np.nan
    badrun = FO.closed_loop(s, p, b, Kn, r["kff"], blk["x"], forces)
    good = FO.closed_loop(s, p, b, r["K"], r["kff"], blk["x"], forces)
    assert np.all(badrun["bad"] == 5)
    assert badrun["u"][:, :5].tobytes() == good["u"][:, :5].tobytes()
    assert np.all(badrun["u"][:, 5:] == np.clip(b.astype(np.float64), -1, 1).reshape(32, 4)[None, 5:])
    assert np.isfinite(badrun["u"]).all() and np.isfinite(badrun["gain"]).all()
