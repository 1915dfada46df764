"""CPU tests of the hold step's oracle (tests/plan_hold_oracle.py) on the fp64 Riccati oracle's own sweep (tests/riccati_oracle.py), the
case of tests/test_feedback_oracle.py: make_problem(seed=17, time=37), hover + 0.1 noise, no disturbance, penyaw reward.

1. the tie to the generator: fed the fp64 closed loop's own state at stage k (tests/feedback_oracle.py), the oracle returns that loop's
   u[:, k] exactly, k in {0, 1, 15, 31}, at three step sizes.
2. at rest: x = xb_j and alpha = 0 give clip(b_j), gain 0, dpos 0.
3. the three fall-backs give what the definition says, and the shift moves the controller state one stage down with u in front.
"""
import functools

import numpy as np

from oracle import ref_np as R
from tests import feedback_oracle as FO
from tests import plan_hold_oracle as PO
from tests import riccati_oracle as RO
from tests.conftest import make_problem

ALPHAS = (1.0, 0.25, 2.0 ** -13)


@functools.lru_cache(maxsize=None)
def _case():
    s, p, rng = make_problem(seed=17, time=37)
    b = (R.hover_action(p, 32, np.float64) + 0.1 * rng.normal(size=(32, 4))).astype(np.float32).reshape(-1)
    forces = RO.step_forces(s, p, "none")
    blk = RO.stage_blocks(s, p, b.astype(np.float64), "penyaw", forces)
    rung, mu, r = RO.ladder(blk)
    return s, p, b, forces, blk, r


def _loop_states(s, p, u, forces):
    """the states x_k [n, H, 13] the fp64 closed loop passed through, from its own actions u [n, H, 4] (feedback_oracle.closed_loop's
    plant stepping, restated: the same calls on the same numbers)"""
    n = u.shape[0]
    st = FO._stack(s, n, np.float64)
    xs = np.zeros((n, PO.H, PO.NX))
    for k in range(PO.H):
        xs[:, k] = np.concatenate([st.pos, st.vel, st.quat, st.omega], axis=-1)
        st = st.replace(f_disturb=np.asarray(forces[k], dtype=np.float64))
        st = R.raw_step(st, u[:, k].astype(np.float64), p, np.zeros(3))
    return xs


def test_the_oracle_is_one_stage_of_the_generators_loop():
    s, p, b, forces, blk, r = _case()
    loop = FO.closed_loop(s, p, b, r["K"], r["kff"], blk["x"], forces, alphas=ALPHAS)
    xs = _loop_states(s, p, loop["u"], forces)
    assert np.all(loop["bad"] == -1)
    for a, alpha in enumerate(ALPHAS):
        for k in (0, 1, 15, 31):
            got = PO.hold_step(xs[a, k], b, r["K"], r["kff"], blk["x"], alpha, k, dtype=np.float64)
            assert got["u"].tobytes() == loop["u"][a, k].tobytes(), (alpha, k)
            assert got["v"].tobytes() == loop["v"][a, k].tobytes(), (alpha, k)
            assert got["flags"] == 0 and got["age"] == k
    # the feedback term is live on this case: ignoring K could not pass
    apart = np.abs(loop["u"] - FO.open_loop(b, r["kff"], ALPHAS).reshape(3, 32, 4)).max()
    print(f"  max |closed - open| over the three step sizes: {apart:.3e}")
    assert apart >= 1e-4


def test_at_rest_the_hold_step_returns_the_plan():
    s, p, b, forces, blk, r = _case()
    want = np.clip(b.astype(np.float64), -1.0, 1.0).reshape(32, 4)
    for j in (0, 1, 15, 31):
        got = PO.hold_step(blk["x"][j], b, r["K"], r["kff"], blk["x"], 0.0, j, dtype=np.float64)
        assert got["u"].tobytes() == want[j].tobytes() and got["gain"] == 0.0 and got["dpos"] == 0.0 and got["flags"] == 0


def test_fall_backs_and_the_shift():
    s, p, b, forces, blk, r = _case()
    j = 5
    x = blk["x"][j] + 0.05
    plan = np.clip(b.reshape(32, 4)[j], -1.0, 1.0).astype(np.float64)
    base = PO.hold_step(x, b, r["K"], r["kff"], blk["x"], 0.5, j, time=42, t_plan=37)
    assert base["flags"] == 0 and base["gain"] > 1e-4 and base["time"] == 42
    # 1: a flagged sweep, whatever gains it left (zeros when no rung was positive definite)
    for K, kff in ((r["K"], r["kff"]), (np.zeros_like(r["K"]), np.zeros_like(r["kff"]))):
        got = PO.hold_step(x, b, K, kff, blk["x"], 0.5, j, flagged=True)
        assert got["flags"] == PO.FLAG_SWEEP and got["u"].tobytes() == plan.tobytes() and got["gain"] == 0.0
    # 2: a command that is not finite -- all four components fall back
    xn = x.copy()
    xn[1] = np.nan
    got = PO.hold_step(xn, b, r["K"], r["kff"], blk["x"], 0.5, j)
    assert got["flags"] == PO.FLAG_NOT_FINITE and got["u"].tobytes() == plan.tobytes() and got["gain"] == 0.0
    # 3: the state's time is not the plan's + j -- the feedback term is dropped, the feed-forward term stays
    got = PO.hold_step(x, b, r["K"], r["kff"], blk["x"], 0.5, j, time=0, t_plan=37)
    v0 = 0.5 * r["kff"][j] + b.reshape(32, 4)[j].astype(np.float64)
    assert got["flags"] == PO.FLAG_TIME and got["gain"] == 0.0
    assert got["u"].tobytes() == np.clip(v0, -1, 1).astype(np.float32).astype(np.float64).tobytes()
    assert np.abs(got["u"] - base["u"]).max() > 1e-5
    # the clipped count follows the applied command
    big = PO.hold_step(x, 5.0 * b, r["K"], r["kff"], blk["x"], 0.0, j)
    assert big["clipped"] == int((np.abs(big["v"]) > 1.0).sum()) >= 1 and np.all(np.abs(big["u"]) <= 1.0)
    # the shift
    mean = np.arange(128, dtype=np.float32)
    cov = (np.arange(32, dtype=np.float32)[:, None, None] + np.eye(4, dtype=np.float32)[None])
    m2, c2 = PO.shift(mean, base["u"], cov)
    assert m2.dtype == np.float32 and np.array_equal(m2[:4], base["u"].astype(np.float32))
    assert np.array_equal(m2[4:124], mean[8:]) and np.array_equal(m2[124:], mean[124:])
    assert np.array_equal(c2[:31], cov[1:]) and np.array_equal(c2[31], cov[31])
