"""CPU: tests/force_observer_oracle.py (the definition the force observer's kernel is held to) against hand-checkable
cases, the open-loop experiment of the issue, and its own np.longdouble re-run (the fp64 loss the GPU test's bar is built from)."""
import functools

import numpy as np

from tests import estimator_oracle as EO
from tests import force_observer_oracle as FO
from tests.conftest import make_problem
from tests.state_atlas import atlas_state

SEEDS = (0, 1, 2)
OBS = tuple(0.05 * FO.OBS_GROUP_SCALE)
STARTS = ("make_problem", "yaw_pi_minus", "inverted", "unnorm_q", "far_fast")
MASSES = (0.027, 0.021, 0.034)


def start():
    s, p, _ = make_problem()
    x = np.concatenate([s.pos, s.vel, s.quat, s.omega])
    hover = np.array([float(p.m) * float(p.g) / float(p.max_thrust) * 2.0 - 1.0, 0.0, 0.0, 0.0], dtype=np.float32)
    return s, p, x, hover


@functools.lru_cache(maxsize=None)
def experiment(plant, seed):
    s, p, _ = make_problem()
    return FO.open_loop(s, p, seed, plant=plant, n_steps=200)


def test_first_call_takes_the_measurement_zeroes_the_force_and_never_reads_the_force_slots():
    s, p, x, hover = start()
    a, b = FO.Filter(p), FO.Filter(p)
    row = FO.pack_row(x.astype(np.float32), [0.3, -0.2, 0.1], int(s.time))
    row[16:25] = np.arange(9)
    out, side = a.call(row, hover)
    want = row.copy()
    want[13:16] = 0
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(a.xi, np.concatenate([row[:13].astype(np.float64), np.zeros(3)])) and np.array_equal(a.P, np.diag(a.P0))
    assert side[0] == FO.FLAG_INIT and side[7] == int(s.time) and side[1] == 0 and side[3] == 0 and side[6] == 0
    R, Q, P0 = FO.constants(p)
    assert np.allclose(np.sqrt(R[[0, 3, 6, 10]]), 0.05 * np.array([0.25, 0.5, 0.02, 0.5]), rtol=1e-15)
    assert not Q[:13].any() and np.allclose(np.sqrt(Q[13:]), float(p.dyn_noise_scale), rtol=1e-15)
    assert np.allclose(np.sqrt(P0[13:]), float(p.disturb_scale) / np.sqrt(3.0), rtol=1e-15) and np.array_equal(P0[:13], R)
    # two filters fed rows that differ in the force slots alone stay equal bit for bit
    b.call(FO.pack_row(x.astype(np.float32), np.zeros(3), int(s.time)), hover)
    r2 = FO.pack_row(x.astype(np.float32), [9.0, 9.0, 9.0], int(s.time) + 1)
    o1, s1 = a.call(r2, hover)
    o2, s2 = b.call(FO.pack_row(x.astype(np.float32), [-1.0, 0.0, 5.0], int(s.time) + 1), hover)
    assert np.array_equal(o1[:16].view(np.uint32), o2[:16].view(np.uint32)) and np.array_equal(s1, s2) and np.array_equal(a.P, b.P)


def test_a_constant_force_at_hover_is_found_from_noise_free_measurements():
    """Hover, 0.05 N along x, measurements without noise: |f^ - f| decreases monotonically and is below 1 % of |f| after 30 steps.

    The issue leaves the filter's constants of this case open.  The truth is a constant force, a random walk of step 0, so the case
    that can be checked by hand is force_walk_std = 0 (the filter is then recursive least squares for a constant): monotone,
    |f^ - f| / |f| = 1.46e-1, 4.10e-2, 1.68e-2 at calls 1 .. 3 and 3.4e-5 at call 30.  At the DEFAULT walk of 0.05 N per step -- as
    large as the force itself -- the gain stays high and the error is NOT monotone: 1.46e-1, 7.78e-3, 1.42e-2 at calls 1 .. 3 (it
    rises at call 3), 2.85e-3 at call 5, 4.1e-6 at call 30, and from call 12 on it wanders at the 1e-5 level the fp32 rounding of the
    measured row sets.  A three-state linear Kalman filter (p, v, f) with the same constants gives 7.29e-3, 3.89e-4, 7.12e-4 N at
    calls 1 .. 3, the same figures, so this is the defined filter and not its arithmetic.  The default is printed and held to the
    1 % bound only."""
    s, p, x, hover = start()
    x = np.concatenate([np.zeros(3), np.zeros(3), [0.0, 0.0, 0.0, 1.0], np.zeros(3)])
    force = np.array([0.05, 0.0, 0.0])
    for walk in (0.0, None):
        f = FO.Filter(p, force_walk_std=walk)
        xi = np.concatenate([x, force])
        errs = []
        for k in range(31):
            out, side = f.call(FO.pack_row(xi[:13].astype(np.float32), force, int(s.time) + k), hover)
            assert side[0] == (FO.FLAG_INIT if k == 0 else 0)
            errs.append(float(np.linalg.norm(f.force - force)))
            xi = f.f(xi, hover.astype(np.float64))[0]
        rises = [k + 1 for k, (a, b) in enumerate(zip(errs, errs[1:])) if not b < a]
        print(f"  force_walk_std={walk}: |f^ - f| / |f| at calls 0, 1, 2, 3, 5, 10, 20, 30:",
              " ".join(f"{errs[k] / 0.05:.2e}" for k in (0, 1, 2, 3, 5, 10, 20, 30)), "; calls where it rose:", rises)
        if walk == 0.0:
            assert not rises, errs
        assert errs[30] < 0.01 * 0.05, errs[30]


def test_without_a_force_state_the_kinematic_block_is_the_state_estimators():
    """force_init_std = force_walk_std = 0: f^ stays exactly 0, and x^ and P[0:13, 0:13] equal tests/estimator_oracle.py's on rows whose
    force slots are 0 with the same proc_std -- one algebra in two codes, to 1e-13 relative."""
    s, p, x, hover = start()
    rng = np.random.default_rng(3)
    proc = (0.0, 0.02, 0.0, 0.0)
    a = FO.Filter(p, proc_std=proc, force_walk_std=0.0, force_init_std=0.0)
    b = EO.Filter(p, proc_std=proc)
    u = hover
    for k in range(12):
        row = FO.pack_row(FO.measure(rng, x, OBS), np.zeros(3), int(s.time) + k)
        oa, sa = a.call(row, u)
        ob, sb = b.call(row, u)
        assert sa[0] == sb[0] == (1 if k == 0 else 0)
        assert not a.force.any() and not a.P[13:, :].any() and not a.P[:, 13:].any(), k
        ex = max(np.abs(a.x[FO.GROUP == g] - b.x[FO.GROUP == g]).max() / np.abs(b.x[FO.GROUP == g]).max() for g in range(4))
        d = np.sqrt(np.diag(b.P))
        eP = (np.abs(a.P[:13, :13] - b.P) / np.outer(d, d)).max()
        assert ex <= 1e-13 and eP <= 1e-13, (k, ex, eP)
        x = b.f(x, np.clip(u.astype(np.float64), -1, 1), np.zeros(3))[0]
        u = (hover + 0.2 * rng.normal(size=4)).astype(np.float32)


def test_fall_backs_of_the_oracle():
    s, p, x, hover = start()
    rng = np.random.default_rng(6)
    f = FO.Filter(p)
    t = int(s.time)
    for k in range(3):
        f.call(FO.pack_row(FO.measure(rng, x, OBS), np.ones(3), t + k), hover)
    row = FO.pack_row(FO.measure(rng, x, OBS), np.ones(3), t + 4)  # (t + 3 was due)
    out, side = f.call(row, hover)
    want = row.copy()
    want[13:16] = 0
    assert side[0] == FO.FLAG_TIME and np.array_equal(out.view(np.uint32), want.view(np.uint32)) and f.t_prev == t + 4
    assert np.array_equal(f.x, row[:13].astype(np.float64)) and not f.force.any() and np.array_equal(f.P, np.diag(f.P0))
    bad = FO.pack_row(FO.measure(rng, x, OBS), np.ones(3), t + 5)
    bad[4] = np.nan
    out, side = f.call(bad, hover)
    assert side[0] == FO.FLAG_NONFINITE and not f.valid and np.array_equal(out.view(np.uint32), bad.view(np.uint32))
    out, side = f.call(FO.pack_row(FO.measure(rng, x, OBS), np.ones(3), t + 6), hover)
    assert side[0] == FO.FLAG_INIT and f.valid
    f.P[2, 14] = np.nan
    row = FO.pack_row(FO.measure(rng, x, OBS), np.ones(3), t + 7)
    out, side = f.call(row, hover)
    want = row.copy()
    want[13:16] = 0
    assert side[0] == FO.FLAG_FAILED and np.array_equal(out.view(np.uint32), want.view(np.uint32)) and np.array_equal(f.P, np.diag(f.P0))


def test_open_loop_a_held_force_is_observed_a_white_one_is_not():
    """200 steps, three seeds.  periodic (0.2 N, held 50 steps): the estimate's error against the next row's force is below the
    force's own RMS.  gaussian (redrawn every step): printed only -- a random walk cannot predict white noise, the ratio is above 1."""
    ratios = {}
    for plant in ("periodic", "gaussian"):
        for seed in SEEDS:
            forces, est, sides = experiment(plant, seed)
            assert (sides[1:, 0] == 0).all(), (plant, seed)
            r = FO.force_ratio(forces, est)
            same = float(np.sqrt(((est[20:] - forces[20:]) ** 2).sum(axis=1).mean()) / np.sqrt((forces[20:] ** 2).sum(axis=1).mean()))
            ratios[(plant, seed)] = r
            print(f"  {plant} seed {seed}: rms |f^_t - f_t+1| / rms |f_t+1| = {r:.3f} (against the row's own force: {same:.3f}); "
                  f"mean nis {sides[20:, 1].mean():.2f} (nominal 13)")
    for seed in SEEDS:
        assert ratios[("periodic", seed)] < 1.0, (seed, ratios)
    mean = float(np.mean([ratios[("periodic", seed)] for seed in SEEDS]))
    print(f"  periodic, mean of the seeds: {mean:.3f}; recorded OPEN_LOOP_PERIODIC_RATIO {FO.OPEN_LOOP_PERIODIC_RATIO:g}")
    assert abs(mean - FO.OPEN_LOOP_PERIODIC_RATIO) <= 0.01, mean


def test_the_fp64_loss_against_the_longdouble_rerun_is_what_the_module_records():
    """The chains of the GPU test (5 start states x 3 masses x 8 calls), the fp64 filter and its np.longdouble shadow each on its own
    state: the largest deviation (FO.deviation) is fp64's own loss on these cases.  FO.FP64_LOSS, the number the GPU bar is 8 x of,
    must cover it and be no more than twice it."""
    assert np.finfo(np.longdouble).eps < 1e-18  # (an extended type: otherwise the re-run measures nothing)
    worst, where = 0.0, None
    for si, name in enumerate(STARTS):
        s, p0, _ = make_problem() if name == "make_problem" else atlas_state(name)
        for mi, mass in enumerate(MASSES):
            p = p0.replace(m=float(np.float32(mass)))
            for k, c in enumerate(FO.build_chain(s, p, 100 * si + mi, OBS, shadow=True)):
                dev = FO.deviation(c["xi"], c["P"], c["xi_ld"], c["P_ld"])
                if dev > worst:
                    worst, where = dev, (name, mi, k)
    print(f"  fp64 loss against np.longdouble: {worst:.3e} at {where}; recorded FP64_LOSS {FO.FP64_LOSS:g}")
    assert worst <= FO.FP64_LOSS <= 2.0 * worst, (worst, FO.FP64_LOSS)
