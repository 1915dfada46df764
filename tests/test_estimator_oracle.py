"""CPU: tests/estimator_oracle.py (the definition the state estimator's kernel is held to) against its own properties."""
import functools

import numpy as np

from tests import estimator_oracle as EO
from tests.conftest import make_problem

SEEDS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def experiment(seed):
    s, p, _ = make_problem()
    return EO.open_loop(s, p, seed, n_steps=200)


def start():
    s, p, _ = make_problem()
    x = np.concatenate([s.pos, s.vel, s.quat, s.omega])
    hover = np.array([float(p.m) * float(p.g) / float(p.max_thrust) * 2.0 - 1.0, 0.0, 0.0, 0.0], dtype=np.float32)
    return s, p, x, hover


def test_first_call_takes_the_measurement_and_R():
    s, p, x, hover = start()
    f = EO.Filter(p)
    row = EO.pack_row(x.astype(np.float32), s.f_disturb, int(s.time))
    row[16:25] = np.arange(9)
    out, side = f.call(row, hover)
    assert np.array_equal(out.view(np.uint32), row.view(np.uint32))
    assert np.array_equal(f.x, row[:13].astype(np.float64)) and np.array_equal(f.P, np.diag(f.R))
    assert side[0] == EO.FLAG_INIT and side[7] == int(s.time) and side[1] == 0 and side[6] == 0
    R, Q = EO.constants(p)
    assert np.allclose(np.sqrt(R[[0, 3, 6, 10]]), 0.05 * np.array([0.25, 0.5, 0.02, 0.5]), rtol=1e-15)
    assert Q[0] == 0 and Q[6] == 0 and Q[10] == 0 and np.isclose(np.sqrt(Q[3]), float(p.dt) * float(p.dyn_noise_scale) / float(p.m), rtol=1e-15)


def test_P_stays_symmetric_and_positive_semidefinite_over_100_steps():
    s, p, x, hover = start()
    rng = np.random.default_rng(5)
    f = EO.Filter(p)
    obs = 0.05 * EO.OBS_GROUP_SCALE
    for k in range(100):
        row = EO.pack_row(EO.measure(rng, x, obs), np.zeros(3), int(s.time) + k)
        out, side = f.call(row, hover)
        assert side[0] == (EO.FLAG_INIT if k == 0 else 0), (k, side)
        assert np.array_equal(f.P, f.P.T), k
        assert np.linalg.eigvalsh(f.P).min() >= -1e-18, (k, np.linalg.eigvalsh(f.P).min())
        x = f.f(x, hover.astype(np.float64), np.zeros(3))[0]


def test_a_time_jump_reinitialises_and_a_nan_invalidates():
    s, p, x, hover = start()
    rng = np.random.default_rng(6)
    f = EO.Filter(p)
    obs = 0.05 * EO.OBS_GROUP_SCALE
    t = int(s.time)
    for k in range(3):
        f.call(EO.pack_row(EO.measure(rng, x, obs), np.zeros(3), t + k), hover)
    row = EO.pack_row(EO.measure(rng, x, obs), np.ones(3), t + 4)  # (t + 3 was due)
    out, side = f.call(row, hover)
    assert side[0] == EO.FLAG_TIME and np.array_equal(out.view(np.uint32), row.view(np.uint32))
    assert np.array_equal(f.x, row[:13].astype(np.float64)) and np.array_equal(f.P, np.diag(f.R)) and f.t_prev == t + 4
    assert np.array_equal(f.f_prev, np.ones(3))
    out, side = f.call(EO.pack_row(EO.measure(rng, x, obs), np.zeros(3), t + 5), hover)
    assert side[0] == 0 and not np.array_equal(out[:13], row[:13])
    bad = EO.pack_row(EO.measure(rng, x, obs), np.zeros(3), t + 6)
    bad[4] = np.nan
    out, side = f.call(bad, hover)
    assert side[0] == EO.FLAG_NONFINITE and not f.valid and np.array_equal(out.view(np.uint32), bad.view(np.uint32))
    out, side = f.call(EO.pack_row(EO.measure(rng, x, obs), np.zeros(3), t + 7), hover)
    assert side[0] == EO.FLAG_INIT and f.valid
    f.P[2, 3] = np.nan
    row = EO.pack_row(EO.measure(rng, x, obs), np.zeros(3), t + 8)
    out, side = f.call(row, hover)
    assert side[0] == EO.FLAG_FAILED and np.array_equal(out.view(np.uint32), row.view(np.uint32)) and np.array_equal(f.P, np.diag(f.R))


def test_the_two_limits_model_prediction_and_measurement():
    s, p, x, hover = start()
    rng = np.random.default_rng(7)
    obs = 0.05 * EO.OBS_GROUP_SCALE
    z0, z1 = EO.measure(rng, x, obs), EO.measure(rng, x, obs)
    t = int(s.time)
    # very large obs_std at the update (the first call leaves P = R of the default scales: it is the update's R that has to dwarf P):
    # the second call returns the model's prediction from the first measurement
    f = EO.Filter(p, proc_std=[0.0, 0.0, 0.0, 0.0])
    f.call(EO.pack_row(z0, np.zeros(3), t), hover)
    f.R = EO.constants(p, obs_std=[1e6] * 4)[0]
    out, _ = f.call(EO.pack_row(z1, np.zeros(3), t + 1), hover)
    pred = f.f(z0.astype(np.float64), hover.astype(np.float64), np.zeros(3))[0]
    assert np.abs(out[:13] - pred).max() <= 1e-6
    # very large proc_std: the measurement
    f = EO.Filter(p, proc_std=[1e6] * 4)
    f.call(EO.pack_row(z0, np.zeros(3), t), hover)
    out, _ = f.call(EO.pack_row(z1, np.zeros(3), t + 1), hover)
    assert np.abs(out[:13] - z1).max() <= 1e-6


def test_closed_loop_condition_position_rms_below_half_the_measurements():
    for seed in SEEDS:
        truth, meas, est, sides = experiment(seed)
        assert (sides[1:, 0] == 0).all(), seed
        rms = lambda a: float(np.sqrt(((a[20:, 0:3] - truth[20:, 0:3]) ** 2).sum(axis=1).mean()))
        r_meas, r_est = rms(meas), rms(est)
        print(f"  seed {seed}: position rms measurement {r_meas * 100:.3f} cm, estimate {r_est * 100:.3f} cm, ratio {r_est / r_meas:.3f}; "
              f"mean nis {sides[20:, 1].mean():.2f}")
        assert r_est < 0.5 * r_meas, (seed, r_est, r_meas)
