"""CPU tests of tests/state_atlas.py: every entry is where its name says, the oracles agree with each other off hover (C against the
literal numpy rollout, C hyper-dual against torch AD Hessians), and the fp32 oracle's own loss against fp64 -- the yardstick the GPU
tests (tests/test_gpu_state_atlas.py) hold the kernels to -- is what the atlas was built for: above 1e-5 at the near-singular
attitude, below it everywhere else."""
import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import ref_np as R
from tests.state_atlas import (ATLAS, BENIGN, NAMES, ROLLOVER_AT_0, atlas_state, loss3, one_ulp_shift, rel_err, rollout_case,
                               yaw_args)


def _fp32(s):
    return all(np.array_equal(np.asarray(x, dtype=np.float32).astype(np.float64), x)
               for x in (s.pos, s.vel, s.quat, s.omega, s.f_disturb, s.pos_tar, s.vel_tar, s.acc_tar, s.pos_traj, s.vel_traj))


def _yaw(s):
    yn, yd = yaw_args(s.quat)
    return np.arctan2(yn, yd)


def test_every_entry_is_where_its_name_says():
    assert len(NAMES) == 12 and len(BENIGN) == 11 and "near_singular" not in BENIGN and set(ROLLOVER_AT_0) <= set(BENIGN)
    for name in NAMES:
        s, p, _ = atlas_state(name)
        assert _fp32(s) and s.time == 37, name
        assert not R.is_terminal(s, p), name  # inside the box, inside the episode
        # (quat[3] < cos(pi/4) is ANY rotation beyond 90 degrees: the large yaws are rollover-terminal as well)
        assert R.is_terminal(s, p, rollover=True) or name not in ROLLOVER_AT_0, name
        if name not in ("double_cover", "near_singular", "unnorm_q"):
            # on a (nearly) unit quaternion away from the singular pitch the reward's yaw is the entry's, up to the 1e-3 noise
            want = ATLAS[name]["euler"][2]
            assert abs(np.angle(np.exp(1j * (_yaw(s) - want)))) < 1e-2, (name, _yaw(s), want)
    signs = []
    for name in ("yaw_pi_minus", "yaw_pi_plus"):
        yn, yd = yaw_args(atlas_state(name)[0].quat)
        assert yd < 0 and abs(yn) < 0.01, (name, yn, yd)
        signs.append(np.sign(yn))
    assert signs == [1.0, -1.0], signs  # both sides of the branch cut
    for name, lo, hi in (("yaw_half_pi", 0.0, 0.01), ("yaw_quarter", 0.69, 0.72), ("yaw_3quarter_neg", 0.69, 0.72)):
        yn, yd = yaw_args(atlas_state(name)[0].quat)
        assert lo <= abs(yd) <= hi and (name != "yaw_3quarter_neg" or (yn < 0 and yd < 0)), (name, yn, yd)
    yn, yd = yaw_args(atlas_state("near_singular")[0].quat)
    assert abs(yn) < 0.05 and abs(yd) < 0.05, (yn, yd)
    for name in ROLLOVER_AT_0:
        assert atlas_state(name)[0].quat[3] < np.cos(np.pi / 4) - 0.1, name
    s, p, _ = atlas_state("unnorm_q")
    assert abs(np.linalg.norm(s.quat) - 1.3) < 5e-3
    s, p, _ = atlas_state("double_cover")
    assert s.quat[3] < -0.98 and abs(_yaw(s)) < 0.1  # the same attitude as make_problem's
    s, p, _ = atlas_state("far_fast")
    assert np.linalg.norm(s.pos - s.pos_tar) > 1.5 and np.linalg.norm(s.vel - s.vel_tar) > 4.0
    # yaw_cross: under the hover action the oracle's yaw changes sign inside the horizon
    s, p, _ = atlas_state("yaw_cross")
    hover = R.hover_action(p, 32, np.float64)
    yaws = [_yaw(s)]
    for k in range(32):
        s, _, _ = R.step_env(s, hover[k], p, np.zeros(3))
        yaws.append(_yaw(s))
    yaws = np.asarray(yaws)
    assert yaws[0] > 0 and np.any(yaws[1:] < 0) and np.abs(yaws).max() < 1.0, yaws
    # inverted: the oracle's PID law asks for negative thrust along the body axis and is clipped at 0 (action[0] = -1)
    s, p, _ = atlas_state("inverted")
    act, _ = R.pid_action(s, p)
    assert act[0] == -1.0, act


@pytest.mark.parametrize("name", NAMES)
def test_c_oracle_matches_literal_numpy(name):
    """The C rollout against R.rollout at every entry (8 samples, rollover off and on), at the bars of
    tests/test_oracle.py::test_c_oracle_matches_literal_numpy_and_golden."""
    s, p, rng = atlas_state(name)
    a = np.clip(R.hover_action(p, 32, np.float64)[None] + 0.5 * rng.normal(size=(8, 32, 4)), -1, 1).astype(np.float32).astype(np.float64)
    for rollover in (False, True):
        c_np, r_np, p_np = R.rollout(s, p, a, 0.97, np.zeros(3), rollover=rollover)
        c64, r64, p64 = CO.rollout(s, p, a, 0.97, np.zeros(3), dtype=np.float64, want_rewards=True, want_poses=True, rollover=rollover)
        print(f"  {name} rollover={rollover}: cost {np.abs(c64 - c_np).max():.1e} rewards {np.abs(r64 - r_np).max():.1e} "
              f"poses {np.abs(p64 - p_np).max():.1e}")
        assert np.all(np.isfinite(c_np))
        assert np.abs(c64 - c_np).max() < 1e-11
        assert np.abs(r64 - r_np).max() < 1e-12 and np.abs(p64 - p_np).max() < 1e-12
        if rollover and name in ROLLOVER_AT_0:
            assert np.all(r_np == r_np[:, :1])  # terminal at step 0: one frozen reward per sample


@pytest.mark.parametrize("name", ["yaw_pi_minus", "near_singular", "roll_120_spin"])
def test_c_hessian_matches_torch_ad_off_hover(name):
    """The two independent Hessian references, with the two clip ties, at the bar of tests/test_oracle.py::
    test_c_hessian_matches_torch_ad (1e-12; relative to the largest entry where that exceeds 1: |R| reaches hundreds at the
    near-singular attitude)."""
    from oracle import ref_torch as RT
    s, p, rng = atlas_state(name)
    a = (R.hover_action(p, 32, np.float64) + 0.1 * rng.normal(size=(32, 4))).astype(np.float32)
    a[3, 1] = 1.0
    a[5, 2] = -1.0
    a = a.reshape(-1).astype(np.float64)
    Rc = CO.hessian(s, p, a, 32)
    Rt = RT.hessian(s, p, a, 32)
    err, big = np.abs(Rc - Rt).max(), np.abs(Rt).max()
    print(f"  {name}: |C - torch| {err:.1e}, max|R| {big:.3g}")
    assert np.all(np.isfinite(Rc)) and np.all(np.isfinite(Rt))
    assert err < 1e-12 * max(1.0, big)
    assert np.abs(Rc - Rc.T).max() == 0.0 and np.abs(Rc[124:]).max() == 0.0
    assert np.abs(Rt[13]).max() > 0


def test_fp32_oracle_loss_is_the_yardstick():
    """What fp32 -- the reference's arithmetic type -- loses against fp64 at every entry (N = 2048, sigma = 0.5): printed; the atlas
    is not vacuous when the near-singular attitude really costs fp32 more than the 1e-5 bar on a share of the samples and no
    benign entry does on its typical sample."""
    for name in NAMES:
        s, p, a = rollout_case(name, 2048)
        c64 = CO.rollout(s, p, a.astype(np.float64), 1.0, np.zeros(3), dtype=np.float64)
        c32 = CO.rollout(s.astype(np.float32), p, a, 1.0, np.zeros(3, np.float32), dtype=np.float32)
        mx, q99, med = loss3(rel_err(c32.astype(np.float64), c64))
        print(f"  {name:18s} fp32 loss max {mx:.1e} q99 {q99:.1e} median {med:.1e}   cost in [{c64.min():.1f}, {c64.max():.1f}]")
        if name == "near_singular":
            assert q99 >= 1e-5, q99
        else:
            assert med < 1e-5, (name, med)


def test_rollout_cases_are_well_conditioned_except_the_near_singular_one():
    """The 1e-5 floor of the GPU rollout rule presumes that the exact cost itself does not move by that much when its fp32 inputs
    move by one ulp.  Measured in fp64 alone (state_atlas.one_ulp_shift) on the very samples the GPU test rolls out: below 1e-5 for
    every sample of every benign entry at both discounts, above it at near_singular -- and at roll_120_spin's seed-0 draw, which
    is why that entry draws from seed 1 (state_atlas.ROLLOUT_SEED)."""
    for name in NAMES:
        s, p, a = rollout_case(name)
        k = [one_ulp_shift(s, p, a, d) for d in (1.0, 0.97)]
        print(f"  {name:18s} one-ulp shift max {k[0].max():.1e} / {k[1].max():.1e}, median {np.median(k[1]):.1e}")
        if name == "near_singular":
            assert max(k[0].max(), k[1].max()) >= 1e-5
        else:
            assert max(k[0].max(), k[1].max()) < 1e-5, name
    s, p, rng = atlas_state("roll_120_spin", seed=0)
    a = np.clip(R.hover_action(p, 32, np.float64)[None] + 0.5 * rng.normal(size=(1024, 32, 4)), -1, 1).astype(np.float32)
    k = one_ulp_shift(s, p, a, 0.97)
    print(f"  roll_120_spin seed 0: one-ulp shift max {k.max():.1e} at sample {k.argmax()}, next {np.sort(k)[-2]:.1e}")
    assert k.max() > 2e-5 and np.sort(k)[-2] < 1e-5
