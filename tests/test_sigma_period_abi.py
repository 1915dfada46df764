"""CPU: the ABI of the Sigma period (covo_set_step_sigma_period, covo_step_sigma_age, covo_sigma_shift; include/covo_hip.h), the
`sigma_period` keyword of the Python surface, and the numpy restatement of a reuse step's covariance with its known
answers.  The restatement (tests/sigma_shift_oracle.py) is written from the definition; tests/test_gpu_sigma_period.py holds the
kernel against it."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)
from tests.sigma_shift_oracle import (DU, N_A, chain_ratios, decoupled_rows, off_structure, random_spd, random_spd_factors, rank_update,
                                      shift_chain_ref, shift_factor_ref, shift_power_ref, shift_S, shift_sigma_ref, volume_scalar)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_factors(sample_sigma, which=(0, 5, 9, 13)):
    """The fp32 factors of covo.py's Sigma (oracle/ref_np.py::optimize_sigma) of matrices `which` of tests/golden/hessians_r03.npz."""
    from oracle import ref_np as R
    g = np.load(os.path.join(ROOT, "tests", "golden", "hessians_r03.npz"))
    Rm = [m for k in g.files for m in g[k]]
    return [np.linalg.cholesky(R.optimize_sigma(np.asarray(Rm[i], dtype=np.float64), sample_sigma, N_A // DU, DU)).astype(np.float32)
            for i in which]


# ---------------------------------------------------------------------------------------------- known answers of the restatement
def test_sigma_squared_identity_is_a_fixed_point():
    for sigma in (0.5, 0.3):
        S = shift_sigma_ref(sigma ** 2 * np.eye(N_A), sigma)
        assert np.abs(S - sigma ** 2 * np.eye(N_A)).max() < 1e-14
        S2, Lp = shift_factor_ref(sigma * np.eye(N_A), sigma)
        assert np.abs(S2 - sigma ** 2 * np.eye(N_A)).max() < 1e-14 and np.abs(Lp - sigma * np.eye(N_A)).max() < 1e-14
    # another input volume: the constraint brings it back
    S = shift_sigma_ref(4.0 * np.eye(N_A), 0.5)
    assert np.abs(S - 0.25 * np.eye(N_A)).max() < 1e-14


def test_block_diagonal_blocks_move_up_and_the_last_repeats():
    rng = np.random.default_rng(5)
    blocks = []
    for t in range(32):
        A = rng.normal(size=(4, 4))
        blocks.append(A @ A.T + (0.5 + 0.1 * t) * np.eye(4))
    Sigma = np.zeros((N_A, N_A))
    for t, B in enumerate(blocks):
        Sigma[4 * t:4 * t + 4, 4 * t:4 * t + 4] = B
    sigma = 0.5
    Sp = shift_sigma_ref(Sigma, sigma)
    moved = blocks[1:] + [blocks[-1]]
    c = Sp[0, 0] / moved[0][0, 0]
    for t, B in enumerate(moved):
        assert np.abs(Sp[4 * t:4 * t + 4, 4 * t:4 * t + 4] - c * B).max() < 1e-12 * np.abs(B).max() * max(c, 1.0)
    off = Sp.copy()
    for t in range(32):
        off[4 * t:4 * t + 4, 4 * t:4 * t + 4] = 0.0
    assert np.all(off == 0.0)
    assert abs(np.linalg.slogdet(Sp)[1] - 2 * N_A * np.log(sigma)) < 1e-10
    # the factor route gives the same matrix
    S2, Lp = shift_factor_ref(np.linalg.cholesky(Sigma), sigma)
    assert np.abs(S2 - Sp).max() < 1e-12 * np.abs(Sp).max()


def test_shift_of_a_random_spd_matrix_has_the_zero_block_and_is_spd():
    rng = np.random.default_rng(11)
    Sigma = random_spd(rng)
    S = shift_S(Sigma)
    assert np.all(S[N_A - DU:, :N_A - DU] == 0.0) and np.all(S[:N_A - DU, N_A - DU:] == 0.0)
    assert np.array_equal(S, S.T)
    assert np.array_equal(S[:N_A - DU, :N_A - DU], Sigma[DU:, DU:]) and np.array_equal(S[N_A - DU:, N_A - DU:], Sigma[N_A - DU:, N_A - DU:])
    assert np.linalg.eigvalsh(S).min() > 0.0
    Sp = shift_sigma_ref(Sigma, 0.5)
    assert abs(np.linalg.slogdet(Sp)[1] - 2 * N_A * np.log(0.5)) < 1e-9
    # Sigma' from the factor == Sigma' from the covariance
    S2, Lp = shift_factor_ref(np.linalg.cholesky(Sigma), 0.5)
    assert np.abs(S2 - Sp).max() < 1e-11 * np.abs(Sp).max()
    assert np.all(np.triu(Lp, 1) == 0.0) and np.all(np.diag(Lp) > 0.0)


def test_rank4_update_equals_the_cholesky_of_the_trailing_block():
    rng = np.random.default_rng(12)
    for cond in (6e2, 7e4):
        Sigma = random_spd(rng, cond)
        L = np.linalg.cholesky(Sigma)
        up = rank_update(L[DU:, DU:], L[DU:, :DU])
        ref = np.linalg.cholesky(Sigma[DU:, DU:])
        assert np.abs(up - ref).max() < 1e-11 * np.abs(ref).max(), cond
        assert np.all(np.triu(up, 1) == 0.0)


# ---------------------------------------------------------------------------------------------- k reuse steps in a row (m <= 64: k <= 63)
def test_k_unrounded_steps_equal_the_closed_form():
    rng = np.random.default_rng(13)
    Sigma = random_spd(rng, 7e4)
    chain = shift_chain_ref(np.linalg.cholesky(Sigma), 63, 0.5, rounded=False, every=True)
    for k, (Sp, Lp) in enumerate(chain, start=1):
        ref = shift_power_ref(Sigma, k, 0.5)
        assert np.abs(Sp - ref).max() <= 1e-10 * np.abs(ref).max(), k
        assert np.abs(Lp - np.linalg.cholesky(ref)).max() <= 1e-10 * np.abs(Lp).max(), k
        assert abs(np.linalg.slogdet(ref)[1] - 2 * N_A * np.log(0.5)) < 1e-9, k
        assert not Sp[off_structure(k)].any() and not Lp[off_structure(k)].any(), k
        # ... and one more S of the previous closed form is the next one
        if k > 1:
            assert np.abs(shift_sigma_ref(shift_power_ref(Sigma, k - 1, 0.5), 0.5) - ref).max() <= 1e-12 * np.abs(ref).max(), k


def test_closed_form_does_not_change_from_k_31_on():
    rng = np.random.default_rng(14)
    Sigma = random_spd(rng)
    at31 = shift_power_ref(Sigma, 31, 0.5)
    for k in (32, 33, 40, 63, 64, 1000):
        assert np.array_equal(shift_power_ref(Sigma, k, 0.5), at31), k
    assert not np.array_equal(shift_power_ref(Sigma, 30, 0.5), at31)
    B = at31[N_A - DU:, N_A - DU:]
    for t in range(N_A // DU):
        assert np.array_equal(at31[DU * t:DU * t + DU, DU * t:DU * t + DU], B), t
    assert not at31[off_structure(31)].any() and off_structure(31).sum() == N_A * N_A - 32 * 16
    assert np.array_equal(off_structure(40), off_structure(31)) and decoupled_rows(63) == DU


@pytest.mark.parametrize("k", [5, 40])
def test_block_diagonal_blocks_move_up_k_times(k):
    """test_block_diagonal_blocks_move_up_and_the_last_repeats carried to k shifts: block t of the result is c times block
    min(t + k, 31) of the input -- by the closed form, by k applications of S, and by the factor route with fp32 between steps."""
    rng = np.random.default_rng(5)
    blocks = []
    for t in range(32):
        A = rng.normal(size=(4, 4))
        blocks.append(A @ A.T + (0.5 + 0.1 * t) * np.eye(4))
    Sigma = np.zeros((N_A, N_A))
    for t, B in enumerate(blocks):
        Sigma[4 * t:4 * t + 4, 4 * t:4 * t + 4] = B
    sigma = 0.5
    moved = [blocks[min(t + k, 31)] for t in range(32)]
    want = np.zeros((N_A, N_A))
    for t, B in enumerate(moved):
        want[4 * t:4 * t + 4, 4 * t:4 * t + 4] = B
    want *= volume_scalar(want, sigma)
    Sp = shift_power_ref(Sigma, k, sigma)
    assert np.abs(Sp - want).max() < 1e-12 * np.abs(want).max()
    off = np.ones((N_A, N_A), dtype=bool)
    for t in range(32):
        off[4 * t:4 * t + 4, 4 * t:4 * t + 4] = False
    assert not Sp[off].any()
    assert abs(np.linalg.slogdet(Sp)[1] - 2 * N_A * np.log(sigma)) < 1e-10
    it = Sigma
    for _ in range(k):
        it = shift_sigma_ref(it, sigma)
    assert np.abs(it - want).max() < 1e-12 * np.abs(want).max() and not it[off].any()
    S2, Lp = shift_chain_ref(np.linalg.cholesky(Sigma), k, sigma, rounded=False)
    assert np.abs(S2 - want).max() < 1e-11 * np.abs(want).max() and not S2[off].any() and not Lp[off].any()


def chain_against_the_closed_form(L32, sigma, where):
    """The worst (log det, L', Sigma') ratio over k = 1 .. 63 of the fp32-rounded chain from the fp32 factor L32 against the closed
    form of Sigma = L32 L32^T, and the k of each; asserts the exact zero structure of every step."""
    Sigma = L32.astype(np.float64) @ L32.astype(np.float64).T
    worst, at = np.zeros(3), np.zeros(3, dtype=int)
    for k, (Sp, Lp) in enumerate(shift_chain_ref(L32, 63, sigma, every=True), start=1):
        Sref = shift_power_ref(Sigma, k, sigma)
        S32, Lp32 = Sp.astype(np.float32), Lp.astype(np.float32)
        m = decoupled_rows(k)
        assert np.all(Lp32[m:, :m] == 0.0) and not Lp32[off_structure(k)].any() and not S32[off_structure(k)].any(), (where, k)
        assert np.all(np.triu(Lp32, 1) == 0.0) and np.array_equal(S32, S32.T), (where, k)
        r = chain_ratios(S32, Lp32, Sref, np.linalg.cholesky(Sref), sigma)
        at = np.where(r > worst, k, at)
        worst = np.maximum(worst, r)
    print(f"  {where}: fp32 chain against the closed form, worst ratio to the one-step bars over k <= 63: "
          f"log det {worst[0]:.2f} (k = {at[0]}), L' {worst[1]:.2f} (k = {at[1]}), Sigma' {worst[2]:.2f} (k = {at[2]})")
    return worst


def test_fp32_chain_stays_within_the_one_step_bars_of_the_closed_form():
    """63 reuse steps with L' rounded to fp32 between them do not drift: every step renormalises the volume, and a stage that has
    decoupled is only ever copied and rescaled.  random_spd at cond 6e2 and 7e4: all three one-step bars hold at every k (worst
    ratios 0.30 log det, 0.06 L', 0.30 Sigma').  Sigma of golden Hessians 0, 5, 9 and 13: the log det bar is a bound, not an
    estimate -- the fp64 L' has log det 2 n log sigma and each diagonal entry moves by at most 2^-24 relative when rounded, all in
    the same direction at worst, which k >= 30 comes close to (four diagonal values, each 31 times: 0.86 at k = 30) -- and is
    asserted; the roundings of L' between the steps do add up in L' and Sigma' (worst 0.18 and 1.12 of the one-step bars, at
    k = 28 and 25 of Hessian 13), which is why tests/test_gpu_ceilings.py holds the kernel's chain to a bar that includes this
    chain's own error at the same k."""
    for i, L32 in enumerate(random_spd_factors()):
        assert np.all(chain_against_the_closed_form(L32, 0.5, ("random_spd", i)) <= 1.0)
    for i, L32 in zip((0, 5, 9, 13), golden_factors(0.5)):
        assert chain_against_the_closed_form(L32, 0.5, ("golden", i))[0] <= 1.0


# ---------------------------------------------------------------------------------------------- the ABI and the keyword
def test_sigma_period_entry_points_exist_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"#define COVO_HAS_SIGMA_PERIOD 1\b", hdr) and built.COVO_HAS_SIGMA_PERIOD == 1
    assert int(re.search(r"#define COVO_MAX_SIGMA_PERIOD\s+(\d+)", hdr).group(1)) == 64 == built.COVO_MAX_SIGMA_PERIOD
    assert re.search(r"\bint covo_set_step_sigma_period\(covo_handle_t h, int32_t period\);", hdr)
    assert re.search(r"\bint covo_step_sigma_age\(covo_handle_t h, int32_t \*next_age, int32_t \*last_age\);", hdr)
    assert re.search(r"\bint covo_sigma_shift\(covo_handle_t h, const float \*L_in, int32_t batch, float sample_sigma, float \*Sigma_out, "
                     r"float \*L_out, void \*stream\);", hdr)
    fn = lib.covo_set_step_sigma_period
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int32]
    fn = lib.covo_sigma_shift
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.covo_step_sigma_age.restype is C.c_int
    for name in ("covo_set_step_sigma_period", "covo_step_sigma_age", "covo_sigma_shift"):
        assert name in built.EXPORTS
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()  # additive
    # a null handle is refused before anything else happens (no GPU needed)
    assert lib.covo_set_step_sigma_period(None, 2) != 0 and b"null handle" in lib.covo_last_error()
    assert lib.covo_sigma_shift(None, None, 1, 0.5, None, None, None) != 0 and b"null handle" in lib.covo_last_error()
    assert lib.covo_step_sigma_age(None, None, None) != 0 and b"null handle" in lib.covo_last_error()


def test_sigma_period_is_a_keyword_defaulting_to_one(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import Args, eval_env_batched, get_controller
    for fn in (SamplingCore.__init__, controllers.MPPIController.__init__, controllers.CoVOController.__init__,
               controllers.BatchedCoVOController.__init__, controllers.BatchedMPPIController.__init__, get_controller,
               eval_env_batched):
        p = inspect.signature(fn).parameters
        assert "sigma_period" in p and p["sigma_period"].default == 1, fn
    assert Args().sigma_period == 1
    assert callable(SamplingCore.sigma_info) and callable(SamplingCore.sigma_shift) and callable(SamplingCore.set_sigma_period)
    assert [built.check_sigma_period(m) for m in (1, 2, 64)] == [1, 2, 64]
    assert built.check_sigma_period(1, "offline") == 1 and built.check_sigma_period(1, "MPPI") == 1


def _env(device=None):
    import covo_mpc_amd as cm
    return cm.envs.Quad3D(task="tracking_zigzag", disturb_type="gaussian", enable_randomizer=False, disable_rollover_terminate=True,
                          generate_noisy_state=True, device=device)


@pytest.mark.parametrize("bad", [0, 65, 2.5, -1, None, "2", True])
def test_constructors_refuse_sigma_period_out_of_range(built, bad):
    """ValueError before anything is built: no device is needed."""
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    env = _env()
    with pytest.raises(ValueError, match="sigma_period="):
        SamplingCore(256, 32, 0.01, 1.0, sigma_period=bad)
    with pytest.raises(ValueError, match="sigma_period="):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, sigma_period=bad)
    with pytest.raises(ValueError, match="sigma_period="):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, sigma_period=bad)
    with pytest.raises(ValueError, match="sigma_period="):
        eval_env_batched(env, 2, "N256_H32_lam0.01", sigma_period=bad)
    for name in ("mppi", "covo-online", "covo-offline"):
        with pytest.raises(ValueError, match="sigma_period="):
            get_controller(env, name, "N256_H32_lam0.01", device="cpu", sigma_period=bad)


def test_modes_without_a_sigma_per_step_refuse_a_period(built):
    """MPPI, covo-offline and the env-batched offline / MPPI controllers: ValueError in words, before anything is built."""
    from covo_mpc_amd import controllers
    from covo_mpc_amd.envs.quadrotor import get_controller
    env = _env()
    with pytest.raises(ValueError, match="sigma_period=2 with mppi"):
        get_controller(env, "mppi", "N256_H32_lam0.01", device="cpu", sigma_period=2)
    with pytest.raises(ValueError, match="sigma_period=2 with covo-offline"):
        get_controller(env, "covo-offline", "N256_H32_lam0.01", device="cpu", sigma_period=2)
    with pytest.raises(ValueError, match="sigma_period=3 with MPPI"):
        controllers.MPPIController(env, None, 256, 32, 0.01, sigma_period=3)
    with pytest.raises(ValueError, match="sigma_period=3 with offline"):
        controllers.CoVOController(env, None, 256, 32, 0.01, "offline", sigma_period=3)
    with pytest.raises(ValueError, match="sigma_period=2 with the env-batched covo-offline controller"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, mode="offline", sigma_period=2)
    with pytest.raises(ValueError, match="sigma_period=2 with the env-batched MPPI controller"):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, sigma_period=2)


def test_sigma_period_in_range_passes_the_keyword_check(built):
    """Without a device the construction gets as far as the device check (CovoError, not ValueError): the keyword was accepted."""
    import torch
    from covo_mpc_amd.envs.quadrotor import get_controller
    if not torch.cuda.is_available():
        with pytest.raises(built.CovoError, match="needs a ROCm GPU"):
            get_controller(_env(), "covo-online", "N256_H32_lam0.01", device="cpu", sigma_period=4)
        return
    c, _ = get_controller(_env("cuda:0"), "covo-online", "N256_H32_lam0.01", device="cuda:0")
    assert c.core.sigma_period == 1 and c.core.sigma_info() == {} and c.core.sigma_age == 0
    c.core.close()
    c, _ = get_controller(_env("cuda:0"), "covo-online", "N256_H32_lam0.01", device="cuda:0", sigma_period=4)
    assert c.core.sigma_period == 4 and c.core.sigma_info() == {"sigma_age": 0} and c.core.sigma_age == 0
    c.core.close()


def test_sharded_core_refuses_a_sigma_period_without_a_device(built, monkeypatch):
    """A process group of two ranks: NotImplementedError, worded like iters', before the device is looked for."""
    import torch.distributed as dist
    from covo_mpc_amd.controllers._core import SamplingCore
    group = object()
    monkeypatch.setattr(dist, "get_world_size", lambda g=None: 2 if g is group else 1)
    monkeypatch.setattr(dist, "get_rank", lambda g=None: 0)
    with pytest.raises(NotImplementedError, match="sigma_period=2 on sample-sharded ranks"):
        SamplingCore(256, 32, 0.01, 1.0, process_group=group, sigma_period=2)
    with pytest.raises(ValueError, match="sigma_period="):  # the range check comes first
        SamplingCore(256, 32, 0.01, 1.0, process_group=group, sigma_period=65)


def test_debug_path_refuses_a_sigma_period(built):
    from covo_mpc_amd.controllers._core import SamplingCore

    class Stub:
        ess_min, compute_plan, compute_diag, compute_fan, arb_mask, update_rule, iters, elite, sigma_period = (
            0.0, False, False, 0, 0, "softmax", 1, 0, 2)

    with pytest.raises(NotImplementedError, match="sigma_period=2 acts in the fused step"):
        SamplingCore.require_fused_for_diag(Stub())
    Stub.sigma_period = 1
    SamplingCore.require_fused_for_diag(Stub())  # no period: the kernel-by-kernel path is free to run
