"""CPU: the ABI of Sigma adapt (covo_set_step_sigma_adapt / covo_sigma_adapt; include/covo_hip.h), the `sigma_adapt` keyword of the
Python surface, and the numpy fp64 restatement of a reuse step's adapted covariance with its known answers.  The
restatement (tests/sigma_shift_oracle.py) is written from the definition; tests/test_gpu_sigma_adapt.py holds the kernel against it."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)
from tests.post_cov_oracle import ref_weighted_cov
from tests.sigma_shift_oracle import DU, N_A, adapt_ref, blend_M, random_spd, shift_sigma_ref, volume_scalar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def block_diag(blocks):
    out = np.zeros((N_A, N_A))
    for t, B in enumerate(blocks):
        out[4 * t:4 * t + 4, 4 * t:4 * t + 4] = B
    return out


def random_blocks(rng, floor=0.5):
    out = []
    for t in range(32):
        A = rng.normal(size=(4, 4))
        out.append(A @ A.T + (floor + 0.1 * t) * np.eye(4))
    return out


GAMMAS = (0.05, 0.5, 0.9)


# ---------------------------------------------------------------------------------------------- known answers of the restatement
def test_gamma_zero_is_the_plain_shift():
    rng = np.random.default_rng(3)
    Sigma = random_spd(rng)
    L = np.linalg.cholesky(Sigma)
    Sp, Lp, fb, c, _ = adapt_ref(L, np.full((N_A, N_A), np.nan), 0.0, 0.5)  # C is not looked at
    ref = shift_sigma_ref(L @ L.T, 0.5)
    assert fb == 0 and np.abs(Sp - ref).max() < 1e-12 * np.abs(ref).max()
    assert np.abs(Lp @ Lp.T - ref).max() < 1e-12 * np.abs(ref).max() and np.all(np.triu(Lp, 1) == 0.0)


@pytest.mark.parametrize("gamma", GAMMAS)
def test_c_equal_to_sigma_and_c_zero_give_the_plain_shift(gamma):
    rng = np.random.default_rng(4)
    Sigma = random_spd(rng)
    L = np.linalg.cholesky(Sigma)
    ref = shift_sigma_ref(L @ L.T, 0.5)
    for Cmat in (L @ L.T, np.zeros((N_A, N_A))):  # C = 0: W = 0 in the previous step; c absorbs the factor 1 - gamma
        Sp, Lp, fb, c, logdet = adapt_ref(L, Cmat, gamma, 0.5)
        assert fb == 0 and np.abs(Sp - ref).max() < 1e-11 * np.abs(ref).max()
        assert abs(np.linalg.slogdet(Sp)[1] - 2 * N_A * np.log(0.5)) < 1e-9
        assert abs(2.0 * np.log(np.diag(Lp)).sum() - 2 * N_A * np.log(0.5)) < 1e-9


@pytest.mark.parametrize("gamma", GAMMAS)
def test_sigma_squared_identity_is_a_fixed_point(gamma):
    for sigma in (0.5, 0.3):
        Sp, Lp, fb, c, _ = adapt_ref(sigma * np.eye(N_A), sigma ** 2 * np.eye(N_A), gamma, sigma)
        assert fb == 0 and abs(c - 1.0) < 1e-13
        assert np.abs(Sp - sigma ** 2 * np.eye(N_A)).max() < 1e-14 and np.abs(Lp - sigma * np.eye(N_A)).max() < 1e-14


@pytest.mark.parametrize("gamma", GAMMAS)
def test_block_diagonal_inputs_blend_block_by_block(gamma):
    rng = np.random.default_rng(6)
    Sb, Cb = random_blocks(rng), random_blocks(rng, 0.1)
    Sp, Lp, fb, c, _ = adapt_ref(np.linalg.cholesky(block_diag(Sb)), block_diag(Cb), gamma, 0.5)
    moved = [(1.0 - gamma) * s + gamma * k for s, k in zip(Sb[1:] + [Sb[-1]], Cb[1:] + [Cb[-1]])]
    assert fb == 0
    for t, B in enumerate(moved):
        assert np.abs(Sp[4 * t:4 * t + 4, 4 * t:4 * t + 4] - c * B).max() < 1e-12 * np.abs(B).max() * max(c, 1.0)
    assert np.all((Sp - block_diag([Sp[4 * t:4 * t + 4, 4 * t:4 * t + 4] for t in range(32)])) == 0.0)
    assert abs(np.linalg.slogdet(Sp)[1] - 2 * N_A * np.log(0.5)) < 1e-9
    assert abs(c - volume_scalar(block_diag(moved), 0.5)) < 1e-12 * c


@pytest.mark.parametrize("gamma", GAMMAS)
def test_diagonal_blocks_equal_mppis_blend_of_the_shifted_blocks(gamma):
    """One step from a block-diagonal Sigma: MPPI (mppi.py:109-125 at gamma_sigma = gamma, gamma_mean = 1) blends every stage's block
    with the weighted covariance of the samples about the new mean, and the next step shifts the blocks (mppi.py:43-49); the 4 x 4
    diagonal blocks of M are those."""
    rng = np.random.default_rng(7)
    N, lam = 300, 0.5
    Sb = random_blocks(rng, 0.05)
    mu = rng.normal(size=(32, 4)) * 0.1
    a = np.stack([mu[t] + rng.multivariate_normal(np.zeros(4), Sb[t], size=N) for t in range(32)], axis=1)  # (N, H, 4)
    cost = rng.normal(size=N)
    # mppi.py:109-125 restated
    cost_exp = np.exp(-(cost - cost.min()) / lam)
    weight = cost_exp / cost_exp.sum()
    a_mean = (weight[:, None, None] * a).sum(axis=0)
    dev = a - a_mean
    a_cov = (weight[:, None, None, None] * (dev[..., None] * dev[:, :, None, :])).sum(axis=0) * gamma + np.stack(Sb) * (1 - gamma)
    a_cov = np.concatenate([a_cov[1:], a_cov[-1:]])  # the next step's shift
    # the full-matrix form
    Cmat = ref_weighted_cov(a.transpose(1, 0, 2), cost, mu.reshape(-1), lam=lam)[0]
    M = blend_M(block_diag(Sb), Cmat, gamma)
    for t in range(32):
        assert np.abs(M[4 * t:4 * t + 4, 4 * t:4 * t + 4] - a_cov[t]).max() < 1e-12 * np.abs(a_cov[t]).max(), t
    assert np.all(M[N_A - DU:, :N_A - DU] == 0.0) and np.all(M[:N_A - DU, N_A - DU:] == 0.0)


@pytest.mark.parametrize("gamma", GAMMAS)
def test_log_det_meets_the_volume_constraint(gamma):
    rng = np.random.default_rng(8)
    L = np.linalg.cholesky(random_spd(rng, 7e4))
    Y = rng.normal(size=(4, N_A)) * 0.3  # rank 4
    Sp, Lp, fb, c, logdet = adapt_ref(L, Y.T @ Y / 4.0, gamma, 0.5)
    assert fb == 0
    assert abs(np.linalg.slogdet(Sp)[1] - 2 * N_A * np.log(0.5)) < 1e-9
    assert abs(N_A * np.log(c) + logdet - 2 * N_A * np.log(0.5)) < 1e-9


@pytest.mark.parametrize("gamma", GAMMAS)
def test_a_nan_or_an_indefinite_c_gives_the_gamma_zero_answer_with_the_flag(gamma):
    rng = np.random.default_rng(9)
    Sigma = random_spd(rng)
    L = np.linalg.cholesky(Sigma)
    S0, L0, fb0, c0, ld0 = adapt_ref(L, np.zeros((N_A, N_A)), 0.0, 0.5)
    assert fb0 == 0
    Cnan = Sigma.copy()
    Cnan[40, 17] = np.nan
    Cneg = -10.0 * (L @ L.T)
    bad = [Cnan, np.full((N_A, N_A), np.inf)] + ([Cneg] if gamma * 10.0 > 1.0 - gamma else [])  # (indefinite M needs 10 gamma > 1 - gamma)
    for Cmat in bad:
        Sp, Lp, fb, c, ld = adapt_ref(L, Cmat, gamma, 0.5)
        assert fb == 1 and np.array_equal(Sp, S0) and np.array_equal(Lp, L0) and c == c0 and ld == ld0
    if gamma * 10.0 <= 1.0 - gamma:  # M = (1 - 11 gamma) S(Sigma) stays positive definite: no fallback, the plain shift
        Sp, _, fb, _, _ = adapt_ref(L, Cneg, gamma, 0.5)
        assert fb == 0 and np.abs(Sp - S0).max() < 1e-11 * np.abs(S0).max()
    # rows and columns 0 .. 3 of C are shifted out: whatever they hold is not looked at
    Cedge = Sigma.copy()
    Cedge[:DU, :] = Cedge[:, :DU] = np.nan
    assert adapt_ref(L, Cedge, gamma, 0.5)[2] == 0


# ---------------------------------------------------------------------------------------------- the ABI and the keyword
def test_sigma_adapt_entry_points_exist_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"#define COVO_HAS_SIGMA_ADAPT 1\b", hdr) and built.COVO_HAS_SIGMA_ADAPT == 1
    assert int(re.search(r"#define COVO_SIGMA_ADAPT_FLOATS\s+(\d+)", hdr).group(1)) == 4 == built.COVO_SIGMA_ADAPT_FLOATS
    assert re.search(r"\bint covo_set_step_sigma_adapt\(covo_handle_t h, float gamma, float \*rows_out[^,]*, int32_t n_inst\);", hdr)
    assert re.search(r"\bint covo_sigma_adapt\(covo_handle_t h, const float \*L_in, const float \*C, int32_t batch, float gamma, "
                     r"float sample_sigma, float \*Sigma_out,\s+float \*L_out, float \*rows_out, void \*stream\);", hdr)
    fn = lib.covo_set_step_sigma_adapt
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_float, C.c_void_p, C.c_int32]
    fn = lib.covo_sigma_adapt
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float,
                                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for name in ("covo_set_step_sigma_adapt", "covo_sigma_adapt"):
        assert name in built.EXPORTS
    assert callable(built.check_sigma_adapt)
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()  # additive
    # a null handle is refused before anything else happens (no GPU needed)
    assert lib.covo_set_step_sigma_adapt(None, 0.2, None, 1) != 0 and b"null handle" in lib.covo_last_error()
    assert lib.covo_sigma_adapt(None, None, None, 1, 0.2, 0.5, None, None, None, None) != 0 and b"null handle" in lib.covo_last_error()


def test_sigma_adapt_is_a_keyword_defaulting_to_zero(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import Args, eval_env_batched, get_controller
    for fn in (SamplingCore.__init__, controllers.CoVOController.__init__, controllers.BatchedCoVOController.__init__, get_controller,
               eval_env_batched):
        p = inspect.signature(fn).parameters
        assert "sigma_adapt" in p and p["sigma_adapt"].default == 0.0, fn
    assert Args().sigma_adapt == 0.0
    assert callable(SamplingCore.sigma_adapt) and callable(SamplingCore.sigma_adapt_info)
    assert [built.check_sigma_adapt(g) for g in (0, 0.0, 0.2, np.float32(0.5))] == [0.0, 0.0, 0.2, 0.5]
    assert built.check_sigma_adapt(0.0, 1, "MPPI") == 0.0 and built.check_sigma_adapt(0.3, 2) == 0.3


def test_cli_and_eval_seeds_pass_the_switch_on():
    q = open(os.path.join(ROOT, "covo_mpc_amd", "envs", "quadrotor.py")).read()
    assert '"--sigma-adapt"' in q and "sigma_adapt=args.sigma_adapt" in q
    s = open(os.path.join(ROOT, "scripts", "eval_seeds.py")).read()
    assert '"--sigma-adapt"' in s and '"sigma_adapt"' in s


def _env(device=None):
    import covo_mpc_amd as cm
    return cm.envs.Quad3D(task="tracking_zigzag", disturb_type="gaussian", enable_randomizer=False, disable_rollover_terminate=True,
                          generate_noisy_state=True, device=device)


@pytest.mark.parametrize("bad", [1.0, -0.1, 1.5, float("nan"), None, "0.2", True, 1j])
def test_constructors_refuse_sigma_adapt_out_of_range(built, bad):
    """ValueError before anything is built: no device is needed."""
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    env = _env()
    with pytest.raises(ValueError, match="sigma_adapt="):
        SamplingCore(256, 32, 0.01, 1.0, sigma_period=2, sigma_adapt=bad)
    with pytest.raises(ValueError, match="sigma_adapt="):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, sigma_period=2, sigma_adapt=bad)
    with pytest.raises(ValueError, match="sigma_adapt="):
        controllers.CoVOController(env, None, 256, 32, 0.01, sigma_period=2, sigma_adapt=bad)
    with pytest.raises(ValueError, match="sigma_adapt="):
        eval_env_batched(env, 2, "N256_H32_lam0.01", sigma_period=2, sigma_adapt=bad)
    with pytest.raises(ValueError, match="sigma_adapt="):
        get_controller(env, "covo-online", "N256_H32_lam0.01", device="cpu", sigma_period=2, sigma_adapt=bad)


def test_a_period_of_one_refuses_sigma_adapt(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    env = _env()
    with pytest.raises(ValueError, match="sigma_adapt=0.2 with sigma_period=1"):
        SamplingCore(256, 32, 0.01, 1.0, sigma_adapt=0.2)
    with pytest.raises(ValueError, match="sigma_adapt=0.2 with sigma_period=1"):
        controllers.CoVOController(env, None, 256, 32, 0.01, sigma_adapt=0.2)
    with pytest.raises(ValueError, match="sigma_adapt=0.2 with sigma_period=1"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, sigma_adapt=0.2)
    with pytest.raises(ValueError, match="sigma_adapt=0.2 with sigma_period=1"):
        get_controller(env, "covo-online", "N256_H32_lam0.01", device="cpu", sigma_adapt=0.2)
    with pytest.raises(ValueError, match="sigma_adapt=0.2 with sigma_period=1"):
        eval_env_batched(env, 2, "N256_H32_lam0.01", sigma_adapt=0.2)


def test_modes_without_reuse_steps_refuse_sigma_adapt(built):
    """MPPI, covo-offline and the env-batched offline / MPPI controllers: ValueError in words, before anything is built."""
    from covo_mpc_amd import controllers
    from covo_mpc_amd.envs.quadrotor import get_controller
    env = _env()
    with pytest.raises(ValueError, match="sigma_adapt=0.2 with mppi"):
        get_controller(env, "mppi", "N256_H32_lam0.01", device="cpu", sigma_adapt=0.2)
    with pytest.raises(ValueError, match="sigma_adapt=0.2 with covo-offline"):
        get_controller(env, "covo-offline", "N256_H32_lam0.01", device="cpu", sigma_adapt=0.2)
    with pytest.raises(ValueError, match="sigma_adapt=0.2 with MPPI"):
        controllers.MPPIController(env, None, 256, 32, 0.01, sigma_adapt=0.2)
    with pytest.raises(ValueError, match="sigma_adapt=0.2 with offline"):
        controllers.CoVOController(env, None, 256, 32, 0.01, "offline", sigma_adapt=0.2)
    with pytest.raises(ValueError, match="sigma_adapt=0.2 with the env-batched covo-offline controller"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, mode="offline", sigma_adapt=0.2)
    with pytest.raises(ValueError, match="sigma_adapt=0.2 with the env-batched MPPI controller"):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, sigma_adapt=0.2)


def test_sigma_adapt_in_range_passes_the_keyword_check(built):
    """Without a device the construction gets as far as the device check (CovoError, not ValueError): the keyword was accepted."""
    import torch
    from covo_mpc_amd.envs.quadrotor import get_controller
    if not torch.cuda.is_available():
        with pytest.raises(built.CovoError, match="needs a ROCm GPU"):
            get_controller(_env(), "covo-online", "N256_H32_lam0.01", device="cpu", sigma_period=4, sigma_adapt=0.1)
        return
    c, _ = get_controller(_env("cuda:0"), "covo-online", "N256_H32_lam0.01", device="cuda:0", sigma_period=4, sigma_adapt=0.1)
    assert c.core.compute_post_cov and c.core.sigma_adapt_gamma == 0.1 and tuple(c.core.sigma_adapt_rows.shape) == (1, 4)
    assert set(c.core.sigma_adapt_info()) == {"sigma_adapt_fallback", "sigma_adapt_scale"}
    c.core.close()


def test_sharded_core_refuses_sigma_adapt_without_a_device(built, monkeypatch):
    """A process group of two ranks: NotImplementedError before the device is looked for.  (The Sigma period it needs is refused
    first, in the same words as without sigma_adapt.)"""
    import torch.distributed as dist
    from covo_mpc_amd.controllers._core import SamplingCore
    group = object()
    monkeypatch.setattr(dist, "get_world_size", lambda g=None: 2 if g is group else 1)
    monkeypatch.setattr(dist, "get_rank", lambda g=None: 0)
    with pytest.raises(NotImplementedError, match="on sample-sharded ranks"):
        SamplingCore(256, 32, 0.01, 1.0, process_group=group, sigma_period=2, sigma_adapt=0.2)
    with pytest.raises(ValueError, match="sigma_adapt="):  # the range check comes first
        SamplingCore(256, 32, 0.01, 1.0, process_group=group, sigma_period=2, sigma_adapt=1.0)


def test_debug_path_refuses_sigma_adapt(built):
    from covo_mpc_amd.controllers._core import SamplingCore

    class Stub:
        ess_min, compute_plan, compute_diag, compute_fan, arb_mask, update_rule, iters, elite, sigma_period, sigma_adapt_gamma = (
            0.0, False, False, 0, 0, "softmax", 1, 0, 1, 0.2)

    with pytest.raises(NotImplementedError, match="sigma_adapt=0.2 acts in the fused step"):
        SamplingCore.require_fused_for_diag(Stub())
    Stub.sigma_adapt_gamma = 0.0
    SamplingCore.require_fused_for_diag(Stub())  # off: the kernel-by-kernel path is free to run
