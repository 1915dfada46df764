"""CPU: the ABI of the posterior covariance (covo_set_step_post_cov / covo_weighted_cov, include/covo_hip.h), the `compute_post_cov`
keyword of the Python surface, and `ref_weighted_cov` (tests/post_cov_oracle.py), the fp64 restatement of the definition the GPU tests
compare against, on hand-derived answers."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)
from tests.post_cov_oracle import NA, ref_weighted_cov, ref_weights


def test_post_cov_entry_points_exist_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"#define COVO_HAS_POST_COV 1\b", hdr) and built.COVO_HAS_POST_COV == 1
    assert int(re.search(r"#define COVO_POST_AUX_FLOATS\s+(\d+)", hdr).group(1)) == 132 == built.COVO_POST_AUX_FLOATS
    P, I = C.c_void_p, C.c_int32
    want = {
        "covo_set_step_post_cov": [P, P, P, I],
        "covo_weighted_cov": [P, P, P, P, I, I, C.c_float, I, P, P, P],
    }
    for name, argtypes in want.items():
        assert re.search(r"\bint %s\(covo_handle_t h," % name, hdr), name
        fn = getattr(lib, name)  # the built library exports it
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        assert name in built.EXPORTS
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()  # additive: the ABI version did not move
    assert lib.covo_set_step_post_cov(None, None, None, 0) != 0 and b"null handle" in lib.covo_last_error()
    assert lib.covo_weighted_cov(None, None, None, None, 0, 0, 0.0, 0, None, None, None) != 0
    assert b"null handle" in lib.covo_last_error()


def test_compute_post_cov_is_a_keyword_defaulting_to_off(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import Args, get_controller
    for fn in (SamplingCore.__init__, controllers.MPPIController.__init__, controllers.CoVOController.__init__,
               controllers.BatchedCoVOController.__init__, controllers.BatchedMPPIController.__init__, get_controller):
        p = inspect.signature(fn).parameters
        assert "compute_post_cov" in p and p["compute_post_cov"].default is False, fn
    assert Args().post_cov is False
    assert callable(SamplingCore.weighted_cov) and callable(SamplingCore.post_cov_info)
    assert list(inspect.signature(SamplingCore.weighted_cov).parameters) == ["self", "a", "cost", "mu", "lam", "elite"]


def test_sharded_core_refuses_post_cov_without_a_device(built, monkeypatch):
    """A process group of two ranks: NotImplementedError, worded like compute_fan's, before the device is looked for."""
    import torch.distributed as dist
    from covo_mpc_amd.controllers._core import SamplingCore
    group = object()
    monkeypatch.setattr(dist, "get_world_size", lambda g=None: 2 if g is group else 1)
    monkeypatch.setattr(dist, "get_rank", lambda g=None: 0)
    with pytest.raises(NotImplementedError, match="compute_post_cov on sample-sharded ranks"):
        SamplingCore(256, 32, 0.01, 1.0, process_group=group, compute_post_cov=True)


def test_debug_path_refusal_is_worded_like_its_neighbours(built):
    from covo_mpc_amd.controllers._core import SamplingCore

    class Stub:
        ess_min, compute_plan, compute_diag, compute_fan, compute_post_cov = 0.0, False, False, 0, True

    with pytest.raises(NotImplementedError, match="compute_post_cov follows the fused step"):
        SamplingCore.require_fused_for_diag(Stub())
    Stub.compute_post_cov = False
    SamplingCore.require_fused_for_diag(Stub())  # nothing attached: the kernel-by-kernel path is free to run


def test_batched_fused_controllers_refuse_post_cov_without_a_device(built):
    """The env-batched MPPI / covo-offline step never puts its samples in HBM: NotImplementedError before anything is built."""
    from covo_mpc_amd import controllers
    with pytest.raises(NotImplementedError, match="compute_post_cov"):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, compute_post_cov=True)
    with pytest.raises(NotImplementedError, match="compute_post_cov"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, mode="offline", compute_post_cov=True)


# ------------------------------------------------------------------------------------------ the reference against hand-derived answers
def _random(N, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (32, N, 4)), rng.uniform(0, 3, N), rng.uniform(-0.5, 0.5, NA)


def test_ref_one_sample_gives_zero_exactly():
    a, cost, mu = _random(1, 0)
    for kw in (dict(lam=0.01), dict(elite=1)):
        C_, d, W, _ = ref_weighted_cov(a, cost, mu, **kw)
        assert W == 1.0 and np.all(C_ == 0.0)
        assert np.array_equal(d, a.transpose(1, 0, 2).reshape(NA) - mu)


def test_ref_two_equal_weights_give_rank_one():
    """x1, x2 with equal weights: C = (x1 - x2)(x1 - x2)^T / 4, whatever mu is."""
    a, _, mu = _random(2, 1)
    x = a.transpose(1, 0, 2).reshape(2, NA)
    want = np.outer(x[0] - x[1], x[0] - x[1]) / 4.0
    for kw in (dict(lam=0.5), dict(elite=2)):
        C_, d, W, _ = ref_weighted_cov(a, np.array([1.25, 1.25]), mu, **kw)
        assert W == 2.0
        assert np.abs(C_ - want).max() < 1e-15
        assert np.linalg.matrix_rank(C_, tol=1e-12) == 1
        assert np.abs(mu + d - x.mean(axis=0)).max() < 1e-15


def test_ref_one_hot_weights_give_zero():
    """A tiny lam leaves one sample with weight 1 (the others underflow to 0), elite = 1 selects it: C = 0, mu + d = that sample;
    NaN and +inf costs weigh 0 and never reach C."""
    a, cost, mu = _random(65, 2)
    cost[7] = -1.0
    cost[3], cost[11] = np.nan, np.inf
    a[:, 3, :] = np.nan
    x = a.transpose(1, 0, 2).reshape(65, NA)
    for kw in (dict(lam=1e-6), dict(elite=1)):
        C_, d, W, _ = ref_weighted_cov(a, cost, mu, **kw)
        assert W == 1.0 and np.all(C_ == 0.0) and np.array_equal(mu + d, mu + (x[7] - mu))
    w = ref_weights(cost, lam=1.0)
    assert w[3] == 0.0 and w[11] == 0.0 and w[7] == 1.0 and np.all(np.isfinite(w))


def test_ref_elite_ties_go_to_the_lowest_indices():
    cost = np.array([2.0, 1.0, 1.0, 1.0, 3.0, 1.0])
    assert np.array_equal(ref_weights(cost, elite=2), [0, 1, 1, 0, 0, 0])
    assert np.array_equal(ref_weights(cost, elite=4), [0, 1, 1, 1, 0, 1])
    assert np.array_equal(ref_weights(cost, elite=6), [1, 1, 1, 1, 1, 1])
