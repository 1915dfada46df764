"""CPU: the ABI of the elite-set update (covo_set_step_elite / covo_elite_select, include/covo_hip.h) and the `elite` keyword of the
Python surface: what _lib.check_elite accepts and refuses, and every refusal a constructor makes before anything touches a GPU."""
import ctypes as C
import inspect
import re
import types

import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def test_header_declares_the_prototypes_and_macros(built):
    hdr = header_text()
    assert re.search(r"int covo_set_step_elite\(covo_handle_t h, int32_t K, float \*rows_out, int32_t n_inst\);", hdr)
    assert re.search(r"int covo_elite_select\(covo_handle_t h, const float \*cost, int32_t n_samples, int32_t n_inst, int32_t K, "
                     r"float \*out, void \*stream\);", hdr)
    assert re.search(r"#define COVO_HAS_ELITE_UPDATE 1\b", hdr)
    assert int(re.search(r"#define COVO_ELITE_FLOATS\s+(\d+)", hdr).group(1)) == 8 == built.COVO_ELITE_FLOATS


def test_symbols_are_exported_with_the_declared_types(built):
    lib = built.load_library()
    fn = lib.covo_set_step_elite
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
    fn = lib.covo_elite_select
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                            C.c_void_p]
    assert "covo_set_step_elite" in built.EXPORTS and "covo_elite_select" in built.EXPORTS


def test_null_handle_is_an_error_with_a_message(built):
    lib = built.load_library()
    assert lib.covo_set_step_elite(None, 8, None, 0) != 0
    assert b"covo_set_step_elite" in lib.covo_last_error() and b"null handle" in lib.covo_last_error()
    assert lib.covo_elite_select(None, None, 16, 1, 4, None, None) != 0
    assert b"covo_elite_select" in lib.covo_last_error() and b"null handle" in lib.covo_last_error()


def test_abi_version_did_not_move(built):
    lib = built.load_library()
    hdr = header_text()
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()


def test_check_elite_accepts_and_refuses(built):
    ce = built.check_elite
    for off in (None, False, 0):
        assert ce(off, 256) == 0
        assert ce(off, 256, 32.0) == 0  # off next to an ESS floor is fine
    assert ce(1, 256) == 1 and ce(256, 256) == 256 and ce(32, 256, None) == 32 and ce(32, 256, 0.0) == 32
    import numpy as np
    assert ce(np.int64(16), 256) == 16
    for bad in (-1, 257, 1.5, 32.0, "8", True):
        with pytest.raises(ValueError, match="elite="):
            ce(bad, 256)
    with pytest.raises(ValueError, match="ess_min"):
        ce(32, 256, 16.0)
    # MPPI's full refit from fewer than 5 elites is singular
    for K in (1, 4):
        with pytest.raises(ValueError, match="gamma_sigma"):
            ce(K, 256, None, 1.0)
    assert ce(5, 256, None, 1.0) == 5 and ce(4, 256, None, 0.99) == 4 and ce(1, 256, None, 0.0) == 1


def test_elite_is_a_keyword_defaulting_to_none(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    for fn in (SamplingCore.__init__, controllers.MPPIController.__init__, controllers.CoVOController.__init__,
               controllers.BatchedCoVOController.__init__, controllers.BatchedMPPIController.__init__, get_controller,
               eval_env_batched):
        p = inspect.signature(fn).parameters
        assert "elite" in p and p["elite"].default is None, fn
    from covo_mpc_amd.envs.quadrotor import Args
    assert Args().elite == 0


def test_constructors_raise_value_errors_without_a_gpu(built):
    """Every ValueError of the keyword is raised before a handle is created (no device is looked for)."""
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    cp = types.SimpleNamespace(gamma_sigma=0.0, discount=1.0)
    cp_full = types.SimpleNamespace(gamma_sigma=1.0, discount=1.0)
    for make in (lambda **kw: SamplingCore(256, 32, 0.01, 1.0, **kw),
                 lambda **kw: controllers.MPPIController(None, cp, 256, 32, 0.01, **kw),
                 lambda **kw: controllers.CoVOController(None, cp, 256, 32, 0.01, "online", **kw),
                 lambda **kw: controllers.CoVOController(None, cp, 256, 32, 0.01, "offline", **kw),
                 lambda **kw: controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, **kw),
                 lambda **kw: controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, **kw)):
        with pytest.raises(ValueError, match="elite=257"):
            make(elite=257)
        with pytest.raises(ValueError, match="elite=-1"):
            make(elite=-1)
        with pytest.raises(ValueError, match="ess_min"):
            make(elite=32, ess_min=16.0)
    with pytest.raises(ValueError, match="gamma_sigma"):
        controllers.MPPIController(None, cp_full, 256, 32, 0.01, elite=4)


def test_refused_batched_modes_raise_without_a_gpu(built):
    """BatchedMPPIController and BatchedCoVOController(mode="offline") have one fused launch per step: the constructor refuses
    elite before it creates a handle."""
    from covo_mpc_amd import controllers
    with pytest.raises(NotImplementedError, match="elite"):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, elite=32)
    with pytest.raises(NotImplementedError, match="elite"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, mode="offline", elite=32)


def test_kernel_by_kernel_path_refuses_elite(built):
    from covo_mpc_amd.controllers._core import SamplingCore

    class Fake:
        ess_min, compute_plan, compute_diag, compute_fan, arb_mask, update_rule, iters, elite = 0.0, False, False, 0, 0, "softmax", 1, 32
    with pytest.raises(NotImplementedError, match="elite=32"):
        SamplingCore.require_fused_for_diag(Fake())
