"""CPU: the ABI of the ESS floor (covo_set_step_ess_floor / covo_ess_lambda, include/covo_hip.h) and the `ess_min` keyword of the
Python surface, including the two env-batched modes that refuse it before anything touches a GPU."""
import ctypes as C
import inspect
import re

import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def test_header_declares_the_prototypes_and_macros(built):
    hdr = header_text()
    assert re.search(r"int covo_set_step_ess_floor\(covo_handle_t h, float ess_min, float \*lam_out, int32_t n_inst\);", hdr)
    assert re.search(r"int covo_ess_lambda\(covo_handle_t h, const float \*cost, int32_t n_samples, int32_t n_inst, float lam0, "
                     r"float ess_min, float \*out, void \*stream\);", hdr)
    assert re.search(r"#define COVO_HAS_ESS_FLOOR 1\b", hdr)
    assert int(re.search(r"#define COVO_LAM_FLOATS\s+(\d+)", hdr).group(1)) == 4 == built.COVO_LAM_FLOATS


def test_symbols_are_exported_with_the_declared_types(built):
    lib = built.load_library()
    fn = lib.covo_set_step_ess_floor
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_float, C.c_void_p, C.c_int32]
    fn = lib.covo_ess_lambda
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                                            C.c_void_p, C.c_void_p]
    assert "covo_set_step_ess_floor" in built.EXPORTS and "covo_ess_lambda" in built.EXPORTS


def test_null_handle_is_an_error_with_a_message(built):
    lib = built.load_library()
    assert lib.covo_set_step_ess_floor(None, 8.0, None, 0) != 0
    assert b"covo_set_step_ess_floor" in lib.covo_last_error() and b"null handle" in lib.covo_last_error()
    assert lib.covo_ess_lambda(None, None, 16, 1, 0.01, 4.0, None, None) != 0
    assert b"covo_ess_lambda" in lib.covo_last_error() and b"null handle" in lib.covo_last_error()


def test_abi_version_did_not_move(built):
    lib = built.load_library()
    hdr = header_text()
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()


def test_ess_min_is_a_keyword_defaulting_to_none(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import get_controller
    for fn in (SamplingCore.__init__, controllers.MPPIController.__init__, controllers.CoVOController.__init__,
               controllers.BatchedCoVOController.__init__, controllers.BatchedMPPIController.__init__, get_controller):
        p = inspect.signature(fn).parameters
        assert "ess_min" in p and p["ess_min"].default is None, fn


def test_refused_batched_modes_raise_without_a_gpu(built):
    """BatchedMPPIController and BatchedCoVOController(mode="offline") have one fused launch per step: the constructor refuses
    ess_min before it creates a handle."""
    from covo_mpc_amd import controllers
    with pytest.raises(NotImplementedError, match="ess_min"):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, ess_min=32.0)
    with pytest.raises(NotImplementedError, match="ess_min"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, mode="offline", ess_min=32.0)
