"""CPU: the ABI of the per-step sampling diagnostics (covo_set_step_diag / covo_set_episode_diag_log, include/covo_hip.h) and the
`compute_diag` keyword of the Python surface."""
import ctypes as C
import inspect
import re

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def test_diag_entry_points_exist_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"int covo_set_step_diag\(covo_handle_t h, float \*diag, int32_t n_inst\);", hdr)
    assert re.search(r"int covo_set_episode_diag_log\(covo_handle_t h, float \*log, int32_t stride\);", hdr)
    for name in ("covo_set_step_diag", "covo_set_episode_diag_log"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_int32], name
        assert name in built.EXPORTS
    # a null handle is refused before anything else happens (no GPU needed)
    assert lib.covo_set_step_diag(None, None, 0) != 0 and b"null handle" in lib.covo_last_error()
    assert lib.covo_set_episode_diag_log(None, None, 0) != 0 and b"null handle" in lib.covo_last_error()


def test_abi_10_everywhere(built):
    hdr = header_text()
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == built.load_library().covo_abi_version()
    assert int(re.search(r"#define COVO_DIAG_FLOATS (\d+)", hdr).group(1)) == 8 == built.COVO_DIAG_FLOATS


def test_existing_structs_are_unchanged(built):
    assert C.sizeof(built.BatchArgsC) == 88 and C.sizeof(built.BatchModeArgsC) == 120


def test_compute_diag_is_a_keyword_defaulting_to_false(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    for fn in (SamplingCore.__init__, controllers.MPPIController.__init__, controllers.CoVOController.__init__,
               controllers.BatchedCoVOController.__init__, controllers.BatchedMPPIController.__init__, get_controller):
        p = inspect.signature(fn).parameters
        assert "compute_diag" in p and p["compute_diag"].default is False, fn
    assert inspect.signature(eval_env_batched).parameters["diag"].default is False
