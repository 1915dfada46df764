"""CPU: the ABI of the update arbiter (covo_arbitrate / covo_set_step_arbiter / covo_set_episode_arbiter_log, include/covo_hip.h) and
the `update` keyword of the Python surface."""
import ctypes as C
import inspect
import re

import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def test_arbiter_entry_points_exist_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"#define COVO_HAS_UPDATE_ARBITER 1\b", hdr) and built.COVO_HAS_UPDATE_ARBITER == 1
    assert int(re.search(r"#define COVO_ARB_FLOATS\s+(\d+)", hdr).group(1)) == 8 == built.COVO_ARB_FLOATS
    P, I = C.c_void_p, C.c_int32
    want = {
        "covo_set_step_arbiter": [P, P, I, I],
        "covo_set_episode_arbiter_log": [P, P, I],
        "covo_arbitrate": [P, P, P, P, I, C.POINTER(built.EnvParamsC), C.POINTER(C.c_float), P, P, P, I, P, P, I, P, P],
    }
    for name, argtypes in want.items():
        assert re.search(r"\bint %s\(covo_handle_t h," % name, hdr), name
        fn = getattr(lib, name)  # the built library exports it
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        assert name in built.EXPORTS
    # the ABI version did not move: the symbols are additive
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()
    # a null handle is refused before anything else happens (no GPU needed)
    assert lib.covo_set_step_arbiter(None, None, 7, 1) != 0 and b"null handle" in lib.covo_last_error()
    assert lib.covo_set_episode_arbiter_log(None, None, 0) != 0 and b"null handle" in lib.covo_last_error()
    assert lib.covo_arbitrate(None, None, None, None, 0, None, None, None, None, None, 0, None, None, 7, None, None) != 0
    assert b"null handle" in lib.covo_last_error()


def test_update_is_a_keyword_defaulting_to_softmax(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import Args, BatchedDeviceEpisode, DeviceEpisode, eval_env_batched, get_controller
    for fn in (SamplingCore.__init__, controllers.MPPIController.__init__, controllers.CoVOController.__init__,
               controllers.BatchedCoVOController.__init__, controllers.BatchedMPPIController.__init__, get_controller,
               eval_env_batched):
        p = inspect.signature(fn).parameters
        assert "update" in p and p["update"].default == "softmax", fn
    assert inspect.signature(eval_env_batched).parameters["arbiter"].default is False
    assert Args().update == "softmax"
    assert built.UPDATE_MASKS == {"softmax": 0, "best": 0b110, "guarded": 0b111}
    assert callable(SamplingCore.update) and callable(SamplingCore.arbitrate) and callable(DeviceEpisode.read_arbiter) and callable(BatchedDeviceEpisode.read_arbiter)


@pytest.mark.parametrize("bad", ["nonsense", "", "Best", None, 7])
def test_constructors_refuse_an_unknown_update_rule(built, bad):
    """ValueError before anything is built: no device is needed."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import get_controller
    env = cm.envs.Quad3D(task="tracking_zigzag", disturb_type="gaussian", enable_randomizer=False, disable_rollover_terminate=True,
                         generate_noisy_state=True, device=None)
    with pytest.raises(ValueError, match="update="):
        SamplingCore(256, 32, 0.01, 1.0, update=bad)
    with pytest.raises(ValueError, match="update="):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, update=bad)
    with pytest.raises(ValueError, match="update="):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, update=bad)
    for name in ("mppi", "covo-online", "covo-offline"):
        with pytest.raises(ValueError, match="update="):
            get_controller(env, name, "N256_H32_lam0.01", device="cpu", update=bad)


def test_softmax_attaches_nothing(built):
    """update="softmax" passes the keyword check and builds a controller whose core has no arbiter buffer.  Without a device the
    construction gets as far as the device check (CovoError, not ValueError): the keyword was accepted."""
    import torch
    import covo_mpc_amd as cm
    from covo_mpc_amd.envs.quadrotor import get_controller
    assert built.check_update("softmax") == 0 and built.check_update("best") == 6 and built.check_update("guarded") == 7
    env = cm.envs.Quad3D(task="tracking_zigzag", disturb_type="gaussian", enable_randomizer=False, disable_rollover_terminate=True,
                         generate_noisy_state=True, device="cuda:0" if torch.cuda.is_available() else None)
    if not torch.cuda.is_available():
        with pytest.raises(built.CovoError, match="needs a ROCm GPU"):
            get_controller(env, "mppi", "N256_H32_lam0.01", device="cpu", update="softmax")
        return
    c, _ = get_controller(env, "mppi", "N256_H32_lam0.01", device="cuda:0", update="softmax")
    assert c.core.arbiter is None and c.core.arb_mask == 0 and c.core.arbiter_info() == {}
    c.core.close()


def test_sharded_core_refuses_the_arbiter_without_a_device(built, monkeypatch):
    """A process group of two ranks: NotImplementedError, worded like compute_fan's, before the device is looked for."""
    import torch.distributed as dist
    from covo_mpc_amd.controllers._core import SamplingCore
    group = object()
    monkeypatch.setattr(dist, "get_world_size", lambda g=None: 2 if g is group else 1)
    monkeypatch.setattr(dist, "get_rank", lambda g=None: 0)
    with pytest.raises(NotImplementedError, match="update='guarded' on sample-sharded ranks"):
        SamplingCore(256, 32, 0.01, 1.0, process_group=group, update="guarded")


def test_debug_path_refuses_the_arbiter(built):
    from covo_mpc_amd.controllers._core import SamplingCore

    class Stub:
        ess_min, compute_plan, compute_diag, compute_fan, arb_mask, update_rule = 0.0, False, False, 0, 6, "best"

    with pytest.raises(NotImplementedError, match="update='best' follows the fused step"):
        SamplingCore.require_fused_for_diag(Stub())
    Stub.arb_mask = 0
    SamplingCore.require_fused_for_diag(Stub())  # nothing attached: the kernel-by-kernel path is free to run
