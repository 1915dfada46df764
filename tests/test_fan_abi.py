"""CPU: the ABI of the sample fan (covo_rollout_fan / covo_set_step_fan / covo_set_episode_fan, include/covo_hip.h) and the
`compute_fan` keyword of the Python surface."""
import ctypes as C
import inspect
import re

import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def test_fan_entry_points_exist_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"#define COVO_HAS_SAMPLE_FAN 1\b", hdr) and built.COVO_HAS_SAMPLE_FAN == 1
    assert int(re.search(r"#define COVO_FAN_FLOATS\s+(\d+)", hdr).group(1)) == 100 == built.COVO_FAN_FLOATS
    assert int(re.search(r"#define COVO_FAN_MAX\s+(\d+)", hdr).group(1)) == 64 == built.COVO_FAN_MAX
    assert built.COVO_FAN_FLOATS == built.COVO_PLAN_FLOATS == 4 + 3 * built.COVO_H  # the layout of a plan row
    P, I = C.c_void_p, C.c_int32
    want = {
        "covo_rollout_fan": [P, P, P, P, I, C.POINTER(built.EnvParamsC), C.POINTER(C.c_float), P, P, I, P, I, P, P],
        "covo_set_step_fan": [P, P, P, I, I],
        "covo_set_episode_fan": [P, P, I],
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
    assert lib.covo_set_step_fan(None, None, None, 0, 0) != 0 and b"null handle" in lib.covo_last_error()
    assert lib.covo_set_episode_fan(None, None, 0) != 0 and b"null handle" in lib.covo_last_error()
    assert lib.covo_rollout_fan(None, None, None, None, 0, None, None, None, None, 0, None, 0, None, None) != 0
    assert b"null handle" in lib.covo_last_error()


def test_compute_fan_is_a_keyword_defaulting_to_off(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import Args, BatchedDeviceEpisode, DeviceEpisode, eval_env_batched, get_controller
    for fn in (SamplingCore.__init__, controllers.MPPIController.__init__, controllers.CoVOController.__init__,
               controllers.BatchedCoVOController.__init__, controllers.BatchedMPPIController.__init__, get_controller):
        p = inspect.signature(fn).parameters
        assert "compute_fan" in p and p["compute_fan"].default is None, fn
    assert inspect.signature(eval_env_batched).parameters["fan"].default is None
    assert Args().fan == 0
    assert callable(SamplingCore.rollout_fan) and callable(DeviceEpisode.read_fan) and callable(BatchedDeviceEpisode.read_fan)


@pytest.mark.parametrize("K", [0, 65, 257, -1])
def test_constructors_refuse_a_fan_size_outside_1_64_or_above_N(built, K):
    """N = 256 everywhere, so 257 is K > N (and > 64); N = 32 with K = 48 is K > N alone.  ValueError before anything is built: no
    device is needed."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import get_controller
    env = cm.envs.Quad3D(task="tracking_zigzag", disturb_type="gaussian", enable_randomizer=False, disable_rollover_terminate=True,
                         generate_noisy_state=True, device=None)
    with pytest.raises(ValueError, match="compute_fan"):
        SamplingCore(256, 32, 0.01, 1.0, compute_fan=K)
    with pytest.raises(ValueError, match="compute_fan"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, compute_fan=K)
    with pytest.raises(ValueError, match="compute_fan"):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, compute_fan=K)
    for name in ("mppi", "covo-online", "covo-offline"):
        with pytest.raises(ValueError, match="compute_fan"):
            get_controller(env, name, "N256_H32_lam0.01", device="cpu", compute_fan=K)


def test_fan_size_above_N_alone(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    with pytest.raises(ValueError, match="> N=32"):
        SamplingCore(32, 32, 0.01, 1.0, compute_fan=48)
    with pytest.raises(ValueError, match="> N=32"):
        controllers.BatchedMPPIController(None, 3, 32, 32, 0.01, compute_fan=48)


def test_sharded_core_refuses_the_fan_without_a_device(built, monkeypatch):
    """A process group of two ranks: NotImplementedError, worded like compute_plan's, before the device is looked for."""
    import torch.distributed as dist
    from covo_mpc_amd.controllers._core import SamplingCore
    group = object()
    monkeypatch.setattr(dist, "get_world_size", lambda g=None: 2 if g is group else 1)
    monkeypatch.setattr(dist, "get_rank", lambda g=None: 0)
    with pytest.raises(NotImplementedError, match="compute_fan on sample-sharded ranks"):
        SamplingCore(256, 32, 0.01, 1.0, process_group=group, compute_fan=8)


def test_debug_path_refusal_is_worded_like_compute_plan(built):
    from covo_mpc_amd.controllers._core import SamplingCore

    class Stub:
        ess_min, compute_plan, compute_diag, compute_fan = 0.0, False, False, 8

    with pytest.raises(NotImplementedError, match="compute_fan follows the fused step"):
        SamplingCore.require_fused_for_diag(Stub())
    Stub.compute_fan = 0
    SamplingCore.require_fused_for_diag(Stub())  # nothing attached: the kernel-by-kernel path is free to run
