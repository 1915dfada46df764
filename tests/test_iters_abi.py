"""CPU: the ABI of iterations per control step (covo_set_step_iters, include/covo_hip.h) and the `iters` keyword of the Python
surface."""
import ctypes as C
import inspect
import re

import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def test_iters_entry_point_exists_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"#define COVO_HAS_STEP_ITERS 1\b", hdr) and built.COVO_HAS_STEP_ITERS == 1
    assert int(re.search(r"#define COVO_MAX_STEP_ITERS\s+(\d+)", hdr).group(1)) == 16 == built.COVO_MAX_STEP_ITERS
    assert re.search(r"\bint covo_set_step_iters\(covo_handle_t h, int32_t iters, float \*iter_log, int32_t n_inst\);", hdr)
    fn = lib.covo_set_step_iters  # the built library exports it, _lib binds it
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
    assert "covo_set_step_iters" in built.EXPORTS
    # the ABI version did not move: the symbol is additive
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()
    # a null handle is refused before anything else happens (no GPU needed)
    assert lib.covo_set_step_iters(None, 2, None, 1) != 0 and b"null handle" in lib.covo_last_error()


def test_iters_is_a_keyword_defaulting_to_one(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import Args, eval_env_batched, get_controller
    for fn in (SamplingCore.__init__, controllers.MPPIController.__init__, controllers.CoVOController.__init__,
               controllers.BatchedCoVOController.__init__, controllers.BatchedMPPIController.__init__, get_controller,
               eval_env_batched):
        p = inspect.signature(fn).parameters
        assert "iters" in p and p["iters"].default == 1, fn
    assert Args().iters == 1
    assert callable(SamplingCore.iter_info)
    assert [built.check_iters(k) for k in (1, 2, 16)] == [1, 2, 16]


@pytest.mark.parametrize("bad", [0, 17, 2.5, -1, None, "2", True])
def test_constructors_refuse_iters_out_of_range(built, bad):
    """ValueError before anything is built: no device is needed."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    env = cm.envs.Quad3D(task="tracking_zigzag", disturb_type="gaussian", enable_randomizer=False, disable_rollover_terminate=True,
                         generate_noisy_state=True, device=None)
    with pytest.raises(ValueError, match="iters="):
        SamplingCore(256, 32, 0.01, 1.0, iters=bad)
    with pytest.raises(ValueError, match="iters="):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, iters=bad)
    with pytest.raises(ValueError, match="iters="):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, iters=bad)
    with pytest.raises(ValueError, match="iters="):
        eval_env_batched(env, 2, "N256_H32_lam0.01", iters=bad)
    for name in ("mppi", "covo-online", "covo-offline"):
        with pytest.raises(ValueError, match="iters="):
            get_controller(env, name, "N256_H32_lam0.01", device="cpu", iters=bad)


def test_iters_in_range_passes_the_keyword_check(built):
    """Without a device the construction gets as far as the device check (CovoError, not ValueError): the keyword was accepted."""
    import torch
    import covo_mpc_amd as cm
    from covo_mpc_amd.envs.quadrotor import get_controller
    env = cm.envs.Quad3D(task="tracking_zigzag", disturb_type="gaussian", enable_randomizer=False, disable_rollover_terminate=True,
                         generate_noisy_state=True, device="cuda:0" if torch.cuda.is_available() else None)
    if not torch.cuda.is_available():
        with pytest.raises(built.CovoError, match="needs a ROCm GPU"):
            get_controller(env, "mppi", "N256_H32_lam0.01", device="cpu", iters=2)
        return
    c, _ = get_controller(env, "mppi", "N256_H32_lam0.01", device="cuda:0")
    assert c.core.iters == 1 and c.core.iter_cost_min is None and c.core.iter_info() == {}
    c.core.close()
    c, _ = get_controller(env, "mppi", "N256_H32_lam0.01", device="cuda:0", iters=3)
    assert c.core.iters == 3 and tuple(c.core.iter_cost_min.shape) == (1, 3) and tuple(c.core.iter_info()["iter_cost_min"].shape) == (3,)
    c.core.close()


def test_sharded_core_refuses_iters_without_a_device(built, monkeypatch):
    """A process group of two ranks: NotImplementedError, worded like compute_fan's, before the device is looked for."""
    import torch.distributed as dist
    from covo_mpc_amd.controllers._core import SamplingCore
    group = object()
    monkeypatch.setattr(dist, "get_world_size", lambda g=None: 2 if g is group else 1)
    monkeypatch.setattr(dist, "get_rank", lambda g=None: 0)
    with pytest.raises(NotImplementedError, match="iters=2 on sample-sharded ranks"):
        SamplingCore(256, 32, 0.01, 1.0, process_group=group, iters=2)
    with pytest.raises(ValueError, match="iters="):  # the range check comes first
        SamplingCore(256, 32, 0.01, 1.0, process_group=group, iters=17)


def test_debug_path_refuses_iters(built):
    from covo_mpc_amd.controllers._core import SamplingCore

    class Stub:
        ess_min, compute_plan, compute_diag, compute_fan, arb_mask, update_rule, iters = 0.0, False, False, 0, 0, "softmax", 2

    with pytest.raises(NotImplementedError, match="iters=2 follows the fused step"):
        SamplingCore.require_fused_for_diag(Stub())
    Stub.iters = 1
    SamplingCore.require_fused_for_diag(Stub())  # one pass: the kernel-by-kernel path is free to run


def test_batched_fused_modes_refuse_iters_with_the_arbiter(built):
    """The env-batched MPPI / covo-offline launch keeps each pass's starting mean in LDS: iters > 1 together with the arbiter is
    refused there, in words, before anything is built."""
    from covo_mpc_amd import controllers
    with pytest.raises(NotImplementedError, match="iters=2 with update='guarded'"):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, iters=2, update="guarded")
    with pytest.raises(NotImplementedError, match="iters=2 with update='best'"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, iters=2, update="best", mode="offline")
