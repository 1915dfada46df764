"""CPU: the ABI of the Newton refinement (covo_cost_gradient / covo_newton_refine / covo_set_step_refine, include/covo_hip.h:
COVO_HAS_NEWTON_REFINE) and the `refine` switch of the Python surface -- a controller switch with a check of its own
(controllers/_options.py: check_refine), not a step option: the step options' table, the update masks and the ABI version stay."""
import ctypes as C
import inspect
import re

import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def _env():
    import covo_mpc_amd as cm
    return cm.envs.Quad3D(task="tracking_zigzag", disturb_type="gaussian", enable_randomizer=False, disable_rollover_terminate=True,
                          generate_noisy_state=True, device=None)


def _two_ranks(monkeypatch):
    """a process group of two ranks, as tests/test_options_abi.py patches it in"""
    import torch.distributed as dist
    group = object()
    monkeypatch.setattr(dist, "get_world_size", lambda g=None: 2 if g is group else 1)
    monkeypatch.setattr(dist, "get_rank", lambda g=None: 0)
    return group


def test_refine_entry_points_exist_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"^#define COVO_HAS_NEWTON_REFINE 1$", hdr, flags=re.M) and built.COVO_HAS_NEWTON_REFINE == 1
    assert int(re.search(r"#define COVO_REFINE_FLOATS\s+(\d+)", hdr).group(1)) == 8 == built.COVO_REFINE_FLOATS
    assert int(re.search(r"#define COVO_REFINE_CANDIDATES\s+(\d+)", hdr).group(1)) == 17 == built.COVO_REFINE_CANDIDATES
    P, I = C.c_void_p, C.c_int32
    EP, F3 = C.POINTER(built.EnvParamsC), C.POINTER(C.c_float)
    want = {
        "covo_cost_gradient": [P, P, P, P, I, EP, P, P, I, P, P],  # covo_hessian's
        "covo_newton_refine": [P, P, P, P, I, EP, F3, P, P, P, P, P, P, I, P, P, P],
        "covo_set_step_refine": [P, P, I],
    }
    for name, argtypes in want.items():
        assert re.search(r"\bint %s\(covo_handle_t h," % name, hdr), name
        fn = getattr(lib, name)  # the built library exports it
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        assert name in built.EXPORTS
    assert list(lib.covo_cost_gradient.argtypes) == list(lib.covo_hessian.argtypes)
    # the ABI version did not move: the symbols are additive
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()
    # a null handle is refused before anything else happens (no GPU needed)
    assert lib.covo_set_step_refine(None, None, 1) != 0 and b"null handle" in lib.covo_last_error()
    assert lib.covo_cost_gradient(None, None, None, None, 0, None, None, None, 0, None, None) != 0
    assert b"null handle" in lib.covo_last_error()
    assert lib.covo_newton_refine(None, None, None, None, 0, None, None, None, None, None, None, None, None, 0, None, None, None) != 0
    assert b"null handle" in lib.covo_last_error()


def test_refine_is_a_switch_not_a_step_option(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers import _core
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import STEP_OPTION_DEFAULTS, check_refine
    from covo_mpc_amd.envs.quadrotor import Args, eval_env_batched, get_controller
    assert list(STEP_OPTION_DEFAULTS) == ["compute_diag", "compute_plan", "ess_min", "compute_fan", "update", "iters", "elite",
                                          "sigma_period", "compute_post_cov", "sigma_adapt"]
    assert built.UPDATE_MASKS == {"softmax": 0, "best": 0b110, "guarded": 0b111}
    assert built.COVO_EPLOG_KINDS == 6 and not any("refine" in k for k in _core.EPISODE_LOGS)
    for fn in (SamplingCore.__init__, controllers.CoVOController.__init__, controllers.BatchedCoVOController.__init__, get_controller,
               eval_env_batched):
        p = inspect.signature(fn).parameters
        assert "refine" in p and p["refine"].default is False, fn
    assert Args().refine is False
    assert callable(SamplingCore.cost_gradient) and callable(SamplingCore.newton_refine) and callable(SamplingCore.refine_info)
    assert check_refine(False, "mppi", sigma_period=4, sharded=True) is False  # off: nothing to object to
    assert check_refine(True, "online") is True


@pytest.mark.parametrize("bad", ["yes", 1, None, 0.0])
def test_refine_must_be_a_bool(built, bad):
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import check_refine
    with pytest.raises(ValueError, match="refine="):
        check_refine(bad, "online")
    with pytest.raises(ValueError, match="refine="):
        SamplingCore(256, 32, 0.01, 1.0, refine=bad)


def test_refusals_need_no_device(built, monkeypatch):
    """MPPI, covo-offline and their env-batched controllers, a Sigma period: ValueError; sample-sharded ranks and the kernel-by-kernel
    path: NotImplementedError -- each before a device is looked for."""
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import check_refine
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    env = _env()
    # no Hessian-derived Sigma at the step's mean
    for name in ("mppi", "covo-offline"):
        with pytest.raises(ValueError, match="refine=True with .*only covo-online computes"):
            get_controller(env, name, "N256_H32_lam0.01", device="cpu", refine=True)
        with pytest.raises(ValueError, match="refine=True with .*only covo-online computes"):
            eval_env_batched(env, 2, "N256_H32_lam0.01", n_steps=1, device="cpu", verbose=False, controller=name, refine=True)
    with pytest.raises(ValueError, match="refine=True with covo-offline"):
        controllers.CoVOController(env, None, 256, 32, 0.01, "offline", refine=True)
    for staged in (False, True):
        with pytest.raises(ValueError, match="refine=True with the env-batched covo-offline controller"):
            controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, mode="offline", staged=staged, refine=True)
    assert "refine" not in inspect.signature(controllers.BatchedMPPIController.__init__).parameters
    assert "refine" not in inspect.signature(controllers.MPPIController.__init__).parameters
    with pytest.raises(ValueError, match="refine=True with the env-batched MPPI controller"):
        check_refine(True, "the env-batched MPPI controller")
    # a reuse step has no R
    with pytest.raises(ValueError, match="refine=True with sigma_period=4"):
        SamplingCore(256, 32, 0.01, 1.0, sigma_period=4, refine=True)
    with pytest.raises(ValueError, match="refine=True with sigma_period=2"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, sigma_period=2, refine=True)
    with pytest.raises(ValueError, match="refine=True with sigma_period=2"):
        get_controller(env, "covo-online", "N256_H32_lam0.01", device="cpu", sigma_period=2, refine=True)
    with pytest.raises(ValueError, match="refine=True with sigma_period=2"):
        controllers.CoVOController(env, None, 256, 32, 0.01, "online", sigma_period=2, refine=True)
    # sample-sharded ranks
    group = _two_ranks(monkeypatch)
    with pytest.raises(NotImplementedError, match="refine=True on sample-sharded ranks"):
        SamplingCore(256, 32, 0.01, 1.0, process_group=group, refine=True)
    with pytest.raises(NotImplementedError, match="refine=True on sample-sharded ranks"):
        get_controller(env, "covo-online", "N256_H32_lam0.01", device="cpu", process_group=group, refine=True)

    # the kernel-by-kernel path
    class Stub:
        refine = True

    with pytest.raises(NotImplementedError, match="refine follows the fused step"):
        SamplingCore.require_fused_for_diag(Stub())
    Stub.refine = False
    SamplingCore.require_fused_for_diag(Stub())  # off: the kernel-by-kernel path is free to run


def test_refine_off_attaches_nothing(built):
    """refine=False passes the check; without a device the construction gets as far as the device check, with one the core has no
    refine buffer and its info has no refine_* keys."""
    import torch
    import covo_mpc_amd as cm
    from covo_mpc_amd.envs.quadrotor import get_controller
    if not torch.cuda.is_available():
        with pytest.raises(built.CovoError, match="needs a ROCm GPU"):
            get_controller(_env(), "covo-online", "N256_H32_lam0.01", device="cpu", refine=True)  # (accepted: it got to the device)
        return
    env = cm.envs.Quad3D(task="tracking_zigzag", disturb_type="gaussian", enable_randomizer=False, disable_rollover_terminate=True,
                         generate_noisy_state=True, device="cuda:0")
    c, _ = get_controller(env, "covo-online", "N256_H32_lam0.01", device="cuda:0")
    assert c.core.refine is False and c.core.refine_rows is None and c.core.refine_info() == {}
    c.core.close()
