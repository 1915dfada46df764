"""CPU: the ABI of the Riccati box (covo_riccati_box / covo_riccati_refine_box / covo_set_step_riccati_box / covo_set_step_ilqr_box,
include/covo_hip.h: COVO_HAS_RICCATI_BOX) and the `riccati_box` switch of the Python surface (controllers/_options.py:
check_riccati_box -- a switch on top of riccati=, like riccati_feedback=, not a step option)."""
import ctypes as C
import inspect
import re

import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def _env(disturb="gaussian"):
    import covo_mpc_amd as cm
    return cm.envs.Quad3D(task="tracking_zigzag", disturb_type=disturb, enable_randomizer=False, disable_rollover_terminate=True,
                          generate_noisy_state=True, device=None)


def test_box_entry_points_exist_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"^#define COVO_HAS_RICCATI_BOX 1$", hdr, flags=re.M) and built.COVO_HAS_RICCATI_BOX == 1
    P, I, D = C.c_void_p, C.c_int32, C.c_double
    EP, F3 = C.POINTER(built.EnvParamsC), C.POINTER(C.c_float)
    want = {
        "covo_riccati_box": [P, P, P, P, I, EP, P, P, I, D, P, P, P, P, P, P, P],
        "covo_riccati_refine_box": [P, P, P, P, I, EP, F3, P, P, P, D, I, P, P, P, I, P, P],
        "covo_set_step_riccati_box": [P, P, I],
        "covo_set_step_ilqr_box": [P, P, I],
    }
    for name, argtypes in want.items():
        assert re.search(r"\bint %s\(covo_handle_t h," % name, hdr), name
        fn = getattr(lib, name)  # the built library exports it
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        assert name in built.EXPORTS
    # covo_riccati_box is covo_riccati plus masks_out, ahead of the stream
    assert list(lib.covo_riccati_box.argtypes)[:15] == list(lib.covo_riccati.argtypes)[:15]
    # additive: the ABI version did not move, the entry points it extends keep their arguments
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()
    assert len(lib.covo_riccati.argtypes) == 16 and len(lib.covo_riccati_refine.argtypes) == 15
    assert len(lib.covo_riccati_refine_feedback.argtypes) == 16 and len(lib.covo_set_step_ilqr.argtypes) == 5
    # a null handle is refused before anything else happens (no GPU needed)
    assert lib.covo_set_step_riccati_box(None, None, 1) != 0 and b"covo_set_step_riccati_box: null handle" in lib.covo_last_error()
    assert lib.covo_set_step_ilqr_box(None, None, 1) != 0 and b"covo_set_step_ilqr_box: null handle" in lib.covo_last_error()
    assert lib.covo_riccati_box(None, None, None, None, 0, None, None, None, 0, 1e-2, None, None, None, None, None, None, None) != 0
    assert b"covo_riccati_box: null handle" in lib.covo_last_error()
    assert lib.covo_riccati_refine_box(None, None, None, None, 0, None, None, None, None, None, 1e-2, 0, None, None, None, 0, None,
                                       None) != 0
    assert b"covo_riccati_refine_box: null handle" in lib.covo_last_error()


def test_riccati_box_is_a_switch_next_to_riccati_feedback(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import STEP_OPTION_DEFAULTS, check_riccati_box
    from covo_mpc_amd.envs.quadrotor import Args, eval_env_batched, get_controller
    assert "riccati_box" not in STEP_OPTION_DEFAULTS
    for fn in (SamplingCore.__init__, controllers.MPPIController.__init__, controllers.CoVOController.__init__,
               controllers.BatchedCoVOController.__init__, controllers.BatchedILQRController.__init__, get_controller,
               eval_env_batched):
        p = inspect.signature(fn).parameters
        assert "riccati_box" in p and p["riccati_box"].default is False, fn
    assert "riccati_box" not in inspect.signature(controllers.BatchedMPPIController.__init__).parameters
    # the single iLQR controller: its constructor's parameter list is a published one and stays; the switch is a class attribute, off
    # by default, on in ILQRBoxController, which get_controller(env, "ilqr", ..., riccati_box=True) builds
    assert controllers.ILQRController.riccati_box is False and controllers.ILQRBoxController.riccati_box is True
    assert issubclass(controllers.ILQRBoxController, controllers.ILQRController)
    assert (inspect.signature(controllers.ILQRBoxController.__init__) == inspect.signature(controllers.ILQRController.__init__)
            and "riccati_box" not in inspect.signature(controllers.ILQRController.__init__).parameters)
    assert Args().riccati_box is False
    assert inspect.signature(SamplingCore.riccati).parameters["box"].default is False
    assert inspect.signature(SamplingCore.riccati_refine).parameters["box"].default is False
    assert callable(SamplingCore.riccati_box_info)
    # off: nothing to object to; on: it needs the sweep
    assert check_riccati_box(False, riccati=False) is False and check_riccati_box(True, riccati=True) is True
    for bad in ("yes", 1, None, 0.0):
        with pytest.raises(ValueError, match="riccati_box="):
            check_riccati_box(bad, riccati=True)
        with pytest.raises(ValueError, match="riccati_box="):
            SamplingCore(256, 32, 0.01, 1.0, riccati=True, riccati_box=bad)
    with pytest.raises(ValueError, match="riccati_box=True with MPPI needs riccati=True"):
        check_riccati_box(True, riccati=False, what="MPPI")


def test_riccati_box_without_riccati_is_refused_everywhere(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    env = _env()
    with pytest.raises(ValueError, match="riccati_box=True with .* needs riccati=True"):
        SamplingCore(256, 32, 0.01, 1.0, riccati_box=True)
    for name in ("mppi", "covo-offline", "covo-online"):
        with pytest.raises(ValueError, match="riccati_box=True with .* needs riccati=True"):
            get_controller(env, name, "N256_H32_lam0.01", device="cpu", riccati_box=True)
    with pytest.raises(ValueError, match="riccati_box=True with .* needs riccati=True"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, riccati_box=True)
    with pytest.raises(ValueError, match="riccati_box=True with .* needs riccati=True"):
        eval_env_batched(env, 2, "N256_H32_lam0.01", n_steps=1, device="cpu", verbose=False, riccati_box=True)
    # whatever riccati refuses stays refused, ahead of the box
    with pytest.raises(ValueError, match="riccati=True together with refine=True"):
        get_controller(env, "covo-online", "N256_H32_lam0.01", device="cpu", refine=True, riccati=True, riccati_box=True)
    with pytest.raises(NotImplementedError, match="riccati=True with the env-batched covo-offline controller"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, mode="offline", riccati=True, riccati_box=True)
    for name in ("mppi", "covo-offline"):
        with pytest.raises(NotImplementedError, match="riccati=True with the env-batched"):
            eval_env_batched(env, 2, "N256_H32_lam0.01", n_steps=1, device="cpu", verbose=False, controller=name, riccati=True,
                             riccati_box=True)


def test_check_ilqr_accepts_the_keyword(built):
    from covo_mpc_amd.controllers._options import check_ilqr
    assert check_ilqr(3, riccati_box=True) == check_ilqr(3) == check_ilqr(3, riccati_box=False)
    assert check_ilqr(2, riccati_box=True, disturb_type="drag") == (2, False, 1)  # the 16-state plants take the box
    with pytest.raises(ValueError, match="riccati_box="):
        check_ilqr(2, riccati_box="yes")
    with pytest.raises(ValueError, match="plan_hold="):  # its place in the order: behind the plan hold
        check_ilqr(2, plan_hold=99, riccati_box="yes")


def test_riccati_box_goes_with_every_controller_that_takes_riccati(built):
    """accepted: the construction gets as far as the device check (no GPU), or builds (GPU)"""
    import torch
    from covo_mpc_amd.envs.quadrotor import get_controller
    for name, kw in (("mppi", dict(riccati=True)), ("covo-offline", dict(riccati=True)), ("covo-online", dict(riccati=True)),
                     ("covo-online", dict(riccati=True, riccati_feedback=True, plan_hold=2)), ("ilqr", dict(iters=3))):
        if torch.cuda.is_available():
            c, _ = get_controller(_env(), name, "N256_H32_lam0.01", device="cuda:0", riccati_box=True, **kw)
            assert c.core.riccati_box_on is True and tuple(c.core.riccati_box_masks.shape) == (1, 32)
            assert c.core.riccati_box_masks.dtype == torch.int32
            if name == "ilqr":
                assert type(c).__name__ == "ILQRBoxController" and tuple(c.core.ilqr_box_count.shape) == (1, 3)
            c.core.close()
        else:
            with pytest.raises(built.CovoError, match="needs a ROCm GPU"):
                get_controller(_env(), name, "N256_H32_lam0.01", device="cpu", riccati_box=True, **kw)
