"""CPU: the ABI of Riccati feedback (covo_feedback_rollout / covo_riccati_refine_feedback / covo_set_step_riccati_feedback,
include/covo_hip.h: COVO_HAS_RICCATI_FEEDBACK) and the `riccati_feedback` switch of the Python surface (controllers/_options.py:
check_riccati_feedback -- a switch on top of riccati=, not a step option)."""
import ctypes as C
import inspect
import re

import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def _env(disturb="gaussian"):
    import covo_mpc_amd as cm
    return cm.envs.Quad3D(task="tracking_zigzag", disturb_type=disturb, enable_randomizer=False, disable_rollover_terminate=True,
                          generate_noisy_state=True, device=None)


def test_feedback_entry_points_exist_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"^#define COVO_HAS_RICCATI_FEEDBACK 1$", hdr, flags=re.M) and built.COVO_HAS_RICCATI_FEEDBACK == 1
    assert int(re.search(r"#define COVO_FEEDBACK_FLOATS\s+(\d+)", hdr).group(1)) == 8 == built.COVO_FEEDBACK_FLOATS
    assert int(re.search(r"#define COVO_FEEDBACK_CANDIDATES\s+(\d+)", hdr).group(1)) == 33 == built.COVO_FEEDBACK_CANDIDATES
    assert built.COVO_FEEDBACK_CANDIDATES == 2 * built.COVO_REFINE_CANDIDATES - 1
    assert built.FEEDBACK_LADDER == tuple(2.0 ** (3 - j) for j in range(1, 17))
    P, I, D = C.c_void_p, C.c_int32, C.c_double
    EP, F3, DP = C.POINTER(built.EnvParamsC), C.POINTER(C.c_float), C.POINTER(C.c_double)
    want = {
        "covo_feedback_rollout": [P, P, P, P, I, EP, F3, P, P, P, P, P, DP, I, I, P, P, P],
        "covo_riccati_refine_feedback": [P, P, P, P, I, EP, F3, P, P, P, D, I, P, P, P, P],
        "covo_set_step_riccati_feedback": [P, P, I],
    }
    for name, argtypes in want.items():
        assert re.search(r"\bint %s\(covo_handle_t h," % name, hdr), name
        fn = getattr(lib, name)  # the built library exports it
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        assert name in built.EXPORTS
    # additive: the ABI version did not move, covo_riccati_refine keeps its 15 arguments and covo_newton_refine its 17
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()
    assert len(lib.covo_riccati_refine.argtypes) == 15 and len(lib.covo_newton_refine.argtypes) == 17
    assert built.COVO_REFINE_CANDIDATES == 17 and built.COVO_RICCATI_FLOATS == 8
    # a null handle is refused before anything else happens (no GPU needed)
    assert lib.covo_set_step_riccati_feedback(None, None, 1) != 0 and b"null handle" in lib.covo_last_error()
    assert lib.covo_feedback_rollout(None, None, None, None, 0, None, None, None, None, None, None, None, None, 0, 0, None, None, None) != 0
    assert b"covo_feedback_rollout: null handle" in lib.covo_last_error()
    assert lib.covo_riccati_refine_feedback(None, None, None, None, 0, None, None, None, None, None, 1e-2, 0, None, None, None, None) != 0
    assert b"covo_riccati_refine_feedback: null handle" in lib.covo_last_error()
    assert lib.covo_riccati_refine(None, None, None, None, 0, None, None, None, None, None, 1e-2, 0, None, None, None) != 0
    assert b"covo_riccati_refine: null handle" in lib.covo_last_error()


def test_riccati_feedback_is_a_switch_with_default_false(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers import _core
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import STEP_OPTION_DEFAULTS, check_riccati_feedback
    from covo_mpc_amd.envs.quadrotor import Args, eval_env_batched, get_controller
    assert "riccati_feedback" not in STEP_OPTION_DEFAULTS
    assert built.COVO_EPLOG_KINDS == 6 and not any("feedback" in k for k in _core.EPISODE_LOGS)  # no episode log of the rows
    for fn in (SamplingCore.__init__, controllers.MPPIController.__init__, controllers.CoVOController.__init__,
               controllers.BatchedCoVOController.__init__, get_controller, eval_env_batched):
        p = inspect.signature(fn).parameters
        assert "riccati_feedback" in p and p["riccati_feedback"].default is False, fn
        assert p["riccati"].default is False, fn  # the riccati keyword stays what it was
    assert "riccati_feedback" not in inspect.signature(controllers.BatchedMPPIController.__init__).parameters
    assert Args().riccati_feedback is False and Args().riccati is False
    assert callable(SamplingCore.feedback_rollout) and callable(SamplingCore.riccati_feedback_info)
    assert inspect.signature(SamplingCore.feedback_rollout).parameters["alphas"].default is None
    assert inspect.signature(SamplingCore.riccati_refine).parameters["feedback"].default is False
    # off: nothing to object to, whatever else is given
    assert check_riccati_feedback(False, riccati=False, disturb_type="drag", what="MPPI") is False
    for kind in (None, "none", "gaussian", "periodic", "sin"):
        assert check_riccati_feedback(True, riccati=True, disturb_type=kind, what="MPPI") is True


def test_check_riccati_feedback_objects_in_a_fixed_order(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import check_riccati_feedback
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    # 1. anything but a bool, whatever else is wrong
    for bad in ("yes", 1, None, 0.0):
        with pytest.raises(ValueError, match="riccati_feedback="):
            check_riccati_feedback(bad, riccati=False, disturb_type="drag", what="MPPI")
        with pytest.raises(ValueError, match="riccati_feedback="):
            SamplingCore(256, 32, 0.01, 1.0, riccati=True, riccati_feedback=bad)
    # 2. True without riccati=True, ahead of the plant's objection
    with pytest.raises(ValueError, match="needs riccati=True"):
        check_riccati_feedback(True, riccati=False, disturb_type="drag", what="MPPI")
    with pytest.raises(ValueError, match="needs riccati=True"):
        SamplingCore(256, 32, 0.01, 1.0, riccati_feedback=True)
    for name in ("mppi", "covo-offline", "covo-online"):
        with pytest.raises(ValueError, match="needs riccati=True"):
            get_controller(_env("drag"), name, "N256_H32_lam0.01", device="cpu", riccati_feedback=True)
    with pytest.raises(ValueError, match="needs riccati=True"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, riccati_feedback=True)
    with pytest.raises(ValueError, match="needs riccati=True"):
        eval_env_batched(_env(), 2, "N256_H32_lam0.01", n_steps=1, device="cpu", verbose=False, riccati_feedback=True)
    # 3. drag / mixed: the 16-state plants
    for kind in ("drag", "mixed"):
        with pytest.raises(NotImplementedError, match="16-state plants"):
            check_riccati_feedback(True, riccati=True, disturb_type=kind, what="MPPI")
        for name in ("mppi", "covo-online"):
            with pytest.raises(NotImplementedError, match=f"disturb_type='{kind}'"):
                get_controller(_env(kind), name, "N256_H32_lam0.01", device="cpu", riccati=True, riccati_feedback=True)
        with pytest.raises(NotImplementedError, match="16-state plants"):
            controllers.BatchedCoVOController(_env(kind), 3, 256, 32, 0.01, riccati=True, riccati_feedback=True)
    # riccati's own objections come first: its keyword and check stay what they were
    with pytest.raises(ValueError, match="riccati='yes'"):
        get_controller(_env(), "mppi", "N256_H32_lam0.01", device="cpu", riccati="yes", riccati_feedback=True)
    with pytest.raises(NotImplementedError, match="riccati=True with the env-batched"):
        eval_env_batched(_env(), 2, "N256_H32_lam0.01", n_steps=1, device="cpu", verbose=False, controller="mppi", riccati=True,
                         riccati_feedback=True)


def test_riccati_feedback_goes_with_every_single_controller(built):
    """accepted: the construction gets as far as the device check (no GPU), or builds (GPU)"""
    import torch
    from covo_mpc_amd.envs.quadrotor import get_controller
    for name, kw in (("mppi", {}), ("covo-offline", {}), ("covo-online", {}), ("covo-online", dict(sigma_period=4))):
        if torch.cuda.is_available():
            c, _ = get_controller(_env(), name, "N256_H32_lam0.01", device="cuda:0", riccati=True, riccati_feedback=True, **kw)
            assert c.core.riccati_feedback_on is True and tuple(c.core.riccati_feedback_rows.shape) == (1, 8)
            c.core.close()
        else:
            with pytest.raises(built.CovoError, match="needs a ROCm GPU"):
                get_controller(_env(), name, "N256_H32_lam0.01", device="cpu", riccati=True, riccati_feedback=True, **kw)
