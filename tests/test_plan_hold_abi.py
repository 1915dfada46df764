"""CPU: the ABI of the plan hold (covo_set_step_plan_hold / covo_step_plan_age / covo_plan_hold / covo_set_episode_hold_log,
include/covo_hip.h: COVO_HAS_PLAN_HOLD) and the `plan_hold` switch of the Python surface (controllers/_options.py: check_plan_hold -- a
switch on top of riccati=, not a step option)."""
import ctypes as C
import inspect
import re

import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def _env(disturb="gaussian"):
    import covo_mpc_amd as cm
    return cm.envs.Quad3D(task="tracking_zigzag", disturb_type=disturb, enable_randomizer=False, disable_rollover_terminate=True,
                          generate_noisy_state=True, device=None)


def test_plan_hold_entry_points_exist_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"^#define COVO_HAS_PLAN_HOLD 1$", hdr, flags=re.M) and built.COVO_HAS_PLAN_HOLD == 1
    assert int(re.search(r"#define COVO_HOLD_FLOATS\s+(\d+)", hdr).group(1)) == 8 == built.COVO_HOLD_FLOATS
    assert int(re.search(r"#define COVO_MAX_PLAN_HOLD\s+(\d+)", hdr).group(1)) == 16 == built.COVO_MAX_PLAN_HOLD
    P, I, IP = C.c_void_p, C.c_int32, C.POINTER(C.c_int32)
    want = {
        "covo_set_step_plan_hold": [P, I, P, I],
        "covo_step_plan_age": [P, IP, IP],
        "covo_plan_hold": [P, P, P, P, P, P, P, P, I, I, P, P, P, P, P, I, P],
        "covo_set_episode_hold_log": [P, P, I],
    }
    for name, argtypes in want.items():
        assert re.search(r"\bint %s\(covo_handle_t h," % name, hdr), name
        fn = getattr(lib, name)  # the built library exports it
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        assert name in built.EXPORTS
    # additive: the ABI version did not move, the episode logs' kinds and the generator's entry stay what they were
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()
    assert built.COVO_EPLOG_KINDS == 6 and len(lib.covo_feedback_rollout.argtypes) == 18
    # a null handle is refused by name before anything else happens (no GPU needed)
    assert lib.covo_set_step_plan_hold(None, 3, None, 1) != 0 and b"covo_set_step_plan_hold: null handle" in lib.covo_last_error()
    assert lib.covo_step_plan_age(None, None, None) != 0 and b"covo_step_plan_age: null handle" in lib.covo_last_error()
    assert lib.covo_plan_hold(None, None, None, None, None, None, None, None, 0, 0, None, None, None, None, None, 0, None) != 0
    assert b"covo_plan_hold: null handle" in lib.covo_last_error()
    assert lib.covo_set_episode_hold_log(None, None, 0) != 0 and b"covo_set_episode_hold_log: null handle" in lib.covo_last_error()


def test_plan_hold_is_a_switch_with_default_one(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers import _core
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import STEP_OPTION_DEFAULTS, check_plan_hold
    from covo_mpc_amd.envs.quadrotor import Args, _EpisodeLogs, eval_env_batched, get_controller
    assert "plan_hold" not in STEP_OPTION_DEFAULTS
    # the hold log is bound next to the episode logs, not one of them
    assert not any("hold" in k for k in _core.EPISODE_LOGS) and not any("hold" in k for k in _EpisodeLogs.LOGS)
    assert callable(_EpisodeLogs.read_hold) and callable(SamplingCore.attach_hold_log)
    for fn in (SamplingCore.__init__, controllers.MPPIController.__init__, controllers.CoVOController.__init__,
               controllers.BatchedCoVOController.__init__, get_controller, eval_env_batched):
        p = inspect.signature(fn).parameters
        assert "plan_hold" in p and p["plan_hold"].default == 1 and isinstance(p["plan_hold"].default, int), fn
        assert p["riccati"].default is False and p["riccati_feedback"].default is False, fn  # the neighbours stay what they were
    assert "plan_hold" not in inspect.signature(controllers.BatchedMPPIController.__init__).parameters
    assert Args().plan_hold == 1
    assert callable(SamplingCore.plan_hold) and callable(SamplingCore.plan_hold_info) and callable(SamplingCore.restart_plan_hold)
    assert inspect.signature(SamplingCore.plan_hold).parameters["t_plan"].default is None
    # off: nothing to object to, whatever else is given
    assert check_plan_hold(1, riccati=False, sigma_period=4, disturb_type="drag", what="MPPI") == 1
    for m in (2, 3, 16):
        for kind in (None, "none", "gaussian", "periodic", "sin"):
            assert check_plan_hold(m, riccati=True, disturb_type=kind, what="MPPI") == m


def test_check_plan_hold_objects_in_a_fixed_order(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import check_plan_hold
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    # 1. not an integer in [1, 16], whatever else is wrong
    for bad in (0, 17, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="plan_hold="):
            check_plan_hold(bad, riccati=False, sigma_period=4, disturb_type="drag", what="MPPI")
        with pytest.raises(ValueError, match="plan_hold="):
            SamplingCore(256, 32, 0.01, 1.0, riccati=True, plan_hold=bad)
    # 2. m > 1 without riccati=True, ahead of the Sigma period's and the plant's objections
    with pytest.raises(ValueError, match="needs riccati=True"):
        check_plan_hold(3, riccati=False, sigma_period=4, disturb_type="drag", what="MPPI")
    with pytest.raises(ValueError, match="needs riccati=True"):
        SamplingCore(256, 32, 0.01, 1.0, plan_hold=3)
    for name in ("mppi", "covo-offline", "covo-online"):
        with pytest.raises(ValueError, match="needs riccati=True"):
            get_controller(_env("drag"), name, "N256_H32_lam0.01", device="cpu", plan_hold=3)
    with pytest.raises(ValueError, match="needs riccati=True"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, plan_hold=3)
    with pytest.raises(ValueError, match="needs riccati=True"):
        eval_env_batched(_env(), 2, "N256_H32_lam0.01", n_steps=1, device="cpu", verbose=False, plan_hold=3)
    # 3. together with a Sigma period, ahead of the plant's objection
    with pytest.raises(ValueError, match="with sigma_period=4"):
        check_plan_hold(3, riccati=True, sigma_period=4, disturb_type="drag", what="covo-online")
    with pytest.raises(ValueError, match="with sigma_period=4"):
        SamplingCore(256, 32, 0.01, 1.0, riccati=True, sigma_period=4, plan_hold=3)
    with pytest.raises(ValueError, match="with sigma_period=4"):
        get_controller(_env("drag"), "covo-online", "N256_H32_lam0.01", device="cpu", riccati=True, sigma_period=4, plan_hold=3)
    with pytest.raises(ValueError, match="with sigma_period=4"):
        controllers.BatchedCoVOController(_env(), 3, 256, 32, 0.01, riccati=True, sigma_period=4, plan_hold=3)
    # 4. drag / mixed: the 16-state plants
    for kind in ("drag", "mixed"):
        with pytest.raises(NotImplementedError, match="16-state plants"):
            check_plan_hold(3, riccati=True, disturb_type=kind, what="MPPI")
        for name in ("mppi", "covo-offline", "covo-online"):
            with pytest.raises(NotImplementedError, match=f"plan_hold=3 with disturb_type='{kind}'"):
                get_controller(_env(kind), name, "N256_H32_lam0.01", device="cpu", riccati=True, plan_hold=3)
        with pytest.raises(NotImplementedError, match="16-state plants"):
            controllers.BatchedCoVOController(_env(kind), 3, 256, 32, 0.01, riccati=True, plan_hold=3)
    # 5. whatever riccati= refuses stays refused, with riccati's own message
    with pytest.raises(ValueError, match="riccati='yes'"):
        get_controller(_env(), "mppi", "N256_H32_lam0.01", device="cpu", riccati="yes", plan_hold=3)
    with pytest.raises(NotImplementedError, match="riccati=True with the env-batched"):
        eval_env_batched(_env(), 2, "N256_H32_lam0.01", n_steps=1, device="cpu", verbose=False, controller="mppi", riccati=True,
                         plan_hold=3)
    with pytest.raises(ValueError, match="riccati=True together with refine=True"):
        get_controller(_env(), "covo-online", "N256_H32_lam0.01", device="cpu", riccati=True, refine=True, plan_hold=3)


def test_plan_hold_goes_with_every_single_controller(built):
    """accepted: the construction gets as far as the device check (no GPU), or builds (GPU)"""
    import torch
    from covo_mpc_amd.envs.quadrotor import get_controller
    for name, kw in (("mppi", {}), ("covo-offline", {}), ("covo-online", {}), ("covo-online", dict(iters=2, riccati_feedback=True))):
        if torch.cuda.is_available():
            c, _ = get_controller(_env(), name, "N256_H32_lam0.01", device="cuda:0", riccati=True, plan_hold=3, **kw)
            assert c.core.plan_hold_period == 3 and tuple(c.core.plan_hold_rows.shape) == (1, 8) and c.core.plan_age == 0
            c.core.close()
        else:
            with pytest.raises(built.CovoError, match="needs a ROCm GPU"):
                get_controller(_env(), name, "N256_H32_lam0.01", device="cpu", riccati=True, plan_hold=3, **kw)
