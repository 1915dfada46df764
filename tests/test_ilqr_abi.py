"""CPU: the ABI of the iLQR controller (COVO_MODE_ILQR / covo_set_step_ilqr, include/covo_hip.h: COVO_HAS_ILQR) and its Python surface
(controllers/_options.py: check_ilqr; controllers/ilqr.py; get_controller(env, "ilqr", ...); eval_env_batched(controller="ilqr"))."""
import ctypes as C
import inspect
import re

import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)

SAMPLING = dict(compute_diag=True, ess_min=4.0, compute_fan=8, update="best", elite=8, sigma_period=4, compute_post_cov=True,
                sigma_adapt=0.25)  # every sampling step option, away from its default, in check_ilqr's order


def _env(disturb="gaussian"):
    import covo_mpc_amd as cm
    return cm.envs.Quad3D(task="tracking_zigzag", disturb_type=disturb, enable_randomizer=False, disable_rollover_terminate=True,
                          generate_noisy_state=True, device=None)


def test_ilqr_symbols_are_exported_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"^#define COVO_HAS_ILQR 1$", hdr, flags=re.M) and built.COVO_HAS_ILQR == 1
    assert int(re.search(r"#define COVO_MODE_ILQR\s+(\d+)", hdr).group(1)) == 3 == built.MODE_ILQR
    assert int(re.search(r"#define COVO_ILQR_FLOATS\s+(\d+)", hdr).group(1)) == 8 == built.COVO_ILQR_FLOATS
    assert (built.MODE_MPPI, built.MODE_COVO_ONLINE, built.MODE_COVO_OFFLINE) == (0, 1, 2)  # the sampling modes stay what they were
    P, I = C.c_void_p, C.c_int32
    assert re.search(r"\bint covo_set_step_ilqr\(covo_handle_t h,", hdr)
    fn = lib.covo_set_step_ilqr  # the built library exports it
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, P, P, P, I] and "covo_set_step_ilqr" in built.EXPORTS
    # additive: the ABI version did not move; the iteration count travels through covo_set_step_iters, which stays what it was
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()
    assert list(lib.covo_set_step_iters.argtypes) == [P, I, P, I] and built.COVO_MAX_STEP_ITERS == 16
    # a null handle is refused by name before anything else happens (no GPU needed)
    assert lib.covo_set_step_ilqr(None, None, None, None, 1) != 0 and b"covo_set_step_ilqr: null handle" in lib.covo_last_error()


def test_the_python_surface(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import STEP_OPTION_DEFAULTS
    p = inspect.signature(controllers.ILQRController.__init__).parameters
    assert list(p) == ["self", "env", "control_params", "H", "iters", "riccati_feedback", "plan_hold", "compute_plan", "device"]
    assert (p["iters"].default, p["riccati_feedback"].default, p["plan_hold"].default, p["compute_plan"].default) == (2, None, 1, False)
    q = inspect.signature(controllers.BatchedILQRController.__init__).parameters
    assert list(q)[:4] == ["self", "env", "n_envs", "H"] and q["iters"].default == 2 and q["riccati_feedback"].default is None
    for name in ("reset", "__call__", "run_episode"):
        assert callable(getattr(controllers.ILQRController, name))
    for name in ("step", "run_episode", "set_instances", "bind_episode"):
        assert callable(getattr(controllers.BatchedILQRController, name))
    assert controllers.ILQRParams(a_mean=None).replace(a_mean=1).a_mean == 1
    assert callable(SamplingCore.attach_ilqr) and callable(SamplingCore.ilqr_info)
    assert "ilqr" not in STEP_OPTION_DEFAULTS and set(SAMPLING) | {"iters", "compute_plan"} == set(STEP_OPTION_DEFAULTS)


def test_riccati_feedback_resolves_per_plant(built):
    from covo_mpc_amd.controllers._options import check_ilqr
    for kind in (None, "none", "gaussian", "periodic", "sin"):
        assert check_ilqr(2, disturb_type=kind) == (2, True, 1)
        assert check_ilqr(2, riccati_feedback=True, disturb_type=kind) == (2, True, 1)
        assert check_ilqr(2, riccati_feedback=False, disturb_type=kind) == (2, False, 1)  # an explicit False is honoured
    for kind in ("drag", "mixed"):
        assert check_ilqr(3, disturb_type=kind) == (3, False, 1)
        assert check_ilqr(3, riccati_feedback=False, disturb_type=kind) == (3, False, 1)
        with pytest.raises(NotImplementedError, match="16-state plants"):  # check_riccati_feedback's own refusal
            check_ilqr(3, riccati_feedback=True, disturb_type=kind)
    for k in (1, 2, 16):
        for m in (1, 3, 16):
            assert check_ilqr(k, plan_hold=m, disturb_type="gaussian", compute_plan=True) == (k, True, m)
    # every step option AT its default (or an equivalent off value) is nothing to object to
    assert check_ilqr(2, compute_diag=False, ess_min=None, compute_fan=None, update="softmax", elite=None, sigma_period=1,
                      compute_post_cov=False, sigma_adapt=0.0) == (2, True, 1)
    assert check_ilqr(2, ess_min=0, compute_fan=False, elite=0) == (2, True, 1)


def test_check_ilqr_objects_in_its_documented_order(built):
    from covo_mpc_amd.controllers._options import check_ilqr
    everything = dict(SAMPLING, refine=True, process_group=object(), riccati_feedback="yes", plan_hold=99, disturb_type="drag")
    # 1. iters outside [1, 16], whatever else is wrong
    for bad in (0, 17, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="iters="):
            check_ilqr(bad, **everything)
    # 2. the sampling step options, in the table's order: each is named, ahead of everything behind it
    names = list(SAMPLING)
    for i, name in enumerate(names):
        kw = dict(everything)
        for gone in names[:i]:
            del kw[gone]
        with pytest.raises(ValueError, match=f"^{name}="):
            check_ilqr(2, **kw)
        with pytest.raises(ValueError, match=f"^{name}=.*an iLQR step has none"):
            check_ilqr(2, **{name: SAMPLING[name]})
    rest = {k: v for k, v in everything.items() if k not in SAMPLING}
    # 3. refine=True
    with pytest.raises(ValueError, match="refine=True with the iLQR controller"):
        check_ilqr(2, **rest)
    with pytest.raises(ValueError, match="refine='no'"):
        check_ilqr(2, **dict(rest, refine="no"))
    del rest["refine"]
    # 4. a process group
    with pytest.raises(NotImplementedError, match="process_group"):
        check_ilqr(2, **rest)
    del rest["process_group"]
    # 5. riccati_feedback: not None / bool, then the 16-state plants
    with pytest.raises(ValueError, match="riccati_feedback='yes'"):
        check_ilqr(2, **rest)
    with pytest.raises(NotImplementedError, match="riccati_feedback=True with disturb_type='drag'"):
        check_ilqr(2, **dict(rest, riccati_feedback=True))
    # 6. the plan hold's own objections
    with pytest.raises(ValueError, match="plan_hold=99"):
        check_ilqr(2, **dict(rest, riccati_feedback=None))
    with pytest.raises(NotImplementedError, match="plan_hold=3 with disturb_type='drag'"):
        check_ilqr(2, riccati_feedback=None, plan_hold=3, disturb_type="drag")
    with pytest.raises(TypeError, match="unknown step options"):
        check_ilqr(2, lam=0.01)


def test_entry_points_refuse_before_anything_is_built(built):
    """device="cpu": a construction that got as far as the SamplingCore would raise CovoError (no GPU), not these"""
    from covo_mpc_amd import controllers
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    for name, v in SAMPLING.items():
        with pytest.raises(ValueError, match=f"^{name}="):
            get_controller(_env(), "ilqr", "N64_H32_lam0.01", device="cpu", **{name: v})
    with pytest.raises(ValueError, match="^elite=8"):
        get_controller(_env(), "ilqr", "N64_H32_lam0.01", device="cpu", elite=8)
    with pytest.raises(ValueError, match="refine=True"):
        get_controller(_env(), "ilqr", "N64_H32_lam0.01", device="cpu", refine=True)
    with pytest.raises(NotImplementedError, match="process_group"):
        get_controller(_env(), "ilqr", "N64_H32_lam0.01", device="cpu", process_group=object())
    with pytest.raises(ValueError, match="iters=17"):
        get_controller(_env(), "ilqr", "N64_H32_lam0.01", device="cpu", iters=17)
    with pytest.raises(NotImplementedError, match="riccati_feedback=True with disturb_type='mixed'"):
        get_controller(_env("mixed"), "ilqr", "N64_H32_lam0.01", device="cpu", riccati_feedback=True)
    with pytest.raises(NotImplementedError, match="plan_hold=3 with disturb_type='drag'"):
        get_controller(_env("drag"), "ilqr", "N64_H32_lam0.01", device="cpu", plan_hold=3)
    for bad in (dict(iters=0), dict(riccati_feedback="yes"), dict(plan_hold=17)):
        with pytest.raises(ValueError):
            controllers.ILQRController(_env(), controllers.ILQRParams(a_mean=None), 32, device="cpu", **bad)
        with pytest.raises(ValueError):
            controllers.BatchedILQRController(_env(), 3, 32, device="cpu", **bad)
    with pytest.raises(ValueError, match="n_envs=0"):
        controllers.BatchedILQRController(_env(), 0, 32, device="cpu")
    with pytest.raises(ValueError, match="^elite=8"):
        eval_env_batched(_env(), 2, "N64_H32_lam0.01", n_steps=1, device="cpu", verbose=False, controller="ilqr", elite=8)
    with pytest.raises(ValueError, match="^compute_diag=True"):
        eval_env_batched(_env(), 2, "N64_H32_lam0.01", n_steps=1, device="cpu", verbose=False, controller="ilqr", diag=True)
    with pytest.raises(ValueError, match="controller='lqr'"):
        eval_env_batched(_env(), 2, "N64_H32_lam0.01", n_steps=1, device="cpu", verbose=False, controller="lqr")


def test_an_accepted_construction_reaches_the_device(built):
    """accepted: the construction gets as far as the device check (no GPU), or builds (GPU)"""
    import torch
    from covo_mpc_amd.envs.quadrotor import get_controller
    for disturb, kw, fb in (("gaussian", dict(iters=3), True), ("drag", {}, False), ("periodic", dict(plan_hold=4, compute_plan=True), True)):
        if torch.cuda.is_available():
            c, cp = get_controller(_env(disturb), "ilqr", "N64_H32_lam0.01", device="cuda:0", **kw)
            k = kw.get("iters", 1)
            assert c.iters == k and c.riccati_feedback is fb and c.core.riccati_on and tuple(c.core.ilqr_rows.shape) == (1, k, 8)
            assert (c.core.riccati_feedback_rows is not None) == fb and tuple(cp.a_mean.shape) == (32, 4)
            c.core.close()
        else:
            with pytest.raises(built.CovoError, match="needs a ROCm GPU"):
                get_controller(_env(disturb), "ilqr", "N64_H32_lam0.01", device="cpu", **kw)
