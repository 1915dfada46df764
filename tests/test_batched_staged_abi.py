"""CPU: the surface of the staged env-batched MPPI / covo-offline step (covo_set_step_batched_staged, include/covo_hip.h;
staged= of BatchedMPPIController / BatchedCoVOController / eval_env_batched): header, binding and library agree, the ABI version
does not move, the keyword is in the three signatures and is no step option, and the refusals that need no device.  No GPU call."""
import ctypes
import inspect
import re

import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def test_header_binding_and_library_agree(built):
    hdr = header_text()
    assert re.search(r"^#define COVO_HAS_BATCHED_STAGED 1$", hdr, flags=re.M)
    assert re.search(r"^int covo_set_step_batched_staged\(covo_handle_t h, int32_t on\);$", hdr, flags=re.M)
    assert built.COVO_HAS_BATCHED_STAGED == 1
    assert int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1)) == built.ABI_VERSION == 10  # additive
    lib = built.load_library()
    assert lib.covo_abi_version() == 10
    fn = lib.covo_set_step_batched_staged
    assert fn.restype is ctypes.c_int and fn.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert fn(None, 1) != 0  # a null handle is refused, nothing dereferenced
    # covo_batch_mode_args does not change
    assert ctypes.sizeof(built.BatchModeArgsC) == 120
    comment = re.sub(r"\s+", " ", hdr.split("typedef struct covo_batch_mode_args")[0][-3000:])
    assert "Unless covo_set_step_batched_staged (below) is on there is no staged fallback" in comment


def test_staged_is_in_the_three_signatures_and_is_no_step_option():
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._options import STEP_OPTION_DEFAULTS, check_step_options
    from covo_mpc_amd.envs.quadrotor import eval_env_batched
    for fn in (controllers.BatchedMPPIController.__init__, controllers.BatchedCoVOController.__init__, eval_env_batched):
        p = inspect.signature(fn).parameters
        assert p["staged"].default is False and p["staged"].annotation in (bool, "bool"), fn
        assert not any(q.kind in (q.VAR_KEYWORD, q.VAR_POSITIONAL) for q in p.values()), fn
    assert "staged" not in STEP_OPTION_DEFAULTS
    with pytest.raises(TypeError, match="staged"):
        check_step_options(256, "online", staged=True)
    assert "staged" not in inspect.signature(controllers.MPPIController.__init__).parameters


def test_eval_env_batched_names_its_controller():
    from covo_mpc_amd.envs.quadrotor import eval_env_batched
    p = inspect.signature(eval_env_batched).parameters
    assert p["controller"].default == "covo-online"
    with pytest.raises(ValueError, match="controller='pid'"):
        eval_env_batched(None, 2, "N256_H32_lam0.01", controller="pid")
    with pytest.raises(ValueError, match="sigma_period=2 with mppi"):  # the option checks name the chosen controller
        eval_env_batched(None, 2, "N256_H32_lam0.01", controller="mppi", sigma_period=2, staged=True)


def test_staged_with_covo_online_is_a_value_error():
    from covo_mpc_amd import controllers
    with pytest.raises(ValueError, match='staged=True with mode="online"'):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, staged=True)
    with pytest.raises(ValueError, match='staged=True with mode="online"'):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, mode="online", staged=True)


def test_refusals_that_stay_under_staged_need_no_device():
    from covo_mpc_amd import controllers
    with pytest.raises(NotImplementedError, match=r"gamma_sigma=0\.2 together with elite=8"):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, gamma_sigma=0.2, elite=8, staged=True)
    with pytest.raises(NotImplementedError, match=r"gamma_sigma=0\.2 together with ess_min=8"):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, gamma_sigma=0.2, ess_min=8, staged=True)
    # the Sigma period and Sigma adapt stay covo-online's
    with pytest.raises(ValueError, match="sigma_period=2 with the env-batched MPPI controller"):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, sigma_period=2, staged=True)
    with pytest.raises(ValueError, match="sigma_adapt=0.2 with the env-batched covo-offline controller"):
        controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, mode="offline", sigma_adapt=0.2, staged=True)
    # a full refit from fewer than 5 elites: the range check of the single MPPI controller, now that gamma_sigma is taken
    with pytest.raises(ValueError, match="elite=4 with gamma_sigma=1.0"):
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, gamma_sigma=1.0, elite=4, staged=True)


def test_staged_off_refuses_as_before_and_points_to_the_switch():
    """The matched prefixes of the fused step's refusals stay; their tails name the switch."""
    from covo_mpc_amd import controllers
    cases = [(dict(elite=8), "elite=8: the elite-set update is not available for the env-batched"),
             (dict(compute_post_cov=True), "compute_post_cov: the posterior covariance is not available"),
             (dict(iters=2, update="best"), "iters=2 with update='best': not available"),
             (dict(ess_min=8), "ess_min=8: the ESS floor is not available")]
    for kw, prefix in cases:
        for build in (lambda **k: controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, **k),
                      lambda **k: controllers.BatchedCoVOController(None, 3, 256, 32, 0.01, mode="offline", **k)):
            with pytest.raises(NotImplementedError, match=re.escape(prefix)) as ei:
                build(**kw)
            assert "staged=True" in str(ei.value)
            with pytest.raises(NotImplementedError, match=re.escape(prefix)):
                build(staged=False, **kw)
    with pytest.raises(NotImplementedError, match="gamma_sigma") as ei:
        controllers.BatchedMPPIController(None, 3, 256, 32, 0.01, gamma_sigma=0.2)
    assert "staged=True" in str(ei.value)
