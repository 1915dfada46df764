"""CPU: the ABI of the annealed MPPI step (covo_set_step_anneal / covo_cost_standardise, include/covo_hip.h: COVO_HAS_STEP_ANNEAL) and
its Python surface (controllers/_options.py: check_dial, anneal_schedule; controllers/dial.py; BatchedDialController;
get_controller(env, "dial", ...); eval_env_batched(controller="dial")), and the self-checks of tests/anneal_oracle.py."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from tests import anneal_oracle as AO
from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def _env(disturb="gaussian"):
    import covo_mpc_amd as cm
    return cm.envs.Quad3D(task="tracking_zigzag", disturb_type=disturb, enable_randomizer=False, disable_rollover_terminate=True,
                          generate_noisy_state=True, device=None)


def test_header_macro_symbols_and_prototypes(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"^#define COVO_HAS_STEP_ANNEAL 1$", hdr, flags=re.M) and built.COVO_HAS_STEP_ANNEAL == 1
    assert re.search(r"int covo_set_step_anneal\(covo_handle_t h, const float \*sigma_table, int32_t n_pass, float temp, "
                     r"float \*rows_out, int32_t n_inst\);", hdr)
    assert re.search(r"int covo_cost_standardise\(covo_handle_t h, const float \*cost, int32_t n_samples, int32_t n_inst, float lam0, "
                     r"float temp, float \*out, void \*stream\);", hdr)
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()
    P, I, F = C.c_void_p, C.c_int32, C.c_float
    fn = lib.covo_set_step_anneal
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, C.POINTER(F), I, F, P, I]
    fn = lib.covo_cost_standardise
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, P, I, I, F, F, P, P]
    assert "covo_set_step_anneal" in built.EXPORTS and "covo_cost_standardise" in built.EXPORTS
    assert built.ANNEAL_FIELDS == ("lam_eff", "inv_lam_eff", "std", "n_finite") and built.ANNEAL_FALLBACK_BIT == 0x80000000
    # the temperature row and the pass count are the existing ones
    assert built.COVO_LAM_FLOATS == 4 and built.COVO_MAX_STEP_ITERS == 16
    # a null handle is refused by name before anything else happens (no GPU needed)
    assert lib.covo_set_step_anneal(None, None, 0, 0.0, None, 0) != 0 and b"covo_set_step_anneal: null handle" in lib.covo_last_error()
    assert lib.covo_cost_standardise(None, None, 16, 1, 0.01, 0.1, None, None) != 0
    assert b"covo_cost_standardise: null handle" in lib.covo_last_error()


def test_the_python_surface(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import STEP_OPTION_DEFAULTS, STEP_SWITCH_DEFAULTS
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    p = inspect.signature(controllers.DialController.__init__).parameters
    assert list(p)[:6] == ["self", "env", "control_params", "N", "H", "lam"]
    assert (p["iters"].default, p["beta_pass"].default, p["beta_stage"].default, p["temp"].default) == (4, 0.5, 0.9, 0.1)
    for name in ("compute_diag", "compute_plan", "compute_fan", "update", "compute_post_cov", "compute_info", "device"):
        assert name in p, name
    # no switches, no ess_min / elite / sigma_* keywords, no process_group, no **kwargs
    assert not (set(STEP_SWITCH_DEFAULTS) | {"ess_min", "elite", "sigma_period", "sigma_adapt", "process_group"}) & set(p)
    assert not any(q.kind in (q.VAR_KEYWORD, q.VAR_POSITIONAL) for q in p.values())
    assert issubclass(controllers.DialController, controllers.MPPIController)
    for name in ("reset", "__call__", "run_episode"):
        assert callable(getattr(controllers.DialController, name))
    q = inspect.signature(controllers.BatchedDialController.__init__).parameters
    assert list(q)[:6] == ["self", "env", "n_envs", "N", "H", "lam"] and "staged" not in q
    assert (q["iters"].default, q["beta_pass"].default, q["beta_stage"].default, q["temp"].default) == (4, 0.5, 0.9, 0.1)
    for name in ("step", "run_episode", "set_instances", "bind_episode"):
        assert callable(getattr(controllers.BatchedDialController, name))
    # one explicit keyword on the core, and the accessors
    c = inspect.signature(SamplingCore.__init__).parameters
    assert c["anneal"].default is None and not any(q.kind in (q.VAR_KEYWORD, q.VAR_POSITIONAL) for q in c.values())
    for name in ("attach_anneal", "anneal_info", "cost_standardise"):
        assert callable(getattr(SamplingCore, name)), name
    assert list(inspect.signature(SamplingCore.cost_standardise).parameters) == ["self", "cost", "temp", "lam0"]
    # not a step option, not a switch: the tables stay what they were
    assert not {"anneal", "beta_pass", "beta_stage", "temp"} & (set(STEP_OPTION_DEFAULTS) | set(STEP_SWITCH_DEFAULTS))
    for fn in (get_controller, eval_env_batched):
        g = inspect.signature(fn).parameters
        assert (g["beta_pass"].default, g["beta_stage"].default, g["temp"].default) == (0.5, 0.9, 0.1), fn


def test_check_dial_objects_in_its_fixed_order(built):
    from covo_mpc_amd.controllers._options import Anneal, check_dial
    with pytest.raises(ValueError, match="iters="):
        check_dial(0, beta_pass=2.0, beta_stage=0.0, temp=-1.0, gamma_sigma=0.5, materialize_eps=True)
    with pytest.raises(ValueError, match="iters="):
        check_dial(17)
    with pytest.raises(ValueError, match="beta_pass="):
        check_dial(4, beta_pass=2.0, beta_stage=0.0, temp=-1.0, gamma_sigma=0.5, materialize_eps=True)
    for bad in (0.0, -0.5, 1.5, float("nan"), True, "0.5", None):
        with pytest.raises(ValueError, match="beta_pass="):
            check_dial(4, beta_pass=bad)
    with pytest.raises(ValueError, match="beta_stage="):
        check_dial(4, beta_stage=0.0, temp=-1.0, gamma_sigma=0.5, materialize_eps=True)
    with pytest.raises(ValueError, match="temp="):
        check_dial(4, temp=-1.0, gamma_sigma=0.5, materialize_eps=True)
    for bad in (0.0, float("inf"), float("nan"), True, "0.1"):
        with pytest.raises(ValueError, match="temp="):
            check_dial(4, temp=bad)
    with pytest.raises(ValueError, match="gamma_sigma=0.5"):
        check_dial(4, gamma_sigma=0.5, materialize_eps=True)
    with pytest.raises(NotImplementedError, match="kernel-by-kernel path"):
        check_dial(4, materialize_eps=True)
    with pytest.raises(NotImplementedError, match="kernel-by-kernel path"):
        check_dial(4, noise_stream="jax")
    # the neutral element attaches nothing; either factor or the temperature alone does
    assert check_dial(3, beta_pass=1.0, beta_stage=1, temp=None) is None
    a = check_dial(3, beta_pass=1.0, beta_stage=1.0, temp=0.25)
    assert isinstance(a, Anneal) and a.temp == 0.25 and a.sigma.shape == (3, 32) and np.all(a.sigma == np.float32(0.5))
    a = check_dial(2, beta_pass=0.5, beta_stage=1.0, temp=None)
    assert a.temp == 0.0 and a.sigma.dtype == np.float32 and np.all(a.sigma[1] == np.float32(0.25))
    assert check_dial(1).sigma.shape == (1, 32) and check_dial(16).sigma.shape == (16, 32)


def test_get_controller_refusals_that_need_no_device(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    env = _env()
    with pytest.raises(ValueError, match="beta_pass=1.5"):
        get_controller(env, "dial", "N256_H32_lam0.01", iters=2, beta_pass=1.5)
    with pytest.raises(ValueError, match="temp=0"):
        get_controller(env, "dial", "N256_H32_lam0.01", temp=0)
    with pytest.raises(ValueError, match="iters=17"):
        get_controller(env, "dial", "N256_H32_lam0.01", iters=17)
    with pytest.raises(ValueError, match="ess_min=8.0 with the annealed MPPI controller"):
        get_controller(env, "dial", "N256_H32_lam0.01", ess_min=8.0)
    with pytest.raises(ValueError, match="elite=8 with the annealed MPPI controller"):
        get_controller(env, "dial", "N256_H32_lam0.01", elite=8)
    with pytest.raises(ValueError, match="riccati=True with the annealed MPPI controller"):
        get_controller(env, "dial", "N256_H32_lam0.01", riccati=True)
    with pytest.raises(ValueError, match="process_group with the annealed MPPI controller"):
        get_controller(env, "dial", "N256_H32_lam0.01", process_group=object())
    with pytest.raises(ValueError, match="beta_stage=0"):
        eval_env_batched(env, 2, "N256_H32_lam0.01", controller="dial", beta_stage=0)
    with pytest.raises(ValueError, match="staged=True with controller='dial'"):
        eval_env_batched(env, 2, "N256_H32_lam0.01", controller="dial", staged=True)
    # the controllers' own constructors, before a handle exists
    cp = controllers.MPPIParams(gamma_mean=1.0, gamma_sigma=0.3, discount=1.0, sample_sigma=0.5, a_mean=None, a_cov=None)
    with pytest.raises(ValueError, match="gamma_sigma=0.3"):
        controllers.DialController(env, cp, 256, 32, 0.01)
    with pytest.raises(ValueError, match="beta_pass=0"):
        controllers.BatchedDialController(env, 3, 256, 32, 0.01, beta_pass=0)
    with pytest.raises(ValueError, match="ONE standard deviation"):
        controllers.BatchedDialController(env, 3, 256, 32, 0.01, sigmas=(0.5, 0.5, 0.4, 0.5))
    # every other controller name ignores the three keywords at their defaults: pid needs no device
    c, _ = get_controller(env, "pid")
    assert type(c).__name__ == "PIDController"


def test_schedule_against_hand_values(built):
    """k = 3, beta_pass = 0.5, beta_stage = 0.9, sigma0 = 0.5: the corners by hand, each the fp32 rounding of the fp64 product."""
    from covo_mpc_amd.controllers._options import anneal_schedule
    s = anneal_schedule(0.5, 3, 0.5, 0.9)
    assert s.shape == (3, 32) and s.dtype == np.float32
    assert s[0, 31] == np.float32(0.5) and s[2, 31] == np.float32(0.5 / 4) and s[1, 31] == np.float32(0.25)
    assert s[0, 0] == np.float32(0.5 * 0.9 ** 31) and s[2, 0] == np.float32(0.5 * 0.25 * 0.9 ** 31)
    assert abs(float(s[0, 0]) - 0.5 * 0.9 ** 31) <= 2.0 ** -24 * 0.5 * 0.9 ** 31  # one rounding
    assert np.all(np.diff(s, axis=1) > 0) and np.all(np.diff(s, axis=0) < 0)  # near stages and later passes get less noise
    assert np.array_equal(s.view(np.uint32), AO.schedule64(0.5, 3, 0.5, 0.9).view(np.uint32))  # the oracle's restatement
    assert np.all(anneal_schedule(0.5, 4, 1.0, 1.0) == np.float32(0.5))
    # the blocks a pass samples from and leaves
    L, S = AO.factor_blocks(s[2]), AO.cov_blocks(s[2])
    assert L.shape == S.shape == (32, 4, 4) and L[31, 1, 1] == np.float32(0.125) and S[31, 2, 2] == np.float32(0.015625)
    assert L[5, 0, 1] == 0.0 and S[0, 3, 3] == s[2, 0] * s[2, 0]


def test_oracle_self_checks_on_known_vectors(built):
    lam0 = 0.01
    r = AO.standardise64(np.array([1, 2, 3, 4], dtype=np.float32), 0.1, lam0)
    assert r["std"] == np.sqrt(1.25) and r["n_finite"] == 4 and not r["fallback"]
    assert r["lam_eff"] == np.float32(float(np.float32(0.1)) * np.sqrt(1.25)) and r["inv_lam_eff"] == np.float32(1.0) / r["lam_eff"]
    w = AO.row_words(r)
    assert w[3] == 4 and AO.split_row(w.view(np.float32))[3:] == (4, False)
    # a constant vector: std = 0 -> fallback at the configured lam
    r = AO.standardise64(np.full(100, 7.5, dtype=np.float32), 0.1, lam0)
    assert r["fallback"] and r["std"] == 0.0 and r["lam_eff"] == np.float32(lam0) and r["n_finite"] == 100
    assert AO.row_words(r)[3] == np.uint32(100) | AO.FALLBACK_BIT
    # one finite value: |F| = 1 -> fallback
    c = np.full(50, np.inf, dtype=np.float32)
    c[7] = 2.0
    r = AO.standardise64(c, 0.1, lam0)
    assert r["fallback"] and r["n_finite"] == 1 and r["std"] == 0.0
    # none finite
    r = AO.standardise64(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), 0.1, lam0)
    assert r["fallback"] and r["n_finite"] == 0 and r["std"] == 0.0
    # NaN and +-inf do not count; the rest is standardised as if they were not there
    r = AO.standardise64(np.array([1, np.nan, 2, np.inf, 3, -np.inf, 4], dtype=np.float32), 0.1, lam0)
    assert r["std"] == np.sqrt(1.25) and r["n_finite"] == 4 and not r["fallback"]
    # a product that is no normal fp32 number: a denormal temperature, an overflowing one
    assert AO.standardise64(np.array([0, 1e-30], dtype=np.float32), 1e-10, lam0)["fallback"]
    assert AO.standardise64(np.array([-3e38, 3e38], dtype=np.float32), 10.0, lam0)["fallback"]
    # the crafted cases are what their names say
    for N in AO.SOLVER_SIZES:
        for e in range(3):
            assert AO.standardise64(AO.solver_costs("equal", N, e), 0.1, lam0)["fallback"]
            assert AO.standardise64(AO.solver_costs("one_finite", N, e), 0.1, lam0)["n_finite"] == 1
            assert AO.standardise64(AO.solver_costs("gauss", N, e), 0.1, lam0)["fallback"] == (N < 2)
            sp = AO.solver_costs("sprinkled", N, e)
            assert not np.isfinite(sp).all() and sp.shape == (N,)
        assert not np.array_equal(AO.solver_costs("gauss", N, 0), AO.solver_costs("gauss", N, 1))
    sp = AO.solver_costs("sprinkled", 65536, 0)
    assert set(np.flatnonzero(~np.isfinite(sp)) % 64) == set(range(64))  # every lane position
    assert AO.ulp_distance(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1
    # the key walk is tests/iters_oracle.py's
    from covo_mpc_amd import random as cr
    from tests import iters_oracle as IO
    k0 = np.asarray(cr.PRNGKey(5))
    raw2, act2 = AO.pass_keys(k0, 2)
    assert np.array_equal(raw2, IO.next_raw_key(IO.next_raw_key(k0))) and np.array_equal(act2, cr.split(raw2)[1])
