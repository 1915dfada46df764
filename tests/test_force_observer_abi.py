"""The force observer's surface on the CPU: header, exports, binding, check_force_observer's refusals, the mutual
refusal with the state estimator, the Python entry points.  No GPU: nothing here creates a handle."""
import ctypes as C
import inspect
import math
import os
import re

import pytest

from tests.abi_support import ROOT, built, header_text  # noqa: F401  (built: a fixture)


def test_header_macros_symbols_and_prototypes(built):
    lib = built.load_library()
    hdr = header_text()
    for name, value in (("COVO_HAS_FORCE_OBSERVER", 1), ("COVO_OBS_FLOATS", 8), ("COVO_OBS_STATE_DOUBLES", 16), ("COVO_OBS_META_INTS", 2),
                        ("COVO_OBS_LOG_FLOATS", 40)):
        assert re.search(rf"^#define {name} {value}$", hdr, flags=re.M) and getattr(built, name) == value, name
    # the state estimator's constants stay as they are
    for name, value in (("COVO_EST_FLOATS", 8), ("COVO_EST_STATE_DOUBLES", 16), ("COVO_EST_META_INTS", 2), ("COVO_EST_LOG_FLOATS", 34)):
        assert re.search(rf"^#define {name} {value}$", hdr, flags=re.M) and getattr(built, name) == value, name
    assert re.search(r"int covo_set_step_force_observer\(covo_handle_t h, const double \*obs_std, const double \*proc_std, double "
                     r"force_walk_std,\s*double force_init_std, double \*xi, double \*P, int32_t \*meta,\s*float \*rows[^,]*, int32_t n_inst\);",
                     hdr)
    assert re.search(r"int covo_force_observer_reset\(covo_handle_t h\);", hdr)
    assert re.search(r"int covo_set_episode_force_observer_log\(covo_handle_t h, float \*log, int32_t stride\);", hdr)
    # the stand-alone entry: state rows in place, u with a stride, per-instance parameters, and the stream spelled hip_stream
    assert re.search(r"int covo_observe_force\(covo_handle_t h, float \*state_rows, const float \*u, int32_t u_stride, const covo_env_params "
                     r"\*params,[^;]*double force_walk_std, double force_init_std, double \*xi, double \*P,\s*int32_t \*meta, float \*rows, "
                     r"int32_t n_inst, int32_t reset, void \*hip_stream\);", hdr)
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()  # additive
    P, I, D = C.c_void_p, C.c_int32, C.c_double
    PD, PE = C.POINTER(C.c_double), C.POINTER(built.EnvParamsC)
    fn = lib.covo_set_step_force_observer
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, PD, PD, D, D, P, P, P, P, I]
    fn = lib.covo_observe_force
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, P, P, I, PE, PD, PD, D, D, P, P, P, P, I, I, P]
    assert list(lib.covo_force_observer_reset.argtypes) == [P] and list(lib.covo_set_episode_force_observer_log.argtypes) == [P, P, I]
    for name in ("covo_set_step_force_observer", "covo_force_observer_reset", "covo_observe_force", "covo_set_episode_force_observer_log"):
        assert name in built.EXPORTS, name
    # a null handle is refused by name before anything else happens
    assert lib.covo_set_step_force_observer(None, None, None, 0.0, 0.0, None, None, None, None, 0) != 0
    assert b"covo_set_step_force_observer: null handle" in lib.covo_last_error()
    assert lib.covo_force_observer_reset(None) != 0 and b"covo_force_observer_reset: null handle" in lib.covo_last_error()
    assert lib.covo_set_episode_force_observer_log(None, None, 0) != 0
    assert b"covo_set_episode_force_observer_log: null handle" in lib.covo_last_error()
    assert lib.covo_observe_force(None, None, None, 4, None, None, None, 0.0, 0.0, None, None, None, None, 1, 0, None) != 0
    assert b"covo_observe_force: null handle" in lib.covo_last_error()


def test_the_kernel_source_is_built_and_the_drivers_launch_it_behind_the_env_step():
    mk = open(os.path.join(ROOT, "covo_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bforce_observer\.hip\b", mk, flags=re.M)
    src = open(os.path.join(ROOT, "covo_mpc_amd", "csrc", "force_observer.hip")).read()
    assert "qm::dyn_step<qm::D1, double, true, qm::D1>" in src and "rebase_global" in src and "__launch_bounds__(FO_BLOCK)" in src
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code.lower().replace("__atomic_acq_rel", "") and "__shfl" not in code and "asm" not in code
    # the five 16 x 16 x 16 products, four fp64 MFMAs each
    assert code.count("fo_mfma4(") == 1 + 5 and code.count("__builtin_amdgcn_mfma_f64_16x16x4f64(") == 1
    capi = open(os.path.join(ROOT, "covo_mpc_amd", "csrc", "capi.hip")).read()
    single = capi[capi.index("int covo_run_episode("):capi.index("int covo_env_step_batched(")]
    batched = capi[capi.index("static int run_episode_batched("):capi.index("int covo_run_episode_batched(")]
    for body, env_step in ((single, "launch_env_step("), (batched, "launch_env_step_batched(")):
        assert body.index(env_step) < body.index("covo_estimator_step(") < body.index("covo_force_observer_step(")
        assert "check_episode_force_observer(" in body
    # two filters must not write one row: each setter refuses while the other filter is attached
    est = capi[capi.index("int covo_set_step_estimator("):capi.index("int covo_estimator_reset(")]
    obs = capi[capi.index("int covo_set_step_force_observer("):capi.index("int covo_force_observer_reset(")]
    assert "REQUIRE(!covo_force_observer_on(h)" in est and "REQUIRE(!covo_estimator_on(h)" in obs


def test_the_python_surface(built):
    from covo_mpc_amd import controllers, envs
    from covo_mpc_amd.controllers._core import SamplingCore
    p = inspect.signature(controllers.ForceObserver.__init__).parameters
    assert list(p) == ["self", "env", "n_inst", "obs_std", "proc_std", "force_walk_std", "force_init_std"]
    assert [p[k].default for k in list(p)[2:]] == [1, None, None, None, None]
    for name in ("attach", "detach", "reset"):
        assert callable(getattr(controllers.ForceObserver, name)), name
    for name in ("rows", "xhat", "force", "P"):
        assert isinstance(getattr(controllers.ForceObserver, name), property), name
    assert list(inspect.signature(SamplingCore.observe_force).parameters)[:7] == ["self", "state_rows", "u", "params_c", "xi", "P", "meta"]
    for name in ("attach_force_observer", "detach_force_observer", "force_observer_reset", "force_observer_info", "attach_force_observer_log"):
        assert callable(getattr(SamplingCore, name)), name
    for cls in (envs.DeviceEpisode, envs.BatchedDeviceEpisode):
        assert callable(cls.read_force)
    # every reset() restarts the observer next to the estimator; the host __call__ goes through the one existing hook
    for mod in ("mppi", "covo", "cma", "ilqr", "batched"):
        text = open(os.path.join(ROOT, "covo_mpc_amd", "controllers", mod + ".py")).read()
        assert text.count("force_observer_reset()") == text.count("estimator_reset()") > 0, mod
    assert "force_observer" in inspect.getsource(SamplingCore.estimated)
    # get_controller and eval_env_batched take no keyword for it (tests/test_nodes_abi.py pins their tails)
    for fn in (envs.get_controller, envs.quadrotor.eval_env_batched):
        assert not any("observer" in k for k in inspect.signature(fn).parameters)
    # the state estimator's class is what it was
    assert list(inspect.signature(controllers.StateEstimator.__init__).parameters) == ["self", "env", "n_inst", "obs_std", "proc_std", "force_std"]


def test_read_force_names_the_option_when_never_attached(built):
    from covo_mpc_amd.envs.quadrotor import _EpisodeLogs
    ep = _EpisodeLogs()
    with pytest.raises(RuntimeError, match="ForceObserver"):
        ep.read_force()


def test_check_force_observer_defaults_and_refusals(built):
    from covo_mpc_amd.controllers._options import check_force_observer
    c = inspect.signature(check_force_observer).parameters
    assert all(x.kind is x.KEYWORD_ONLY for x in c.values())
    r = check_force_observer()
    assert r.obs_std == tuple(0.05 * g for g in (0.25, 0.5, 0.02, 0.5)) and r.proc_std == (0.0, 0.0, 0.0, 0.0)
    assert r.force_walk_std == 0.05 and r.force_init_std == 0.2 / math.sqrt(3.0)
    r = check_force_observer(obs_noise_scale=0.1, dyn_noise_scale=0.2, disturb_scale=0.3, proc_std=(0, 0.3, 0, 0))
    assert r.obs_std[0] == 0.1 * 0.25 and r.force_walk_std == 0.2 and r.force_init_std == 0.3 / math.sqrt(3.0) and r.proc_std == (0.0, 0.3, 0.0, 0.0)
    r = check_force_observer(force_walk_std=0, force_init_std=0, n_inst=64)
    assert r.force_walk_std == 0.0 and r.force_init_std == 0.0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(n_inst=0), dict(n_inst=65), dict(n_inst=1.0), dict(n_inst=True),
               dict(obs_std=(0.1, 0.1, 0.1)), dict(obs_std=(0.1, 0.0, 0.1, 0.1)), dict(obs_std=(0.1, -0.1, 0.1, 0.1)),
               dict(obs_std=(0.1, nan, 0.1, 0.1)), dict(obs_std=(0.1, inf, 0.1, 0.1)), dict(obs_std=0.1), dict(obs_std=(0.1, True, 0.1, 0.1)),
               dict(proc_std=(-1.0, 0.0, 0.0, 0.0)), dict(proc_std=(0.0, -1.0, 0.0, 0.0)), dict(proc_std=(0.0, nan, 0.0, 0.0)),
               dict(proc_std=(0.0, 0.0, inf, 0.0)), dict(proc_std=(0.0, 0.0)),
               dict(force_walk_std=-0.1), dict(force_walk_std=nan), dict(force_walk_std=inf), dict(force_walk_std="1"),
               dict(force_init_std=-0.1), dict(force_init_std=nan), dict(force_init_std=inf), dict(force_init_std=True)):
        with pytest.raises(ValueError, match=next(iter(kw)) + "="):
            check_force_observer(**kw)
    # the order: the values first, then the second filter, then the two paths that are not implemented
    with pytest.raises(ValueError, match="obs_std="):
        check_force_observer(obs_std=(0, 0, 0, 0), state_estimator=True, process_group=object(), materialize_eps=True)
    with pytest.raises(ValueError, match="StateEstimator"):
        check_force_observer(state_estimator=True, process_group=object(), materialize_eps=True)
    with pytest.raises(NotImplementedError, match="process_group"):
        check_force_observer(process_group=object(), materialize_eps=True)
    with pytest.raises(NotImplementedError, match="kernel-by-kernel"):
        check_force_observer(materialize_eps=True)
    with pytest.raises(NotImplementedError, match="kernel-by-kernel"):
        check_force_observer(noise_stream="jax")


def test_no_product_file_imports_the_oracle():
    for top in ("covo_mpc_amd", "scripts", "include"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hip", ".hpp", ".h")):
                    text = open(os.path.join(d, f), errors="replace").read()
                    assert "force_observer_oracle" not in text, os.path.join(d, f)
    for f in ("bench.py", "__graft_entry__.py"):
        assert "force_observer_oracle" not in open(os.path.join(ROOT, f)).read(), f
