"""The state estimator's surface on the CPU: header, exports, binding, check_estimator's refusals, the Python entry
points.  No GPU: nothing here creates a handle."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.abi_support import ROOT, built, header_text  # noqa: F401  (built: a fixture)


def test_header_macros_symbols_and_prototypes(built):
    lib = built.load_library()
    hdr = header_text()
    for name, value in (("COVO_HAS_STATE_ESTIMATOR", 1), ("COVO_EST_FLOATS", 8), ("COVO_EST_STATE_DOUBLES", 16), ("COVO_EST_META_INTS", 2),
                        ("COVO_EST_LOG_FLOATS", 34)):
        assert re.search(rf"^#define {name} {value}$", hdr, flags=re.M) and getattr(built, name) == value, name
    assert re.search(r"int covo_set_step_estimator\(covo_handle_t h, const double \*obs_std, const double \*proc_std, double force_std, "
                     r"double \*xhat, double \*P,\s*int32_t \*meta, float \*rows[^,]*, int32_t n_inst\);", hdr)
    assert re.search(r"int covo_estimator_reset\(covo_handle_t h\);", hdr)
    assert re.search(r"int covo_set_episode_estimator_log\(covo_handle_t h, float \*log, int32_t stride\);", hdr)
    # the stand-alone entry: state rows in place, u with a stride, per-instance parameters, and the stream spelled hip_stream
    assert re.search(r"int covo_estimate\(covo_handle_t h, float \*state_rows, const float \*u, int32_t u_stride, const covo_env_params "
                     r"\*params,[^;]*double \*xhat, double \*P, int32_t \*meta, float \*rows,\s*int32_t n_inst, int32_t reset, "
                     r"void \*hip_stream\);", hdr)
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()  # additive
    P, I, D = C.c_void_p, C.c_int32, C.c_double
    PD, PE = C.POINTER(C.c_double), C.POINTER(built.EnvParamsC)
    fn = lib.covo_set_step_estimator
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, PD, PD, D, P, P, P, P, I]
    fn = lib.covo_estimate
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, P, P, I, PE, PD, PD, D, P, P, P, P, I, I, P]
    assert list(lib.covo_estimator_reset.argtypes) == [P] and list(lib.covo_set_episode_estimator_log.argtypes) == [P, P, I]
    for name in ("covo_set_step_estimator", "covo_estimator_reset", "covo_estimate", "covo_set_episode_estimator_log"):
        assert name in built.EXPORTS, name
    # a null handle is refused by name before anything else happens
    assert lib.covo_set_step_estimator(None, None, None, 0.0, None, None, None, None, 0) != 0
    assert b"covo_set_step_estimator: null handle" in lib.covo_last_error()
    assert lib.covo_estimator_reset(None) != 0 and b"covo_estimator_reset: null handle" in lib.covo_last_error()
    assert lib.covo_set_episode_estimator_log(None, None, 0) != 0 and b"covo_set_episode_estimator_log: null handle" in lib.covo_last_error()
    assert lib.covo_estimate(None, None, None, 4, None, None, None, 0.0, None, None, None, None, 1, 0, None) != 0
    assert b"covo_estimate: null handle" in lib.covo_last_error()


def test_the_kernel_source_is_built_and_the_drivers_launch_it_behind_the_env_step():
    mk = open(os.path.join(ROOT, "covo_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bstate_estimator\.hip\b", mk, flags=re.M)
    src = open(os.path.join(ROOT, "covo_mpc_amd", "csrc", "state_estimator.hip")).read()
    assert "qm::dyn_step<qm::D1, double" in src and "rebase_global" in src and "__launch_bounds__(SE_BLOCK)" in src
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code.lower() and "__shfl" not in code
    capi = open(os.path.join(ROOT, "covo_mpc_amd", "csrc", "capi.hip")).read()
    single = capi[capi.index("int covo_run_episode("):capi.index("int covo_env_step_batched(")]
    batched = capi[capi.index("static int run_episode_batched("):capi.index("int covo_run_episode_batched(")]
    for body, env_step in ((single, "launch_env_step("), (batched, "launch_env_step_batched(")):
        assert body.index(env_step) < body.index("covo_estimator_step(") and "check_episode_estimator(" in body


def test_the_python_surface(built):
    from covo_mpc_amd import controllers, envs
    from covo_mpc_amd.controllers import _options as O
    from covo_mpc_amd.controllers._core import SamplingCore
    p = inspect.signature(controllers.StateEstimator.__init__).parameters
    assert list(p) == ["self", "env", "n_inst", "obs_std", "proc_std", "force_std"]
    assert (p["n_inst"].default, p["obs_std"].default, p["proc_std"].default, p["force_std"].default) == (1, None, None, None)
    for name in ("attach", "detach", "reset"):
        assert callable(getattr(controllers.StateEstimator, name)), name
    for name in ("rows", "xhat", "P"):
        assert isinstance(getattr(controllers.StateEstimator, name), property), name
    assert list(inspect.signature(SamplingCore.estimated).parameters)[:3] == ["self", "dstate", "a_mean"]
    assert list(inspect.signature(SamplingCore.estimate).parameters)[:7] == ["self", "state_rows", "u", "params_c", "xhat", "P", "meta"]
    for name in ("attach_estimator", "detach_estimator", "estimator_reset", "estimator_info", "attach_estimator_log"):
        assert callable(getattr(SamplingCore, name)), name
    for cls in (envs.DeviceEpisode, envs.BatchedDeviceEpisode):
        assert callable(cls.read_estimate)
    # every host __call__ passes its noisy state through the one hook, and every reset() restarts the filter
    for mod in ("mppi", "covo", "cma", "ilqr", "batched"):
        text = open(os.path.join(ROOT, "covo_mpc_amd", "controllers", mod + ".py")).read()
        assert "core.estimated(" in text and "estimator_reset()" in text, mod
    # get_controller and eval_env_batched take no keyword for it (tests/test_nodes_abi.py pins their tails)
    assert "estimator" not in inspect.signature(envs.get_controller).parameters
    assert "estimator" not in inspect.signature(envs.quadrotor.eval_env_batched).parameters


def test_read_estimate_names_the_option_when_never_attached(built):
    from covo_mpc_amd.envs.quadrotor import _EpisodeLogs
    ep = _EpisodeLogs()
    with pytest.raises(RuntimeError, match="StateEstimator"):
        ep.read_estimate()


def test_check_estimator_defaults_and_refusals(built):
    from covo_mpc_amd.controllers._options import check_estimator
    c = inspect.signature(check_estimator).parameters
    assert all(x.kind is x.KEYWORD_ONLY for x in c.values())
    r = check_estimator()
    assert r.obs_std == tuple(0.05 * g for g in (0.25, 0.5, 0.02, 0.5)) and r.proc_std == (0.0, -1.0, 0.0, 0.0) and r.force_std == 0.05
    r = check_estimator(obs_noise_scale=0.1, dyn_noise_scale=0.2, proc_std=(0, 0.3, 0, 0))
    assert r.obs_std[0] == 0.1 * 0.25 and r.force_std == 0.2 and r.proc_std == (0.0, 0.3, 0.0, 0.0)
    assert check_estimator(force_std=0).force_std == 0.0 and check_estimator(n_inst=64).obs_std == check_estimator().obs_std
    nan, inf = float("nan"), float("inf")
    for kw in (dict(n_inst=0), dict(n_inst=65), dict(n_inst=1.0), dict(n_inst=True),
               dict(obs_std=(0.1, 0.1, 0.1)), dict(obs_std=(0.1, 0.0, 0.1, 0.1)), dict(obs_std=(0.1, -0.1, 0.1, 0.1)),
               dict(obs_std=(0.1, nan, 0.1, 0.1)), dict(obs_std=(0.1, inf, 0.1, 0.1)), dict(obs_std=0.1), dict(obs_std=(0.1, True, 0.1, 0.1)),
               dict(proc_std=(-1.0, 0.0, 0.0, 0.0)), dict(proc_std=(0.0, 0.0, 0.0, -0.5)), dict(proc_std=(0.0, nan, 0.0, 0.0)),
               dict(proc_std=(0.0, 0.0, inf, 0.0)), dict(proc_std=(0.0, 0.0)),
               dict(force_std=-0.1), dict(force_std=nan), dict(force_std=inf), dict(force_std="1")):
        with pytest.raises(ValueError, match=next(iter(kw)) + "="):
            check_estimator(**kw)
    # the order: the values first, then the two paths that are not implemented
    with pytest.raises(ValueError, match="obs_std="):
        check_estimator(obs_std=(0, 0, 0, 0), process_group=object(), materialize_eps=True)
    with pytest.raises(NotImplementedError, match="process_group"):
        check_estimator(process_group=object(), materialize_eps=True)
    with pytest.raises(NotImplementedError, match="kernel-by-kernel"):
        check_estimator(materialize_eps=True)
    with pytest.raises(NotImplementedError, match="kernel-by-kernel"):
        check_estimator(noise_stream="jax")


def test_no_product_file_imports_the_oracle():
    for top in ("covo_mpc_amd", "scripts", "include"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hip", ".hpp", ".h")):
                    text = open(os.path.join(d, f), errors="replace").read()
                    assert "estimator_oracle" not in text, os.path.join(d, f)
    for f in ("bench.py", "__graft_entry__.py"):
        assert "estimator_oracle" not in open(os.path.join(ROOT, f)).read(), f
