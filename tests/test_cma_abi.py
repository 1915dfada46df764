"""The CMA controller's surface on the CPU: header, exports, binding, check_cma's refusals and their order, the Python
entry points.  No GPU: nothing here creates a handle."""
import ctypes as C
import inspect
import os
import re

import pytest

from tests.abi_support import ROOT, built, header_text  # noqa: F401  (built: a fixture)


def test_header_macros_symbols_and_prototypes(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"^#define COVO_HAS_CMA 1$", hdr, flags=re.M) and built.COVO_HAS_CMA == 1
    assert re.search(r"^#define COVO_CMA_FLOATS 8$", hdr, flags=re.M) and built.COVO_CMA_FLOATS == 8
    # the mode's number: 4 stays invalid (tests/golden/step_refusals.txt walks it), 5 is the binding's
    assert re.search(r"^#define COVO_MODE_CMA 5$", hdr, flags=re.M) and built.MODE_CMA == 5
    assert re.search(r"int covo_set_step_cma\(covo_handle_t h, float gamma, int32_t step_size, float damping, float s_min, float s_max,\s*"
                     r"float \*rows_out[^,]*, double \*path_out[^,]*,\s*int32_t n_inst\);", hdr)
    assert re.search(r"int covo_cma_reset\(covo_handle_t h\);", hdr)
    assert re.search(r"int covo_cma_path\(covo_handle_t h, const float \*L_prev, const float \*aux, int32_t aux_stride, const float \*ess, "
                     r"int32_t ess_stride,", hdr)
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()  # additive
    P, I, F = C.c_void_p, C.c_int32, C.c_float
    fn = lib.covo_set_step_cma
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, F, I, F, F, F, P, P, I]
    fn = lib.covo_cma_path
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, P, P, I, P, I, P, P, P, I, I, I, F, F, F, P, P, P, P, P, P]
    assert list(lib.covo_cma_reset.argtypes) == [P]
    for name in ("covo_set_step_cma", "covo_cma_reset", "covo_cma_path"):
        assert name in built.EXPORTS, name
    # a null handle is refused by name before anything else happens
    assert lib.covo_set_step_cma(None, 0.2, 1, 1.0, 0.1, 4.0, None, None, 0) != 0 and b"covo_set_step_cma: null handle" in lib.covo_last_error()
    assert lib.covo_cma_reset(None) != 0 and b"covo_cma_reset: null handle" in lib.covo_last_error()
    assert lib.covo_cma_path(None, None, None, 132, None, 8, None, None, None, 1, 256, 1, 1.0, 0.1, 4.0, None, None, None, None, None,
                             None) != 0
    assert b"covo_cma_path: null handle" in lib.covo_last_error()
    # the rows the step reads are the existing ones
    assert built.COVO_POST_AUX_FLOATS == 132 and built.COVO_DIAG_FLOATS == 8 and built.COVO_SIGMA_ADAPT_FLOATS == 4


def test_the_kernel_source_is_built_and_names_its_reductions():
    mk = open(os.path.join(ROOT, "covo_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bcma_path\.hip\b", mk, flags=re.M)
    src = open(os.path.join(ROOT, "covo_mpc_amd", "csrc", "cma_path.hip")).read()
    assert '#include "wave_reduce.hpp"' in src and "wr::wave64_allsum" in src
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code.lower() and "__shfl" not in code
    # sigma_adapt.hip is called as it is: the step hands it the handle's second buffer
    step = open(os.path.join(ROOT, "covo_mpc_amd", "csrc", "step.hip")).read()
    assert "launch_sigma_adapt(v.L, h->post_cov_out, v.E, h->cma_gamma" in step and "launch_cma_path(d, s)" in step


def test_the_python_surface(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers import _options as O
    from covo_mpc_amd.controllers._core import SamplingCore
    p = inspect.signature(controllers.CMAController.__init__).parameters
    assert list(p)[:6] == ["self", "env", "control_params", "N", "H", "lam"]
    assert (p["gamma"].default, p["step_size"].default, p["damping"].default, p["s_min"].default, p["s_max"].default) == (0.2, True, 1.0, 0.1, 4.0)
    assert all(q.kind is q.KEYWORD_ONLY for name, q in p.items() if name not in list(p)[:6])
    for name in ("compute_plan", "compute_fan", "update", "ess_min", "elite", "iters", "compute_info", "device"):
        assert name in p, name
    # compute_post_cov and compute_diag are implied, not keywords
    assert "compute_post_cov" not in p and "compute_diag" not in p
    assert not any(q.kind in (q.VAR_KEYWORD, q.VAR_POSITIONAL) for q in p.values())
    for name in ("reset", "__call__", "run_episode"):
        assert callable(getattr(controllers.CMAController, name))
    assert [f.name for f in controllers.CMAParams.__dataclass_fields__.values()] == ["gamma_mean", "discount", "sample_sigma", "a_mean", "a_cov"]
    assert list(inspect.signature(controllers.CMAController.__call__).parameters) == list(
        inspect.signature(controllers.MPPIController.__call__).parameters)
    q = inspect.signature(controllers.BatchedCMAController.__init__).parameters
    assert list(q)[:6] == ["self", "env", "n_envs", "N", "H", "lam"] and q["gamma"].default == 0.2 and "staged" not in q
    for name in ("step", "run_episode", "set_instances", "bind_episode", "reset"):
        assert callable(getattr(controllers.BatchedCMAController, name))
    assert list(inspect.signature(SamplingCore.cma_path).parameters)[:8] == ["self", "L_prev", "d", "ess", "p", "log_s", "L_hat", "Sigma_hat"]
    for name in ("attach_cma", "cma_info", "cma_reset"):
        assert callable(getattr(SamplingCore, name)), name
    c = inspect.signature(O.check_cma).parameters
    assert all(x.kind is x.KEYWORD_ONLY for x in c.values())
    assert (c["gamma"].default, c["step_size"].default, c["damping"].default, c["s_min"].default, c["s_max"].default) == (0.2, True, 1.0, 0.1, 4.0)
    r = O.check_cma()
    assert (r.gamma, r.step_size, r.damping, r.s_min, r.s_max) == (0.2, True, 1.0, 0.1, 4.0)
    assert O.check_cma(gamma=0, step_size=False).gamma == 0.0


def test_check_cma_refuses_in_the_stated_order(built):
    from covo_mpc_amd.controllers._options import check_cma
    # every offender at once: the first of the list speaks; take it away and the next one does
    bad = dict(sigma_period=4, sigma_adapt=0.3, sigma_nodes=8, refine=True, riccati=True, riccati_feedback=True, plan_hold=2,
               riccati_box=True, gamma=1.0, step_size=1, damping=0.0, s_min=2.0, s_max=0.5, process_group=object(),
               materialize_eps=True)
    order = [("sigma_period", ValueError, 1), ("sigma_adapt", ValueError, 0.0), ("sigma_nodes", ValueError, None),
             ("refine", ValueError, False), ("riccati", ValueError, False), ("riccati_feedback", ValueError, False),
             ("plan_hold", ValueError, 1), ("riccati_box", ValueError, False), ("gamma", ValueError, 0.2),
             ("step_size", ValueError, True), ("damping", ValueError, 1.0), ("s_min", ValueError, 0.1)]
    for name, exc, good in order:
        with pytest.raises(exc, match=rf"\b{name}="):
            check_cma(**bad)
        bad[name] = good
    with pytest.raises(ValueError, match=r"s_max="):  # (s_min is fine now: 1 > s_max)
        check_cma(**bad)
    bad["s_max"] = 4.0
    with pytest.raises(NotImplementedError, match="process_group"):
        check_cma(**bad)
    bad["process_group"] = None
    with pytest.raises(NotImplementedError, match="kernel-by-kernel"):
        check_cma(**bad)
    bad["materialize_eps"] = False
    with pytest.raises(NotImplementedError, match="kernel-by-kernel"):
        check_cma(**bad, noise_stream="jax")
    assert check_cma(**bad).gamma == 0.2
    # the ranges' edges
    for kw in (dict(gamma=-0.1), dict(gamma=float("nan")), dict(gamma=True), dict(damping=-1.0), dict(damping=float("inf")),
               dict(s_min=0.0), dict(s_min=1.5), dict(s_max=0.99), dict(s_max=float("inf"))):
        with pytest.raises(ValueError, match=next(iter(kw)) + "="):
            check_cma(**kw)
    assert check_cma(s_min=1.0, s_max=1.0).s_min == 1.0


def test_get_controller_refuses_what_check_cma_refuses_before_anything_is_built(built):
    import covo_mpc_amd as cm
    env = cm.envs.Quad3D(task="tracking_zigzag", disturb_type="gaussian", enable_randomizer=False, disable_rollover_terminate=True,
                         generate_noisy_state=True, device=None)
    for kw, exc, word in ((dict(sigma_period=2), ValueError, "sigma_period=2"), (dict(riccati=True), ValueError, "riccati=True"),
                          (dict(refine=True), ValueError, "refine=True"), (dict(process_group=object()), NotImplementedError, "process_group")):
        with pytest.raises(exc, match=word):
            cm.envs.get_controller(env, "cma", "N256_H32_lam0.01", **kw)


def test_no_product_file_imports_the_oracle():
    for top in ("covo_mpc_amd", "scripts", "include"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hip", ".hpp", ".h")):
                    text = open(os.path.join(d, f), errors="replace").read()
                    assert "cma_oracle" not in text, os.path.join(d, f)
    for f in ("bench.py", "__graft_entry__.py"):
        assert "cma_oracle" not in open(os.path.join(ROOT, f)).read(), f
