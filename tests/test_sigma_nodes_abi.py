"""CPU: the ABI of covo-online in spline-node space (covo_set_step_sigma_nodes / covo_step_sigma_nodes / covo_sigma_nodes /
covo_noise_factor_philox, include/covo_hip.h: COVO_HAS_SIGMA_NODES), its Python surface (controllers/_options.py: check_sigma_nodes; the
covo-online controllers' keyword-only sigma_nodes= / node_interp=), and the self-checks of tests/sigma_nodes_oracle.py.  No GPU call."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from tests import sigma_nodes_oracle as SO
from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def _env(disturb="gaussian"):
    import covo_mpc_amd as cm
    return cm.envs.Quad3D(task="tracking_zigzag", disturb_type=disturb, enable_randomizer=False, disable_rollover_terminate=True,
                          generate_noisy_state=True, device=None)


# ------------------------------------------------------------------------------------------ 1: header and ABI
def test_header_macro_symbols_and_prototypes(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"^#define COVO_HAS_SIGMA_NODES 1$", hdr, flags=re.M) and built.COVO_HAS_SIGMA_NODES == 1
    assert re.search(r"^#define COVO_SIGMA_NODES_MAX 16$", hdr, flags=re.M) and built.COVO_SIGMA_NODES_MAX == 16
    assert re.search(r"^#define COVO_SIGMA_NODES_FLOATS 8$", hdr, flags=re.M) and built.COVO_SIGMA_NODES_FLOATS == 8
    assert len(built.SIGMA_NODES_FIELDS) == 8
    assert re.search(r"int covo_set_step_sigma_nodes\(covo_handle_t h, const double \*W, int32_t M, float \*rows, int32_t n_inst\);", hdr)
    assert re.search(r"int covo_sigma_nodes\(covo_handle_t h, const double \*R, int32_t batch, const double \*W_dev, int32_t M, "
                     r"float sample_sigma,\s+double \*SigmaM_out, float \*G_out, float \*Sigma_out, float \*rows_out, void \*stream\);", hdr)
    assert re.search(r"int covo_noise_factor_philox\(covo_handle_t h, const float \*G, int32_t d, const float \*mu, uint32_t key0, "
                     r"uint32_t key1,\s+int64_t sample_offset, int32_t N, float \*a_out, void \*stream\);", hdr)
    assert re.search(r"int covo_step_sigma_nodes\(covo_handle_t h, int32_t \*M, double \*SigmaM_out, float \*G_out, int32_t n_inst, "
                     r"void \*stream\);", hdr)
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()  # additive: the version does not move
    P, I, F, U32, I64 = C.c_void_p, C.c_int32, C.c_float, C.c_uint32, C.c_int64
    fn = lib.covo_set_step_sigma_nodes
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, C.POINTER(C.c_double), I, P, I]
    fn = lib.covo_sigma_nodes
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, P, I, P, I, F, P, P, P, P, P]
    fn = lib.covo_noise_factor_philox
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, P, I, P, U32, U32, I64, I, P, P]
    fn = lib.covo_step_sigma_nodes
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, C.POINTER(I), P, P, I, P]
    for name in ("covo_set_step_sigma_nodes", "covo_sigma_nodes", "covo_noise_factor_philox", "covo_step_sigma_nodes"):
        assert name in built.EXPORTS, name
    # a null handle is refused by name before anything else happens (no GPU needed)
    assert lib.covo_set_step_sigma_nodes(None, None, 0, None, 0) != 0
    assert b"covo_set_step_sigma_nodes: null handle" in lib.covo_last_error()
    assert lib.covo_sigma_nodes(None, None, 1, None, 8, 0.5, None, None, None, None, None) != 0
    assert b"covo_sigma_nodes: null handle" in lib.covo_last_error()
    assert lib.covo_noise_factor_philox(None, None, 8, None, 0, 0, 0, 16, None, None) != 0
    assert b"covo_noise_factor_philox: null handle" in lib.covo_last_error()
    assert lib.covo_step_sigma_nodes(None, None, None, None, 0, None) != 0 and b"covo_step_sigma_nodes: null handle" in lib.covo_last_error()


def test_the_python_surface_and_the_pinned_tables(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers import _options as O
    from covo_mpc_amd.controllers._core import SamplingCore
    for fn in (controllers.CoVOController.__init__, controllers.BatchedCoVOController.__init__, SamplingCore.__init__):
        p = inspect.signature(fn).parameters
        assert p["sigma_nodes"].default is None and p["node_interp"].default == "linear", fn
        assert p["sigma_nodes"].kind is p["node_interp"].kind is inspect.Parameter.KEYWORD_ONLY, fn
        assert list(p)[-2:] == ["sigma_nodes", "node_interp"], fn  # behind every parameter that was there
        assert not any(q.kind in (q.VAR_KEYWORD, q.VAR_POSITIONAL) for q in p.values()), fn
    # the controllers that form no Hessian per step do not carry it
    for cls in (controllers.MPPIController, controllers.DialController, controllers.ILQRController, controllers.BatchedMPPIController,
                controllers.BatchedDialController, controllers.BatchedILQRController):
        assert "sigma_nodes" not in inspect.signature(cls.__init__).parameters, cls
    c = inspect.signature(O.check_sigma_nodes).parameters
    assert list(c) == ["sigma_nodes", "node_interp", "what", "sigma_period", "sigma_adapt", "refine", "sharded"]
    assert all(c[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("what", "sigma_period", "sigma_adapt", "refine", "sharded"))
    assert list(inspect.signature(SamplingCore.sigma_nodes).parameters) == ["self", "R", "M", "node_interp", "sample_sigma"]
    assert list(inspect.signature(SamplingCore.noise_factor).parameters) == ["self", "G", "mu", "key"]
    assert callable(SamplingCore.sigma_nodes_info) and callable(SamplingCore.read_sigma_node_cov)
    # not a step option, not a switch: the two tables are what they were
    assert list(O.STEP_OPTION_DEFAULTS.items()) == [
        ("compute_diag", False), ("compute_plan", False), ("ess_min", None), ("compute_fan", None), ("update", "softmax"), ("iters", 1),
        ("elite", None), ("sigma_period", 1), ("compute_post_cov", False), ("sigma_adapt", 0.0)]
    assert list(O.STEP_SWITCH_DEFAULTS.items()) == [
        ("refine", False), ("riccati", False), ("riccati_feedback", False), ("plan_hold", 1), ("riccati_box", False)]
    assert ("sigma_nodes_rows", "sigma_nodes_rows") in controllers.batched.CORE_BUFFERS


# ------------------------------------------------------------------------------------------ 2: check_sigma_nodes
def test_check_sigma_nodes_objects_in_its_fixed_order(built):
    from covo_mpc_amd.controllers._options import SigmaNodes, check_sigma_nodes, node_basis
    assert check_sigma_nodes(None) is None and check_sigma_nodes(None, "cubic", what="the MPPI controller", sigma_period=4) is None
    for bad in (1, 17, 0, -3, 2.0, 8.5, True, False, "8", 32):
        with pytest.raises(ValueError, match="sigma_nodes="):
            check_sigma_nodes(bad)
    for bad in ("quadratic", None, 3, ""):
        with pytest.raises(ValueError, match="node_interp="):
            check_sigma_nodes(8, bad)
    with pytest.raises(ValueError, match="node_interp="):  # (also without sigma_nodes: the name is checked as given)
        check_sigma_nodes(None, "spline")
    everything = dict(what="the MPPI controller", sigma_period=4, sigma_adapt=0.5, refine=True, sharded=True)
    with pytest.raises(ValueError, match="sigma_nodes=1 "):  # a bad M wins over everything behind it
        check_sigma_nodes(1, "x", **everything)
    with pytest.raises(ValueError, match="node_interp='x'"):
        check_sigma_nodes(8, "x", **everything)
    for what in ("the MPPI controller", "covo-offline", "the annealed MPPI controller", "the iLQR controller",
                 "the env-batched covo-offline controller"):
        with pytest.raises(ValueError, match=f"sigma_nodes=8 with {re.escape(what)}"):
            check_sigma_nodes(8, "linear", **dict(everything, what=what))
    with pytest.raises(ValueError, match="sigma_nodes=8 with sigma_period=4"):
        check_sigma_nodes(8, **dict(everything, what="online"))
    with pytest.raises(ValueError, match="sigma_nodes=8 with sigma_adapt=0.5"):
        check_sigma_nodes(8, **dict(everything, what="online", sigma_period=1))
    with pytest.raises(ValueError, match="sigma_nodes=8 with refine=True"):
        check_sigma_nodes(8, **dict(everything, what="online", sigma_period=1, sigma_adapt=0.0))
    with pytest.raises(NotImplementedError, match="sigma_nodes=8 on sample-sharded ranks"):
        check_sigma_nodes(8, what="online", sharded=True)
    s = check_sigma_nodes(np.int64(5), "cubic")
    assert isinstance(s, SigmaNodes) and s.M == 5 and type(s.M) is int and s.node_interp == "cubic"
    assert s.weights.dtype == np.float64 and np.array_equal(s.weights, node_basis(5, "cubic"))
    for M in (2, 16):
        assert check_sigma_nodes(M).weights.shape == (32, M)


def test_kernel_path_refuses_it_at_the_call(built):
    from covo_mpc_amd.controllers._options import check_kernel_path

    class Core:
        sigma_nodes_M = 8
    with pytest.raises(NotImplementedError, match="sigma_nodes=8 acts in the fused step"):
        check_kernel_path(Core())
    Core.sigma_nodes_M = None
    check_kernel_path(Core())


def test_constructor_refusals_that_need_no_device(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.envs.quadrotor import get_controller
    env = _env()
    cp = controllers.CoVOParams(gamma_mean=1.0, gamma_sigma=0.0, discount=1.0, sample_sigma=0.5, a_mean=None, a_cov=None, a_cov_offline=None)
    C_, B_ = controllers.CoVOController, controllers.BatchedCoVOController
    with pytest.raises(ValueError, match="sigma_nodes=1 "):
        C_(env, cp, 256, 32, 0.01, sigma_nodes=1)
    with pytest.raises(ValueError, match="sigma_nodes=17"):
        C_(env, cp, 256, 32, 0.01, sigma_nodes=17, node_interp="x", refine=True)
    with pytest.raises(ValueError, match="node_interp='quintic'"):
        C_(env, cp, 256, 32, 0.01, sigma_nodes=8, node_interp="quintic")
    with pytest.raises(ValueError, match="sigma_nodes=8 with covo-offline"):
        C_(env, cp, 256, 32, 0.01, "offline", sigma_nodes=8)
    with pytest.raises(ValueError, match="sigma_nodes=8 with sigma_period=3"):
        C_(env, cp, 256, 32, 0.01, sigma_nodes=8, sigma_period=3)
    with pytest.raises(ValueError, match="sigma_nodes=8 with sigma_period=3"):  # (sigma_adapt needs the period: the period objects first)
        C_(env, cp, 256, 32, 0.01, sigma_nodes=8, sigma_period=3, sigma_adapt=0.25)
    with pytest.raises(ValueError, match="sigma_nodes=8 with refine=True"):
        C_(env, cp, 256, 32, 0.01, sigma_nodes=8, refine=True)
    with pytest.raises(ValueError, match="sigma_period=0"):  # the step options object first, as for every other keyword
        C_(env, cp, 256, 32, 0.01, sigma_nodes=1, sigma_period=0)
    with pytest.raises(ValueError, match="sigma_nodes=2.5"):
        B_(env, 3, 256, 32, 0.01, sigma_nodes=2.5)
    with pytest.raises(ValueError, match="sigma_nodes=4 with the env-batched covo-offline controller"):
        B_(env, 3, 256, 32, 0.01, mode="offline", sigma_nodes=4)
    with pytest.raises(ValueError, match="sigma_nodes=4 with refine=True"):
        B_(env, 3, 256, 32, 0.01, sigma_nodes=4, refine=True)
    with pytest.raises(ValueError, match="sigma_nodes=4 with sigma_period=2"):
        B_(env, 3, 256, 32, 0.01, sigma_nodes=4, sigma_period=2)
    # the factory's own nodes= stays dial's: a covo controller ignores it (pid needs no device)
    c, _ = get_controller(env, "pid", nodes=8)
    assert type(c).__name__ == "PIDController"


# ------------------------------------------------------------------------------------------ 3: the oracle's self-checks
def _hessian_like(seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(SO.NA, SO.NA))
    return A @ A.T / SO.NA + 3.0 * np.diag(rng.uniform(0.1, 2.0, SO.NA)) + 0.01 * rng.normal(size=(SO.NA, SO.NA))


def test_oracle_at_32_linear_nodes_is_the_reference_optimize_sigma():
    """P = I: the d = 128 restatement equals oracle/ref_np.py's optimize_sigma of the same R (M = 32 is outside the keyword's range --
    the controller that already exists -- but inside the oracle's)."""
    from covo_mpc_amd.controllers._options import node_basis
    from oracle import ref_np
    W = node_basis(32, "linear")
    assert np.array_equal(SO.projector(W), np.eye(128))
    for seed, sigma in ((1, 0.5), (2, 0.2)):
        R = _hessian_like(seed)
        out = SO.solve(R, W, sigma)
        ref = ref_np.optimize_sigma(R, sigma, 32, 4)
        assert np.abs(out["SigmaM"] - ref).max() <= 1e-13 * np.linalg.norm(ref, 2)
        sign, logdet = np.linalg.slogdet(out["SigmaM"])
        assert sign == 1.0 and abs(logdet - 2 * 128 * np.log(sigma)) <= 1e-9
    out = SO.solve(SO.crafted("repeated", W), W, 0.5)
    assert np.sum(np.abs(out["lam"] - 3.0) < 1e-9) == 3 and np.sum(np.abs(out["lam"] - 7.0) < 1e-9) == 2


@pytest.mark.parametrize("interp", SO.INTERPS)
@pytest.mark.parametrize("M", SO.MS)
def test_oracle_identities(M, interp):
    from covo_mpc_amd.controllers._options import node_basis
    W = node_basis(M, interp)
    d, sigma = 4 * M, 0.37
    P = SO.projector(W)
    assert P.shape == (128, d) and np.linalg.matrix_rank(P) == d
    for R in (_hessian_like(M), SO.crafted("indefinite"), SO.crafted("graded"), SO.crafted("repeated", W)):
        out = SO.solve(R, W, sigma)
        assert np.array_equal(out["RM"], out["RM"].T) and np.array_equal(out["SigmaM"], out["SigmaM"].T)
        sign, logdet = np.linalg.slogdet(out["SigmaM"])
        assert sign == 1.0 and abs(logdet - 2 * d * np.log(sigma)) <= 1e-9 * d     # log det Sigma_M = 2 d log sigma
        nrm = np.linalg.norm(out["Sigma_stage"], 2)
        assert np.abs(out["G64"] @ out["G64"].T - out["Sigma_stage"]).max() <= 1e-13 * nrm   # G G^T = P Sigma_M P^T
        G = out["G"].astype(np.float64)
        assert np.abs(G @ G.T - out["Sigma_stage"]).max() <= 2e-7 * nrm                      # ... and after the one rounding
        assert np.linalg.matrix_rank(out["Sigma_stage"], tol=1e-9 * nrm) == d
        assert np.all(np.triu(out["L"], 1) == 0.0) and np.all(np.diag(out["L"]) > 0.0)
    rm = SO.project(SO.crafted("repeated", W), W)
    ev = np.linalg.eigvalsh(rm)
    assert np.sum(np.abs(ev - 3.0) < 1e-8) == 3 and np.sum(np.abs(ev - 7.0) < 1e-8) == 2
    # R = 0 gives Sigma_M = sigma^2 I, the fallback's covariance
    z = SO.solve(SO.crafted("zero"), W, sigma)
    assert np.abs(z["SigmaM"] - sigma * sigma * np.eye(d)).max() <= 1e-15
    fb = SO.fallback(W, sigma)
    assert np.abs(z["Sigma_stage"] - fb["Sigma_stage"]).max() <= 1e-15 and np.abs(z["G64"] - sigma * P).max() <= 1e-15
    assert np.array_equal(fb["G"], (sigma * P).astype(np.float32))


def test_oracle_sampler_self_checks():
    rng = np.random.default_rng(0)
    d, N = 12, 40
    G = SO.random_factor(d, 0)
    mu = SO.clip_live_mean(0)
    eps = rng.normal(size=(N, 32, 4)).astype(np.float32)
    a64, pre, mag = SO.sample64(G, mu, eps)
    assert a64.shape == mag.shape == (N, 32, 4) and a64.min() == -1.0 and a64.max() == 1.0  # the clip is live on both sides
    assert ((a64 > -1.0) & (a64 < 1.0)).any()
    # the explicit fmaf chain lies within the forward bound of the fp64 value (plus the one add of mu), and is no plain copy of it
    w = SO.sample_words(G, mu, eps)
    bound = SO.chain_bound(d, mag) + 2 * SO.U * (np.abs(mu.reshape(1, 32, 4).astype(np.float64)) + mag)
    assert w.dtype == np.float32 and np.all(np.abs(w.astype(np.float64) - a64) <= bound)
    assert not np.array_equal(w.astype(np.float64), a64)
    # draws m >= d / 4 are not read
    eps2 = eps.copy()
    eps2[:, d // 4:] = 99.0
    assert np.array_equal(SO.sample64(G, mu, eps2)[0], a64) and np.array_equal(SO.sample_words(G, mu, eps2), w)
    # entry c of the chain is component c mod 4 of draw c div 4
    one = np.zeros((128, d), dtype=np.float32)
    one[5, 6] = 1.0
    small = (0.1 * eps).astype(np.float32)  # (no clip)
    a1, _, _ = SO.sample64(one, np.zeros(128, np.float32), small)
    assert np.array_equal(a1[:, 1, 1], small[:, 1, 2].astype(np.float64)) and np.count_nonzero(a1) == N
