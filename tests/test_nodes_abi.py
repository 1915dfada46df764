"""CPU: the ABI of the annealed step's spline nodes (covo_set_step_nodes / covo_step_nodes / covo_noise_nodes_philox,
include/covo_hip.h: COVO_HAS_STEP_NODES), its Python surface (controllers/_options.py: node_basis, node_schedule, check_dial's nodes= /
node_interp=; the controllers' keyword-only nodes=), and the self-checks of tests/nodes_oracle.py."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from tests import nodes_oracle as NO
from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)


def _env(disturb="gaussian"):
    import covo_mpc_amd as cm
    return cm.envs.Quad3D(task="tracking_zigzag", disturb_type=disturb, enable_randomizer=False, disable_rollover_terminate=True,
                          generate_noisy_state=True, device=None)


# ------------------------------------------------------------------------------------------ 1: header and ABI
def test_header_macro_symbols_and_prototypes(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"^#define COVO_HAS_STEP_NODES 1$", hdr, flags=re.M) and built.COVO_HAS_STEP_NODES == 1
    assert re.search(r"int covo_set_step_nodes\(covo_handle_t h, const float \*basis_table, int32_t n_pass, int32_t n_nodes\);", hdr)
    assert re.search(r"int covo_noise_nodes_philox\(covo_handle_t h, const float \*basis, int32_t n_nodes, const float \*mu, "
                     r"uint32_t key0, uint32_t key1,\s+int64_t sample_offset, int32_t N, float \*a_out, void \*stream\);", hdr)
    assert re.search(r"int covo_step_nodes\(covo_handle_t h, int32_t \*n_pass, int32_t \*n_nodes\);", hdr)
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()
    P, I, F, U32, I64 = C.c_void_p, C.c_int32, C.c_float, C.c_uint32, C.c_int64
    fn = lib.covo_set_step_nodes
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, C.POINTER(F), I, I]
    fn = lib.covo_noise_nodes_philox
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, P, I, P, U32, U32, I64, I, P, P]
    fn = lib.covo_step_nodes
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, C.POINTER(I), C.POINTER(I)]
    for name in ("covo_set_step_nodes", "covo_noise_nodes_philox", "covo_step_nodes"):
        assert name in built.EXPORTS, name
    # a null handle is refused by name before anything else happens (no GPU needed)
    assert lib.covo_set_step_nodes(None, None, 0, 0) != 0 and b"covo_set_step_nodes: null handle" in lib.covo_last_error()
    assert lib.covo_noise_nodes_philox(None, None, 8, None, 0, 0, 0, 16, None, None) != 0
    assert b"covo_noise_nodes_philox: null handle" in lib.covo_last_error()
    assert lib.covo_step_nodes(None, None, None) != 0 and b"covo_step_nodes: null handle" in lib.covo_last_error()


def test_the_python_surface(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers import _options as O
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    for fn in (controllers.DialController.__init__, controllers.BatchedDialController.__init__, get_controller, eval_env_batched):
        p = inspect.signature(fn).parameters
        assert p["nodes"].default is None and p["node_interp"].default == "linear", fn
        assert p["nodes"].kind is p["node_interp"].kind is inspect.Parameter.KEYWORD_ONLY, fn
    # every existing parameter position is unchanged: the new keywords stand behind the old ones
    g = list(inspect.signature(get_controller).parameters)
    assert g[-5:] == ["beta_pass", "beta_stage", "temp", "nodes", "node_interp"]
    e = list(inspect.signature(eval_env_batched).parameters)
    assert e[-5:] == ["beta_pass", "beta_stage", "temp", "nodes", "node_interp"]
    c = inspect.signature(O.check_dial).parameters
    assert c["nodes"].default is None and c["node_interp"].default == "linear"
    for name in ("noise_nodes", "step_nodes", "attach_anneal"):
        assert callable(getattr(SamplingCore, name)), name
    assert list(inspect.signature(SamplingCore.noise_nodes).parameters) == ["self", "basis", "mu", "key"]
    assert callable(O.node_basis) and callable(O.node_schedule)
    f = {x.name: x for x in O.Anneal.__dataclass_fields__.values()}
    assert list(f)[:4] == ["sigma", "temp", "beta_pass", "beta_stage"]
    assert [f[n].default for n in ("nodes", "node_interp", "node_sigma", "basis", "weights")] == [None, "linear", None, None, None]
    # not a step option, not a switch
    assert not {"nodes", "node_interp"} & (set(O.STEP_OPTION_DEFAULTS) | set(O.STEP_SWITCH_DEFAULTS))


# ------------------------------------------------------------------------------------------ 2: node_basis
@pytest.mark.parametrize("interp", NO.INTERPS)
@pytest.mark.parametrize("M", NO.MS)
def test_node_basis_properties(M, interp):
    from covo_mpc_amd.controllers._options import node_basis
    W = node_basis(M, interp)
    t = NO.node_times(M)
    assert W.shape == (32, M) and W.dtype == np.float64
    assert np.abs(W.sum(axis=1) - 1.0).max() <= 1e-12 * 31
    assert np.abs(W @ t - np.arange(32)).max() <= 1e-12 * 31
    first, last = np.zeros(M), np.zeros(M)
    first[0] = last[-1] = 1.0
    assert np.array_equal(W[0], first) and np.array_equal(W[31], last)
    if M == 2:
        h = np.arange(32, dtype=np.float64)
        assert np.abs(W - np.stack([1.0 - h / 31.0, h / 31.0], axis=1)).max() <= 1e-15
        assert np.abs(node_basis(2, "cubic") - node_basis(2, "linear")).max() <= 1e-15
    if interp == "linear":
        assert W.min() >= 0.0 and W.max() <= 1.0 and ((W != 0.0).sum(axis=1) <= 2).all()
        if M == 32:
            assert np.array_equal(W, np.eye(32))
    # a stage that is a node carries that node's unit vector; the oracle's restatement by the plain formulas agrees to rounding
    for m, tm in enumerate(t):
        if tm == int(tm):
            assert W[int(tm), m] == 1.0 and np.count_nonzero(W[int(tm)]) == 1, (m, tm)
    assert np.abs(W - NO.basis64(M, interp)).max() <= 1e-12


def test_node_basis_refuses_what_is_no_basis():
    from covo_mpc_amd.controllers._options import node_basis
    for M, interp in ((1, "linear"), (33, "linear"), (8, "quintic")):
        with pytest.raises(ValueError, match="node_basis"):
            node_basis(M, interp)


# ------------------------------------------------------------------------------------------ 3: tables
def test_tables_at_the_neutral_element_are_the_schedule():
    from covo_mpc_amd.controllers._options import anneal_schedule, check_dial, node_schedule
    for k, bp, bs in ((3, 0.5, 0.9), (1, 1.0, 1.0), (4, 0.7, 0.83)):
        s = anneal_schedule(0.5, k, bp, bs)
        sn, B, se, W = node_schedule(0.5, k, bp, bs, 32, "linear")
        assert B.shape == (k, 32, 32) and B.dtype == se.dtype == np.float32 and sn.dtype == np.float64
        for i in range(k):
            assert np.array_equal(B[i].view(np.uint32), np.diag(s[i]).astype(np.float32).view(np.uint32))
        assert np.array_equal(se.view(np.uint32), s.view(np.uint32))
        a = check_dial(k, beta_pass=bp, beta_stage=bs, temp=None, nodes=32)
        assert np.array_equal(a.sigma.view(np.uint32), s.view(np.uint32)) and a.nodes == 32 and a.temp == 0.0


def test_tables_against_hand_values():
    """M = 2, k = 2, sigma0 = 0.5, beta_pass = 0.5, beta_stage = 0.9: W[h] = [1 - h / 31, h / 31], sigma_n = [[0.45, 0.5], [0.225, 0.25]];
    every entry the fp32 rounding of the fp64 product, sigma_e from the rounded entries."""
    from covo_mpc_amd.controllers._options import node_schedule
    f32, f64 = np.float32, np.float64
    sn, B, se, W = node_schedule(0.5, 2, 0.5, 0.9, 2, "linear")
    assert np.array_equal(sn, np.array([[0.5 * 0.9, 0.5], [0.5 * 0.5 * 0.9, 0.5 * 0.5]]))
    assert B.shape == (2, 32, 2) and se.shape == (2, 32)
    assert B[0, 0, 0] == f32(0.5 * 0.9) and B[0, 0, 1] == 0.0 and B[0, 31, 0] == 0.0 and B[0, 31, 1] == f32(0.5)
    assert B[1, 31, 1] == f32(0.25) and B[1, 0, 0] == f32(0.5 * 0.5 * 0.9)
    assert B[0, 10, 0] == f32((0.5 * 0.9) * (21.0 / 31.0)) and B[0, 10, 1] == f32(0.5 * (10.0 / 31.0))
    assert B[1, 20, 0] == f32((0.5 * 0.5 * 0.9) * (11.0 / 31.0)) and B[1, 20, 1] == f32(0.25 * (20.0 / 31.0))
    assert se[0, 0] == f32(0.5 * 0.9) and se[0, 31] == f32(0.5) and se[1, 31] == f32(0.25)
    assert se[0, 10] == f32(np.sqrt(f64(B[0, 10, 0]) ** 2 + f64(B[0, 10, 1]) ** 2))
    assert se[1, 20] == f32(np.sqrt(f64(B[1, 20, 0]) ** 2 + f64(B[1, 20, 1]) ** 2))
    # between two independent nodes the marginal dips below both
    assert se[0, 15] < min(se[0, 0], se[0, 31])
    # the oracle's restatement, every M and both interpolations, as words
    from covo_mpc_amd.controllers._options import node_basis
    for M in NO.MS:
        for interp in NO.INTERPS:
            sn, B, se, W = node_schedule(0.5, 3, 0.5, 0.9, M, interp)
            assert np.array_equal(W, node_basis(M, interp))
            sn2, B2, se2 = NO.tables64(0.5, 3, 0.5, 0.9, M, W)
            assert np.array_equal(sn, sn2) and np.array_equal(B.view(np.uint32), B2.view(np.uint32))
            assert np.array_equal(se.view(np.uint32), se2.view(np.uint32))


# ------------------------------------------------------------------------------------------ 4: check_dial and the constructors
def test_check_dial_old_calls_behave_as_before(built):
    from covo_mpc_amd.controllers._options import Anneal, anneal_schedule, check_dial
    assert check_dial(3, beta_pass=1.0, beta_stage=1, temp=None) is None
    a = check_dial(3, beta_pass=1.0, beta_stage=1.0, temp=0.25)
    assert isinstance(a, Anneal) and a.temp == 0.25 and a.sigma.shape == (3, 32) and np.all(a.sigma == np.float32(0.5))
    assert a.nodes is None and a.basis is None and a.node_sigma is None and a.weights is None and a.node_interp == "linear"
    a = check_dial(2, beta_pass=0.5, beta_stage=0.9, temp=None)
    assert np.array_equal(a.sigma, anneal_schedule(0.5, 2, 0.5, 0.9))
    with pytest.raises(ValueError, match="iters="):
        check_dial(0, beta_pass=2.0, beta_stage=0.0, temp=-1.0, gamma_sigma=0.5, materialize_eps=True)
    with pytest.raises(ValueError, match="gamma_sigma=0.5"):
        check_dial(4, gamma_sigma=0.5, materialize_eps=True)
    with pytest.raises(NotImplementedError, match="kernel-by-kernel path"):
        check_dial(4, materialize_eps=True)


def test_check_dial_nodes_objections_and_their_place_in_the_order(built):
    from covo_mpc_amd.controllers._options import Anneal, check_dial
    for bad in (1, 33, 2.5, True, "8"):
        with pytest.raises(ValueError, match="nodes="):
            check_dial(4, nodes=bad)
    for bad in ("quadratic", None, 3):
        with pytest.raises(ValueError, match="node_interp="):
            check_dial(4, nodes=8, node_interp=bad)
    with pytest.raises(ValueError, match="node_interp="):  # (also without nodes: the name is checked as given)
        check_dial(4, node_interp="spline")
    with pytest.raises(ValueError, match="temp="):  # a bad temp wins over a bad nodes
        check_dial(4, temp=-1.0, nodes=1, gamma_sigma=0.5)
    with pytest.raises(ValueError, match="beta_stage="):
        check_dial(4, beta_stage=0.0, nodes=1)
    with pytest.raises(ValueError, match="nodes="):  # a bad nodes wins over node_interp, gamma_sigma and the path
        check_dial(4, nodes=1, node_interp="x", gamma_sigma=0.5, materialize_eps=True)
    with pytest.raises(ValueError, match="node_interp="):
        check_dial(4, nodes=8, node_interp="x", gamma_sigma=0.5)
    with pytest.raises(ValueError, match="gamma_sigma=0.5"):
        check_dial(4, nodes=8, gamma_sigma=0.5, materialize_eps=True)
    with pytest.raises(NotImplementedError, match="kernel-by-kernel path"):
        check_dial(4, nodes=8, materialize_eps=True)
    # with nodes given there is always an attachment, also at the schedule's neutral element
    a = check_dial(3, beta_pass=1.0, beta_stage=1.0, temp=None, nodes=8)
    assert isinstance(a, Anneal) and a.temp == 0.0 and a.nodes == 8 and a.node_interp == "linear"
    assert a.basis.shape == (3, 32, 8) and a.basis.dtype == np.float32 and a.node_sigma.shape == (3, 8) and a.weights.shape == (32, 8)
    assert a.sigma.shape == (3, 32) and a.sigma.dtype == np.float32 and np.all(a.node_sigma == 0.5)
    assert a.sigma[0, 0] == np.float32(0.5) and a.sigma[0, 2] < np.float32(0.5)
    a = check_dial(2, nodes=np.int64(4), node_interp="cubic")
    assert a.nodes == 4 and type(a.nodes) is int and a.node_interp == "cubic" and a.temp == 0.1


def test_constructor_refusals_that_need_no_device(built):
    from covo_mpc_amd import controllers
    from covo_mpc_amd.envs.quadrotor import eval_env_batched, get_controller
    env = _env()
    with pytest.raises(ValueError, match="nodes=1"):
        get_controller(env, "dial", "N256_H32_lam0.01", nodes=1)
    with pytest.raises(ValueError, match="nodes=33"):
        get_controller(env, "dial", "N256_H32_lam0.01", iters=2, nodes=33)
    with pytest.raises(ValueError, match="node_interp='quintic'"):
        get_controller(env, "dial", "N256_H32_lam0.01", nodes=8, node_interp="quintic")
    with pytest.raises(ValueError, match="temp=0"):  # the order holds through the factory
        get_controller(env, "dial", "N256_H32_lam0.01", temp=0, nodes=1)
    with pytest.raises(ValueError, match="ess_min=8.0 with the annealed MPPI controller"):
        get_controller(env, "dial", "N256_H32_lam0.01", nodes=8, ess_min=8.0)
    with pytest.raises(ValueError, match="nodes=2.5"):
        eval_env_batched(env, 2, "N256_H32_lam0.01", controller="dial", nodes=2.5)
    with pytest.raises(ValueError, match="node_interp="):
        eval_env_batched(env, 2, "N256_H32_lam0.01", controller="dial", nodes=8, node_interp="")
    cp = controllers.MPPIParams(gamma_mean=1.0, gamma_sigma=0.0, discount=1.0, sample_sigma=0.5, a_mean=None, a_cov=None)
    with pytest.raises(ValueError, match="nodes=True"):
        controllers.DialController(env, cp, 256, 32, 0.01, nodes=True)
    with pytest.raises(ValueError, match="nodes='8'"):
        controllers.BatchedDialController(env, 3, 256, 32, 0.01, nodes="8")
    # every other controller name ignores the keywords at their defaults: pid needs no device
    c, _ = get_controller(env, "pid")
    assert type(c).__name__ == "PIDController"


# ------------------------------------------------------------------------------------------ the oracle's self-checks
def test_oracle_self_checks():
    rng = np.random.default_rng(0)
    M, N = 5, 40
    B = NO.random_basis(M, 0)
    mu = NO.clip_live_mean(0)
    eps = rng.normal(size=(N, 32, 4)).astype(np.float32)
    a64, mag = NO.sample64(B, mu, eps)
    assert a64.shape == mag.shape == (N, 32, 4) and a64.min() == -1.0 and a64.max() == 1.0  # the clip is live on both sides
    assert ((a64 > -1.0) & (a64 < 1.0)).any()
    # the explicit fmaf chain of the C oracle lies within the forward bound of the fp64 value, and is no plain copy of it
    w = NO.sample_words(B, mu, eps)
    assert w.dtype == np.float32 and np.all(np.abs(w.astype(np.float64) - a64) <= NO.bound(M, mag))
    # entries m >= M of eps are not read
    eps2 = eps.copy()
    eps2[:, M:] = 99.0
    assert np.array_equal(NO.sample64(B, mu, eps2)[0], a64) and np.array_equal(NO.sample_words(B, mu, eps2), w)
    # a diagonal basis is the per-stage draw
    s = np.linspace(0.1, 0.5, 32).astype(np.float32)
    a_d, _ = NO.sample64(np.diag(s), np.zeros(128, np.float32), eps)
    assert np.array_equal(a_d, np.clip(s.astype(np.float64)[None, :, None] * eps.astype(np.float64), -1, 1))
    # the host restatement of the device stream: standard normal, different per node and component
    z = NO.normal4_host(np.array([7, 9], dtype=np.uint32), 4096, 8)
    assert z.shape == (4096, 8, 4) and abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    assert abs(np.corrcoef(z[:, 0, 0], z[:, 0, 1])[0, 1]) < 0.06 and abs(np.corrcoef(z[:, 0, 0], z[:, 1, 0])[0, 1]) < 0.06


def test_rank_case_has_its_gap_on_the_cpu():
    """The GPU rank test's case, on the CPU: with the chosen key the oracle's sample matrix has singular value number 4 M more than 100
    times above the bar that number 4 M + 1 must stay under (and number 4 M + 1 of the EXACT product is rounding noise of fp64)."""
    from covo_mpc_amd import random as cr
    from covo_mpc_amd.controllers._options import node_schedule
    N, M = NO.RANK_N, NO.RANK_M
    for interp in NO.INTERPS:
        _, B, _, _ = node_schedule(NO.RANK_SIGMA, 1, 0.5, 0.9, M, interp)
        eps = NO.normal4_host(cr.PRNGKey(NO.RANK_KEY_SEED), N, M)
        a64, _ = NO.sample64(B[0], np.zeros(128, np.float32), eps.astype(np.float32))
        assert np.abs(a64).max() < 1.0  # no clip
        sv = np.linalg.svd(a64.reshape(N, 128), compute_uv=False)
        bar = NO.rank_bar(N, M, np.abs(a64).max())
        print(f"  {interp}: sv[4M-1] {sv[4 * M - 1]:.4g} sv[4M] {sv[4 * M]:.4g} bar {bar:.4g}")
        assert sv[4 * M - 1] > 100.0 * bar and sv[4 * M] <= bar
