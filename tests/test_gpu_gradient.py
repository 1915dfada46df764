"""GPU tests (-m gpu) of covo_cost_gradient (csrc/cost_gradient.hip; SamplingCore.cost_gradient): the gradient of the Hessian's own
objective by the first-order adjoint, fp64, against torch.func.jacfwd of oracle/ref_torch.py::make_objective.

Cases: the state of tests/test_gpu_models.py's Hessian test (make_problem(seed=3, time=41), a[3, 1] = 1.0: a clip tie, two clips on
the path) and three upset states of tests/state_atlas.py (yaw_pi_minus, inverted, far_fast), each with kinds none / periodic / drag
(adj13 without and with a force table, adj16) and both rewards.  Bars, the Hessian test's:
  kind none                       1e-9 max(1, max|g|)
  kernel fed its fp32 table       1e-9 against the oracle fed the same rows (periodic: the table's rows ARE the held draws, so the
                                  oracle takes them as its draws; drag: the table is all zeros -- the force is the model's own function
                                  of the velocity -- so the model functions are "the same rows")
  against the fp64 model functions  1e-6 (periodic: what the draws' fp32 rounding moves the gradient by)
Rows 124 .. 127 are exactly 0; a batch gives the bits of its singles; covo_hessian's result is untouched by a gradient call.

The consistency check that needs no oracle: g(a + eps v) - g(a - eps v) against R (a+ - a-) with R = core.hessian(a), eps = 1e-4, v a
unit vector that is 0 at the clip tie (the objective is not smooth across it), a+- rounded to fp32 as the device takes them.  The bar
is 10 x the torch oracle's own finite-difference error on the same case -- |(g_ref(a+) - g_ref(a-)) - R_ref (a+ - a-)|_max = 1.7e-14 on
differences of 7.8e-5 (truncation eps^3 and fp64 rounding; measured once on the CPU) -- FD_BAR = 1.7e-13.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from oracle import ref_torch as RT  # noqa: E402
from tests.conftest import make_problem  # noqa: E402
from tests.gpu_support import DEV, DP, dev_state, params_c, uniform_draws  # noqa: E402
from tests.state_atlas import atlas_state  # noqa: E402

CASES = ("hessian_case", "yaw_pi_minus", "inverted", "far_fast")
KINDS = ("none", "periodic", "drag")
REWARDS = ("penyaw", "realworld")
KEY = cr.PRNGKey(21)
FD_BAR = 1.7e-13


@functools.lru_cache(maxsize=None)
def _core():
    return SamplingCore(256, 32, 0.01, 1.0, device=DEV)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(s, p, a [128] fp32): the state, the parameters with every disturbance parameter live, the action the gradient is taken at"""
    s, p, rng = make_problem(seed=3, time=41) if name == "hessian_case" else atlas_state(name)
    p = p.replace(disturb_params=DP)
    a = (R.hover_action(p, 32, np.float64) + 0.1 * rng.normal(size=(32, 4))).astype(np.float32)
    if name == "hessian_case":
        a[3, 1] = 1.0
    return s, p, a.reshape(-1)


def _grad_ref(s, p, a, reward, kind, draws):
    f = RT.make_objective(s, p, 32, reward, kind, draws)
    return torch.func.jacfwd(f)(torch.as_tensor(a, dtype=torch.float64)).numpy()


def _table(core, pc, packed, kind, batch=1, keys_dev=None):
    if kind == "none":
        return None
    return core.disturb_table(pc, packed, key=None if keys_dev is not None else KEY, keys_dev=keys_dev,
                              key_mode=_lib.DISTURB_KEYS_HESSIAN, deterministic=True, batch=batch)


def _device_gradient(name, kind, reward):
    core = _core()
    s, p, a = _case(name)
    ds = dev_state(s)
    pc = params_c(p, kind, reward)
    tab = _table(core, pc, ds.packed, kind)
    g = core.cost_gradient(ds, pc, torch.from_numpy(a).to(DEV), f_steps=tab)
    return g[0].cpu().numpy(), (tab[0].cpu().numpy() if tab is not None else None)


@pytest.mark.parametrize("reward", REWARDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", CASES)
def test_cost_gradient_vs_ad_oracle(name, kind, reward):
    s, p, a = _case(name)
    g, tab = _device_gradient(name, kind, reward)
    assert g.shape == (128,) and g.dtype == np.float64 and np.all(np.isfinite(g))
    assert np.all(g[124:] == 0.0)  # the last action reaches no rewarded state
    a64 = a.astype(np.float64)
    draws = uniform_draws(p, KEY, _lib.DISTURB_KEYS_HESSIAN).astype(np.float64) if kind == "periodic" else None
    ref = _grad_ref(s, p, a64, reward, kind, draws)
    big = max(1.0, np.abs(ref).max())
    err = np.abs(g - ref).max()
    print(f"{name} {kind} {reward}: max|g| {np.abs(ref).max():.3e} err vs model functions {err:.3e}")
    assert np.abs(ref[:124]).max() > 1e-3  # a live gradient
    if kind == "periodic":
        # the oracle fed the kernel's own rows: row k + 1 holds the force step k's redraw leaves (held between redraws)
        rows = np.vstack([tab[1:, :3], np.zeros((1, 3))]).astype(np.float64)
        ref_t = _grad_ref(s, p, a64, reward, kind, rows)
        err_t = np.abs(g - ref_t).max()
        print(f"    err vs the oracle fed the same rows {err_t:.3e}")
        assert err_t < 1e-9 * max(1.0, np.abs(ref_t).max()), err_t
        assert err < 1e-6 * big, err
        assert np.abs(ref - _grad_ref(s, p, a64, reward, "none", None)).max() > 1e-6  # the force matters
    else:
        assert tab is None or not tab.any()  # drag: nothing in the table, the rows are the model functions
        assert err < 1e-9 * big, err
    if name == "hessian_case":
        assert abs(g[13] - ref[13]) < 1e-9 and ref[13] != 0.0  # the tie entry is live (jnp.clip's JVP passes 0.5 per clip)


@pytest.mark.parametrize("kind,reward", [("none", "penyaw"), ("periodic", "realworld"), ("drag", "penyaw")])
def test_batch_equals_singles_bit_for_bit(kind, reward):
    """Four entries with their own states, actions and (periodic) keys and tables: entry b of the batch is the single call's bits."""
    core = _core()
    names = ("yaw_pi_minus", "inverted", "far_fast", "yaw_cross")  # (one trajectory: the atlas entries share make_problem's)
    cases = [_case(n) for n in names]
    p = cases[0][1]
    pc = params_c(p, kind, reward)
    packed = torch.stack([dev_state(s).packed for s, _, _ in cases])
    am = torch.stack([torch.from_numpy(a).to(DEV) for _, _, a in cases])
    keys = np.stack([cr.PRNGKey(100 + b) for b in range(4)]).astype(np.uint32)
    kd = torch.from_numpy(keys.view(np.int32)).to(DEV)
    tab = _table(core, pc, packed, kind, batch=4, keys_dev=kd)
    ds0 = dev_state(cases[0][0])
    gb = core.cost_gradient(ds0, pc, am, f_steps=tab, packed=packed).cpu().numpy()
    assert gb.shape == (4, 128)
    for b in range(4):
        one = core.cost_gradient(ds0, pc, am[b], f_steps=None if tab is None else tab[b:b + 1].contiguous(),
                                 packed=packed[b:b + 1].contiguous()).cpu().numpy()[0]
        assert np.array_equal(one.view(np.uint64), gb[b].view(np.uint64)), b
    assert len({gb[b].tobytes() for b in range(4)}) == 4  # four different gradients


def test_hessian_is_untouched_by_a_gradient_call():
    """The gradient has a workspace of its own: core.hessian before and after a cost_gradient call gives the same bits."""
    core = _core()
    s, p, a = _case("hessian_case")
    ds = dev_state(s)
    pc = params_c(p, "drag", "penyaw")
    tab = _table(core, pc, ds.packed, "drag")
    ad = torch.from_numpy(a).to(DEV)
    R0 = core.hessian(ds.packed, ds, pc, ad, f_steps=tab).cpu().numpy()
    g = core.cost_gradient(ds, pc, ad, f_steps=tab)
    R1 = core.hessian(ds.packed, ds, pc, ad, f_steps=tab).cpu().numpy()
    assert np.isfinite(g.cpu().numpy()).all()
    assert np.array_equal(R0.view(np.uint64), R1.view(np.uint64))


def test_gradient_differences_equal_the_hessian_along_a_direction():
    core = _core()
    s, p, a = _case("hessian_case")
    ds = dev_state(s)
    pc = params_c(p, "none", "penyaw")
    v = np.random.default_rng(7).normal(size=128)
    v[13] = 0.0  # the clip tie: not smooth across it
    v /= np.linalg.norm(v)
    eps = 1e-4
    ap = (a.astype(np.float64) + eps * v).astype(np.float32)
    am = (a.astype(np.float64) - eps * v).astype(np.float32)
    g = core.cost_gradient(ds, pc, torch.from_numpy(np.stack([ap, am])).to(DEV)).cpu().numpy()
    Rm = core.hessian(ds.packed, ds, pc, torch.from_numpy(a).to(DEV))[0].cpu().numpy()
    step = ap.astype(np.float64) - am.astype(np.float64)
    want = Rm @ step
    err = np.abs((g[0] - g[1]) - want).max()
    print(f"finite difference against R: err {err:.3e} on differences of {np.abs(want).max():.3e} (bar {FD_BAR:.1e})")
    assert np.abs(want).max() > 1e-5
    assert err < FD_BAR, err
