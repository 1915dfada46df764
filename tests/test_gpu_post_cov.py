"""GPU tests (-m gpu) of the posterior covariance (covo_weighted_cov / covo_set_step_post_cov; `compute_post_cov`, core.weighted_cov):
the weighted 128 x 128 sample covariance of a step's own samples under the step's own weights (csrc/post_cov.hip).

Bars.  Against ref_weighted_cov (tests/test_post_cov_abi.py: the definition in fp64) on the kernel's own fp32 a, cost and mu,
elementwise:   |C - C_ref|[j,k] <= (N_ACC + 4) 2^-24 sum_i w_i |y_ij| |y_ik| / W + 2^-24 |C_ref[j,k]|,
N_ACC = 64 = PC_NACC of post_cov.hip: the products one fp32 accumulator sums before it is flushed into an fp64 total; + 4: the
roundings of w y, of the two y = x - mu and of the partial; 2^-24 |C_ref|: the final rounding.  Every test prints its worst ratio
to the bar.  Symmetry, batch against single launches, run against run, N = 1, the attached matrix against the stand-alone call on
the step's buffers, the env-batched controller against its instances run singly, a step with the option against its twin without:
none (torch.equal).  mu + d against covo_softmax_update's a_mean at gamma_mean = 1: 1e-5, the bar tests/test_gpu_parity.py holds
that update to against its oracle.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from tests.gpu_support import DEV, batched_controller, quad_env, start_episode  # noqa: E402
from tests.post_cov_oracle import ref_weighted_cov  # noqa: E402

H, NA = 32, 128
N_ACC = 64  # post_cov.hip: PC_NACC
U = 2.0 ** -24
SIZES = [1, 63, 64, 65, 257, 4096]
MEAN_BAR = 1e-5


@pytest.fixture(scope="module")
def core():
    c = SamplingCore(4096, H, 0.5, 1.0, device=DEV)
    yield c
    assert c.device_status() == 0
    c.close()


def _inputs(N, seed):
    """random clipped stripes a [H, N, 4] about a mean away from 0, costs [N], mu [128] -- fp32, on the device"""
    rng = np.random.default_rng(1000 * seed + N)
    mu = rng.uniform(-0.3, 0.6, NA).astype(np.float32)
    a = np.clip(mu.reshape(H, 1, 4) + 0.4 * rng.normal(size=(H, N, 4)), -1, 1).astype(np.float32)
    cost = (5.0 + 2.0 * rng.normal(size=N)).astype(np.float32)
    return torch.from_numpy(a).to(DEV), torch.from_numpy(cost).to(DEV), torch.from_numpy(mu).to(DEV)


def _ratio(C, a, cost, mu, where, **kw):
    """C (device) against the reference on the same fp32 inputs -> the worst ratio to the bar, printed and asserted <= 1"""
    Cr, dr, Wr, absS = ref_weighted_cov(a.cpu().numpy(), cost.cpu().numpy(), mu.cpu().numpy(), **kw)
    Cd = C.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(Cd)), where
    bar = (N_ACC + 4) * U * absS + U * np.abs(Cr)
    err = np.abs(Cd - Cr)
    ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"  {where}: worst |C - C_ref| / bar = {ratio:.3f}")
    assert ratio <= 1.0, (where, ratio)
    return Cr, dr, Wr


def _sym(C):
    return torch.equal(C, C.transpose(-1, -2).contiguous())


# ------------------------------------------------------------------------------------------ 1: the stand-alone entry
@pytest.mark.parametrize("N", SIZES)
def test_weighted_cov_vs_reference(core, N):
    """Random a and cost at a temperature that keeps many samples alive (lam = 0.5) and at one that keeps few (0.05): the bar, symmetry
    bit for bit, two runs bit-identical, d and W; N = 1: C = 0 exactly."""
    a, cost, mu = _inputs(N, 1)
    for lam in (0.5, 0.05):
        C, d, W = core.weighted_cov(a, cost, mu, lam=lam)
        C2, d2, W2 = core.weighted_cov(a, cost, mu, lam=lam)
        torch.cuda.synchronize()
        _, dr, Wr = _ratio(C, a, cost, mu, f"N={N} lam={lam}", lam=lam)
        assert _sym(C), N
        assert torch.equal(C, C2) and torch.equal(d, d2) and torch.equal(W, W2), N
        assert abs(float(W) - Wr) <= 1e-5 * Wr and np.abs(d.cpu().numpy() - dr).max() <= 1e-5, N
        if N == 1:
            assert bool((C == 0).all()) and float(W) == 1.0
            assert torch.equal(d, a[:, 0, :].reshape(-1) - mu)


def test_equal_costs_give_the_plain_covariance(core):
    N = 257
    a, cost, mu = _inputs(N, 2)
    cost.fill_(3.25)
    C, d, W = core.weighted_cov(a, cost, mu, lam=0.01)
    torch.cuda.synchronize()
    _ratio(C, a, cost, mu, "equal costs", lam=0.01)
    x = a.permute(1, 0, 2).reshape(N, NA).cpu().numpy().astype(np.float64)
    plain = np.cov(x.T, bias=True)
    assert float(W) == float(N) and _sym(C)
    assert np.abs(C.cpu().numpy() - plain).max() < 1e-5


def test_tiny_lam_gives_one_hot_weights_and_zero(core):
    N = 257
    a, cost, mu = _inputs(N, 3)
    cost[100] = float(cost.min()) - 1.0
    C, d, W = core.weighted_cov(a, cost, mu, lam=1e-6)
    torch.cuda.synchronize()
    Cr, _, Wr = _ratio(C, a, cost, mu, "one-hot", lam=1e-6)
    assert Wr == 1.0 and float(W) == 1.0 and np.all(Cr == 0.0) and _sym(C)
    assert torch.equal(d, a[:, 100, :].reshape(-1) - mu)


def test_nonfinite_costs_get_weight_zero(core):
    """One NaN and one +inf cost, the NaN sample's stripe NaN as well: both weigh 0 and C is finite and within the bar."""
    N = 257
    a, cost, mu = _inputs(N, 4)
    cost[5], cost[200] = float("nan"), float("inf")
    a[:, 5, :] = float("nan")
    C, d, W = core.weighted_cov(a, cost, mu, lam=0.5)
    torch.cuda.synchronize()
    _ratio(C, a, cost, mu, "NaN + inf costs", lam=0.5)
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(W)) and _sym(C)


@pytest.mark.parametrize("N", [65, 4096])
def test_elite_weights_with_ties_at_the_boundary(core, N):
    """elite_K in {1, 5, N}; the 3rd .. 8th cheapest costs are equal, so K = 5 cuts through a tie: the set must be the selector's --
    lowest indices win -- which the reference's weights restate."""
    a, cost, mu = _inputs(N, 5)
    order = torch.argsort(cost)
    cost[order[2:8]] = float(cost[order[2]])
    for K in (1, 5, N):
        C, d, W = core.weighted_cov(a, cost, mu, elite=K)
        torch.cuda.synchronize()
        _, dr, Wr = _ratio(C, a, cost, mu, f"elite N={N} K={K}", elite=K)
        assert float(W) == float(K) == Wr and _sym(C)
        assert np.abs(d.cpu().numpy() - dr).max() <= 1e-5
        if K == 1:
            assert bool((C == 0).all())


def test_batch_of_three_equals_three_single_launches(core):
    N = 257
    trip = [_inputs(N, 10 + e) for e in range(3)]
    a, cost, mu = (torch.stack([t[i] for t in trip]).contiguous() for i in range(3))
    for kw in (dict(lam=0.5), dict(elite=16)):
        Cb, db, Wb = core.weighted_cov(a, cost, mu, **kw)
        assert tuple(Cb.shape) == (3, NA, NA) and tuple(db.shape) == (3, NA) and tuple(Wb.shape) == (3,)
        for e in range(3):
            C1, d1, W1 = core.weighted_cov(*trip[e], **kw)
            assert torch.equal(Cb[e], C1) and torch.equal(db[e], d1) and torch.equal(Wb[e], W1), (kw, e)
    torch.cuda.synchronize()


@pytest.mark.parametrize("N", [257, 4096])
def test_posterior_mean_is_the_softmax_mean(N):
    """mu + d against the a_mean covo_softmax_update forms from the same cost, a and mu at gamma_mean = 1."""
    lam = 0.5
    a, cost, mu = _inputs(N, 6)
    c = SamplingCore(N, H, lam, 1.0, device=DEV)
    c.a.copy_(a)
    c.cost.copy_(cost)
    c.blockmin.copy_(torch.stack([cost[i:i + 64].min() for i in range(0, N, 64)]))
    mean = c.update(mu, 1.0)
    _, d, _ = c.weighted_cov(c.a, c.cost, mu)  # lam: the core's
    torch.cuda.synchronize()
    err = float((mu + d - mean).abs().max())
    print(f"  N={N}: |mu + d - a_mean| {err:.2e}")
    assert err < MEAN_BAR
    assert c.device_status() == 0
    c.close()


# ------------------------------------------------------------------------------------------ 2: attached to the step
def _controller(env, name, N, post, **kw):
    import covo_mpc_amd as cm
    c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV, compute_info=False, compute_post_cov=post, **kw)
    return c, c.init_control_params


CASES = [("mppi", {}), ("covo-offline", {}), ("covo-online", {}), ("covo-online", dict(ess_min=32.0)), ("mppi", dict(elite=16)),
         ("covo-online", dict(elite=16)), ("covo-online", dict(iters=2)), ("mppi", dict(iters=2)),
         ("covo-online", dict(compute_diag=True, compute_plan=True, compute_fan=8, update="guarded", sigma_period=2))]


@pytest.mark.parametrize("name,kw", CASES, ids=[f"{n}-{'+'.join(k) or 'plain'}" for n, k in CASES])
def test_step_post_cov_is_the_stand_alone_call_on_the_steps_buffers(name, kw):
    """N = 256, two steps of every controller, plain and next to the ESS floor, the elite set, two passes per step and everything
    else at once: info["post_cov"] / ["post_shift"] equal core.weighted_cov on the step's a and cost with the mean the (last) pass
    sampled around, at lam_eff / elite where those define the weights, bit for bit; u and a_mean equal a twin's built without the
    option, bit for bit.  (The bar against the reference is the stand-alone tests': a closed-loop step at lam = 0.01 is all but one-hot,
    with weights and products below fp32's normal range, where a relative bar says nothing.)"""
    N = 256
    env = quad_env(task="tracking_zigzag")
    ca, cpa = _controller(env, name, N, True, **kw)
    cb, cpb = _controller(env, name, N, False, **kw)
    cpa, obs, info, state, params = start_episode(env, ca, cpa, name)
    if name == "covo-offline":
        cpb = cpb.replace(a_cov_offline=cpa.a_cov_offline, a_chol_offline=cpa.a_chol_offline)
    key = cr.PRNGKey(21)
    core = ca.core
    for step in range(2):
        key, k_act, k_step = cr.split(key, 3)
        ua, cpa, ia = ca(obs, state, params, k_act, cpa, info)
        ub, cpb, ib = cb(obs, state, params, k_act, cpb, info)
        where = f"{name} {kw} step {step}"
        assert tuple(ia["post_cov"].shape) == (NA, NA) and tuple(ia["post_shift"].shape) == (NA,), where
        assert ia["post_cov"].data_ptr() == core.post_cov.data_ptr()  # views: no copy, no sync
        assert not any(k.startswith("post_") for k in ib), where
        mu = core._persistent("a_mean_shift", (NA,))  # the mean the step's last pass sampled around
        sel = dict(elite=kw["elite"]) if "elite" in kw else dict(lam=float(ia["lam_eff"]) if "ess_min" in kw else None)
        C, d, W = core.weighted_cov(core.a, core.cost, mu, **sel)
        torch.cuda.synchronize()
        assert torch.equal(ia["post_cov"], C) and torch.equal(ia["post_shift"], d) and torch.equal(ia["post_weight"], W), where
        assert _sym(C) and float(W) > 0.0, where
        assert torch.equal(ua, ub) and torch.equal(cpa.a_mean, cpb.a_mean), where
        assert torch.equal(core.cost, cb.core.cost) and torch.equal(core.a, cb.core.a), where
        obs, state, _, _, info = env.step(k_step, state, ua.cpu().numpy(), params)
    assert ca.core.device_status() == 0 and cb.core.device_status() == 0
    ca.core.close()
    cb.core.close()


def test_batched_online_post_cov_equals_its_instances_run_singly():
    """E = 3 domain-randomised instances, N = 256, one step from a BatchedDeviceEpisode's states: controller.post_cov[e] and
    post_aux[e] equal the single controller's on instance e alone, bit for bit."""
    import covo_mpc_amd as cm
    N, E = 256, 3
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    act_keys = np.stack([np.asarray(cr.PRNGKey(60 + e)) for e in range(E)])
    singles = []
    for e in range(E):
        c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False, compute_post_cov=True)
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        cp = c.reset(se.state0, params[e], c.init_control_params, cr.PRNGKey(2))
        c(None, None, params[e], act_keys[e], cp, {"noisy_state": se.noisy_state})
        torch.cuda.synchronize()
        singles.append((c.core.post_cov[0].clone(), c.core.post_aux[0].clone()))
        cp0 = c.init_control_params
        assert c.core.device_status() == 0
        c.core.close()
    b = batched_controller(env, "covo-online", cp0, E, N, 0.01, compute_post_cov=True)
    assert tuple(b.post_cov.shape) == (E, NA, NA) and tuple(b.post_aux.shape) == (E, _lib.COVO_POST_AUX_FLOATS)
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    b.bind_episode(ep)
    b(None, act_keys)
    torch.cuda.synchronize()
    for e in range(E):
        assert torch.equal(b.post_cov[e], singles[e][0]) and torch.equal(b.post_aux[e], singles[e][1]), e
        assert _sym(b.post_cov[e]) and float(b.post_aux[e, NA]) > 0.0
    assert b.core.device_status() == 0
    b.core.close()
