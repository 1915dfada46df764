"""GPU tests (-m gpu) of the Newton refinement (covo_newton_refine / covo_set_step_refine; `refine=` of the covo-online controllers;
csrc/newton_refine.hip, csrc/cost_gradient.hip).

1. stand-alone against numpy on the device's own inputs: g from cost_gradient, the fp32 Sigma of core.sigma, 1 / c^2 from
   numpy.linalg.eigh(R) -> d_ref = -Sigma (Sigma g) / c^2 in fp64.  choice == first argmin(costs_out) with NaN as +inf;
   costs_out[0] == covo_arbitrate's candidate-0 cost on b, bit for bit; the committed mean == fp32(clip(b + alpha d_ref)) within
   1.2e-7 (one fp32 rounding at |x| <= 1 = 6e-8, plus the fp64 sums' 1e-13 -- the rounding can fall the other way); costs_out[j]
   within 1e-5 relative (the rollout bar) of the fp64 oracle's cost of reference candidate j; cost_chosen <= cost_base.
2. it descends where it should: hover + 0.3 noise at far_fast (the seed picked on the CPU: the fp64 oracle's candidates fall from 36.6
   to 22.4, best at j = 3); g = 0 and NaN in Sigma keep the mean, bit for bit.
3. the production step against a twin without refine (same key, compute_plan, update="guarded"), disturbance gaussian / periodic / drag.
   refine_slope: the row is float32, so the device's fp64 g.d arrives rounded once more -- the bar is the issue's 1e-9 |Sigma g|^2 / c^2
   plus half an fp32 ulp of the reference value (2^-24 relative).  A c^2 from anywhere but this step's chain would miss it by orders.
4. batched (E = 3) equals three singles bit for bit; iters=2: the row is the last pass's; a 12-step run_episode equals 12 host calls.
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
from covo_mpc_amd.dynamics.dataclass import as_device_state  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from tests.conftest import make_problem  # noqa: E402
from tests.gpu_support import (DEV, DP, H, batched_controller, dev_state, disturb_key, params_c, quad_env, start_episode,  # noqa: E402
                               to_stripes)
from tests.state_atlas import atlas_state  # noqa: E402

RF = _lib.COVO_REFINE_FLOATS
NC = _lib.COVO_REFINE_CANDIDATES
ALPHA = 2.0 ** (3 - np.arange(1, NC))  # 4, 2, 1, ..., 2^-13
SIGMA = 0.5
COST_BAR = 1e-5
MEAN_BAR = 1.2e-7


def split_row(row):
    """refine row [8] (device tensor) -> (cost_base, cost_chosen, choice, alpha, |g|, g.d, word 6, flags) as numpy scalars / ints"""
    r = row.detach().cpu().numpy()
    i = np.ascontiguousarray(r).view(np.int32)
    return r[0], r[1], int(i[2]), r[3], r[4], r[5], r[6], int(i[7])


def host_choice(costs):
    """first argmin with NaN as +inf; nothing finite: 0"""
    c = np.where(np.isnan(costs), np.inf, costs.astype(np.float64))
    return int(np.argmin(c))


def inv_c2_of(Rm, sigma=SIGMA):
    """1 / c^2, c^2 = sigma^4 det(R + delta I)^(1/n) with delta = 1e-2 - lambda_min(R) (covo.py:116-128)"""
    e = np.linalg.eigh((Rm + Rm.T) / 2.0)[0]
    o = e - e.min() + 1e-2
    return 1.0 / (sigma ** 4 * np.exp(np.log(o).sum() / Rm.shape[0]))


def reference_candidates(b, Sigma, g, inv_c2):
    """(d_ref [128] fp64, candidates [17, 128] fp64 holding fp32 numbers) from the device's own inputs"""
    S = Sigma.astype(np.float64)
    d = -(S @ (S @ g)) * inv_c2
    b64 = b.astype(np.float64)
    cands = np.clip(b64[None] + ALPHA[:, None] * d[None], -1.0, 1.0).astype(np.float32).astype(np.float64)
    return d, np.concatenate([np.clip(b64, -1.0, 1.0)[None], cands])


def _tables(core, pc, ds, kind, key):
    """(rollout table, Hessian table, the oracle's disturbance) of a stand-alone case"""
    if kind == "none":
        return None, None, {}
    p = R.Params().fp32().replace(disturb_params=DP)
    tab_r = core.disturb_table(pc, ds.packed, key=key, key_mode=_lib.DISTURB_KEYS_SHARED, deterministic=True)
    tab_h = core.disturb_table(pc, ds.packed, key=key, key_mode=_lib.DISTURB_KEYS_HESSIAN, deterministic=True)
    draw = cr.uniform(disturb_key(key), (3,), -p.disturb_scale, p.disturb_scale).astype(np.float64)
    return tab_r, tab_h, dict(disturb=R.Disturb(kind, draw, True))


def _standalone_inputs(core, s, p, b, kind, reward):
    ds = dev_state(s)
    pc = params_c(p, kind, reward)
    tab_r, tab_h, dist = _tables(core, pc, ds, kind, cr.PRNGKey(5))
    bd = torch.from_numpy(b).to(DEV)
    Rm = core.hessian(ds.packed, ds, pc, bd, f_steps=tab_h)
    Sigma = core.sigma(Rm, SIGMA)[0][0].contiguous()
    g = core.cost_gradient(ds, pc, bd, f_steps=tab_h)[0]
    return ds, pc, tab_r, tab_h, dist, bd, Rm[0].cpu().numpy(), Sigma, g


# ------------------------------------------------------------------------------------------ 1: stand-alone against numpy
@pytest.mark.parametrize("kind,reward", [("none", "penyaw"), ("periodic", "realworld"), ("drag", "penyaw")])
def test_newton_refine_vs_numpy_on_the_devices_inputs(kind, reward):
    s, p, rng = make_problem(seed=17, time=37)
    p = p.replace(disturb_params=DP)
    b = (R.hover_action(p, 32, np.float64) + 0.3 * rng.normal(size=(32, 4))).astype(np.float32).reshape(-1)
    assert np.abs(b).max() > 1.0  # the clip has something to do
    core = SamplingCore(256, H, 0.01, 1.0, device=DEV, compute_info=False)
    ds, pc, tab_r, tab_h, dist, bd, Rm, Sigma, g = _standalone_inputs(core, s, p, b, kind, reward)
    ic = inv_c2_of(Rm)
    am = bd.clone()
    row, costs = core.newton_refine(ds, pc, am, Sigma, ic, f_steps=tab_r, f_steps_hessian=tab_h)
    # the gradient the entry point computes itself is cost_gradient's: handing it in changes no bit
    am2 = bd.clone()
    row2, costs2 = core.newton_refine(ds, pc, am2, Sigma, ic, f_steps=tab_r, f_steps_hessian=tab_h, g=g)
    torch.cuda.synchronize()
    assert torch.equal(row, row2) and torch.equal(costs, costs2) and torch.equal(am, am2)
    base, chosen, choice, alpha, gnorm, slope, w6, flags = split_row(row)
    c = costs.cpu().numpy()
    g64 = g.cpu().numpy()
    d_ref, cands = reference_candidates(b, Sigma.cpu().numpy(), g64, ic)
    where = f"{kind} {reward}: costs {c} choice {choice} flags {flags}"
    print("  " + where)
    assert flags == 0 and w6 == 0.0, where
    assert choice == host_choice(c), where
    assert base.tobytes() == c[0].tobytes() and chosen.tobytes() == c[choice].tobytes() and chosen <= base, where
    assert alpha == (ALPHA[choice - 1] if choice else 0.0), where
    # candidate 0 is the arbiter's candidate 0 on b (mask 1: the softmax mean alone)
    core.a.copy_(to_stripes(np.zeros((256, H, 4), dtype=np.float32)))
    core.cost.zero_()
    arb = core.arbitrate(ds, pc, bd.clone(), bd.clone(), 1, f_steps=tab_r)
    assert torch.equal(arb[0:1], costs[0:1]), (where, float(arb[0]))
    # the committed mean
    got = am.cpu().numpy()
    if choice == 0:
        assert got.tobytes() == b.tobytes(), where
    else:
        err = np.abs(got.astype(np.float64) - cands[choice]).max()
        print(f"    committed mean vs fp32(clip(b + alpha d_ref)): {err:.3e}; |d_ref|max {np.abs(d_ref).max():.3e}")
        assert err <= MEAN_BAR, (where, err)
    # every candidate's cost against the fp64 oracle on the reference candidates
    ref = CO.rollout(s, p, cands.reshape(NC, H, 4), 1.0, np.zeros(3), dtype=np.float64, reward=reward, **dist)
    rel = np.abs(c - ref) / np.maximum(np.abs(ref), 1.0)
    print(f"    rel err of the 17 costs vs the oracle: max {rel.max():.3e}")
    assert rel.max() < COST_BAR, (where, rel)
    # the row's fp64 side values, rounded to fp32
    assert abs(gnorm - np.linalg.norm(g64)) <= 2.0 ** -23 * np.linalg.norm(g64), where
    assert abs(slope - g64 @ d_ref) <= 1e-9 * abs(g64 @ d_ref) + 2.0 ** -24 * abs(g64 @ d_ref), where
    assert slope < 0.0, where
    assert core.device_status() == 0
    core.close()


# ------------------------------------------------------------------------------------------ 2: it descends where it should
def test_refine_descends_from_a_poor_mean_and_keeps_it_without_a_direction():
    s, p, _ = atlas_state("far_fast")
    b = (R.hover_action(p, 32, np.float64) + 0.3 * np.random.default_rng(1001).normal(size=(32, 4))).astype(np.float32).reshape(-1)
    core = SamplingCore(256, H, 0.01, 1.0, device=DEV, compute_info=False)
    ds, pc, _, _, _, bd, Rm, Sigma, g = _standalone_inputs(core, s, p, b, "none", "penyaw")
    ic = inv_c2_of(Rm)
    _, cands = reference_candidates(b, Sigma.cpu().numpy(), g.cpu().numpy(), ic)
    ref = CO.rollout(s, p, cands.reshape(NC, H, 4), 1.0, np.zeros(3), dtype=np.float64)
    gain = (ref[0] - ref[1:].min()) / abs(ref[0])
    print(f"  oracle costs {ref}, relative gain {gain:.3e}")
    assert gain >= 1e-3, ref  # the precondition, on the oracle alone
    am = bd.clone()
    row, costs = core.newton_refine(ds, pc, am, Sigma, ic)
    base, chosen, choice, alpha, _, _, _, flags = split_row(row)
    print(f"  device costs {costs.cpu().numpy()}, choice {choice}")
    assert flags == 0 and choice >= 1 and chosen < base and not torch.equal(am, bd)
    assert torch.equal(am, am.clamp(-1, 1))  # the candidate as it was rolled out
    # g = 0: d = 0, every candidate is clip(b), equal costs go to the lowest lane -- the mean is not written
    am0 = bd.clone()
    row0, costs0 = core.newton_refine(ds, pc, am0, Sigma, ic, g=torch.zeros(128, dtype=torch.float64, device=DEV))
    r0 = split_row(row0)
    assert r0[2] == 0 and r0[7] == 0 and r0[3] == 0.0 and r0[4] == 0.0 and r0[5] == 0.0, r0
    assert torch.equal(am0, bd)  # untouched
    assert len(set(costs0.cpu().numpy().tobytes()[4 * j:4 * j + 4] for j in range(NC))) == 1
    # NaN in Sigma: no direction, no candidate, the flag says so
    bad = Sigma.clone()
    bad[7, 9] = float("nan")
    amn = bd.clone()
    rown, costsn = core.newton_refine(ds, pc, amn, bad, ic)
    rn = split_row(rown)
    assert rn[2] == 0 and (rn[7] & 2) == 2 and rn[3] == 0.0, rn
    assert torch.equal(amn, bd) and rn[0].tobytes() == split_row(row)[0].tobytes()
    # 1 / c^2 not finite: bit 2
    amc = bd.clone()
    rowc, _ = core.newton_refine(ds, pc, amc, Sigma, float("inf"))
    assert split_row(rowc)[2] == 0 and (split_row(rowc)[7] & 4) == 4 and torch.equal(amc, bd)
    assert core.device_status() == 0
    core.close()


# ------------------------------------------------------------------------------------------ 3: the production step
def _controller(env, N, refine, **kw):
    import covo_mpc_amd as cm
    c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False, refine=refine, **kw)
    return c, c.init_control_params


@pytest.mark.parametrize("kind", ["gaussian", "periodic", "drag"])
def test_production_step_against_a_twin_without_refine(kind):
    N = 256
    env = quad_env(task="tracking_zigzag", disturb=kind)
    kw = dict(compute_plan=True, update="guarded")
    ca, cpa0 = _controller(env, N, True, **kw)
    cb, _ = _controller(env, N, False, **kw)
    assert cb.core.refine_rows is None and tuple(ca.core.refine_rows.shape) == (1, RF)
    cp, obs, info, state, params = start_episode(env, ca, cpa0, "covo-online")
    if kind != "gaussian":
        params = params.replace(disturb_params=np.asarray(DP, dtype=np.float32))
    key = cr.PRNGKey(11)
    choices = []
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        dstate = as_device_state(info["noisy_state"], DEV)
        ua, cpa, ia = ca(obs, state, params, k_act, cp, info)
        ub, cpb, ib = cb(obs, state, params, k_act, cp, info)
        torch.cuda.synchronize()
        core = ca.core
        base, chosen, choice, alpha, gnorm, slope, _, flags = split_row(core.refine_rows[0])
        where = f"{kind} step {step}: base {base} chosen {chosen} choice {choice} alpha {alpha} flags {flags}"
        print("  " + where)
        choices.append(choice)
        assert not any(k.startswith("refine_") for k in ib)
        assert ia["refine_cost"].data_ptr() == core.refine_rows[0, 1:2].data_ptr() and ia["refine_choice"].dtype == torch.int32
        assert int(ia["refine_choice"]) == choice and float(ia["refine_alpha"]) == float(alpha), where
        # nothing of the step itself changes
        assert torch.equal(core.a, cb.core.a) and torch.equal(core.cost, cb.core.cost) and torch.equal(cpa.a_cov, cpb.a_cov), where
        assert torch.equal(core.arbiter, cb.core.arbiter), where
        # the base is the committed mean's cost: the twin's plan, the arbiter's chosen cost
        assert torch.equal(core.refine_rows[0, 0:1], cb.core.plan[0, 0:1]), (where, float(cb.core.plan[0, 0]))
        assert torch.equal(core.refine_rows[0, 0:1], core.arbiter[0, 3:4]), where
        assert torch.equal(ia["cost_plan"].reshape(1), core.refine_rows[0, 1:2]), (where, float(ia["cost_plan"]))
        assert flags == 0 and chosen <= base, where
        if choice == 0:
            assert torch.equal(cpa.a_mean, cpb.a_mean), where
        else:
            assert not torch.equal(cpa.a_mean, cpb.a_mean) and torch.equal(cpa.a_mean, cpa.a_mean.clamp(-1, 1)), where
        # the slope: g at the twin's (= the committed) mean, Sigma as the step left it, c^2 from eigh of the Hessian at the nominal
        pc = ca._params_c(params)
        tab_h = None
        if pc.disturb_kind in _lib.TABLE_DISTURB_KINDS:
            tab_h = core.disturb_table(pc, dstate.packed, key=k_act, key_mode=_lib.DISTURB_KEYS_HESSIAN, deterministic=True)
        nominal = core.shift_mean(cp.a_mean.reshape(-1).contiguous())
        Rm = core.hessian(dstate.packed, dstate, pc, nominal, f_steps=tab_h)[0].cpu().numpy()
        g = core.cost_gradient(dstate, pc, cpb.a_mean.reshape(-1).contiguous(), f_steps=tab_h)[0].cpu().numpy()
        S = cpb.a_cov.cpu().numpy().astype(np.float64)
        ic = inv_c2_of(Rm, float(cp.sample_sigma))
        t = S @ g
        want = -(g @ (S @ t)) * ic
        scale = (t @ t) * ic
        print(f"    slope {slope:.9e} want {want:.9e} (|Sigma g|^2 / c^2 {scale:.3e}), |g| {gnorm:.4e}")
        assert abs(float(slope) - want) <= 1e-9 * scale + 2.0 ** -24 * abs(want), (where, slope, want)
        assert abs(float(gnorm) - np.linalg.norm(g)) <= 2.0 ** -23 * np.linalg.norm(g), where
        cp = cpa
        obs, state, _, _, info = env.step(k_step, state, ua.cpu().numpy(), params)
    assert ca.core.device_status() == 0
    ca.core.close()
    cb.core.close()


# ------------------------------------------------------------------------------------------ 4: batched, iterated, closed loop
def test_batched_refine_equals_singles():
    import covo_mpc_amd as cm
    N, E = 256, 3
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    act = [np.stack([np.asarray(cr.PRNGKey(60 + 10 * k + e)) for e in range(E)]) for k in range(2)]
    rows, means = [], []
    for e in range(E):
        c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False, refine=True)
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        cp = c.reset(se.state0, params[e], c.init_control_params, cr.PRNGKey(2))
        r, m = [], []
        for k in range(2):
            _, cp, _ = c(None, None, params[e], act[k][e], cp, {"noisy_state": se.noisy_state})
            torch.cuda.synchronize()
            r.append(c.core.refine_rows[0].clone())
            m.append(cp.a_mean.reshape(-1).clone())
        rows.append(r)
        means.append(m)
        cp0 = c.init_control_params
        c.core.close()
    b = batched_controller(env, "covo-online", cp0, E, N, 0.01, refine=True)
    assert tuple(b.refine.shape) == (E, RF)
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    b.bind_episode(ep)
    for k in range(2):
        b(None, act[k])
        torch.cuda.synchronize()
        for e in range(E):
            assert torch.equal(b.refine[e], rows[e][k]), (k, e, b.refine[e], rows[e][k])
            assert torch.equal(b.a_mean[e].reshape(-1), means[e][k]), (k, e)
    print(f"  choices {[[split_row(rows[e][k])[2] for k in range(2)] for e in range(E)]}")
    assert b.core.device_status() == 0
    b.core.close()


def test_iterated_step_leaves_the_last_passes_row():
    """iters=2: every pass runs the refinement; the row is the last pass's -- its chosen cost is the plan's, which follows the last pass"""
    env = quad_env(task="tracking_zigzag")
    c, cp0 = _controller(env, 256, True, iters=2, compute_plan=True)
    cp, obs, info, state, params = start_episode(env, c, cp0, "covo-online")
    u, cp1, i1 = c(obs, state, params, cr.PRNGKey(11), cp, info)
    torch.cuda.synchronize()
    base, chosen, choice, _, _, _, _, flags = split_row(c.core.refine_rows[0])
    print(f"  base {base} chosen {chosen} choice {choice}; pass minima {i1['iter_cost_min'].cpu().numpy()}")
    assert flags == 0 and chosen <= base
    assert torch.equal(i1["cost_plan"].reshape(1), c.core.refine_rows[0, 1:2])
    assert bool(torch.isfinite(i1["iter_cost_min"]).all())
    assert c.core.device_status() == 0
    c.core.close()


def test_run_episode_equals_host_calls():
    import covo_mpc_amd as cm
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    T = 12
    got = {}
    for mode in ("fused", "hand"):
        c, _ = _controller(env, 256, True, compute_plan=True)
        c.alias_outputs = True
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (c.core.lib, c.core.h), DEV)
        cp = c.reset(ep.state0, params, c.init_control_params, cr.PRNGKey(42))
        rng = cr.PRNGKey(43)
        if mode == "hand":
            us, ch = [], []
            for _ in range(T):
                rng, rng_act, rng_step, _c = cr.split(rng, 4)
                u, cp, _ = c(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                us.append(u.clone())
                ch.append(c.core.refine_rows[0].clone())
                ep.step(rng_step, u)
                rng, _c = cr.split(rng)
            got["hand"] = (torch.stack(us).cpu().numpy(), ep.read_log(), [split_row(r)[2] for r in ch])
        else:
            cp, rng = c.run_episode(ep, params, cp, rng, 7)
            cp, rng = c.run_episode(ep, params, cp, rng, T - 7)
            got["fused"] = (ep.read_trace()["u"][:T].copy(), ep.read_log())
        assert c.core.device_status() == 0
        c.core.close()
    print(f"  choices of the 12 steps: {got['hand'][2]}")
    assert got["fused"][0].shape == (T, 4) and got["fused"][0].tobytes() == got["hand"][0].tobytes()
    assert np.array_equal(got["fused"][1], got["hand"][1])
