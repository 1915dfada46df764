"""GPU tests (-m gpu) of the update arbiter (covo_arbitrate / covo_set_step_arbiter / covo_set_episode_arbiter_log; `update=`,
read_arbiter(); csrc/update_arbiter.hip): a step commits the best of {softmax mean, nominal, best sample}.

Bars.  n_best against numpy's first minimum over the non-NaN costs, choice against the host rule on the row's own costs, the committed
mean against the chosen candidate, cost_best against cost[n_best], cost_softmax / cost_nominal against covo_rollout_cost on the
clipped candidate, arb_cost[0] against the twin's cost_plan, the plan row against cost_chosen, batched against single and the
episode log against the hand-stepped loop: none (torch.equal / equal bytes: the same stage functions on the same stripes).  The three
costs against the fp64 oracle: 1e-5 relative, the rollout cost's bar.  The three scenarios of test 4: the fp64 oracle
separates winner and runner-up by >= 1e-3 relative, a hundred times the fp32 kernel's error bar, so the kernel cannot flip them.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd._lib import CovoError, check, ptr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from covo_mpc_amd.dynamics.dataclass import as_device_state  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from tests.conftest import make_problem  # noqa: E402
from tests.gpu_support import (DEV, DP, H, batched_controller, dev_state, disturb_key, params_c, quad_env, sample_actions,  # noqa: E402
                               set_time, start_episode, step_inputs, to_stripes)
from tests.oracle_support import oracle_state  # noqa: E402

AF = _lib.COVO_ARB_FLOATS
COST_BAR = 1e-5


def split_row(row):
    """arbiter row [8] (device tensor) -> (cost [3] f32, cost_chosen, choice, n_best, words 6..7) as numpy / ints"""
    r = row.detach().cpu().numpy()
    i = np.ascontiguousarray(r[4:6]).view(np.int32)
    return r[0:3].copy(), r[3], int(i[0]), int(i[1]), r[6:8]


def host_choice(cost3):
    """the definition on a row's own costs: NaN counts as +inf, equal costs -> the lowest candidate, all +inf -> 0"""
    c = np.where(np.isnan(cost3), np.inf, cost3.astype(np.float64))
    return int(np.argmin(c)) if np.isfinite(c).any() or (c == -np.inf).any() else 0


def host_best(cost):
    """first minimum over the non-NaN costs, -1 when there is none"""
    return -1 if np.isnan(cost).all() else int(np.nanargmin(cost))


def candidate(choice, a_mean0, a_nom, a, n_best):
    """the [H, 4] tensor choice commits: the softmax mean as it was, the nominal unclipped, the best sample's stripe"""
    return (a_mean0.view(H, 4), a_nom.view(H, 4), a[:, n_best, :] if n_best >= 0 else None)[choice]


# ------------------------------------------------------------------------------------------ 1: stand-alone, crafted costs
def _crafted(N, place, g):
    """-> cost [N] float32 with the minimum where `place` says"""
    c = g.uniform(1.0, 9.0, N).astype(np.float32)
    if place == "first":
        c[0] = -3.5
    elif place == "last":
        c[N - 1] = -3.5
    elif place == "dup":
        i, j = (N // 3, N - 1) if N > 1 else (0, 0)
        c[i] = c[j] = -3.5
    elif place == "nans":
        c[g.random(N) < 0.4] = np.nan
        c[0] = np.nan
        if N > 2:
            c[N - 2] = -3.5
            c[N - 1] = np.nan
    elif place == "allnan":
        c[:] = np.nan
    return c


@pytest.mark.parametrize("N", [1, 3, 64, 197, 65536])
def test_arbitrate_crafted_costs(N):
    """covo_arbitrate on costs written by hand: the minimum at index 0, at N - 1, duplicated (lowest index wins), NaNs scattered (one
    in front of and one behind the minimum), all NaN (n_best = -1, candidate 2 never chosen); every mask 1..7.  The means lie outside
    [-1, 1] in places: the committed nominal is the unclipped one.  The cost buffer is also passed at a 4-byte offset, where the
    16-byte loads start behind a scalar head."""
    s, p, rng = make_problem(seed=17, time=37)
    a = sample_actions(p, rng, min(N, 256))
    g = np.random.default_rng(N)
    if N > 256:
        a = a[g.integers(0, 256, N)]
    ds = dev_state(s)
    pc = params_c(p, "none", "penyaw", rollover=False)
    core = SamplingCore(N, H, 0.01, 1.0, device=DEV, compute_info=False)
    core.a.copy_(to_stripes(a))
    a_nom = torch.tensor(g.uniform(-1.4, 1.4, 128).astype(np.float32), device=DEV)
    a_sm = torch.tensor(g.uniform(-1.4, 1.4, 128).astype(np.float32), device=DEV)
    pad = torch.zeros((N + 1,), dtype=torch.float32, device=DEV)
    for place in ("first", "last", "dup", "nans", "allnan"):
        c = _crafted(N, place, g)
        want_n = host_best(c)
        for off in (0, 1):
            pad[off:off + N].copy_(torch.from_numpy(c))
            for mask in range(1, 8):
                am = a_sm.clone()
                row = core.arbitrate(ds, pc, a_nom, am, mask, cost=pad[off:off + N])
                cost3, chosen, choice, n_best, tail = split_row(row)
                where = f"N={N} {place} off={off} mask={mask}: row {cost3} choice {choice} n_best {n_best}"
                assert n_best == want_n, where
                for q in range(3):  # a masked-out or absent candidate costs +inf, an enabled one what its rollout gives
                    on = bool(mask >> q & 1) and (q < 2 or want_n >= 0)
                    assert np.isfinite(cost3[q]) if on else cost3[q] == np.inf, where
                assert choice == host_choice(cost3), where
                assert chosen.tobytes() == cost3[choice].tobytes() and np.all(tail == 0.0), where
                assert not (choice == 2 and want_n < 0), where
                assert torch.equal(am.view(H, 4), candidate(choice, a_sm, a_nom, core.a, n_best)), where
    assert core.device_status() == 0
    core.close()


# ------------------------------------------------------------------------------------------ 2: stand-alone, real costs
@pytest.mark.parametrize("N", [197, 64])
@pytest.mark.parametrize("kind", ["none", "gaussian", "periodic", "drag"])
def test_arbitrate_real_costs_vs_rollout_and_oracle(kind, N):
    """covo_rollout_cost, then covo_arbitrate on the same `a` and its costs; both rewards, rollover on and off, discount 1 and 0.9;
    NONE, GAUSSIAN with a non-zero shared vector, PERIODIC and DRAG tables.  cost_best == cost[n_best] == cost.min(); cost_softmax
    and cost_nominal == covo_rollout_cost on the one clipped candidate (N = 1); all three within 1e-5 of the fp64 oracle."""
    s, p, rng = make_problem(seed=17, time=37)
    p = p.replace(disturb_params=DP)
    a = sample_actions(p, rng, N)
    ds = dev_state(s)
    key = cr.PRNGKey(5)
    g = np.random.default_rng(3)
    a_nom = torch.tensor((a[:8].mean(axis=0) + g.normal(0, 0.4, (H, 4))).astype(np.float32).reshape(-1), device=DEV)
    a_sm = torch.tensor((a[8:24].mean(axis=0) + g.normal(0, 0.4, (H, 4))).astype(np.float32).reshape(-1), device=DEV)
    assert float(a_nom.abs().max()) > 1.0 and float(a_sm.abs().max()) > 1.0  # the evaluation clip has something to do
    for discount in (1.0, 0.9):
        core = SamplingCore(N, H, 0.01, discount, device=DEV, compute_info=False)
        one = SamplingCore(1, H, 0.01, discount, device=DEV, compute_info=False)
        core.a.copy_(to_stripes(a))
        for reward in ("penyaw", "realworld"):
            for rollover in (False, True):
                pc = params_c(p, kind, reward, rollover=rollover)
                tab, fs, dist = None, (0.0, 0.0, 0.0), {}
                if kind in ("periodic", "drag"):
                    tab = core.disturb_table(pc, ds.packed, key=key, key_mode=_lib.DISTURB_KEYS_SHARED, deterministic=True)
                    draw = cr.uniform(disturb_key(key), (3,), -p.disturb_scale, p.disturb_scale).astype(np.float64)
                    dist = dict(disturb=R.Disturb(kind, draw, True))
                elif kind == "gaussian":
                    fs = (0.02, -0.03, 0.01)
                cost = core.rollout(ds, pc, fs, False, f_steps=tab).clone()
                am = a_sm.clone()
                row = core.arbitrate(ds, pc, a_nom, am, 7, f_shared=fs, f_steps=tab)
                cost3, chosen, choice, n_best, _ = split_row(row)
                where = f"{kind} N={N} disc={discount} {reward} roll={rollover}: row {cost3} choice {choice} n_best {n_best}"
                ch = cost.cpu().numpy()
                assert n_best == host_best(ch), where
                assert cost3[2].tobytes() == ch[n_best].tobytes() == ch.min().tobytes(), where
                cands = [a_sm.view(H, 4).clamp(-1, 1), a_nom.view(H, 4).clamp(-1, 1), core.a[:, n_best, :]]
                for q in range(2):
                    one.a.copy_(cands[q].reshape(H, 1, 4))
                    c1 = one.rollout(ds, pc, fs, False, f_steps=tab)
                    assert torch.equal(row[q:q + 1], c1), (where, q, float(c1))
                a64 = torch.stack(cands).cpu().numpy().astype(np.float64)
                if dist:
                    ref = CO.rollout(s, p, a64, discount, dtype=np.float64, rollover=rollover, reward=reward, **dist)
                else:
                    ref = CO.rollout(s, p, a64, discount, np.asarray(fs, dtype=np.float64), dtype=np.float64, rollover=rollover,
                                     reward=reward)
                rel = np.abs(cost3 - ref) / np.maximum(np.abs(ref), 1.0)
                print(f"  {where}: rel err vs oracle {rel}")
                assert rel.max() < COST_BAR, (where, rel)
                assert choice == host_choice(cost3) and torch.equal(am.view(H, 4), candidate(choice, a_sm, a_nom, core.a, n_best)), where
        assert core.device_status() == 0
        core.close()
        one.close()


# ------------------------------------------------------------------------------------------ 3: behind every step path
def _controller(env, name, N, update, extras, plan=False, lam="0.01"):
    import covo_mpc_amd as cm
    c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam{lam}", device=DEV, compute_info=False, compute_diag=extras,
                                  compute_plan=extras or plan, ess_min=32.0 if extras else None, compute_fan=8 if extras else None,
                                  update=update)
    return c, c.init_control_params


def _check_step(env, name, params, k_act, dstate, cp_in, ca, cpa, ia, ua, cb, cpb, update, extras, one, where):
    """every assertion of test 3 on one teacher-forced step: ca arbitrates, cb is the softmax twin with the plan attached"""
    core = ca.core
    cost3, chosen, choice, n_best, _ = split_row(core.arbiter[0])
    where = f"{where}: row {cost3} choice {choice} n_best {n_best}"
    assert ia["arb_cost"].data_ptr() == core.arbiter.data_ptr() and ia["arb_choice"].dtype == torch.int32  # views: no copy, no sync
    assert int(ia["arb_choice"]) == choice and int(ia["arb_best"]) == n_best and float(ia["arb_cost_chosen"]) == float(chosen), where
    if update == "guarded":
        assert torch.equal(core.arbiter[0, 0:1], cb.core.plan[0, 0:1]), (where, float(cb.core.plan[0, 0]))
    else:
        assert np.isinf(cost3[0]) and choice != 0, where
    assert n_best == host_best(core.cost.cpu().numpy()) and choice == host_choice(cost3), where
    assert torch.equal(core.arbiter[0, 2:3], core.cost[n_best:n_best + 1]), where
    # nothing else of the step changes
    assert torch.equal(core.cost, cb.core.cost) and torch.equal(core.a, cb.core.a) and torch.equal(cpa.a_cov, cpb.a_cov), where
    if extras:
        assert torch.equal(core.diag, cb.core.diag) and torch.equal(core.lam_eff, cb.core.lam_eff), where
    # a_mean and u are the chosen candidate
    nominal = core.shift_mean(cp_in.a_mean.reshape(-1).contiguous())
    cand = candidate(choice, cpb.a_mean.reshape(-1), nominal, core.a, n_best)
    assert torch.equal(cpa.a_mean.view(H, 4), cand) and torch.equal(ua, cand[0]), where
    if core.plan is not None:
        # the plan row is the chosen candidate's: its cost is cost_chosen, its positions those of the candidate's own rollout
        assert torch.equal(core.plan[0, 0:1], core.arbiter[0, 3:4]), (where, float(core.plan[0, 0]))
        fs, tab = step_inputs(env, ca, name, params, k_act, dstate, one)
        one.a.copy_(cand.clamp(-1, 1).reshape(H, 1, 4))
        fan = one.rollout_fan(dstate, ca._params_c(params), None, f_shared=fs, f_steps=tab, K=1)
        assert torch.equal(core.plan[0, 4:], fan[0, 4:]) and torch.equal(core.plan[0, 0:1], fan[0, 0:1]), where
    return choice


@pytest.mark.parametrize("update", ["guarded", "best"])
@pytest.mark.parametrize("extras", [False, True], ids=["alone", "plan+fan+diag+ess"])
@pytest.mark.parametrize("graph", ["graph", "eager"])
@pytest.mark.parametrize("name,N", [("mppi", 256), ("covo-offline", 256), ("covo-online", 256), ("mppi", 1024), ("covo-offline", 1024),
                                    ("covo-online", 1024)])
def test_step_arbiter_on_every_path(name, N, graph, extras, update, monkeypatch):
    """MPPI, covo-offline (the one-launch step; with the ESS floor the staged one) and covo-online (eager: the streamed path) at
    N = 256 and 1 024; graph replay and COVO_FLAG_NO_GRAPH, shared_device; alone, and next to plan, fan, diagnostics and ESS floor.
    Three teacher-forced steps against a twin with update="softmax", compute_plan=True that is fed the arbitrated controller's
    inputs."""
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    monkeypatch.setenv("COVO_SHARED_DEVICE", "1")
    env = quad_env(task="tracking_zigzag")
    ca, cpa = _controller(env, name, N, update, extras)
    cb, cpb = _controller(env, name, N, "softmax", extras, plan=True)
    assert ca.core.shared_device and ca.core.uses_graph == (graph == "graph") and cb.core.arbiter is None
    one = SamplingCore(1, H, 0.01, 1.0, device=DEV, compute_info=False)
    cp, obs, info, state, params = start_episode(env, ca, cpa, name)
    key = cr.PRNGKey(11)
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        dstate = as_device_state(info["noisy_state"], DEV)
        ua, cpa, ia = ca(obs, state, params, k_act, cp, info)
        ub, cpb, ib = cb(obs, state, params, k_act, cp, info)
        torch.cuda.synchronize()
        assert not any(k.startswith("arb_") for k in ib)
        _check_step(env, name, params, k_act, dstate, cp, ca, cpa, ia, ua, cb, cpb, update, extras, one,
                    f"{name} N={N} {graph} extras={extras} {update} step {step}")
        cp = cpa
        obs, state, _, _, info = env.step(k_step, state, ua.cpu().numpy(), params)
    assert ca.core.device_status() == 0
    for c in (ca.core, cb.core, one):
        c.close()


def test_step_arbiter_headline_size():
    """one covo-online step at N = 65 536 (the cost scan over 1 024 cache lines), guarded, with the plan attached"""
    env = quad_env(task="tracking_zigzag")
    name, N = "covo-online", 65536
    ca, cpa = _controller(env, name, N, "guarded", False, plan=True)
    cb, cpb = _controller(env, name, N, "softmax", False, plan=True)
    one = SamplingCore(1, H, 0.01, 1.0, device=DEV, compute_info=False)
    cp, obs, info, state, params = start_episode(env, ca, cpa, name)
    k_act = cr.PRNGKey(12)
    dstate = as_device_state(info["noisy_state"], DEV)
    ua, cpa, ia = ca(obs, state, params, k_act, cp, info)
    ub, cpb, ib = cb(obs, state, params, k_act, cp, info)
    torch.cuda.synchronize()
    _check_step(env, name, params, k_act, dstate, cp, ca, cpa, ia, ua, cb, cpb, "guarded", False, one, f"{name} N={N}")
    for c in (ca.core, cb.core, one):
        c.close()


SCENARIOS = {
    # name: (controller, N, lam, task, sample sigma of MPPI's covariance, offset of the start position [m], expected choice)
    "hover-on-target-wide-noise": ("mppi", 64, "0.01", "hovering", 1.0, 0.0, 1),
    "half-metre-off-flat-weights": ("mppi", 1024, "1000000.0", "tracking_zigzag", 0.5, 0.5, 2),
    "covo-online-tracking-lam0.5": ("covo-online", 1024, "0.5", "tracking_zigzag", 0.5, 0.0, 0),
}


# ------------------------------------------------------------------------------------------ 4: all three choices occur
@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_all_three_choices_occur(scenario):
    """Three named scenarios, the issue's suggested starting points, disturbance off (one shared vector would move all three costs
    alike): hovering on target with the equilibrium mean and sigma = 1 at N = 64 -> the nominal wins; 0.5 m off the reference with
    lambda = 1e6 (flat weights: the mean is the sample average) at N = 1 024 -> the best sample wins; the covo-online tracking step at
    lambda = 0.5 -> the softmax mean wins.  The third differs from the suggestion: at the default lambda = 0.01 the first tracking
    step has an effective sample size near 1, the softmax mean IS the best sample up to rounding, and the fp64 oracle separates the
    two by 9e-6 relative only (-21.837031 against -21.836835); at lambda = 0.5 the average of many good samples beats the best one
    by 7e-2 (-23.54 against -21.84; nominal -12.15).  Observed margins of the other two: 1.4e-1 (nominal -30.68 against -26.47) and
    3.9e-1 (best sample -7.72 against -4.69).  The margin is checked where the test runs: the fp64 oracle rolls out the three
    candidates the step formed and must separate winner and runner-up by >= 1e-3 relative before the expected choice is asserted."""
    import covo_mpc_amd as cm
    name, N, lam, task, sigma, off, want = SCENARIOS[scenario]
    env = quad_env(task=task, disturb="none")
    ca, cp0 = _controller(env, name, N, "guarded", False, lam=lam)
    cb, _ = _controller(env, name, N, "softmax", False, lam=lam)
    cp, obs, info, state, params = start_episode(env, ca, cp0, name)
    if name == "mppi":
        cp = cp.replace(a_cov=(torch.eye(4, dtype=torch.float32, device=DEV) * sigma ** 2).repeat(H, 1, 1))
    ns = info["noisy_state"]
    if off:
        ns = ns.replace(pos=(np.asarray(ns.pos, dtype=np.float32) + np.asarray([off, 0.0, 0.0], dtype=np.float32)))
        info = dict(info, noisy_state=ns)
    k_act = cr.PRNGKey(21)
    ua, cpa, ia = ca(obs, state, params, k_act, cp, info)
    ub, cpb, _ = cb(obs, state, params, k_act, cp, info)
    torch.cuda.synchronize()
    cost3, chosen, choice, n_best, _ = split_row(ca.core.arbiter[0])
    nominal = ca.core.shift_mean(cp.a_mean.reshape(-1).contiguous()).view(H, 4)
    cands = torch.stack([cpb.a_mean.view(H, 4).clamp(-1, 1), nominal.clamp(-1, 1), ca.core.a[:, n_best, :]])
    ref = CO.rollout(oracle_state(ns), R.Params().fp32(), cands.cpu().numpy().astype(np.float64), 1.0, np.zeros(3), dtype=np.float64)
    order = np.argsort(ref, kind="stable")
    margin = (ref[order[1]] - ref[order[0]]) / max(abs(ref[order[0]]), 1e-30)
    print(f"  {scenario}: oracle costs {ref}, device row {cost3}, margin {margin:.3e}, choice {choice}")
    assert int(order[0]) == want and margin >= 1e-3, (scenario, ref, margin)
    assert choice == want, (scenario, cost3)
    ca.core.close()
    cb.core.close()


# ------------------------------------------------------------------------------------------ 5: the env-batched controllers
def _batch_setup(E):
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    return env, params, reset_keys


@pytest.mark.parametrize("update", ["best", "guarded"])
@pytest.mark.parametrize("name", ["covo-online", "covo-offline", "mppi"])
def test_batched_arbiter_equals_single(name, update):
    """E = 3 domain-randomised instances, N = 256, two steps: controller.arbiter[e] and a_mean[e] equal the single controller's on
    instance e alone, bit for bit."""
    import covo_mpc_amd as cm
    N, E = 256, 3
    env, params, reset_keys = _batch_setup(E)
    act = [np.stack([np.asarray(cr.PRNGKey(60 + 10 * k + e)) for e in range(E)]) for k in range(2)]
    rows, means, tables = [], [], []
    for e in range(E):
        c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV, compute_info=False, update=update)
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        cp = c.reset(se.state0, params[e], c.init_control_params, cr.PRNGKey(2))
        if name == "covo-offline":
            tables.append((cp.a_cov_offline, cp.a_chol_offline))
        r, m = [], []
        for k in range(2):
            _, cp, _ = c(None, None, params[e], act[k][e], cp, {"noisy_state": se.noisy_state})
            torch.cuda.synchronize()
            r.append(c.core.arbiter[0].clone())
            m.append(cp.a_mean.reshape(-1).clone())
        rows.append(r)
        means.append(m)
        cp0 = c.init_control_params
        c.core.close()
    b = batched_controller(env, name, cp0, E, N, 0.01, update=update)
    assert tuple(b.arbiter.shape) == (E, AF)
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    b.bind_episode(ep)
    if name == "covo-offline":
        b.set_tables(torch.stack([t[0] for t in tables]), torch.stack([t[1] for t in tables]))
    for k in range(2):
        b(None, act[k])
        torch.cuda.synchronize()
        for e in range(E):
            assert torch.equal(b.arbiter[e], rows[e][k]), (name, update, k, e, b.arbiter[e], rows[e][k])
            assert torch.equal(b.a_mean[e].reshape(-1), means[e][k]), (name, update, k, e)
    assert b.core.device_status() == 0
    b.core.close()


@pytest.mark.parametrize("name", ["mppi", "covo-online"])
def test_batched_after_step_launches_follow_rebound_instances(name):
    """The three launches behind an env-batched step (arbiter, plan, fan) read their argument blocks from device copies that are
    re-uploaded only when they change.  E = 2, N = 64 (one 64-sample group: the smallest the fan and the arbiter's argmin take with
    K = 4), plan + fan + update="guarded": two steps, set_instances with freshly allocated trajectories of another task -- every
    launch's blocks change -- two more.  After every step a_mean[e], plan[e], fan[e] and arbiter[e] equal the single controller's on
    instance e alone, bit for bit."""
    import covo_mpc_amd as cm
    N, E, K = 64, 2, 4
    env, params, reset_keys = _batch_setup(E)
    other = quad_env(task="tracking_zigzag", randomizer=True)
    starts = [[e_.reset(reset_keys[e], params[e]) for e in range(E)] for e_ in (env, other)]  # [phase][e] = (obs, info, state)
    act = [np.stack([np.asarray(cr.PRNGKey(60 + 10 * k + e)) for e in range(E)]) for k in range(4)]
    kw = dict(compute_plan=True, compute_fan=K, update="guarded")
    want = []  # [e][k] = (a_mean, plan row, fan rows, arbiter row)
    for e in range(E):
        c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV, compute_info=False, **kw)
        cp, w = c.init_control_params, []
        for k in range(4):
            _, cp, _ = c(None, None, params[e], act[k][e], cp, {"noisy_state": starts[k // 2][e][1]["noisy_state"]})
            torch.cuda.synchronize()
            w.append((cp.a_mean.reshape(-1).clone(), c.core.plan[0].clone(), c.core.fan[0].clone(), c.core.arbiter[0].clone()))
        want.append(w)
        cp0 = c.init_control_params
        c.core.close()
    b = batched_controller(env, name, cp0, E, N, 0.01, **kw)
    assert tuple(b.plan.shape) == (E, _lib.COVO_PLAN_FLOATS) and tuple(b.fan.shape) == (E, K, _lib.COVO_FAN_FLOATS)
    for k in range(4):
        if k % 2 == 0:
            b.set_instances([s[2] for s in starts[k // 2]], params)
        b([s[1]["noisy_state"] for s in starts[k // 2]], act[k])
        torch.cuda.synchronize()
        for e in range(E):
            got = (b.a_mean[e].reshape(-1), b.plan[e], b.fan[e], b.arbiter[e])
            for what, g, w in zip(("a_mean", "plan", "fan", "arbiter"), got, want[e][k]):
                assert torch.equal(g, w), (name, k, e, what, g, w)
    assert b.core.device_status() == 0
    b.core.close()


@pytest.mark.parametrize("update", ["best", "guarded"])
@pytest.mark.parametrize("name", ["covo-online", "mppi"])
def test_batched_episode_arbiter_log(name, update):
    """covo_run_episode_batched[_mode] for 12 steps in two segments on E = 3 instances, instance 1 starting at time 294 so that it
    terminates and auto-resets inside the run: read_arbiter() equals the hand-stepped loop of __call__ + episode.step bit for bit,
    the env log too; under "guarded" every row has cost_chosen <= min(row[0:3])."""
    import covo_mpc_amd as cm
    N, E, T = 256, 3, 12
    env, params, reset_keys = _batch_setup(E)
    rngs0 = np.stack([np.asarray(cr.PRNGKey(60 + e)) for e in range(E)])
    c0, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    cp0 = c0.init_control_params
    c0.core.close()
    got = {}
    for mode in ("fused", "hand"):
        b = batched_controller(env, name, cp0, E, N, 0.01, update=update)
        ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
        set_time(ep, 1, 294)
        if mode == "hand":
            b.bind_episode(ep)
            rngs, rows = [rngs0[e] for e in range(E)], []
            for _ in range(T):
                sp = [cr.split(r, 4) for r in rngs]
                b(None, np.stack([np.asarray(x[1]) for x in sp]))
                rows.append(b.arbiter.clone())
                ep.step(np.stack([np.asarray(x[2]) for x in sp]), b.a_mean)
                rngs = [cr.split(x[0])[0] for x in sp]
            got["hand"] = (torch.stack(rows, dim=1).cpu().numpy(), ep.read_log())
        else:
            keys = b.run_episode(ep, rngs0.copy(), 7)
            b.run_episode(ep, keys, T - 7)
            got["fused"] = (ep.read_arbiter(), ep.read_log(), ep.arblog.cpu().numpy())
        assert b.core.device_status() == 0
        b.core.close()
    arb, log, raw = got["fused"]
    assert arb["cost"].shape == (E, T, 3) and arb["choice"].shape == (E, T) and arb["best"].dtype == np.int32
    assert np.ascontiguousarray(raw[:, :T]).tobytes() == got["hand"][0].tobytes()
    assert np.all(raw[:, T:] == 0.0)
    assert np.array_equal(log, got["hand"][1])
    assert (log[1, :, 3] > 0).any(), "instance 1 did not terminate inside the run: the case is vacuous"
    print(f"  {name} {update}: choices per instance {[np.bincount(arb['choice'][e], minlength=3).tolist() for e in range(E)]}")
    if update == "guarded":
        assert np.all(arb["cost_chosen"] <= arb["cost"].min(axis=2)), arb
    else:
        assert np.all(np.isinf(arb["cost"][..., 0])) and np.all(arb["choice"] != 0)


def test_single_episode_arbiter_log_and_eval_env_batched():
    """covo_run_episode (6 steps, 4 + 2) against the hand-stepped loop; eval_env_batched(update=, arbiter=True) returns the log."""
    import covo_mpc_amd as cm
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    got = {}
    for mode in ("fused", "hand"):
        c, _ = cm.envs.get_controller(env, "mppi", "N256_H32_lam0.01", device=DEV, compute_info=False, update="guarded")
        c.alias_outputs = True
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (c.core.lib, c.core.h), DEV)
        cp = c.reset(ep.state0, params, c.init_control_params, cr.PRNGKey(42))
        rng = cr.PRNGKey(43)
        if mode == "hand":
            rows = []
            for _ in range(6):
                rng, rng_act, rng_step, _c = cr.split(rng, 4)
                u, cp, _ = c(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                rows.append(c.core.arbiter[0].clone())
                ep.step(rng_step, u)
                rng, _c = cr.split(rng)
            with pytest.raises(RuntimeError):
                ep.read_arbiter()  # no run_episode segment: no arbiter log
            got["hand"] = (torch.stack(rows).cpu().numpy(), ep.read_log())
        else:
            cp, rng = c.run_episode(ep, params, cp, rng, 4)
            cp, rng = c.run_episode(ep, params, cp, rng, 2)
            got["fused"] = (ep.arblog.cpu().numpy(), ep.read_log(), ep.read_arbiter())
        c.core.close()
    assert got["fused"][0][:6].tobytes() == got["hand"][0].tobytes() and np.all(got["fused"][0][6:] == 0.0)
    assert np.array_equal(got["fused"][1], got["hand"][1])
    assert got["fused"][2]["cost"].shape == (6, 3)
    envr = quad_env(task="tracking", randomizer=True)
    err, arb = cm.envs.quadrotor.eval_env_batched(envr, 2, "N256_H32_lam0.01", n_steps=3, device=DEV, verbose=False, update="best",
                                                  arbiter=True)
    assert err.shape == (2,) and arb["cost"].shape == (2, 3, 3) and arb["choice"].shape == (2, 3) and np.all(arb["choice"] > 0)
    with pytest.raises(ValueError, match="arbiter=True"):
        cm.envs.quadrotor.eval_env_batched(envr, 2, "N256_H32_lam0.01", n_steps=3, device=DEV, verbose=False, arbiter=True)


# ------------------------------------------------------------------------------------------ 6: refusals
def test_arbiter_refusals_leave_the_handle_usable():
    """Every refusal at the C boundary, matched on its message, nothing launched; afterwards the status is clean and a normal step
    is finite."""
    import covo_mpc_amd as cm
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    N = 256
    c, _ = cm.envs.get_controller(env, "mppi", f"N{N}_H32_lam0.01", device=DEV, compute_info=False, update="guarded")
    core = c.core
    lib, h = core.lib, core.h
    obs, info, state = env.reset(cr.PRNGKey(1), params)
    dstate = as_device_state(info["noisy_state"], DEV)
    cp = c.init_control_params
    pc = c._params_c(params)
    rows = torch.zeros((4, AF), dtype=torch.float32, device=DEV)
    vec = torch.zeros((128,), dtype=torch.float32, device=DEV)
    # (a) mask outside 1..7
    for bad in (0, 8, -1):
        with pytest.raises(CovoError, match=r"mask=-?\d+ outside \[1, 7\]"):
            check(lib.covo_set_step_arbiter(h, ptr(rows), bad, 1), "covo_set_step_arbiter")
        with pytest.raises(CovoError, match=r"mask=-?\d+ outside \[1, 7\]"):
            core.arbitrate(dstate, pc, vec, vec.clone(), bad)
    # (b) n_inst outside (0, COVO_MAX_ENVS]
    for bad in (0, 65):
        with pytest.raises(CovoError, match="n_inst"):
            check(lib.covo_set_step_arbiter(h, ptr(rows), 7, bad), "covo_set_step_arbiter")
    # (c) a sample-sharded step
    args, am, _, _ = core._prepare_step(_lib.MODE_MPPI, dstate, cp.a_mean, a_cov=cp.a_cov, gamma_mean=1.0, sample_sigma=0.5,
                                        derive_keys=True, rollout_deterministic=False)
    core.cost.fill_(-7.0)
    core.partial.fill_(-7.0)
    core.arbiter.fill_(-7.0)
    args.partial_out = core.partial.data_ptr()
    with pytest.raises(CovoError, match="update arbiter.*sample-sharded"):
        check(lib.covo_mpc_step(h, C.byref(pc), C.byref(args), 1, 2, None, core.stream()), "covo_mpc_step")
    args.partial_out = None
    torch.cuda.synchronize()
    assert bool((core.cost == -7.0).all()) and bool((core.partial == -7.0).all()) and bool((core.arbiter == -7.0).all())
    # (d) an episode segment that would leave the log; the log needs the arbiter
    c.alias_outputs = True
    ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (lib, h), DEV)
    cpe = c.reset(ep.state0, params, cp, cr.PRNGKey(42))
    attach = core.attach_log
    core.attach_log = lambda name, episode, rows_left: attach(name, episode, 5 if name == "arblog" else rows_left)
    before = ep.true.clone()
    with pytest.raises(CovoError, match="episode arbiter log"):
        c.run_episode(ep, params, cpe, cr.PRNGKey(43), 6)
    torch.cuda.synchronize()
    assert torch.equal(ep.true, before) and bool((ep.arblog == 0).all())
    del core.attach_log
    check(lib.covo_set_episode_arbiter_log(h, None, 0), "covo_set_episode_arbiter_log")
    fresh = SamplingCore(N, H, 0.01, 1.0, device=DEV, compute_info=False)
    with pytest.raises(CovoError, match="covo_set_step_arbiter"):
        check(fresh.lib.covo_set_episode_arbiter_log(fresh.h, ptr(rows), 4), "covo_set_episode_arbiter_log")
    fresh.close()
    # (e) the kernel-by-kernel debug path
    c.materialize_eps = True
    with pytest.raises(NotImplementedError, match="update='guarded' follows the fused step"):
        c(obs, state, params, cr.PRNGKey(9), cp, info)
    c.materialize_eps = False
    # the handle is usable: a normal step with the arbiter
    assert core.device_status() == 0
    u, cp2, cinfo = c(obs, state, params, cr.PRNGKey(9), cp, info)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(cinfo["arb_cost"]).all())
    assert core.device_status() == 0
    core.close()
    # (f) a batched step with more instances than n_inst
    E = 3
    envr = quad_env(task="tracking", randomizer=True)
    c0, _ = cm.envs.get_controller(envr, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    cp0 = c0.init_control_params
    c0.core.close()
    for name in ("covo-online", "mppi"):
        b = batched_controller(envr, name, cp0, E, N, 0.01, update="best")
        check(b.core.lib.covo_set_step_arbiter(b.core.h, ptr(b.arbiter), 6, 2), "covo_set_step_arbiter")
        ps = [envr.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
        ep = cm.envs.BatchedDeviceEpisode(envr, [cr.PRNGKey(50 + e) for e in range(E)], ps, (b.core.lib, b.core.h), DEV)
        keys = np.stack([np.asarray(cr.PRNGKey(60 + e)) for e in range(E)])
        b.bind_episode(ep)
        b._cost.fill_(-7.0)
        with pytest.raises(CovoError, match="arbiter buffer"):
            b(None, keys)
        before = ep.true.clone()
        with pytest.raises(CovoError, match="arbiter buffer"):
            b.run_episode(ep, keys, 2)
        torch.cuda.synchronize()
        assert torch.equal(ep.true, before) and bool((b._cost == -7.0).all())
        check(b.core.lib.covo_set_step_arbiter(b.core.h, ptr(b.arbiter), 6, E), "covo_set_step_arbiter")
        assert b.core.device_status() == 0
        u = b(None, keys)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(b.arbiter[:, 1:4]).all())
        b.core.close()
