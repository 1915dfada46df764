"""GPU tests (-m gpu) of the iLQR controller (COVO_MODE_ILQR / covo_set_step_ilqr; controllers/ilqr.py, BatchedILQRController;
csrc/ilqr.hip around the unchanged kernels of riccati=, riccati_feedback= and plan_hold=).  One instance, or E = 3 where batched.

1. the step equals the chained primitive: ILQRController at k = 3 on make_problem(seed=17, time=37) (incoming mean hover + 0.1 noise)
   against core.shift_mean + three core.riccati_refine(feedback=True) with the same derived inputs, cases (none, penyaw), (periodic,
   realworld), (gaussian, penyaw) -- a_mean, every iteration's row, feedback row and 33 costs as words; k = 1 equals one call; on a
   drag env the chain runs with feedback=False and ilqr_closed == 0.
2. chain and fixed point, k = 6: rows[j + 1, 0] == rows[j, 1] as words, rows[j, 1] <= rows[j, 0], the summary row equals its definition
   recomputed on the host; on the input `rest` (tests/ilqr_oracle.py: rest_case -- at rest 1 cm beside the hovering target with the
   hover mean, where the fp64 loop commits choice 0 from iteration 0 on rung 0, unflagged) a choice 0 falls within the six iterations,
   no row is flagged, and from the first choice 0 on the mean, the rows and the costs repeat as words.
3. nothing is sampled: core.a and core.cost keep a NaN sentinel over three steps.
4. a flagged sweep (a NaN in a_mean[5]) is data: flag bit 0 in every row, the mean is the shifted mean, nothing moved, no error.
5. against fp64, case (none, penyaw), k = 3: the oracle's cost of the device's mean after each iteration against that row's
   cost_chosen at the rollout cost's bar (1e-5 relative); the three oracle costs do not rise by more than twice it.
6. batched (E = 3, different parameters, states and keys) equals three singles over 4 steps, with and without plan_hold=3: means and
   all three row buffers as words.
7. the device episode equals the host loop over 7 steps with plan_hold=3 and compute_plan: trace u, hold log, final mean; ages
   0, 1, 2, 0, 1, 2, 0 -- single and batched; batched also under the periodic disturbance (per-step tables behind a hold step).
8. the plan hold uses the last iteration: at k = 2 the latch's b is b_1, and hold step 1's u is core.plan_hold on that latch.
9. the C side refuses a step in COVO_MODE_ILQR on a handle without the sweep or with a sampling attachment, by name, before any launch.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from covo_mpc_amd.dynamics import utils  # noqa: E402
from covo_mpc_amd.dynamics.dataclass import EnvParams3D  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from tests import ilqr_oracle as IO  # noqa: E402
from tests.conftest import make_problem  # noqa: E402
from tests.gpu_support import DEV, DP, H, dev_state, quad_env  # noqa: E402
from tests.oracle_support import rel_err_scalar  # noqa: E402

RF, FF, SF = _lib.COVO_RICCATI_FLOATS, _lib.COVO_FEEDBACK_FLOATS, _lib.COVO_ILQR_FLOATS
NC, NCF = _lib.COVO_REFINE_CANDIDATES, _lib.COVO_FEEDBACK_CANDIDATES
KEY = cr.PRNGKey(5)
COST_BAR = 1e-5  # the rollout cost against the fp64 oracle, relative


def bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def ints(t):
    """float32 device tensor -> its int32 words (numpy)"""
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.int32)


@functools.lru_cache(maxsize=None)
def _core():
    """the primitives' core: another handle than any controller's"""
    return SamplingCore(256, H, 0.01, 1.0, device=DEV, compute_info=False)


def _env(kind, reward="penyaw"):
    env = quad_env(task="tracking_zigzag", disturb=kind)
    if reward == "realworld":
        env.reward_fn = utils.tracking_realworld_reward_fn
    return env


def _env_params(p):
    return EnvParams3D(disturb_params=np.asarray(p.disturb_params, dtype=np.float32), disturb_period=p.disturb_period,
                       disturb_scale=p.disturb_scale, dyn_noise_scale=p.dyn_noise_scale)


@functools.lru_cache(maxsize=None)
def _problem(noise=0.1):
    s, p, rng = make_problem(seed=17, time=37)
    p = p.replace(disturb_params=DP)
    mean = (R.hover_action(p, 32, np.float64) + noise * rng.normal(size=(32, 4))).astype(np.float32)
    return s, p, mean


def _controller(env, k, mean, **kw):
    cp = cm.controllers.ILQRParams(a_mean=torch.from_numpy(np.ascontiguousarray(mean, dtype=np.float32).reshape(H, 4)).to(DEV))
    return cm.controllers.ILQRController(env, cp, H, iters=k, device=DEV, **kw), cp


def _chain(ds, pc, mean_in, key, k, feedback):
    """core.shift_mean, then k stand-alone line searches with the inputs an iLQR step derives from `key` -> (the k + 1 means b_0 ..
    b_k, the k result tuples (row, costs[, feedback row]))"""
    core = _core()
    b = core.shift_mean(mean_in.reshape(-1).contiguous().clone())
    tab = tab_h = None
    if pc.disturb_kind in _lib.TABLE_DISTURB_KINDS:
        step_key = cr.split(cr.split(key)[0])[1]  # covo.py:212,225
        tab = core.disturb_table(pc, ds.packed, key=step_key, key_mode=_lib.DISTURB_KEYS_SHARED, deterministic=True)
        tab_h = core.disturb_table(pc, ds.packed, key=key, key_mode=_lib.DISTURB_KEYS_HESSIAN, deterministic=True)
    means, out = [b.clone()], []
    for _ in range(k):
        r = core.riccati_refine(ds, pc, b, f_shared=(0.0, 0.0, 0.0), f_steps=tab, f_steps_hessian=tab_h, feedback=feedback)
        out.append(tuple(t.clone() for t in r))
        means.append(b.clone())
    torch.cuda.synchronize()
    assert core.device_status() == 0
    return means, out


def _step_once(c, cp, env_params, ds, key=KEY):
    u, cp2, info = c(None, None, env_params, key, cp, {"noisy_state": ds})
    torch.cuda.synchronize()
    assert c.core.device_status() == 0
    return u, cp2, info


def _check_summary(core, e, k):
    rows = core.ilqr_rows[e].cpu().numpy()
    want = IO.summary(rows, k)
    got = core.ilqr_summary[e].cpu().numpy()
    w = np.ascontiguousarray(got).view(np.int32)
    assert np.float32(got[0]).tobytes() == np.float32(want[0]).tobytes() and np.float32(got[1]).tobytes() == np.float32(want[1]).tobytes()
    assert (int(w[2]), int(w[3]), int(w[4]), int(w[5])) == want[2:6], (w, want)
    assert np.float32(got[6]).tobytes() == np.float32(want[6]).tobytes() and int(w[7]) == 0
    return want


# ------------------------------------------------------------------------------------------ 1: the step is the chained primitive
@pytest.mark.parametrize("kind,reward,k", [("none", "penyaw", 3), ("periodic", "realworld", 3), ("gaussian", "penyaw", 3),
                                           ("none", "penyaw", 1)])
def test_step_equals_the_chained_primitive(kind, reward, k):
    s, p, mean = _problem()
    env, ep = _env(kind, reward), _env_params(p)
    ds = dev_state(s)
    c, cp = _controller(env, k, mean)
    assert c.riccati_feedback is True and tuple(c.core.ilqr_rows.shape) == (1, k, RF) and tuple(c.core.ilqr_summary.shape) == (1, SF)
    costs = c.core.ilqr_costs()
    u, cp2, info = _step_once(c, cp, ep, ds)
    means, out = _chain(ds, c._params_c(ep), cp.a_mean, KEY, k, True)
    assert torch.equal(bits32(cp2.a_mean.reshape(-1)), bits32(means[k])) and torch.equal(bits32(u), bits32(means[k][:4]))
    choices = []
    for j, (row, cj, fb) in enumerate(out):
        assert torch.equal(bits32(info["ilqr_rows"][j]), bits32(row)), (j, info["ilqr_rows"][j], row)
        assert torch.equal(bits32(info["ilqr_feedback_rows"][j]), bits32(fb)), j
        assert torch.equal(bits32(costs[0, j]), bits32(cj)), j
        choices.append(int(ints(row)[2]))
    print(f"  ({kind}, {reward}) k = {k}: choices {choices} cost {float(info['ilqr_cost_first']):.6f} -> {float(info['ilqr_cost']):.6f}")
    assert any(ch != 0 for ch in choices)  # the step moved: there was something to compare
    # the handle's own rows describe the last iteration, the info keys are the summary's
    assert torch.equal(bits32(c.core.riccati_rows[0]), bits32(out[-1][0])) and torch.equal(bits32(c.core.riccati_feedback_rows[0]), bits32(out[-1][2]))
    assert int(info["ilqr_moved"]) == sum(ch != 0 for ch in choices) and int(info["ilqr_closed"]) == sum(ch >= NC for ch in choices)
    assert int(info["ilqr_fixed_at"]) == (choices.index(0) if 0 in choices else k)
    assert float(info["riccati_cost"]) == float(info["ilqr_cost"]) and "iter_cost_min" not in info
    _check_summary(c.core, 0, k)
    c.core.close()


def test_drag_runs_the_open_loop_chain():
    s, p, mean = _problem()
    env, ep = _env("drag"), _env_params(p)
    ds = dev_state(s)
    k = 3
    c, cp = _controller(env, k, mean)
    assert c.riccati_feedback is False and c.core.riccati_feedback_rows is None
    costs = c.core.ilqr_costs()
    u, cp2, info = _step_once(c, cp, ep, ds)
    means, out = _chain(ds, c._params_c(ep), cp.a_mean, KEY, k, False)
    assert torch.equal(bits32(cp2.a_mean.reshape(-1)), bits32(means[k]))
    for j, (row, cj) in enumerate(out):
        assert torch.equal(bits32(info["ilqr_rows"][j]), bits32(row)), j
        assert torch.equal(bits32(costs[0, j, :NC]), bits32(cj)), j
    assert int(info["ilqr_closed"]) == 0 and not bits32(info["ilqr_feedback_rows"]).any() and int(info["ilqr_moved"]) >= 1
    with pytest.raises(NotImplementedError, match="riccati_feedback=True with disturb_type='drag'"):
        _controller(env, k, mean, riccati_feedback=True)
    # an explicit False is honoured on a 13-state plant: the open-loop chain
    env2 = _env("none")
    c2, cp = _controller(env2, 2, mean, riccati_feedback=False)
    u, cp2, info = _step_once(c2, cp, ep, ds)
    means, out = _chain(ds, c2._params_c(ep), cp.a_mean, KEY, 2, False)
    assert torch.equal(bits32(cp2.a_mean.reshape(-1)), bits32(means[2])) and int(info["ilqr_closed"]) == 0
    c.core.close()
    c2.core.close()


# ------------------------------------------------------------------------------------------ 2: chain and fixed point
@pytest.mark.parametrize("name", ["hover_03", "rest"])
def test_costs_chain_and_the_fixed_point_holds(name):
    k = 6
    if name == "rest":
        s, p, mean = IO.rest_case()
    else:
        s, p, mean = _problem(0.3)
    env, ep = _env("none"), _env_params(p)
    ds = dev_state(s)
    c, cp = _controller(env, k, mean)
    costs = c.core.ilqr_costs()
    mean_in = cp.a_mean.clone()
    u, cp2, info = _step_once(c, cp, ep, ds)
    rows = info["ilqr_rows"]
    w = ints(rows)
    choices = w[:, 2].tolist()
    print(f"  {name}: choices {choices} rungs {(w[:, 7] >> 8).tolist()} base {rows[:, 0].tolist()} chosen {rows[:, 1].tolist()}")
    for j in range(k):
        assert float(rows[j, 1]) <= float(rows[j, 0]), j
        if j + 1 < k:
            assert w[j + 1, 0] == w[j, 1], j  # as words: the committed candidate is the next iteration's candidate 0
    want = _check_summary(c.core, 0, k)
    fixed = want[3]
    assert int(info["ilqr_fixed_at"]) == fixed
    if name == "rest":
        assert fixed < k, choices  # the input was chosen so that there is something to check ...
        assert not (w[:, 7] & 0xFF).any()  # ... on the line search's own path, not the flagged sweep's
    # from the first choice 0 on, the mean, the rows and the costs repeat as words
    means, _ = _chain(ds, c._params_c(ep), mean_in, KEY, min(fixed + 1, k), True)
    for j in range(fixed, k):
        assert choices[j] == 0, (j, choices)
        assert torch.equal(bits32(rows[j]), bits32(rows[fixed])) and torch.equal(bits32(costs[0, j]), bits32(costs[0, fixed])), j
        assert torch.equal(bits32(info["ilqr_feedback_rows"][j]), bits32(info["ilqr_feedback_rows"][fixed])), j
    if fixed < k:  # the committed mean is the one the first choice 0 left, which is the one it found
        assert torch.equal(bits32(cp2.a_mean.reshape(-1)), bits32(means[fixed]))
        assert torch.equal(bits32(means[fixed + 1]), bits32(means[fixed]))
    c.core.close()


# ------------------------------------------------------------------------------------------ 3: nothing sampled
def test_nothing_is_sampled():
    env = quad_env(task="tracking_zigzag")
    c, cp = cm.envs.get_controller(env, "ilqr", "N64_H32_lam0.01", device=DEV, iters=2)
    assert isinstance(c, cm.controllers.ILQRController) and c.iters == 2 and c.core.N == 1
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(1), params)
    c.core.a.view(torch.int32).fill_(0x7FC0BEEF)  # a quiet NaN with a payload
    c.core.cost.view(torch.int32).fill_(0x7FC0BEEF)
    cp = c.reset(state, params, c.init_control_params, cr.PRNGKey(2))
    for k in range(3):
        u, cp, cinfo = c(obs, state, params, cr.PRNGKey(10 + k), cp, info)
        obs, state, _, _, info = env.step(cr.PRNGKey(20 + k), state, u.cpu().numpy(), params)
    torch.cuda.synchronize()
    assert c.core.device_status() == 0 and int(cinfo["ilqr_moved"]) >= 1
    assert bool((bits32(c.core.a) == 0x7FC0BEEF).all()) and bool((bits32(c.core.cost) == 0x7FC0BEEF).all())
    c.core.close()


# ------------------------------------------------------------------------------------------ 4: a flagged sweep
def test_a_flagged_sweep_is_data():
    s, p, mean = _problem()
    env, ep = _env("none"), _env_params(p)
    ds = dev_state(s)
    bad = mean.copy().reshape(-1)
    bad[5] = np.nan
    k = 3
    c, cp = _controller(env, k, bad)
    shifted = _core().shift_mean(cp.a_mean.reshape(-1).contiguous().clone())
    u, cp2, info = _step_once(c, cp, ep, ds)  # (no error is raised, the status is clean)
    w = ints(info["ilqr_rows"])
    print(f"  flag words {[hex(int(x)) for x in w[:, 7]]} choices {w[:, 2].tolist()}")
    assert all(int(w[j, 7]) & 1 for j in range(k))
    assert torch.equal(bits32(cp2.a_mean.reshape(-1)), bits32(shifted))
    assert int(info["ilqr_moved"]) == 0 and int(info["ilqr_fixed_at"]) == 0 and int(info["ilqr_closed"]) == 0
    assert int(ints(c.core.ilqr_summary[0])[5]) & 1
    c.core.close()


# ------------------------------------------------------------------------------------------ 5: against fp64
def test_costs_against_the_fp64_oracle():
    s, p, mean = _problem()
    env, ep = _env("none"), _env_params(p)
    ds = dev_state(s)
    k = 3
    c, cp = _controller(env, k, mean)
    mean_in = cp.a_mean.clone()
    u, cp2, info = _step_once(c, cp, ep, ds)
    means, _ = _chain(ds, c._params_c(ep), mean_in, KEY, k, True)  # (the means between the iterations: test 1 holds them equal)
    assert torch.equal(bits32(cp2.a_mean.reshape(-1)), bits32(means[k]))
    rows = info["ilqr_rows"].cpu().numpy()
    c64 = [float(IO.plan_cost(s, p, means[j + 1].cpu().numpy().astype(np.float64))[0]) for j in range(k)]
    errs = [rel_err_scalar(float(rows[j, 1]), c64[j]) for j in range(k)]
    print(f"  device cost_chosen {rows[:, 1].tolist()} fp64 {c64} rel err {errs}")
    assert max(errs) <= COST_BAR
    for j in range(k - 1):
        assert c64[j + 1] <= c64[j] + 2 * COST_BAR * max(abs(c64[j]), 1.0), j
    c.core.close()


# ------------------------------------------------------------------------------------------ 6: batched equals singles
@pytest.mark.parametrize("m", [1, 3])
def test_batched_equals_singles(m):
    E, T, k = 3, 4, 2
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    act = [np.stack([np.asarray(cr.PRNGKey(60 + 10 * t + e)) for e in range(E)]) for t in range(T)]
    stp = [np.stack([np.asarray(cr.PRNGKey(600 + 10 * t + e)) for e in range(E)]) for t in range(T)]
    want = []
    for e in range(E):
        c, _ = cm.envs.get_controller(env, "ilqr", "N64_H32_lam0.01", device=DEV, iters=k, plan_hold=m)
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        cp = c.reset(se.state0, params[e], c.init_control_params, cr.PRNGKey(2))
        steps = []
        for t in range(T):
            u, cp, info = c(None, None, params[e], act[t][e], cp, {"noisy_state": se.noisy_state})
            assert m == 1 or info["plan_age"] == t % m
            steps.append((cp.a_mean.reshape(-1).clone(), c.core.ilqr_rows[0].clone(), c.core.ilqr_feedback_rows[0].clone(),
                          c.core.ilqr_summary[0].clone()))
            se.step(stp[t][e], u)
        torch.cuda.synchronize()
        assert c.core.device_status() == 0
        want.append(steps)
        cp0 = c.init_control_params
        c.core.close()
    b = cm.controllers.BatchedILQRController(env, E, H, iters=k, plan_hold=m, a_mean_init=cp0.a_mean, device=DEV)
    assert tuple(b.ilqr_rows.shape) == (E, k, RF) and tuple(b.ilqr_feedback_rows.shape) == (E, k, FF) and tuple(b.ilqr_summary.shape) == (E, SF)
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    b.bind_episode(ep)
    b.reset(None, None, None)
    for t in range(T):
        u = b.step(None, act[t])
        torch.cuda.synchronize()
        assert b.plan_age == (t % m if m > 1 else 0)
        for e in range(E):
            am, rows, fbs, summ = want[e][t]
            assert torch.equal(bits32(b.a_mean[e]), bits32(am)) and torch.equal(bits32(u[e]), bits32(am[:4])), (t, e)
            assert torch.equal(bits32(b.ilqr_rows[e]), bits32(rows)), (t, e, b.ilqr_rows[e], rows)
            assert torch.equal(bits32(b.ilqr_feedback_rows[e]), bits32(fbs)), (t, e)
            assert torch.equal(bits32(b.ilqr_summary[e]), bits32(summ)), (t, e)
            _check_summary(b.core, e, k)
        ep.step(stp[t], b.a_mean)
    print(f"  m = {m}: last summaries {[ints(b.ilqr_summary[e])[2:5].tolist() for e in range(E)]}")
    assert b.core.device_status() == 0
    b.core.close()


# ------------------------------------------------------------------------------------------ 7: the device episode equals the host loop
def test_run_episode_equals_the_host_loop():
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    T, m = 7, 3
    got = {}
    for mode in ("fused", "hand"):
        c, _ = cm.envs.get_controller(env, "ilqr", "N64_H32_lam0.01", device=DEV, iters=2, plan_hold=m, compute_plan=True)
        c.alias_outputs = True
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (c.core.lib, c.core.h), DEV)
        cp = c.reset(ep.state0, params, c.init_control_params, cr.PRNGKey(42))
        rng = cr.PRNGKey(43)
        if mode == "hand":
            us, ages, rows = [], [], []
            for _ in range(T):
                rng, rng_act, rng_step, _c = cr.split(rng, 4)
                u, cp, info = c(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                us.append(u.clone())
                ages.append(info["plan_age"])
                rows.append(c.core.plan_hold_rows[0].clone())
                ep.step(rng_step, u)
                rng, _c = cr.split(rng)
            got["hand"] = (torch.stack(us).cpu().numpy(), ep.read_log(), ages, torch.stack(rows).cpu().numpy())
        else:
            cp, rng = c.run_episode(ep, params, cp, rng, 4)
            cp, rng = c.run_episode(ep, params, cp, rng, T - 4)
            got["fused"] = (ep.read_trace()["u"][:T].copy(), ep.read_log(), ep.read_hold())
        got[mode + "_mean"] = cp.a_mean.cpu().numpy().copy()
        assert c.core.device_status() == 0
        c.core.close()
    hold = got["fused"][2]
    print(f"  single: ages {hold['age'][:T].tolist()} flags {hold['flags'][:T].tolist()}")
    assert got["hand"][2] == [0, 1, 2, 0, 1, 2, 0] and hold["age"][:T].tolist() == [0, 1, 2, 0, 1, 2, 0]
    assert got["fused"][0].tobytes() == got["hand"][0].tobytes()
    assert np.array_equal(got["fused"][1], got["hand"][1])
    hr = got["hand"][3]
    assert np.ascontiguousarray(hr).view(np.int32)[:, 0].tolist() == hold["age"][:T].tolist()
    assert np.array_equal(hold["gain"][:T], hr[:, 2]) and np.array_equal(hold["alpha"][:T], hr[:, 1])
    assert np.array_equal(hold["time"][:T], np.ascontiguousarray(hr[:, 6]).view(np.int32))
    assert got["fused_mean"].tobytes() == got["hand_mean"].tobytes()


def test_batched_run_episode_equals_the_host_loop():
    _batched_run_episode_equals_the_host_loop("gaussian")
    # per-step disturbance tables: the hold steps' plan trace forms its own from the instances' parked keys
    _batched_run_episode_equals_the_host_loop("periodic")


def _batched_run_episode_equals_the_host_loop(disturb):
    E, T, m = 3, 7, 3
    env = quad_env(task="tracking", randomizer=True, disturb=disturb)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    rngs0 = np.stack([np.asarray(cr.PRNGKey(60 + e)) for e in range(E)])
    dp = env.default_params
    th = (dp.m * dp.g / dp.max_thrust) * 2.0 - 1.0
    mean0 = np.tile(np.array([th, 0.0, 0.0, 0.0], dtype=np.float32), H)
    got = {}
    for mode in ("fused", "hand"):
        b = cm.controllers.BatchedILQRController(env, E, H, iters=2, plan_hold=m, compute_plan=True, a_mean_init=mean0, device=DEV)
        ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
        b.reset(None, None, None)
        if mode == "hand":
            b.bind_episode(ep)
            rngs = [rngs0[e] for e in range(E)]
            us, rows = [], []
            for _ in range(T):
                sp = [cr.split(r, 4) for r in rngs]
                u = b.step(None, np.stack([np.asarray(x[1]) for x in sp]))
                us.append(u.clone())
                rows.append(b.plan_hold_rows.clone())
                ep.step(np.stack([np.asarray(x[2]) for x in sp]), b.a_mean)
                rngs = [cr.split(x[0])[0] for x in sp]
            got["hand"] = (torch.stack(us, dim=1).cpu().numpy(), ep.read_log(), torch.stack(rows, dim=1).cpu().numpy())
        else:
            keys = b.run_episode(ep, rngs0.copy(), 4)
            b.run_episode(ep, keys, T - 4)
            got["fused"] = (ep.read_trace()["u"][:, :T].copy(), ep.read_log(), ep.read_hold())
        got[mode + "_mean"] = b.a_mean.cpu().numpy().copy()
        assert b.core.device_status() == 0
        b.core.close()
    hold = got["fused"][2]
    print(f"  batched: ages {hold['age'][:, :T].tolist()}")
    assert hold["age"][:, :T].tolist() == [[0, 1, 2, 0, 1, 2, 0]] * E
    assert got["fused"][0].tobytes() == got["hand"][0].tobytes()
    assert np.array_equal(got["fused"][1], got["hand"][1])
    hr = got["hand"][2]
    assert np.array_equal(hold["gain"][:, :T], hr[:, :, 2]) and np.array_equal(hold["alpha"][:, :T], hr[:, :, 1])
    assert np.array_equal(hold["time"][:, :T], np.ascontiguousarray(hr[:, :, 6]).view(np.int32))
    assert got["fused_mean"].tobytes() == got["hand_mean"].tobytes()


# ------------------------------------------------------------------------------------------ 8: the plan hold uses the last iteration
def test_plan_hold_latches_the_last_iteration():
    s, p, mean = _problem()
    env, ep = _env("none"), _env_params(p)
    ds = dev_state(s)
    c, cp = _controller(env, 2, mean, plan_hold=3)
    mean_in = cp.a_mean.clone()
    u0, cp1, info0 = _step_once(c, cp, ep, ds)
    assert info0["plan_age"] == 0
    means, out = _chain(ds, c._params_c(ep), mean_in, KEY, 2, True)
    latch = c.core.plan_latch()
    assert torch.equal(bits32(latch["b"][0]), bits32(means[1]))  # b_1: the mean the LAST iteration's sweep ran at ...
    assert not torch.equal(bits32(means[1]), bits32(means[0]))   # ... which is not b_0
    assert int(latch["t"][0]) == int(s.time)
    # the hold step on the next state of the plan (the time word + 1): the primitive on that latch, alpha of the last iteration's row
    s1 = s.replace(time=int(s.time) + 1, pos=s.pos + 0.01, vel=s.vel - 0.02)
    ds1 = dev_state(s1)
    mean1 = cp1.a_mean.reshape(-1).clone()
    u1, cp2, info1 = _step_once(c, cp1, ep, ds1, key=cr.PRNGKey(6))
    assert info1["plan_age"] == 1
    ric = c.core.riccati_rows[0]
    assert torch.equal(bits32(ric), bits32(out[1][0]))  # (a hold step leaves the plan step's rows: the last iteration's)
    side = torch.tensor([[0.0, 0.0, 0.0, float(ints(ric)[7] & 0xFF)]], dtype=torch.float64, device=DEV)
    am = mean1.clone().reshape(1, -1)
    up, rp = c.core.plan_hold(ds1.packed, latch["b"], latch["K"], latch["kff"], latch["x"], ric[3:4].clone(), 1, t_plan=latch["t"],
                              a_mean=am, rows=side)
    torch.cuda.synchronize()
    assert torch.equal(bits32(u1), bits32(up[0])) and torch.equal(bits32(c.core.plan_hold_rows[0]), bits32(rp[0]))
    assert torch.equal(bits32(cp2.a_mean.reshape(-1)), bits32(am[0]))
    assert (int(ints(rp[0])[4]) & 4) == 0 and float(rp[0][2]) > 0.0  # no time mismatch, the feedback term is live
    assert c.core.device_status() == 0
    c.core.close()


# ------------------------------------------------------------------------------------------ 9: the C side's refusals
def test_c_refusals_name_their_condition_before_any_launch():
    """check_ilqr_step (csrc/step_attach.hip): a handle that lacks the sweep, or carries something of a sampling step, refuses a step in
    COVO_MODE_ILQR with a message that says which -- and the mean it was given is untouched"""
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(1), params)
    c0, cp0 = cm.envs.get_controller(env, "ilqr", "N64_H32_lam0.01", device=DEV)
    pc = c0._params_c(params)
    ds = info["noisy_state"].to_device(DEV)
    mean = cp0.a_mean.reshape(-1).clone()
    cases = ((dict(), "without the Riccati refinement"),
             (dict(riccati=True, update="best"), "update arbiter"),
             (dict(riccati=True, compute_diag=True), "sampling diagnostics"),
             (dict(riccati=True, elite=8), "elite-set update"),
             (dict(riccati=True, ess_min=4.0), "ESS floor"),
             (dict(riccati=True, compute_fan=4), "sample fan"),
             (dict(riccati=True, compute_post_cov=True), "posterior covariance"),
             (dict(riccati=True, sigma_period=4), "Sigma period"),
             (dict(refine=True), "without the Riccati refinement"))  # (refine and riccati never share a core: the sweep is missed first)
    for kw, what in cases:
        core = SamplingCore(64, H, 0.01, 1.0, device=DEV, compute_info=False, **kw)
        am = mean.clone()
        with pytest.raises(_lib.CovoError, match=f"COVO_MODE_ILQR.*({what})"):
            core.step(_lib.MODE_ILQR, ds, pc, am, KEY, derive_keys=True, rollout_deterministic=True)
        torch.cuda.synchronize()
        assert torch.equal(bits32(am), bits32(mean)) and core.device_status() == 0
        core.close()
    # the raw key must be derived on the device; the phase timer has no iLQR phases
    with pytest.raises(_lib.CovoError, match="needs derive_keys = 1"):
        c0.core.step(_lib.MODE_ILQR, ds, pc, mean.clone(), KEY, derive_keys=False, rollout_deterministic=True)
    u, cp, _ = c0(obs, state, params, KEY, cp0, info)
    with pytest.raises(_lib.CovoError, match="covo_debug_time_step: the phase masks"):
        c0.core.time_phases()
    torch.cuda.synchronize()
    assert c0.core.device_status() == 0
    c0.core.close()
