"""GPU tests (-m gpu) of the plan hold (covo_plan_hold / covo_set_step_plan_hold / covo_set_episode_hold_log; `plan_hold=` on top of
`riccati=`; csrc/plan_hold.hip).  N = 256 samples, at most 3 instances, m = 3 unless stated.

1. the primitive against the oracle (tests/plan_hold_oracle.py) on the device's own sweeps (core.riccati at make_problem's state and at
   the atlas entries yaw_half_pi and far_fast; hover + 0.1 noise), stages 1 and 15, alpha in {0, 1, 2^-13}, the measured state
   xb_j + delta with delta chosen on the CPU so that in the oracle at least one component clips and at least one does not.  u within
   1.2e-7 absolute -- one fp32 ulp at 1: the kernel's fp64 chain of 14 fmas differs from numpy's unfused one by <= 14 * 2^-53 * the sum
   of the terms' magnitudes, far below half an fp32 ulp, so only a rounding tie can move the result, and by one ulp --, clipped
   components exactly +-1, row entries 0, 3, 4, 6 exact, entries 2 and 5 within 1e-6 relative; for one instance and for three.
2. stage 0 on the start state is the generator's first action (core.feedback_rollout) bit for bit, alpha in {4, 1, 2^-13}.
3. the fall-backs, bit for bit, with their flags.
4. the controller state: the mean one stage down with u in front, MPPI's covariance blocks one stage down.
5. the schedule of mppi, covo-offline and covo-online over 7 teacher-forced states: ages 0 1 2 0 1 2 0; a plan step equals a riccati=True
   controller without plan_hold on the same mean, state and key; a hold step equals the primitive on the latch; reset() restarts.
6. plan_hold=1 is off.
7. run_episode (12 steps, m = 4) equals the Python loop; the hold log's ages; the trace's u rows of hold steps.  Also covo-online
   under the periodic disturbance at m = 3: the hold steps' plan trace then runs on per-step tables formed from the parked keys.
8. batched (E = 3): hold steps equal the single controllers' -- under the periodic disturbance with the plan attached, their plan
   rows too; an instance reset on the device during a hold segment drops its feedback term (flag bit 2), the others are untouched.
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
from covo_mpc_amd.dynamics.dataclass import as_device_state  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from tests import plan_hold_oracle as PO  # noqa: E402
from tests.conftest import make_problem  # noqa: E402
from tests.gpu_support import DEV, H, batched_controller, dev_state, params_c, quad_env, single_controller  # noqa: E402
from tests.state_atlas import atlas_state  # noqa: E402

HF = _lib.COVO_HOLD_FLOATS
CASES = ("make_problem", "yaw_half_pi", "far_fast")
ALPHAS = (0.0, 1.0, 2.0 ** -13)


def bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def ints(t):
    """float32 device tensor -> its int32 words (numpy)"""
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.int32)


def clip32(x):
    return np.clip(np.asarray(x, dtype=np.float32), np.float32(-1), np.float32(1))


@functools.lru_cache(maxsize=None)
def _core():
    return SamplingCore(256, H, 0.01, 1.0, device=DEV, compute_info=False)


@functools.lru_cache(maxsize=None)
def _sweep(name):
    """the device's own sweep at the case's plan: (s, b [128] float32, ds, pc, numpy K, kff, x and the side row)"""
    s, p, rng = make_problem(seed=17, time=37) if name == "make_problem" else atlas_state(name)
    b = (R.hover_action(p, 32, np.float64) + 0.1 * rng.normal(size=(32, 4))).astype(np.float32).reshape(-1)
    core = _core()
    ds, pc = dev_state(s), params_c(p)
    out = core.riccati(ds, pc, torch.from_numpy(b).to(DEV))
    torch.cuda.synchronize()
    assert core.device_status() == 0
    g = {k: out[k][0].cpu().numpy() for k in ("K", "kff", "x", "rows")}
    print(f"  sweep at {name}: rung {g['rows'][1]:.0f} flags {g['rows'][3]:.0f} |K|max {np.abs(g['K']).max():.3f}")
    return s, b, ds, pc, g["K"], g["kff"], g["x"], g["rows"]


def _delta(b, K, kff, x, alpha, j):
    """a measured state float32 [13] near xb_j at which, in the oracle, at least one component clips and at least one does not"""
    v0 = alpha * kff[j] + b.reshape(32, 4)[j].astype(np.float64)
    for scale in (1.5, 2.0, 3.0, 5.0):
        for i in range(4):
            row = K[j, i, :13]
            if not np.abs(row).max() > 1e-9:
                continue
            for sign in (1.0, -1.0):
                d = row * (sign * scale - v0[i]) / (row @ row)
                xm = (x[j, :13] + d).astype(np.float32)
                o = PO.hold_step(xm, b, K, kff, x, alpha, j)
                if 1 <= o["clipped"] <= 3 and o["flags"] == 0:
                    return xm
    raise AssertionError("no state found at which one component clips and one does not")


def _packed(xm, time):
    st = np.zeros(32, dtype=np.float32)
    st[:13] = xm
    st[25:26] = np.asarray([time], dtype=np.int32).view(np.float32)
    return st


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _check_against_oracle(u, rows, want, tag):
    u = u.cpu().numpy().astype(np.float64)
    r, ri = rows.cpu().numpy(), ints(rows)
    for e, o in enumerate(want):
        err = np.abs(u[e] - o["u"]).max()
        print(f"    {tag} inst {e}: |u - oracle| {err:.3e} v {o['v']} clipped {o['clipped']} gain {o['gain']:.4f}")
        assert err <= 1.2e-7, (tag, e, err)
        sat = np.abs(o["v"]) > 1.0 + 1e-6
        assert np.all(u[e][sat] == np.sign(o["v"][sat])), (tag, e)  # exactly +-1
        assert ri[e, 0] == o["age"] and ri[e, 3] == o["clipped"] and ri[e, 4] == o["flags"] == 0 and ri[e, 6] == o["time"], (tag, e, ri[e])
        assert abs(r[e, 2] - o["gain"]) <= 1e-6 * o["gain"] and abs(r[e, 5] - o["dpos"]) <= 1e-6 * o["dpos"], (tag, e, r[e])
        assert r[e, 1] == np.float32(o["alpha"]) and r[e, 7] == 0.0


# ------------------------------------------------------------------------------------------ 1: the primitive against the oracle
@pytest.mark.parametrize("j", [1, 15])
def test_primitive_against_the_oracle(j):
    core = _core()
    sw = [_sweep(n) for n in CASES]
    for alpha in ALPHAS:
        xs = [_delta(s[1], s[4], s[5], s[6], alpha, j) for s in sw]
        want = [PO.hold_step(xm, s[1], s[4], s[5], s[6], alpha, j, time=50 + e) for e, (xm, s) in enumerate(zip(xs, sw))]
        assert all(1 <= o["clipped"] <= 3 for o in want)
        packed = _t(np.stack([_packed(xm, 50 + e) for e, xm in enumerate(xs)]))
        b = _t(np.stack([s[1] for s in sw]))
        K, kff, x = (_t(np.stack([s[i] for s in sw])) for i in (4, 5, 6))
        # three instances in one launch, then each alone
        u, rows = core.plan_hold(packed, b, K, kff, x, alpha, j)
        _check_against_oracle(u, rows, want, f"E=3 alpha={alpha} j={j}")
        for e in range(3):
            u1, rows1 = core.plan_hold(packed[e:e + 1], b[e:e + 1], K[e:e + 1], kff[e:e + 1], x[e:e + 1], alpha, j)
            _check_against_oracle(u1, rows1, want[e:e + 1], f"E=1 ({CASES[e]}) alpha={alpha} j={j}")
            assert torch.equal(bits32(u1[0]), bits32(u[e])) and torch.equal(bits32(rows1[0]), bits32(rows[e]))
    torch.cuda.synchronize()
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ 2: stage 0 equals the generator
@pytest.mark.parametrize("name", CASES)
def test_stage_zero_is_the_generators_first_action(name):
    s, b, ds, pc, K, kff, x, side = _sweep(name)
    core = _core()
    bd = _t(b)
    alphas = [4.0, 1.0, 2.0 ** -13]
    a_out, aux = core.feedback_rollout(ds, pc, bd, _t(K), _t(kff), _t(x), alphas=alphas)
    for a, alpha in enumerate(alphas):
        u, rows = core.plan_hold(ds.packed, bd, _t(K), _t(kff), _t(x), alpha, 0)
        assert torch.equal(bits32(u[0]), bits32(a_out[0, a, 0:4])), (name, alpha, u, a_out[0, a, 0:4])
        assert ints(rows)[0, 4] == 0
    torch.cuda.synchronize()
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ 3: the fall-backs
def test_fall_backs_bit_for_bit():
    s, b, ds, pc, K, kff, x, side = _sweep("make_problem")
    core = _core()
    j, alpha = 5, 0.5
    bd, Kd, kd, xd = _t(b), _t(K), _t(kff), _t(x)
    xm = (x[j, :13] + 0.02).astype(np.float32)
    plan = clip32(b.reshape(32, 4)[j])
    good = _t(_packed(xm, 37 + j))
    tp = torch.tensor([37], dtype=torch.int32, device=DEV)
    u, rows = core.plan_hold(good, bd, Kd, kd, xd, alpha, j, t_plan=tp)
    assert ints(rows)[0, 4] == 0 and rows[0, 2].item() > 1e-4 and not np.array_equal(u[0].cpu().numpy(), plan)
    # the sweep is flagged: zeroed gains, its side row says no rung was positive definite
    flagged = torch.tensor([[0.0, 8.0, 0.0, 8.0]], dtype=torch.float64, device=DEV)
    u, rows = core.plan_hold(good, bd, torch.zeros_like(Kd), torch.zeros_like(kd), xd, 0.0, j, t_plan=tp, rows=flagged)
    assert u[0].cpu().numpy().tobytes() == plan.tobytes() and ints(rows)[0, 4] == 1 and rows[0, 2].item() == 0.0
    # ... and with the gains it might have left all the same
    u, rows = core.plan_hold(good, bd, Kd, kd, xd, alpha, j, t_plan=tp, rows=flagged)
    assert u[0].cpu().numpy().tobytes() == plan.tobytes() and ints(rows)[0, 4] == 1
    # a NaN position: all four components fall back
    bad = good.clone()
    bad[0] = float("nan")
    u, rows = core.plan_hold(bad, bd, Kd, kd, xd, alpha, j, t_plan=tp)
    assert u[0].cpu().numpy().tobytes() == plan.tobytes() and ints(rows)[0, 4] == 2 and rows[0, 2].item() == 0.0
    # t_plan off by one: the feedback term is dropped (alpha is a power of two: fma(alpha, kff, b) is the unfused sum)
    u, rows = core.plan_hold(good, bd, Kd, kd, xd, alpha, j, t_plan=tp + 1)
    v0 = alpha * kff[j] + b.reshape(32, 4)[j].astype(np.float64)
    assert u[0].cpu().numpy().tobytes() == np.clip(v0, -1.0, 1.0).astype(np.float32).tobytes()
    assert ints(rows)[0, 4] == 4 and rows[0, 2].item() == 0.0 and ints(rows)[0, 6] == 37 + j
    torch.cuda.synchronize()
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ 4: the controller state
@pytest.mark.parametrize("n_inst", [1, 3])
def test_hold_step_shifts_the_controller_state(n_inst):
    s, b, ds, pc, K, kff, x, side = _sweep("make_problem")
    core = _core()
    j = 2
    rng = np.random.default_rng(4)
    mean0 = (0.5 * rng.normal(size=(n_inst, 128))).astype(np.float32)
    cov0 = np.stack([np.stack([(0.25 + 0.01 * k + e) * np.eye(4, dtype=np.float32) for k in range(32)]) for e in range(n_inst)])
    xm = (x[j, :13] + 0.01).astype(np.float32)
    packed = _t(np.stack([_packed(xm + np.float32(0.01 * e), 39) for e in range(n_inst)]))
    rep = lambda a: _t(np.stack([a] * n_inst))
    for with_cov in (True, False):
        am, ac = _t(mean0.copy()), (_t(cov0.copy()) if with_cov else None)
        u, rows = core.plan_hold(packed, rep(b), rep(K), rep(kff), rep(x), 0.25, j, a_mean=am, a_cov=ac)
        torch.cuda.synchronize()
        for e in range(n_inst):
            want = PO.shift(mean0[e], u[e].cpu().numpy(), cov0[e] if with_cov else None)
            wm = want[0] if with_cov else want
            assert am[e].cpu().numpy().tobytes() == wm.tobytes(), (e, with_cov)
            if with_cov:
                assert ac[e].cpu().numpy().tobytes() == want[1].tobytes(), e
        assert n_inst == 1 or not torch.equal(u[0], u[1])
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ 5: the schedule
def _states(env, params, n, seed=1):
    """n consecutive host states of one episode (time words t, t + 1, ...), reached with small random actions"""
    obs, info, state = env.reset(cr.PRNGKey(seed), params)
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        out.append((obs, info, state))
        u = (0.2 * rng.standard_normal(4)).clip(-1, 1).astype(np.float32)
        obs, state, _, _, info = env.step(cr.PRNGKey(7000 + k), state, u, params)
    return out


@pytest.mark.parametrize("name", ["mppi", "covo-offline", "covo-online"])
def test_schedule_plans_and_holds(name):
    env = quad_env(task="tracking_zigzag")
    ch, cph, _, _, _, params = single_controller(env, name, 256, riccati=True, plan_hold=3)
    cr_, cpr, _, _, _, _ = single_controller(env, name, 256, riccati=True)
    assert tuple(ch.core.plan_hold_rows.shape) == (1, HF) and cr_.core.plan_hold_rows is None
    seq = _states(env, params, 7)
    ages = []
    for k, (obs, info, state) in enumerate(seq):
        key = cr.PRNGKey(100 + k)
        before = cph
        mean0 = cph.a_mean.reshape(-1).clone()
        cov0 = cph.a_cov.clone() if name == "mppi" else None
        u, cph, ih = ch(obs, state, params, key, cph, info)
        torch.cuda.synchronize()
        age = ih["plan_age"]
        ages.append(age)
        assert isinstance(age, int) and ih["hold_flags"].dtype == torch.int32
        row = ch.core.plan_hold_rows[0]
        if age == 0:
            # the step of a riccati=True controller without plan_hold, on the same mean (MPPI: covariances), state and key
            kw = dict(a_mean=before.a_mean.clone()) if name != "mppi" else dict(a_mean=before.a_mean.clone(), a_cov=before.a_cov.clone())
            ur, cpr2, ir = cr_(obs, state, params, key, cpr.replace(**kw), info)
            torch.cuda.synchronize()
            assert torch.equal(bits32(u), bits32(ur)) and torch.equal(bits32(cph.a_mean), bits32(cpr2.a_mean)), (name, k)
            assert torch.equal(bits32(ch.core.riccati_rows), bits32(cr_.core.riccati_rows)), (name, k)
            if name == "mppi":
                assert torch.equal(bits32(cph.a_cov), bits32(cpr2.a_cov))
            assert ints(row)[:6].tolist() == [0] * 6 and ints(row)[6] == int(state.time) and ints(row)[7] == 0
            latch = ch.core.plan_latch()
            assert int(latch["t"][0]) == int(state.time)
        else:
            # the primitive on the latch, the handle's gains and the Riccati row's alpha; the sweep's flags from that row
            ric = ch.core.riccati_rows[0]
            alpha = ric[3:4].clone()
            fl = float(ints(ric)[7] & 0xFF)
            side = torch.tensor([[0.0, 0.0, 0.0, fl]], dtype=torch.float64, device=DEV)
            packed = as_device_state(info["noisy_state"], DEV).packed
            am = mean0.clone().reshape(1, -1)
            ac = cov0.clone().reshape(1, H, 4, 4) if cov0 is not None else None
            up, rp = ch.core.plan_hold(packed, latch["b"], latch["K"], latch["kff"], latch["x"], alpha, age, t_plan=latch["t"],
                                       a_mean=am, a_cov=ac, rows=side)
            torch.cuda.synchronize()
            assert torch.equal(bits32(u), bits32(up[0])), (name, k, u, up)
            assert torch.equal(bits32(row), bits32(rp[0])), (name, k, row, rp)
            assert torch.equal(bits32(cph.a_mean.reshape(-1)), bits32(am[0])) and torch.equal(bits32(cph.a_mean[0]), bits32(u))
            if name == "mppi":
                assert torch.equal(bits32(cph.a_cov), bits32(ac[0]))
            assert ints(row)[0] == age and (ints(row)[4] & 4) == 0 and float(ih["hold_alpha"]) == float(alpha)
            assert float(row[2]) > 0.0 or fl != 0.0  # the feedback term is live
        print(f"  {name} step {k}: age {age} hold row gain {float(row[2]):.3e} clipped {ints(row)[3]} flags {ints(row)[4]}")
    assert ages == [0, 1, 2, 0, 1, 2, 0]
    assert ch.core.plan_age == 1
    cph = ch.reset(seq[0][2], params, cph, cr.PRNGKey(2)) or cph  # (covo-offline: with its table rebuilt)
    assert ch.core.plan_age == 0
    obs, info, state = seq[0]
    _, _, ih = ch(obs, state, params, cr.PRNGKey(3), cph, info)
    assert ih["plan_age"] == 0 and ch.core.plan_age == 1
    torch.cuda.synchronize()
    assert ch.core.device_status() == 0 and cr_.core.device_status() == 0
    ch.core.close()
    cr_.core.close()


# ------------------------------------------------------------------------------------------ 6: plan_hold=1 is off
def test_plan_hold_one_is_off():
    env = quad_env(task="tracking_zigzag")
    ca, cpa, _, _, _, params = single_controller(env, "covo-online", 256, riccati=True, plan_hold=1)
    cb, cpb, _, _, _, _ = single_controller(env, "covo-online", 256, riccati=True)
    assert ca.core.plan_hold_rows is None and ca.core.plan_hold_info() == {}
    for k, (obs, info, state) in enumerate(_states(env, params, 3)):
        ua, cpa, ia = ca(obs, state, params, cr.PRNGKey(100 + k), cpa, info)
        ub, cpb, ib = cb(obs, state, params, cr.PRNGKey(100 + k), cpb, info)
        torch.cuda.synchronize()
        assert "plan_age" not in ia and sorted(ia) == sorted(ib)
        assert torch.equal(bits32(ua), bits32(ub)) and torch.equal(bits32(cpa.a_mean), bits32(cpb.a_mean))
        assert torch.equal(bits32(cpa.a_cov), bits32(cpb.a_cov)) and torch.equal(bits32(ca.core.riccati_rows), bits32(cb.core.riccati_rows))
        assert torch.equal(ca.core.a, cb.core.a) and torch.equal(ca.core.cost, cb.core.cost)
    assert ca.core.plan_age == 0 and ca.core.device_status() == 0
    ca.core.close()
    cb.core.close()


# ------------------------------------------------------------------------------------------ 7: the device loop equals the Python loop
@pytest.mark.parametrize("name, disturb, m", [pytest.param("mppi", "gaussian", 4, id="mppi"),
                                              pytest.param("covo-online", "gaussian", 4, id="covo-online"),
                                              # a hold step's plan trace on per-step tables formed from its parked keys, at two hold ages
                                              pytest.param("covo-online", "periodic", 3, id="covo-online-periodic")])
def test_run_episode_equals_the_python_loop(name, disturb, m):
    import covo_mpc_amd as cm
    env = quad_env(task="tracking_zigzag", disturb=disturb)
    params = env.default_params
    T = 12
    got = {}
    for mode in ("fused", "hand"):
        c, _ = cm.envs.get_controller(env, name, "N256_H32_lam0.01", device=DEV, compute_info=False, riccati=True, plan_hold=m,
                                      compute_plan=True)
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
            cp, rng = c.run_episode(ep, params, cp, rng, 5)
            cp, rng = c.run_episode(ep, params, cp, rng, T - 5)
            got["fused"] = (ep.read_trace()["u"][:T].copy(), ep.read_log(), ep.read_hold())
        got[mode + "_state"] = (ep.true.cpu().numpy().copy(), ep.noisy.cpu().numpy().copy(), cp.a_mean.cpu().numpy().copy())
        assert c.core.device_status() == 0
        c.core.close()
    want_ages = [t % m for t in range(T)]
    hold = got["fused"][2]
    print(f"  {name}: ages {hold['age'].tolist()} flags {hold['flags'].tolist()} clipped {hold['clipped'].tolist()}")
    assert got["hand"][2] == want_ages and hold["age"].tolist() == want_ages
    assert np.array_equal(got["fused"][1], got["hand"][1])  # the env log
    for f, h in zip(got["fused_state"], got["hand_state"]):
        assert f.tobytes() == h.tobytes()
    # the trace's u rows are the applied actions: on hold steps the held ones
    assert got["fused"][0].tobytes() == got["hand"][0].tobytes()
    # the hold log's rows are the handle's rows of every step
    hr = got["hand"][3]
    assert np.array_equal(hold["gain"], hr[:, 2]) and np.array_equal(hold["time"], np.ascontiguousarray(hr[:, 6]).view(np.int32))
    assert np.all((hold["flags"] & 4) == 0) and np.all(hold["gain"][np.asarray(want_ages) > 0] > 0.0)


# ------------------------------------------------------------------------------------------ 8: batched
def test_batched_hold_steps_equal_singles():
    _batched_hold_steps_equal_singles("gaussian", plan=False)
    # the same with the plan attached under a disturbance with per-step tables: a hold step's plan trace on the instances' parked keys
    _batched_hold_steps_equal_singles("periodic", plan=True)


def _batched_hold_steps_equal_singles(disturb, plan):
    import covo_mpc_amd as cm
    N, E, m, T = 256, 3, 3, 4
    env = quad_env(task="tracking", randomizer=True, disturb=disturb)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    act = [np.stack([np.asarray(cr.PRNGKey(60 + 10 * k + e)) for e in range(E)]) for k in range(T)]
    stp = [np.stack([np.asarray(cr.PRNGKey(600 + 10 * k + e)) for e in range(E)]) for k in range(T)]
    rows, means, us, plans = [], [], [], []
    for e in range(E):
        c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False, riccati=True, plan_hold=m,
                                      compute_plan=plan)
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        cp = c.reset(se.state0, params[e], c.init_control_params, cr.PRNGKey(2))
        r, mm, uu, pp = [], [], [], []
        for k in range(T):
            u, cp, info = c(None, None, params[e], act[k][e], cp, {"noisy_state": se.noisy_state})
            assert info["plan_age"] == k % m
            r.append(c.core.plan_hold_rows[0].clone())
            mm.append(cp.a_mean.reshape(-1).clone())
            uu.append(u.reshape(-1).clone())
            pp.append(c.core.plan[0].clone() if plan else None)
            se.step(stp[k][e], u)
        torch.cuda.synchronize()
        rows.append(r), means.append(mm), us.append(uu), plans.append(pp)
        cp0 = c.init_control_params
        assert c.core.device_status() == 0
        c.core.close()
    b = batched_controller(env, "covo-online", cp0, E, N, 0.01, riccati=True, plan_hold=m, compute_plan=plan)
    assert tuple(b.plan_hold_rows.shape) == (E, HF)
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    b.bind_episode(ep)
    for k in range(T):
        u = b(None, act[k])
        torch.cuda.synchronize()
        assert b.plan_age == k % m
        for e in range(E):
            assert torch.equal(bits32(u[e].reshape(-1)), bits32(us[e][k])), (k, e)
            assert torch.equal(bits32(b.a_mean[e]), bits32(means[e][k])), (k, e)
            assert torch.equal(bits32(b.plan_hold_rows[e]), bits32(rows[e][k])), (k, e, b.plan_hold_rows[e], rows[e][k])
            if plan and k % m != 0:
                assert bool(torch.isfinite(b.plan[e]).all()) and torch.equal(bits32(b.plan[e]), bits32(plans[e][k])), (k, e)
        ep.step(stp[k], b.a_mean)
    print(f"  hold rows of the last hold step: gains {[float(rows[e][2][2]) for e in range(E)]} flags {[int(ints(rows[e][2])[4]) for e in range(E)]}")
    assert all(float(rows[e][1][2]) > 0.0 and (int(ints(rows[e][1])[4]) & 4) == 0 for e in range(E))
    assert b.core.device_status() == 0
    b.core.close()


def test_batched_reset_during_a_hold_segment():
    """instance 1 leaves the box on step 0 and is reset on the device by the env step of step 1 (forced as tests/test_gpu_reset.py
    forces it): the hold step of age 2 finds another time word, drops the feedback term and says so; instances 0 and 2 are what they
    are without the push"""
    import covo_mpc_amd as cm
    N, E, m = 256, 3, 3
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    rngs0 = np.stack([np.asarray(cr.PRNGKey(60 + e)) for e in range(E)])
    c0, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    cp0 = c0.init_control_params
    c0.core.close()
    out = {}
    for push in (True, False):
        b = batched_controller(env, "covo-online", cp0, E, N, 0.01, riccati=True, plan_hold=m)
        ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
        if push:
            ep.true[1, 0:3] = torch.tensor([2.96, 0.0, 0.0], device=DEV)
            ep.true[1, 3:6] = torch.tensor([2.5, 0.0, 0.0], device=DEV)
            ep.noisy[1].copy_(ep.true[1])
        b.run_episode(ep, rngs0.copy(), m)
        out[push] = (ep.read_log(), ep.read_hold(), b.a_mean.clone(), ep.true.clone())
        assert b.core.device_status() == 0
        b.core.close()
    log, hold = out[True][0], out[True][1]
    print(f"  done rows {log[:, :, 3].tolist()} ages {hold['age'].tolist()} flags {hold['flags'].tolist()} times {hold['time'].tolist()}")
    assert hold["age"].tolist() == [[0, 1, 2]] * E
    assert [int(log[e, :, 3].sum()) for e in range(E)] == [0, 1, 0] and log[1, 1, 3] == 1.0
    assert hold["flags"][1, 2] & 4 and hold["gain"][1, 2] == 0.0 and hold["time"][1, 2] == 0
    assert (hold["flags"][1, 1] & 4) == 0 and hold["gain"][1, 1] > 0.0
    for e in (0, 2):
        assert np.all((hold["flags"][e] & 4) == 0)
        assert np.array_equal(log[e], out[False][0][e])
        for f in ("age", "alpha", "gain", "clipped", "flags", "dpos", "time"):
            assert np.array_equal(hold[f][e], out[False][1][f][e]), (e, f)
        assert torch.equal(bits32(out[True][2][e]), bits32(out[False][2][e])) and torch.equal(bits32(out[True][3][e]), bits32(out[False][3][e]))
