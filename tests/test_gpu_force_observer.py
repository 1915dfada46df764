"""GPU: the force observer -- csrc/force_observer.hip against tests/force_observer_oracle.py and against the shipped
state estimator's kernel, the entry's extents and stream, the episode drivers against the Python loop, the host path, and the
closed-loop condition: it observes a held force.

Bars.  xi and P: BAR = 8 x FO.FP64_LOSS, the fp64 filter's own loss against its np.longdouble re-run on these very chains
(tests/test_force_observer_oracle.py measures it: 4.35e-15), in the measure FO.deviation: xi per coordinate group, the force group on
the scale of max(|f|, its standard deviation), P on the scale of its own diagonal.  The margin is for a different summation order and
the matrix core's accumulation; the measured worst over the cases of test 1 is printed.  The side row is fp32: the two words exact, the
floats within one fp32 ulp of the fp32 rounding of the oracle's value.  Everything else is bit for bit."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

pytestmark = pytest.mark.gpu

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers import ForceObserver, StateEstimator  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from tests import contract_support as CS  # noqa: E402
from tests import force_observer_oracle as FO  # noqa: E402
from tests.conftest import make_problem  # noqa: E402
from tests.gpu_support import DEV, H, batched_controller, bits, params_c, quad_env, set_time, ulps  # noqa: E402
from tests.state_atlas import atlas_state  # noqa: E402

BAR = 8.0 * FO.FP64_LOSS
STARTS = ("make_problem", "yaw_pi_minus", "inverted", "unnorm_q", "far_fast")
MASSES = (0.027, 0.021, 0.034)
OBS = tuple(0.05 * FO.OBS_GROUP_SCALE)
CONSTS = dict(obs_std=OBS, proc_std=(0.0, 0.0, 0.0, 0.0), force_walk_std=0.05, force_init_std=0.2 / np.sqrt(3.0))
f64 = dict(dtype=torch.float64, device=DEV)
f32 = dict(dtype=torch.float32, device=DEV)
E_BADARG = -1  # include/covo_hip.h: COVO_E_BADARG


@pytest.fixture(scope="module")
def core():
    c = SamplingCore(64, H, 0.01, 1.0, device=DEV, use_graph=False, compute_info=False)
    yield c
    c.close()


def state_buffers(E):
    return (torch.zeros((E, 16), **f64), torch.zeros((E, 16, 16), **f64), torch.zeros((E, 2), dtype=torch.int32, device=DEV))


def launch(core, rows, u, pcs, bufs, reset=False, consts=CONSTS):
    """covo_observe_force on numpy rows [E, 32] / u [E, 4] -> (rows after, side rows) as numpy; bufs (xi, P, meta) updated in place"""
    E = len(rows)
    st = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(DEV)
    ud = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(DEV)
    arr = (_lib.EnvParamsC * E)(*pcs)
    side = core.observe_force(st, ud, arr, *bufs, reset=reset, **consts)
    torch.cuda.synchronize()
    return st.cpu().numpy(), side.cpu().numpy()


def model_of(mass):
    _, p, _ = make_problem()
    m = float(np.float32(mass))
    pc = params_c(p)
    pc.m = m
    return p.replace(m=m), pc


@pytest.fixture(scope="module")
def chains():
    """Per start state and mass: FO.build_chain's 8 measured rows with their actions and the oracle's answer to every call -- the
    chains the CPU test measures the fp64 loss on.  Computed once."""
    out = {}
    for si, name in enumerate(STARTS):
        s, _, _ = make_problem() if name == "make_problem" else atlas_state(name)
        for mi, mass in enumerate(MASSES):
            p, pc = model_of(mass)
            out[(name, mi)] = (pc, FO.build_chain(s, p, 100 * si + mi, OBS, **{k: v for k, v in CONSTS.items() if k != "obs_std"}))
    return out


def check_call(got_row, got_side, bufs, e, call, where):
    xi, P, meta = (b.cpu().numpy() for b in bufs)
    dev = FO.deviation(xi[e], P[e], call["xi"], call["P"])
    assert dev <= BAR, (where, dev)
    assert np.array_equal(P[e], P[e].T), where
    assert meta[e].tolist() == [1, call["t_prev"]], where
    assert np.array_equal(bits(got_row[16:]), bits(call["row"][16:])), where
    flags = int(got_side.view(np.int32)[0])
    assert flags == int(call["ref_side"][0]) and int(got_side.view(np.int32)[7]) == int(call["ref_side"][7]), (where, got_side)
    if flags == 0:
        assert np.array_equal(bits(got_row[:16]), bits(xi[e].astype(np.float32))), where
        assert ulps(got_row[:16], call["ref_row"][:16]) <= 1.0, (where, got_row[:16], call["ref_row"][:16])
    else:
        assert np.array_equal(bits(got_row[:13]), bits(call["row"][:13])) and not bits(got_row[13:16]).any(), where
    assert ulps(got_side[1:7], call["ref_side"][1:7].astype(np.float32)) <= 1.0, (where, got_side, call["ref_side"])
    return dev


# ---- 1. the kernel against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STARTS)
def test_kernel_against_the_oracle_alone_and_as_a_batch_of_three_masses(core, chains, name):
    worst = 0.0
    pc, calls = chains[(name, 0)]
    bufs = state_buffers(1)
    for k, call in enumerate(calls):
        rows, side = launch(core, call["row"][None], call["u"][None], [pc], bufs, reset=(k == 0))
        worst = max(worst, check_call(rows[0], side[0], bufs, 0, call, (name, "alone", k)))
    bufs = state_buffers(3)
    for k in range(8):
        cs = [chains[(name, mi)][1][k] for mi in range(3)]
        rows, side = launch(core, np.stack([c["row"] for c in cs]), np.stack([c["u"] for c in cs]),
                            [chains[(name, mi)][0] for mi in range(3)], bufs, reset=(k == 0))
        for e in range(3):
            worst = max(worst, check_call(rows[e], side[e], bufs, e, cs[e], (name, "batch", e, k)))
    print(f"  {name}: worst deviation of xi and P from the oracle {worst:.2e} (bar {BAR:g} = 8 x the fp64 loss {FO.FP64_LOSS:g})")
    assert core.device_status() == 0


# ---- 2. batch equals single, run to run -------------------------------------------------------------------------------------------
def run_chain(core, chains, name, masses, n=4):
    E = len(masses)
    bufs = state_buffers(E)
    outs = []
    for k in range(n):
        cs = [chains[(name, mi)][1][k] for mi in masses]
        rows, side = launch(core, np.stack([c["row"] for c in cs]), np.stack([c["u"] for c in cs]), [chains[(name, mi)][0] for mi in masses],
                            bufs, reset=(k == 0))
        outs.append((rows, side, bufs[0].cpu().numpy().copy(), bufs[1].cpu().numpy().copy(), bufs[2].cpu().numpy().copy()))
    return outs


def test_batch_equals_single_and_run_to_run(core, chains):
    a = run_chain(core, chains, "far_fast", (0, 1, 2))
    b = run_chain(core, chains, "far_fast", (0, 1, 2))
    for x, y in zip(a, b):
        for p, q in zip(x, y):
            assert p.tobytes() == q.tobytes()
    for e in range(3):
        s = run_chain(core, chains, "far_fast", (e,))
        for k, (x, y) in enumerate(zip(a, s)):
            for p, q in zip(x, y):
                assert p[e].tobytes() == q[0].tobytes(), (e, k)


# ---- 3. the cross-check with the shipped kernel -----------------------------------------------------------------------------------
def test_without_a_force_state_it_agrees_with_the_state_estimators_kernel(core, chains):
    """force_init_std = force_walk_std = 0 on force-free rows: x^ and P[0:13, 0:13] against covo_estimate with the same proc_std, at
    the bar of test 1 (the state estimator's measure: x per group, P on its own diagonal); f^ and its rows of P stay exactly 0."""
    consts = dict(obs_std=OBS, proc_std=(0.0, 0.02, 0.0, 0.0), force_walk_std=0.0, force_init_std=0.0)
    worst = 0.0
    for name in ("make_problem", "far_fast"):
        pcs = [chains[(name, mi)][0] for mi in range(3)]
        a, b = state_buffers(3), (torch.zeros((3, 16), **f64), torch.zeros((3, 13, 13), **f64), torch.zeros((3, 2), dtype=torch.int32, device=DEV))
        for k in range(8):
            cs = [chains[(name, mi)][1][k] for mi in range(3)]
            rows = np.stack([c["row"] for c in cs])
            rows[:, 13:16] = 0
            u = np.stack([c["u"] for c in cs])
            ra, _ = launch(core, rows, u, pcs, a, reset=(k == 0), consts=consts)
            st = torch.from_numpy(rows).to(DEV)
            core.estimate(st, torch.from_numpy(u).to(DEV), (_lib.EnvParamsC * 3)(*pcs), *b, obs_std=OBS, proc_std=consts["proc_std"],
                          reset=(k == 0))
            torch.cuda.synchronize()
            xi, P = a[0].cpu().numpy(), a[1].cpu().numpy()
            xe, Pe = b[0].cpu().numpy()[:, :13], b[1].cpu().numpy()
            assert not xi[:, 13:].any() and not P[:, 13:, :].any() and not P[:, :, 13:].any(), (name, k)
            for e in range(3):
                ex = max(np.abs(xi[e, :13][FO.GROUP == g] - xe[e][FO.GROUP == g]).max() / np.abs(xe[e][FO.GROUP == g]).max() for g in range(4))
                d = np.sqrt(np.diag(Pe[e]))
                worst = max(worst, ex, (np.abs(P[e, :13, :13] - Pe[e]) / np.outer(d, d)).max())
            assert worst <= BAR, (name, k, worst)
            if k > 0:
                assert ulps(ra[:, :13], st.cpu().numpy()[:, :13]) <= 1.0, (name, k)
    print(f"  worst deviation of x^ and P[0:13, 0:13] from covo_estimate's {worst:.2e} (bar {BAR:g})")


# ---- 4. fall-backs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault,flag", [("fresh", 1), ("time", 2), ("nan", 4), ("bad P", 8)])
def test_fall_backs_flag_one_instance_and_leave_its_neighbours_alone(core, chains, fault, flag):
    """A batch of three whose middle instance meets the fault at call 2: its flag, its row what the definition says (untouched under
    flag 4, else the kinematic floats untouched and the force slots 0), the filter's state what the definition says; the neighbours'
    outputs are the bits of the same batch without the fault; the next call is clean."""
    name = "make_problem"
    pcs = [chains[(name, mi)][0] for mi in range(3)]
    calls = [[dict(c) for c in chains[(name, mi)][1][:4]] for mi in range(3)]

    def run(faulty):
        bufs = state_buffers(3)
        outs = []
        for k in range(4):
            rows = np.stack([calls[e][k]["row"] for e in range(3)])
            if faulty and k == 2:
                if fault == "time":
                    rows[1].view(np.int32)[FO.ST_TIME] += 1  # (off by 2 against the row before)
                elif fault == "nan":
                    rows[1, 4] = np.nan
                elif fault == "bad P":
                    bufs[1][1, 5, 14] = float("nan")
                elif fault == "fresh":
                    bufs[2][1, 0] = 0  # (what a fresh handle's buffers hold: no valid state)
            if faulty and k == 3 and fault == "time":
                rows[1].view(np.int32)[FO.ST_TIME] += 1  # (the chain goes on from the jumped time word)
            got, side = launch(core, rows, np.stack([calls[e][k]["u"] for e in range(3)]), pcs, bufs, reset=(k == 0))
            outs.append((rows, got, side, [b.cpu().numpy().copy() for b in bufs]))
        return outs
    clean, bad = run(False), run(True)
    rows, got, side, (xi, P, meta) = bad[2]
    assert int(side[1].view(np.int32)[0]) == flag, side[1]
    want = rows[1].copy()
    if fault != "nan":
        want[13:16] = 0
    assert np.array_equal(bits(got[1]), bits(want))
    _, _, P0 = FO.constants(model_of(MASSES[1])[0], **CONSTS)
    if fault == "nan":
        assert meta[1, 0] == 0 and not side[1, 1:7].any()
        for x, y in zip((xi, P), bad[1][3][:2]):
            assert x[1].tobytes() == y[1].tobytes()  # (the invalidated filter's buffers are not written)
    else:
        assert meta[1].tolist() == [1, int(rows[1].view(np.int32)[FO.ST_TIME])]
        assert np.array_equal(xi[1, :13], rows[1, :13].astype(np.float64)) and not xi[1, 13:].any() and np.array_equal(P[1], np.diag(P0))
    for j in (0, 2):
        for k in range(4):
            for x, y in zip(bad[k][1:3], clean[k][1:3]):
                assert x[j].tobytes() == y[j].tobytes(), (fault, j, k)
            for x, y in zip(bad[k][3], clean[k][3]):
                assert x[j].tobytes() == y[j].tobytes(), (fault, j, k)
    rows, got, side, (xi, P, meta) = bad[3]
    nxt = int(side[1].view(np.int32)[0])
    assert nxt == (1 if fault == "nan" else 0), side[1]
    assert np.isfinite(xi[1]).all() and np.isfinite(P[1]).all() and np.array_equal(P[1], P[1].T) and meta[1, 0] == 1
    if nxt == 0:
        assert np.array_equal(bits(got[1, :16]), bits(xi[1].astype(np.float32))) and side[1, 1] > 0
    assert core.device_status() == 0


# ---- 5. extents and stream --------------------------------------------------------------------------------------------------------
def raw_inputs(chains, k):
    name = "inverted"
    cs = [chains[(name, mi)][1][k] for mi in range(3)]
    return dict(rows=np.stack([c["row"] for c in cs]), u=np.stack([c["u"] for c in cs])), [chains[(name, mi)][0] for mi in range(3)]


def raw_call(core, T, pcs, reset, stream=None):
    arr = (_lib.EnvParamsC * 3)(*pcs)
    return core.lib.covo_observe_force(core.h, _lib.ptr(T["rows"]), _lib.ptr(T["u"]), 4, arr, (C.c_double * 4)(*OBS),
                                       (C.c_double * 4)(*CONSTS["proc_std"]), CONSTS["force_walk_std"], CONSTS["force_init_std"],
                                       _lib.ptr(T["xi"]), _lib.ptr(T["P"]), _lib.ptr(T["meta"]), _lib.ptr(T["side"]), 3,
                                       1 if reset else 0, core.stream() if stream is None else stream)


@pytest.mark.parametrize("poison", CS.POISONS)
def test_extents_only_floats_0_to_15_and_the_filters_buffers_are_written(core, chains, poison):
    """Two calls of a batch of three (an initialisation, an update) with every buffer inside guard bands: no band loses a word, u
    keeps its bits, floats 16 .. 31 of every row keep theirs, and the results are those of the plain calls whatever the poison."""
    want = run_chain(core, chains, "inverted", (0, 1, 2), n=2)
    state = dict(xi=CS.banded_empty((3, 16), torch.float64, poison, device=DEV, name="xi"),
                 P=CS.banded_empty((3, 16, 16), torch.float64, poison, device=DEV, name="P"),
                 meta=CS.banded_empty((3, 2), torch.int32, poison, device=DEV, name="meta"))
    for k in range(2):
        X, pcs = raw_inputs(chains, k)
        al = {n: CS.banded(v, poison, device=DEV, name=n) for n, v in X.items()}
        al["side"] = CS.banded_empty((3, 8), torch.float32, poison, device=DEV, name="side")
        al.update(state)
        torch.cuda.synchronize()
        assert raw_call(core, {n: a.view for n, a in al.items()}, pcs, reset=(k == 0)) == 0
        torch.cuda.synchronize()
        for n, a in al.items():
            assert CS.bands_intact(a) is None, (k, CS.bands_intact(a))
        for n in ("side", "xi", "P", "meta"):
            assert CS.unwritten(al[n]).size == 0, (k, n)
        got = al["rows"].view.cpu().numpy()
        assert np.array_equal(bits(al["u"].view), bits(X["u"])) and np.array_equal(bits(got[:, 16:]), bits(X["rows"][:, 16:])), k
        for x, y in zip((got, al["side"].view.cpu().numpy(), al["xi"].view.cpu().numpy(), al["P"].view.cpu().numpy(),
                         al["meta"].view.cpu().numpy()), want[k]):
            assert x.tobytes() == y.tobytes(), k


def test_the_launch_runs_on_the_callers_stream(core, chains):
    """The rows and u hold NaN; a side stream sleeps, then copies the real values in, then the call follows on it and the inputs are
    spoiled again behind it: work on another stream would read NaN (flag 4, rows untouched) -- the outputs must be the update's."""
    want = run_chain(core, chains, "inverted", (0, 1, 2), n=2)
    X0, pcs = raw_inputs(chains, 0)
    X1, _ = raw_inputs(chains, 1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    T = dict(rows=dev(X0["rows"]), u=dev(X0["u"]), side=torch.zeros((3, 8), **f32))
    T["xi"], T["P"], T["meta"] = state_buffers(3)
    assert raw_call(core, T, pcs, reset=True) == 0
    stage = dict(rows=dev(X1["rows"]), u=dev(X1["u"]))
    bad = {k: torch.full_like(v, float("nan")) for k, v in stage.items()}
    out_rows = torch.zeros_like(stage["rows"])
    for k in stage:
        T[k].copy_(bad[k])
    side = torch.cuda.Stream()
    per_ms = CS.sleep_cycles_per_ms(torch)
    torch.cuda.synchronize()

    def call():
        rc = raw_call(core, T, pcs, reset=False)
        out_rows.copy_(T["rows"], non_blocking=True)  # (on the side stream too: behind the launch, ahead of the spoiling)
        return rc
    rc, slept = CS.delayed(side, [(T[k], stage[k]) for k in stage], cycles=int(per_ms * 10.0), call=call, spoil=[(T["u"], bad["u"])])
    torch.cuda.synchronize()
    assert rc == 0 and slept >= 5.0, slept
    for x, y in zip((out_rows.cpu().numpy(), T["side"].cpu().numpy(), T["xi"].cpu().numpy(), T["P"].cpu().numpy(), T["meta"].cpu().numpy()),
                    want[1]):
        assert x.tobytes() == y.tobytes()


# ---- 6. the drivers equal the loop ------------------------------------------------------------------------------------------------
def obs_consts(params):
    """what ForceObserver(env) attaches at the defaults, for the stand-alone launches of the loops"""
    return dict(obs_std=tuple(float(params.obs_noise_scale) * g for g in FO.OBS_GROUP_SCALE), proc_std=(0.0, 0.0, 0.0, 0.0),
                force_walk_std=float(params.dyn_noise_scale), force_init_std=float(params.disturb_scale) / np.sqrt(3.0))


@pytest.mark.parametrize("name,kw,n", [("mppi", {}, 12), ("covo-online", dict(riccati=True, plan_hold=2), 6)], ids=["mppi", "covo-online-hold"])
def test_run_episode_equals_the_python_loop(name, kw, n):
    """run_episode with the observer attached equals controller step -> covo_env_step -> core.observe_force, word for word in states,
    actions and observer log (N = 256; covo-online with a plan hold of 2: every second step is a hold step, which reads the
    observer's row)."""
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    got = {}
    for mode in ("driver", "loop"):
        c, _ = cm.envs.get_controller(env, name, "N256_H32_lam0.01", device=DEV, compute_info=False, **kw)
        c.alias_outputs = True
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (c.core.lib, c.core.h), DEV)
        rng = cr.PRNGKey(43)
        if mode == "driver":
            obs = ForceObserver(env).attach(c)
            cp = c.reset(ep.state0, params, c.init_control_params, cr.PRNGKey(42))
            cp, rng = c.run_episode(ep, params, cp, rng, 2)
            cp, rng = c.run_episode(ep, params, cp, rng, n - 2)
            e = ep.read_force()
            log = np.concatenate([e["measured"], e["force_true"], e["written"]], axis=1)
            sides = e["rows"]
            assert torch.equal(obs.rows[0], ep.obslog[n - 1, 32:]) and obs.xhat.shape == (1, 13) and obs.force.shape == (1, 3)
            assert obs.P.shape == (1, 16, 16) and np.array_equal(e["force_est"], e["written"][:, 13:16])
            flags = np.ascontiguousarray(sides[:, 0]).view(np.int32)
            assert flags.tolist() == [1] + [0] * (n - 1) and (sides[1:, 1] > 0).all() and (sides[1:, 6] > 0).all()
        else:
            cp = c.reset(ep.state0, params, c.init_control_params, cr.PRNGKey(42))
            bufs, pc = state_buffers(1), c._params_c(params)
            meas, sides = [], []
            for t in range(n):
                rng, rng_act, rng_step, _c = cr.split(rng, 4)
                u, cp, info = c(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                ep.step(rng_step, u)
                z = ep.noisy[:16].clone()
                side = c.core.observe_force(ep.noisy, cp.a_mean.reshape(-1)[:4], pc, *bufs, reset=(t == 0), **obs_consts(params))
                meas.append(torch.cat([z, ep.noisy[:16]]).cpu().numpy())
                sides.append(side[0].cpu().numpy())
                rng, _c = cr.split(rng)
            log, sides = np.stack(meas), np.stack(sides)
        torch.cuda.synchronize()
        got[mode] = (ep.read_log().copy(), ep.true.cpu().numpy().copy(), ep.noisy.cpu().numpy().copy(), cp.a_mean.cpu().numpy().copy(),
                     np.asarray(rng).copy(), np.ascontiguousarray(log), np.ascontiguousarray(sides))
        assert c.core.device_status() == 0
        c.core.close()
    for k, (x, y) in enumerate(zip(got["driver"], got["loop"])):
        assert x.tobytes() == y.tobytes(), (name, k)
    log = got["driver"][5]
    assert not np.array_equal(log[1:, :16], log[1:, 16:])  # (the written row is not the measured one)
    assert np.array_equal(got["driver"][1][13:16], log[-1, 13:16])  # (the plant's own force is untouched: the true row still holds it)


def test_run_episode_batched_equals_the_loop_through_an_auto_reset():
    """E = 2 on the batched driver, MPPI at N = 256; instance 1 starts two steps before its episode's end, so the device env step
    resets it inside the segment: flag bit 1 at exactly the reset steps of exactly that instance."""
    E, n, N = 2, 6, 256
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(140 + e)) for e in range(E)]
    c0, _ = cm.envs.get_controller(env, "mppi", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    cp0 = c0.init_control_params
    c0.core.close()
    reset_keys = [cr.PRNGKey(150 + e) for e in range(E)]
    rngs0 = np.stack([np.asarray(cr.PRNGKey(160 + e)) for e in range(E)])
    got = {}
    for mode in ("driver", "loop"):
        b = batched_controller(env, "mppi", cp0, E, N, 0.01)
        ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
        set_time(ep, 1, params[1].max_steps_in_episode - 2)
        if mode == "driver":
            obs = ForceObserver(env, n_inst=E).attach(b)
            b.reset(None, None, None)
            rngs = b.run_episode(ep, rngs0.copy(), 2)
            rngs = b.run_episode(ep, rngs, n - 2)
            e = ep.read_force()
            log = np.concatenate([e["measured"], e["force_true"], e["written"]], axis=2)
            sides = e["rows"]
            flags = np.ascontiguousarray(sides[..., 0]).view(np.int32)
            assert torch.equal(obs.rows, ep.obslog[:, n - 1, 32:]) and obs.xhat.shape == (E, 13) and obs.force.shape == (E, 3)
        else:
            b.bind_episode(ep)
            b.reset(None, None, None)
            bufs = state_buffers(E)
            rngs, meas, sides = rngs0.copy(), [], []
            for t in range(n):
                k_act, k_step, nxt = [], [], []
                for i in range(E):
                    r, ka, ks, _c = cr.split(rngs[i], 4)
                    k_act.append(np.asarray(ka))
                    k_step.append(np.asarray(ks))
                    nxt.append(np.asarray(cr.split(r)[0]))
                b(None, np.stack(k_act))
                ep.step(np.stack(k_step), b.a_mean)
                z = ep.noisy[:, :16].clone()
                side = b.core.observe_force(ep.noisy, b.a_mean.reshape(-1), ep.params_c, *bufs, reset=(t == 0), u_stride=128,
                                            **obs_consts(env.default_params))
                meas.append(torch.cat([z, ep.noisy[:, :16]], dim=1).cpu().numpy())
                sides.append(side.cpu().numpy())
                rngs = np.stack(nxt)
            log, sides = np.stack(meas, axis=1), np.stack(sides, axis=1)
        torch.cuda.synchronize()
        got[mode] = (ep.read_log().copy(), ep.true.cpu().numpy().copy(), ep.noisy.cpu().numpy().copy(), b.a_mean.cpu().numpy().copy(),
                     np.asarray(rngs, dtype=np.uint32).copy(), np.ascontiguousarray(log), np.ascontiguousarray(sides))
        assert b.core.device_status() == 0
        b.core.close()
    for k, (x, y) in enumerate(zip(got["driver"], got["loop"])):
        assert x.tobytes() == y.tobytes(), k
    done = got["driver"][0][:, :, 3]
    assert done[0].sum() == 0 and done[1].sum() >= 1 and done[1, 0] == 0
    assert flags[:, 0].tolist() == [1, 1] and np.array_equal(flags[:, 1:], (2 * done[:, 1:]).astype(np.int32)), (flags, done)


# ---- 7. the host path, the refusals of a second filter ----------------------------------------------------------------------------
def test_host_call_plans_from_the_written_row_and_detach_restores_the_controller():
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    N = 256
    a, _ = cm.envs.get_controller(env, "mppi", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    b, _ = cm.envs.get_controller(env, "mppi", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    obs_ = ForceObserver(env).attach(a)
    obs, info, state = env.reset(cr.PRNGKey(5), params)
    cpa = a.reset(state, params, a.init_control_params, cr.PRNGKey(6))
    cpb = b.reset(state, params, b.init_control_params, cr.PRNGKey(6))
    bufs, pc, key = state_buffers(1), b._params_c(params), cr.PRNGKey(7)
    for t in range(4):
        key, k_act, k_step = cr.split(key, 3)
        if t == 3:
            obs_.detach()
        ds = info["noisy_state"].to_device(DEV)
        row = ds.packed.clone()
        if t < 3:
            side = b.core.observe_force(row, cpb.a_mean.reshape(-1)[:4].contiguous(), pc, *bufs, reset=(t == 0), **obs_consts(params))
        ua, cpa, ia = a(obs, state, params, k_act, cpa, info)
        ub, cpb, ib = b(obs, state, params, k_act, cpb, {"noisy_state": dataclasses.replace(ds, packed=row)})
        torch.cuda.synchronize()
        assert torch.equal(ua, ub) and torch.equal(cpa.a_mean, cpb.a_mean) and torch.equal(a.core.cost, b.core.cost), t
        if t < 3:
            assert torch.equal(ia["obs_rows"], side[0]) and int(ia["obs_flags"]) == (1 if t == 0 else 0), t
            assert torch.equal(ia["obs_nis"], side[0, 1]) and torch.equal(ia["obs_force"], bufs[0][0, 13:16]) and "obs_rows" not in ib
            assert not torch.equal(row, ds.packed) and torch.equal(row[16:], ds.packed[16:])
            assert torch.equal(info["noisy_state"].to_device(DEV).packed, ds.packed)  # (the caller's state is copied, not written)
        else:
            assert "obs_rows" not in ia and torch.equal(row, ds.packed)
        obs, state, _, _, info = env.step(k_step, state, ua.cpu().numpy(), params)
    with pytest.raises(RuntimeError, match="not attached"):
        obs_.rows
    assert a.core.device_status() == 0
    a.core.close()
    b.core.close()


def test_two_filters_on_one_handle_are_refused_both_ways():
    env = quad_env(task="hovering")
    c, _ = cm.envs.get_controller(env, "mppi", "N256_H32_lam0.01", device=DEV, compute_info=False)
    est = StateEstimator(env).attach(c)
    with pytest.raises(ValueError, match="StateEstimator"):
        ForceObserver(env).attach(c)
    x = state_buffers(1)
    rows = torch.zeros((1, 8), **f32)
    o4, p4 = (C.c_double * 4)(*OBS), (C.c_double * 4)(0, 0, 0, 0)
    assert c.core.lib.covo_set_step_force_observer(c.core.h, o4, p4, 0.05, 0.1, _lib.ptr(x[0]), _lib.ptr(x[1]), _lib.ptr(x[2]),
                                                   _lib.ptr(rows), 1) == E_BADARG
    assert b"a state estimator is attached" in c.core.lib.covo_last_error()
    est.detach()
    obs = ForceObserver(env).attach(c)
    with pytest.raises(_lib.CovoError, match="a force observer is attached"):
        StateEstimator(env).attach(c)
    # the other refusals of the entry, each before any launch and by name
    for kw, msg in ((dict(obs=(0.1, 0.0, 0.1, 0.1)), b"obs_std[1]"), (dict(proc=(0.0, 0.0, -1.0, 0.0)), b"proc_std[2]"),
                    (dict(walk=float("nan")), b"force_walk_std"), (dict(init=-0.1), b"force_init_std"), (dict(n=65), b"n_inst=65")):
        rc = c.core.lib.covo_set_step_force_observer(c.core.h, (C.c_double * 4)(*kw.get("obs", OBS)), (C.c_double * 4)(*kw.get("proc", (0,) * 4)),
                                                     kw.get("walk", 0.05), kw.get("init", 0.1), _lib.ptr(x[0]), _lib.ptr(x[1]),
                                                     _lib.ptr(x[2]), _lib.ptr(rows), kw.get("n", 1))
        assert rc == E_BADARG and msg in c.core.lib.covo_last_error(), (kw, c.core.lib.covo_last_error())
    # a log shorter than the segment
    ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(1), env.default_params, (c.core.lib, c.core.h), DEV)
    cp = c.reset(ep.state0, env.default_params, c.init_control_params, cr.PRNGKey(2))
    log = torch.zeros((2, 40), **f32)
    real = c.core.attach_force_observer_log
    c.core.attach_force_observer_log = lambda episode, rows_left: _lib.check(
        c.core.lib.covo_set_episode_force_observer_log(c.core.h, _lib.ptr(log), 2), "covo_set_episode_force_observer_log")
    with pytest.raises(_lib.CovoError, match="episode force observer log rows"):
        c.run_episode(ep, env.default_params, cp, cr.PRNGKey(3), 3)
    c.core.attach_force_observer_log = real
    obs.detach()
    c.core.close()


# ---- 8. it observes ---------------------------------------------------------------------------------------------------------------
def test_it_observes_a_held_force_in_closed_loop():
    """A 120-step device episode under MPPI at N = 1 024, hovering, the periodic disturbance (0.2 N, held 50 steps), noisy states on,
    fixed seed: from step 20 the RMS of force_est[t] - force_true[t + 1] over the RMS of force_true is below 1.5 x the CPU open-loop
    ratio (FO.OPEN_LOOP_PERIODIC_RATIO, tests/test_force_observer_oracle.py) and below 1."""
    n = 120
    env = quad_env(task="hovering", disturb="periodic")
    params = env.default_params
    c, _ = cm.envs.get_controller(env, "mppi", "N1024_H32_lam0.01", device=DEV, compute_info=False)
    c.alias_outputs = True
    ForceObserver(env).attach(c)
    ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(11), params, (c.core.lib, c.core.h), DEV)
    cp = c.reset(ep.state0, params, c.init_control_params, cr.PRNGKey(12))
    cp, rng = c.run_episode(ep, params, cp, cr.PRNGKey(13), n)
    e = ep.read_force()
    flags = np.ascontiguousarray(e["rows"][:, 0]).view(np.int32)
    assert ep.read_log()[:, 3].sum() == 0 and flags.tolist() == [1] + [0] * (n - 1)
    ft, fe = e["force_true"].astype(np.float64), e["force_est"].astype(np.float64)
    rms = lambda a: float(np.sqrt((a ** 2).sum(axis=1).mean()))
    ratio = rms(fe[20:n - 1] - ft[21:n]) / rms(ft[21:n])
    print(f"  rms |f^_t - f_t+1| / rms |f_t+1| = {ratio:.3f} (rms force {rms(ft[21:n]):.3f} N; CPU open loop "
          f"{FO.OPEN_LOOP_PERIODIC_RATIO:g}); mean nis {e['rows'][20:, 1].mean():.2f} (nominal 13)")
    assert ratio < 1.5 * FO.OPEN_LOOP_PERIODIC_RATIO and ratio < 1.0, ratio
    assert c.core.device_status() == 0
    c.core.close()
