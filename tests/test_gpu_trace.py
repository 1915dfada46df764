"""GPU tests (-m gpu) of the flight recorder (covo_set_step_plan / covo_set_episode_trace; `compute_plan`, read_trace(), render_env):
per control step the plan -- the rollout of the new mean itself with the step's own inputs (csrc/plan_trace.hip) -- and, inside the
episode drivers, the trace row {true state, noisy state, u, plan}.

Bars.  cost_plan against covo_rollout_cost on the same single action sequence: none (the same device functions).  Against the fp64
oracle: |pos_plan - poses| < 2e-5 and the cost within 1e-5 relative (|x - ref| / max(|ref|, 1)), the bars pos_mean and the rollout
cost are held to (tests/test_gpu_parity.py).  Trace rows against the hand-stepped episode: none.  err_pos of a trace row
against the env log: 2e-5, what the env tests allow a log row.
"""
import dataclasses
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.dynamics.dataclass import as_device_state  # noqa: E402
from tests.gpu_cases import check_plan_against_oracle  # noqa: E402
from tests.gpu_support import DEV, H, batched_controller, build_with_discount, quad_env, start_episode, step_inputs  # noqa: E402


PLAN_CASES = [
    # name, N, disturbance, task (reward: tracking_slow = realworld), rollover, discount
    ("mppi", 1024, "gaussian", "tracking_zigzag", False, 1.0),
    ("mppi", 1024, "none", "tracking_zigzag", True, 0.9),
    ("mppi", 65536, "periodic", "tracking_zigzag", False, 1.0),
    ("mppi", 1024, "drag", "tracking_slow", True, 0.9),
    ("covo-offline", 1024, "gaussian", "tracking_zigzag", True, 1.0),
    ("covo-offline", 65536, "drag", "tracking_zigzag", False, 0.9),
    ("covo-offline", 1024, "periodic", "tracking_slow", False, 1.0),
    ("covo-online", 1024, "none", "tracking_zigzag", False, 0.9),
    ("covo-online", 65536, "gaussian", "tracking_zigzag", True, 1.0),
    ("covo-online", 1024, "periodic", "tracking_zigzag", True, 1.0),
    ("covo-online", 65536, "drag", "tracking_slow", False, 0.9),
]


@pytest.mark.parametrize("name,N,disturb,task,rollover,discount", PLAN_CASES)
def test_plan_cost_is_the_rollout_kernels(name, N, disturb, task, rollover, discount):
    """After each of three closed-loop steps: cost_plan == covo_rollout_cost(N = 1, a = clip(a_mean_new), the step's f_disturb_shared /
    f_disturb_steps)[0], bit for bit."""
    from covo_mpc_amd.controllers._core import SamplingCore
    env = quad_env(task=task, rollover=rollover, disturb=disturb)
    c, cp = build_with_discount(env, name, N, discount=discount)
    cp, obs, info, state, params = start_episode(env, c, cp, name)
    core1 = SamplingCore(1, H, 0.01, discount, device=DEV, compute_info=False)
    key = cr.PRNGKey(3)
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        dstate = as_device_state(info["noisy_state"], DEV)
        u, cp, cinfo = c(obs, state, params, k_act, cp, info)
        assert tuple(cinfo["pos_plan"].shape) == (H, 3) and cinfo["cost_plan"].dim() == 0
        assert cinfo["cost_plan"].data_ptr() == c.core.plan.data_ptr()  # views: no copy, no sync
        f_shared, tab = step_inputs(env, c, name, params, k_act, dstate, core1)
        core1.a.copy_(cp.a_mean.clamp(-1.0, 1.0).view(H, 1, 4))
        ref = core1.rollout(dstate, c._params_c(params), f_shared, False, f_steps=tab)
        torch.cuda.synchronize()
        row = c.core.plan[0].cpu().numpy()
        print(f"  {name} N={N} {disturb} {task} roll={rollover} disc={discount} step {step}: cost_plan {row[0]!r} rollout {float(ref[0])!r}")
        assert row[0] == ref.cpu().numpy()[0], (name, N, disturb, task, rollover, discount, step, row[0], float(ref[0]))
        assert row[1] == row[2] == row[3] == 0.0 and np.all(np.isfinite(row))
        obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
    assert c.core.device_status() == 0
    c.core.close()
    core1.close()


@pytest.mark.parametrize("name,N,time0", [("covo-online", 1024, None), ("covo-offline", 1024, None), ("mppi", 1024, None),
                                          ("covo-online", 65536, 290), ("mppi", 65536, 290)])
def test_plan_against_the_fp64_oracle(name, N, time0):
    """oracle.c_oracle.rollout in fp64 on clip(a_mean_new) from the same noisy state with the same shared vector: positions within
    2e-5, cost within 1e-5 relative.  time0 = 290: the plan terminates inside the horizon (time >= 300 from rollout step 10), so
    the reward freeze is exercised while the positions keep integrating."""
    env = quad_env(task="tracking_zigzag")
    c, cp = build_with_discount(env, name, N)
    cp, obs, info, state, params = start_episode(env, c, cp, name)
    key = cr.PRNGKey(7)
    for step in range(2):
        key, k_act, k_step = cr.split(key, 3)
        ns = info["noisy_state"]
        if time0 is not None:
            ns = ns.replace(time=time0 + step)
            info = dict(info, noisy_state=ns)
        u, cp, cinfo = c(obs, state, params, k_act, cp, info)
        torch.cuda.synchronize()
        rew, poses = check_plan_against_oracle(env, name, params, ns, k_act, cp, cinfo, f"{name} N={N} time0={time0} step {step}")
        if time0 is not None:
            assert rew[0, -1] == rew[0, -2] and not np.array_equal(poses[-1, 0], poses[-2, 0])  # frozen rewards, moving positions
        obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
    c.core.close()


@pytest.mark.parametrize("name,N,diag", [("mppi", 1024, False), ("covo-offline", 1024, True), ("covo-online", 2048, True),
                                         ("covo-online", 65536, False)])
@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_nothing_else_moves(name, N, diag, graph, monkeypatch):
    """Two controllers on the same inputs, one with compute_plan (both with diagnostics in the `diag` pairs): u, a_mean, a_cov, the
    actions, the costs and the diagnostics are torch.equal over 10 closed-loop steps."""
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    ca, cpa = build_with_discount(env, name, N, plan=True, diag=diag)
    cb, cpb = build_with_discount(env, name, N, plan=False, diag=diag)
    cpa, obs, info, state, params = start_episode(env, ca, cpa, name)
    if name == "covo-offline":
        cpb = cpb.replace(a_cov_offline=cpa.a_cov_offline, a_chol_offline=cpa.a_chol_offline)
    key = cr.PRNGKey(11)
    for step in range(10):
        key, k_act, k_step = cr.split(key, 3)
        ua, cpa, ia = ca(obs, state, params, k_act, cpa, info)
        ub, cpb, ib = cb(obs, state, params, k_act, cpb, info)
        torch.cuda.synchronize()
        where = (name, N, graph, step)
        assert "pos_plan" in ia and "pos_plan" not in ib and "cost_plan" not in ib
        assert torch.equal(cpa.a_mean, cpb.a_mean) and torch.equal(ua, ub), where
        assert torch.equal(ca.core.a, cb.core.a) and torch.equal(ca.core.cost, cb.core.cost), where
        assert torch.equal(cpa.a_cov, cpb.a_cov), where
        if diag:
            assert torch.equal(ca.core.diag, cb.core.diag), where
        obs, state, _, _, info = env.step(k_step, state, ua.cpu().numpy(), params)
    assert ca.core.device_status() == 0
    ca.core.close()
    cb.core.close()


@pytest.mark.parametrize("name", ["covo-online", "mppi", "covo-offline"])
def test_trace_rows_are_the_episode(name):
    """run_episode for 24 steps with the trace against the same controller stepped by hand (the loop of
    test_run_episode_equals_python_loop) copying ep.true, ep.noisy and u before every env step."""
    import covo_mpc_amd as cm
    env = quad_env(task="hovering" if name == "mppi" else "tracking_zigzag")
    params = env.default_params
    n = 24
    got = {}
    for fused in (False, True):
        controller, _ = cm.envs.get_controller(env, name, "N2048_H32_lam0.01", device=DEV, compute_info=False, compute_plan=True)
        controller.alias_outputs = True
        core = controller.core
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (core.lib, core.h), DEV)
        cp = controller.reset(ep.state0, params, controller.init_control_params, cr.PRNGKey(42))
        rng = cr.PRNGKey(43)
        if fused:
            cp, rng = controller.run_episode(ep, params, cp, rng, n)
            got["trace"] = ep.read_trace()
            got["log"] = ep.read_log()
        else:
            rows = dict(state=[], noisy=[], u=[], cost_plan=[], pos_plan=[])
            for _ in range(n):
                rng, rng_act, rng_step, rng_control = cr.split(rng, 4)
                u, cp, cinfo = controller(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                rows["state"].append(ep.true.clone())
                rows["noisy"].append(ep.noisy.clone())
                rows["u"].append(u.clone())
                rows["cost_plan"].append(cinfo["cost_plan"].clone())
                rows["pos_plan"].append(cinfo["pos_plan"].clone())
                ep.step(rng_step, u)
                rng, rng_control = cr.split(rng)
            with pytest.raises(RuntimeError):
                ep.read_trace()  # no run_episode segment: no trace
            got["hand"] = {k: torch.stack(v).cpu().numpy() for k, v in rows.items()}
            got["hand_log"] = ep.read_log()
        core.close()
    tr, hand = got["trace"], got["hand"]
    assert tr["state"].shape == (n, 32) and tr["noisy"].shape == (n, 32) and tr["u"].shape == (n, 4)
    assert tr["cost_plan"].shape == (n,) and tr["pos_plan"].shape == (n, H, 3)
    for k in ("state", "noisy", "u", "cost_plan", "pos_plan"):
        assert tr[k].tobytes() == hand[k].tobytes(), k
    assert np.array_equal(got["log"], got["hand_log"])
    assert [int(np.ascontiguousarray(tr["state"][k, 25:26]).view(np.int32)[0]) for k in range(n)] == list(range(n))
    err = np.linalg.norm(tr["state"][:, 16:19].astype(np.float64) - tr["state"][:, 0:3].astype(np.float64), axis=1)
    print(f"  {name}: max |err_pos(trace) - err_pos(log)| {np.abs(err - got['log'][:, 1]).max():.2e}")
    assert np.abs(err - got["log"][:, 1]).max() < 2e-5


def test_trace_through_a_reset():
    """A start 5 cm inside the box with outward velocity (the scripted terminal episode of tests/test_gpu_reset.py): the row whose
    log has done = 1 holds the terminal pre-step state, the next row the reset state with time 0."""
    import covo_mpc_amd as cm
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    controller, _ = cm.envs.get_controller(env, "mppi", "N1024_H32_lam0.01", device=DEV, compute_info=False, compute_plan=True)
    controller.alias_outputs = True
    core = controller.core
    ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (core.lib, core.h), DEV)
    cp = controller.reset(ep.state0, params, controller.init_control_params, cr.PRNGKey(42))
    st = dataclasses.replace(ep.state0, pos=np.asarray([0.0, 0.0, 2.95], dtype=np.float32), vel=np.asarray([0.0, 0.0, 2.5], dtype=np.float32))
    ep.true.copy_(torch.from_numpy(st.pack()).to(DEV))
    ep.noisy.copy_(ep.true)
    controller.run_episode(ep, params, cp, cr.PRNGKey(43), 14)
    tr, log = ep.read_trace(), ep.read_log()
    assert log[:, 3].sum() == 1.0
    r = int(np.argmax(log[:, 3]))
    time = lambda k: int(np.ascontiguousarray(tr["state"][k, 25:26]).view(np.int32)[0])
    assert 0 < r < 13 and np.abs(tr["state"][r, 0:3]).max() > 3.0 and time(r) == r  # the terminal pre-step state
    assert np.abs(tr["state"][:r, 0:3]).max() <= 3.0
    assert time(r + 1) == 0 and np.abs(tr["state"][r + 1, 0:3]).max() < 1.0 and np.all(tr["state"][r + 1, 3:6] == 0.0)  # reset_env's state
    assert time(r + 2) == 1
    core.close()


@pytest.mark.parametrize("name", ["covo-online", "covo-offline", "mppi"])
def test_batched_trace_equals_single(name):
    """E = 4 domain-randomised instances, 8 closed-loop steps from one covo_run_episode_batched[_mode] call: instance e's trace rows
    (states, u, plan) and its row of controller.plan equal covo_run_episode on instance e alone, bit for bit."""
    import covo_mpc_amd as cm
    N, E, n = 1024, 4, 8
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    rngs0 = np.stack([np.asarray(cr.PRNGKey(60 + e)) for e in range(E)])
    singles, tables = [], []
    for e in range(E):
        c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV, compute_info=False, compute_plan=True)
        c.alias_outputs = True
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        cp = c.reset(se.state0, params[e], c.init_control_params, cr.PRNGKey(2))
        if name == "covo-offline":
            tables.append((cp.a_cov_offline, cp.a_chol_offline))
        c.run_episode(se, params[e], cp, rngs0[e], n)
        singles.append((se.read_trace(), se.read_log(), c.core.plan[0].cpu().numpy().copy()))
        cp0 = c.init_control_params
        c.core.close()
    b = batched_controller(env, name, cp0, E, N, 0.01, compute_plan=True)
    assert tuple(b.plan.shape) == (E, _lib.COVO_PLAN_FLOATS)
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    if name == "covo-offline":
        b.bind_episode(ep)
        b.set_tables(torch.stack([t[0] for t in tables]), torch.stack([t[1] for t in tables]))
    b.run_episode(ep, rngs0.copy(), n)
    tr, log = ep.read_trace(), ep.read_log()
    plan = b.plan.cpu().numpy()
    assert tr["state"].shape == (E, n, 32) and tr["pos_plan"].shape == (E, n, H, 3) and tr["cost_plan"].shape == (E, n)
    for e in range(E):
        assert np.array_equal(log[e], singles[e][1]), e
        for k in ("state", "noisy", "u", "cost_plan", "pos_plan"):
            assert tr[k][e].tobytes() == singles[e][0][k].tobytes(), (name, e, k)
        assert plan[e].tobytes() == singles[e][2].tobytes(), (name, e)
        assert plan[e, 0] == tr["cost_plan"][e, n - 1]
    assert b.core.device_status() == 0
    b.core.close()


def test_eval_env_batched_trace_shapes():
    import covo_mpc_amd as cm
    env = quad_env(task="tracking", randomizer=True)
    err, tr = cm.envs.quadrotor.eval_env_batched(env, 3, "N1024_H32_lam0.01", n_steps=6, device=DEV, verbose=False, trace=True)
    assert err.shape == (3,)
    assert tr["state"].shape == (3, 6, 32) and tr["noisy"].shape == (3, 6, 32) and tr["u"].shape == (3, 6, 4)
    assert tr["cost_plan"].shape == (3, 6) and tr["pos_plan"].shape == (3, 6, H, 3)
    assert np.all(np.isfinite(tr["pos_plan"])) and np.all(np.isfinite(tr["cost_plan"]))


def test_refusals():
    """A sample-sharded step with a plan attached, fewer plan rows than instances, a segment past the trace's stride: CovoError
    naming the condition, nothing launched (every output buffer keeps its fill)."""
    import ctypes as C
    import covo_mpc_amd as cm
    from covo_mpc_amd._lib import CovoError, check, ptr
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    # (a) sample-sharded single step
    c, _ = cm.envs.get_controller(env, "mppi", "N1024_H32_lam0.01", device=DEV, compute_info=False, compute_plan=True)
    core = c.core
    obs, info, state = env.reset(cr.PRNGKey(1), params)
    dstate = as_device_state(info["noisy_state"], DEV)
    cp = c.init_control_params
    args, am, _, _ = core._prepare_step(_lib.MODE_MPPI, dstate, cp.a_mean, a_cov=cp.a_cov, gamma_mean=1.0, sample_sigma=0.5,
                                        derive_keys=True, rollout_deterministic=False)
    core.partial.fill_(-7.0)
    core.cost.fill_(-7.0)
    args.partial_out = core.partial.data_ptr()
    pc = c._params_c(params)
    with pytest.raises(CovoError, match="sample-sharded"):
        check(core.lib.covo_mpc_step(core.h, C.byref(pc), C.byref(args), 1, 2, None, core.stream()), "covo_mpc_step")
    torch.cuda.synchronize()
    assert bool((core.cost == -7.0).all()) and bool((core.partial == -7.0).all())
    # (b) n_inst outside (0, COVO_MAX_ENVS]
    with pytest.raises(CovoError, match="n_inst"):
        check(core.lib.covo_set_step_plan(core.h, ptr(core.plan), 0), "covo_set_step_plan")
    with pytest.raises(CovoError, match="n_inst"):
        check(core.lib.covo_set_step_plan(core.h, ptr(core.plan), _lib.COVO_MAX_ENVS + 1), "covo_set_step_plan")
    # (c) a segment past the trace's stride
    c.alias_outputs = True
    ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (core.lib, core.h), DEV)
    cp = c.reset(ep.state0, params, cp, cr.PRNGKey(42))
    ep.alloc_log("trace")
    real_segment = ep.log_segment
    ep.log_segment = lambda name: real_segment(name)[:5] if name == "trace" else real_segment(name)
    attach = core.attach_log
    core.attach_log = lambda name, episode, rows_left: attach(name, episode, 5 if name == "trace" else rows_left)
    before = ep.true.clone()
    with pytest.raises(CovoError, match="episode trace"):
        c.run_episode(ep, params, cp, cr.PRNGKey(43), 6)
    torch.cuda.synchronize()
    assert torch.equal(ep.true, before) and bool((ep.trace == 0).all())
    core.close()
    # (d) a batched step with more instances than plan rows
    E, N = 3, 1024
    envr = quad_env(task="tracking", randomizer=True)
    c0, _ = cm.envs.get_controller(envr, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    cp0 = c0.init_control_params
    c0.core.close()
    b = batched_controller(envr, "covo-online", cp0, E, N, 0.01, compute_plan=True)
    check(b.core.lib.covo_set_step_plan(b.core.h, ptr(b.plan), 2), "covo_set_step_plan")
    ps = [envr.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    ep = cm.envs.BatchedDeviceEpisode(envr, [cr.PRNGKey(50 + e) for e in range(E)], ps, (b.core.lib, b.core.h), DEV)
    before = ep.true.clone()
    with pytest.raises(CovoError, match="plan buffer"):
        b.run_episode(ep, np.stack([np.asarray(cr.PRNGKey(60 + e)) for e in range(E)]), 2)
    torch.cuda.synchronize()
    assert torch.equal(ep.true, before)
    b.core.close()


def test_render_env_on_the_device_is_a_consistent_episode(tmp_path, monkeypatch):
    """covo-offline, N = 1 024, zigzag, gaussian through render_env's device path.  A device closed loop cannot be compared with a
    host closed loop state by state (a 1e-5 difference in the noisy state moves the softmax at lambda = 0.01), so the check is
    teacher-forced, as test_env_step_kernel_vs_host_env is: the recorded u sequence replayed through the HOST env.step with the step
    keys the driver's threading gives from the same starting key."""
    import covo_mpc_amd as cm
    from covo_mpc_amd.envs.quadrotor import render_env
    monkeypatch.chdir(tmp_path)
    env = quad_env(task="tracking_zigzag")
    controller, cp = cm.envs.get_controller(env, "covo-offline", "N1024_H32_lam0.01", device=DEV, compute_info=False, compute_plan=True)
    seq = render_env(env, controller, cp, filename="dev", save=True)
    controller.core.close()
    # the keys of render_env (quadrotor.py:599-611), then run_one_step's threading (:520-538)
    rng = cr.PRNGKey(1)
    rng, rng_params = cr.split(rng)
    params = env.sample_params(rng_params)
    rng, rng_reset = cr.split(rng)
    obs, info, state = env.reset(rng_reset, params)
    rng, rng_control = cr.split(rng)
    assert [int(e["time"]) for e in seq] == list(range(len(seq)))
    assert len(seq) == params.max_steps_in_episode + 1  # the first done is time >= 300, entering the 301st step
    worst = 0.0
    for k in range(60):
        e = seq[k]
        for f in ("pos", "vel", "quat", "omega"):
            worst = max(worst, float(np.abs(np.asarray(getattr(state, f), dtype=np.float64) - e[f]).max()))
        assert e["pos_plan"].shape == (H, 3) and e["u"].shape == (4,) and np.isfinite(e["cost_plan"]) and np.isfinite(e["reward"])
        assert np.array_equal(e["pos_traj"], state.pos_traj)
        rng, rng_act, rng_step, _ = cr.split(rng, 4)
        obs, state, reward, done, info = env.step(rng_step, state, e["u"], params)
        assert not done
        rng, _ = cr.split(rng)
    print(f"  teacher-forced replay, 60 steps: max |host - device| over pos / vel / quat / omega {worst:.2e}")
    assert worst < 2e-5
    with open(tmp_path / "results" / "state_seq_dev.pkl", "rb") as f:
        loaded = pickle.load(f)
    assert len(loaded) == len(seq)
    for a, b in zip(loaded, seq):
        assert set(a) == set(b)
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
