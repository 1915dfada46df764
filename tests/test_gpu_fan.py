"""GPU tests (-m gpu) of the sample fan (covo_rollout_fan / covo_set_step_fan / covo_set_episode_fan; `compute_fan`, read_fan()): K of
a step's N sampled rollouts as rows {cost_s, bits(n_s), 0, 0, pos_s[H][3]} (csrc/sample_fan.hip).

Bars.  fan_cost against the cost the step's own rollout left for that sample: none (the same stage functions on the same action
stripe: torch.equal).  fan_idx against the definition (clamp into [0, N), or the stride (s N) / K): none.  fan_pos against the fp64
oracle's poses[:, n_s]: 2e-5, the bar pos_plan and pos_mean are held to (tests/test_gpu_trace.py).  Batched against single,
episode log against the hand-stepped loop, a step with the fan against its twin without: none.
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
from tests.gpu_support import (DEV, DP, H, POS_BAR, batched_controller, dev_state, disturb_key, params_c, quad_env,  # noqa: E402
                               sample_actions, shared_vector, split_rows, start_episode, to_stripes, want_idx)
from tests.oracle_support import oracle_params, oracle_state  # noqa: E402

FF = _lib.COVO_FAN_FLOATS


def check_rows(rows, N, K, idx, cost_dev, poses, where):
    """The assertions of test 1 on one fan: the indices are the definition's, the costs the step's own bit for bit, the positions the
    oracle's (poses [H, N, 3] fp64) within 2e-5, words 2 and 3 zero.  -> the indices."""
    cost, n, pad, pos = split_rows(rows)
    assert rows.shape == (K, FF), where
    assert np.array_equal(n, want_idx(N, K, idx)), (where, n)
    assert torch.equal(rows[:, 0], cost_dev[torch.from_numpy(n.astype(np.int64)).to(cost_dev.device)]), (where, cost, cost_dev.cpu().numpy()[n])
    assert np.all(pad == 0.0), where
    dpos = np.abs(pos - np.transpose(poses[:, n], (1, 0, 2))).max()
    print(f"  {where}: |fan_pos - poses| {dpos:.2e}")
    assert dpos < POS_BAR, (where, dpos)
    return n


# ------------------------------------------------------------------------------------------ 1: the stand-alone entry
@pytest.mark.parametrize("N", [197, 64])
@pytest.mark.parametrize("kind,box", [("none", False), ("gaussian", False), ("periodic", False), ("drag", False), ("none", True)])
def test_rollout_fan_vs_oracle(kind, box, N):
    """covo_rollout_cost, then covo_rollout_fan on the same `a`: N = 197 (ragged last group) and 64; K in {1, 8, 64} with idx = None
    and one explicit idx holding 0, N - 1, a duplicate, one value < 0 and one >= N; both rewards, rollover on and off, discount 1
    and 0.9; NONE, GAUSSIAN with a non-zero shared vector, PERIODIC and DRAG tables.  box: the state sits 3 cm inside the 3 m box
    with 2.5 m/s outward, so every sample terminates after rollout step 0 -- frozen rewards, moving positions."""
    s, p, rng = make_problem(seed=17, time=37)  # time 37: step 13 (time 50) redraws the periodic part
    p = p.replace(disturb_params=DP)
    if box:
        f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)  # (every input is an fp32 number, as in make_problem)
        s = s.replace(pos=f32([0.1, -0.2, 2.97]), vel=f32([0.0, 0.0, 2.5]))
    a = sample_actions(p, rng, N)
    a64 = a.astype(np.float64)
    ds = dev_state(s)
    key = cr.PRNGKey(5)
    explicit = [0, N - 1, 5, 5, -3, N + 10, 17, N // 2]
    terminated = 0
    for discount in (1.0, 0.9):
        core = SamplingCore(N, H, 0.01, discount, device=DEV, compute_info=False)
        core.a.copy_(to_stripes(a))
        for reward in ("penyaw", "realworld"):
            for rollover in (False, True):
                pc = params_c(p, kind, reward, rollover=rollover)
                tab, fs = None, (0.0, 0.0, 0.0)
                if kind in ("periodic", "drag"):
                    tab = core.disturb_table(pc, ds.packed, key=key, key_mode=_lib.DISTURB_KEYS_SHARED, deterministic=True)
                    draw = cr.uniform(disturb_key(key), (3,), -p.disturb_scale, p.disturb_scale).astype(np.float64)
                    _, rew, poses = CO.rollout(s, p, a64, discount, dtype=np.float64, want_rewards=True, want_poses=True,
                                               rollover=rollover, reward=reward, disturb=R.Disturb(kind, draw, True))
                else:
                    if kind == "gaussian":
                        fs = (0.02, -0.03, 0.01)
                    _, rew, poses = CO.rollout(s, p, a64, discount, np.asarray(fs, dtype=np.float64), dtype=np.float64,
                                               want_rewards=True, want_poses=True, rollover=rollover, reward=reward)
                cost = core.rollout(ds, pc, fs, False, f_steps=tab).clone()
                fans = [(K, None) for K in (1, 8, 64) if K <= N] + [(len(explicit), explicit)]
                for K, idx in fans:
                    it = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=DEV)
                    rows = core.rollout_fan(ds, pc, it, f_shared=fs, f_steps=tab, K=K)
                    torch.cuda.synchronize()
                    where = f"{kind} box={box} N={N} disc={discount} {reward} roll={rollover} K={K} idx={'given' if idx else 'stride'}"
                    n = check_rows(rows, N, K, idx, cost, poses, where)
                    if box:
                        # the sample left the box mid-horizon: its rewards freeze (its cost is the step's, asserted above) while
                        # its positions keep moving
                        out = [int(m) for m in n if np.abs(poses[:H - 2, m]).max() > 3.0 and rew[m, -1] == rew[m, -2]]
                        pos = split_rows(rows)[3]
                        for j, m in enumerate(n):
                            if int(m) in out:
                                assert not np.array_equal(pos[j, -1], pos[j, -2]), where
                        terminated += len(out)
        assert core.device_status() == 0
        core.close()
    if box:
        assert terminated > 0, "no fan sample terminated inside the horizon: the case is vacuous"


# ------------------------------------------------------------------------------------------ 2: behind every step path
def _controller(env, name, N, fan, extras):
    import covo_mpc_amd as cm
    c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV, compute_info=False, compute_diag=extras,
                                  compute_plan=extras, ess_min=32.0 if extras else None, compute_fan=fan)
    return c, c.init_control_params


@pytest.mark.parametrize("extras", [False, True], ids=["fan", "fan+plan+diag+ess"])
@pytest.mark.parametrize("graph", ["graph", "eager"])
@pytest.mark.parametrize("name,N", [("mppi", 256), ("covo-offline", 256), ("covo-online", 256), ("covo-online", 1024)])
def test_step_fan_on_every_path(name, N, graph, extras, monkeypatch):
    """MPPI and covo-offline at N = 256 (the one-launch step; with the ESS floor the staged one), covo-online at 256 and 1 024; graph
    replay and COVO_FLAG_NO_GRAPH, shared_device; with and without plan, diagnostics and ESS floor attached as well.  Two steps:
    after each the fan against the oracle on the controller's own `a` (as test 1), and every other output torch.equal to a twin
    without the fan on the same keys (u, a_mean, a_cov, cost, the action buffer -- i.e. the derived sampling key --, diag, plan and
    lam_eff rows)."""
    K = 8
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    monkeypatch.setenv("COVO_SHARED_DEVICE", "1")
    env = quad_env(task="tracking_zigzag")
    ca, cpa = _controller(env, name, N, K, extras)
    cb, cpb = _controller(env, name, N, None, extras)
    assert ca.core.shared_device and ca.core.uses_graph == (graph == "graph")
    cpa, obs, info, state, params = start_episode(env, ca, cpa, name)
    if name == "covo-offline":
        cpb = cpb.replace(a_cov_offline=cpa.a_cov_offline, a_chol_offline=cpa.a_chol_offline)
    key = cr.PRNGKey(11)
    for step in range(2):
        key, k_act, k_step = cr.split(key, 3)
        ns = info["noisy_state"]
        ua, cpa, ia = ca(obs, state, params, k_act, cpa, info)
        ub, cpb, ib = cb(obs, state, params, k_act, cpb, info)
        torch.cuda.synchronize()
        where = f"{name} N={N} {graph} extras={extras} step {step}"
        assert tuple(ia["fan_pos"].shape) == (K, H, 3) and tuple(ia["fan_cost"].shape) == (K,) and ia["fan_idx"].dtype == torch.int32
        assert ia["fan_cost"].data_ptr() == ca.core.fan.data_ptr()  # views: no copy, no sync
        assert not any(k.startswith("fan_") for k in ib)
        assert torch.equal(ia["fan_idx"].cpu(), ca.core.fan_idx[0].cpu()), where
        a64 = ca.core.a.permute(1, 0, 2).contiguous().cpu().numpy().astype(np.float64)
        _, poses = CO.rollout(oracle_state(ns), R.Params().fp32(), a64, 1.0, shared_vector(env, name, params, k_act),
                              dtype=np.float64, want_poses=True)
        check_rows(ca.core.fan[0], N, K, None, ca.core.cost, poses, where)
        assert torch.equal(ua, ub) and torch.equal(cpa.a_mean, cpb.a_mean) and torch.equal(cpa.a_cov, cpb.a_cov), where
        assert torch.equal(ca.core.cost, cb.core.cost) and torch.equal(ca.core.a, cb.core.a), where
        if extras:
            assert torch.equal(ca.core.diag, cb.core.diag) and torch.equal(ca.core.plan, cb.core.plan), where
            assert torch.equal(ca.core.lam_eff, cb.core.lam_eff), where
        obs, state, _, _, info = env.step(k_step, state, ua.cpu().numpy(), params)
    assert ca.core.device_status() == 0
    ca.core.close()
    cb.core.close()


# ------------------------------------------------------------------------------------------ 3: the env-batched controllers
@pytest.mark.parametrize("name", ["covo-online", "covo-offline", "mppi"])
def test_batched_fan_equals_single(name):
    """E = 2 domain-randomised instances, N = 256, K = 8, one step from a BatchedDeviceEpisode's states: controller.fan[e] equals the
    single controller's fan on instance e alone bit for bit, and instance 1's fan is the oracle's as in test 1."""
    import covo_mpc_amd as cm
    N, E, K = 256, 2, 8
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    act_keys = np.stack([np.asarray(cr.PRNGKey(60 + e)) for e in range(E)])
    singles, tables = [], []
    for e in range(E):
        c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV, compute_info=False, compute_fan=K)
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        cp = c.reset(se.state0, params[e], c.init_control_params, cr.PRNGKey(2))
        if name == "covo-offline":
            tables.append((cp.a_cov_offline, cp.a_chol_offline))
        c(None, None, params[e], act_keys[e], cp, {"noisy_state": se.noisy_state})
        torch.cuda.synchronize()
        singles.append(c.core.fan[0].clone())
        cp0 = c.init_control_params
        c.core.close()
    b = batched_controller(env, name, cp0, E, N, 0.01, compute_fan=K)
    assert tuple(b.fan.shape) == (E, K, FF) and tuple(b.core.fan_idx.shape) == (E, K)
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    b.bind_episode(ep)
    if name == "covo-offline":
        b.set_tables(torch.stack([t[0] for t in tables]), torch.stack([t[1] for t in tables]))
    b(None, act_keys)
    torch.cuda.synchronize()
    for e in range(E):
        assert torch.equal(b.fan[e], singles[e]), (name, e)
    e = 1
    s0 = ep.states0[e]
    row = ep.noisy[e].cpu().numpy()
    so = R.State(pos=row[0:3], vel=row[3:6], quat=row[6:10], omega=row[10:13], f_disturb=row[13:16], pos_tar=row[16:19],
                 vel_tar=row[19:22], acc_tar=row[22:25], time=int(row[25:26].view(np.int32)[0]), pos_traj=s0.pos_traj,
                 vel_traj=s0.vel_traj, acc_traj=s0.acc_traj).astype(np.float64)
    a64 = b._a[e].permute(1, 0, 2).contiguous().cpu().numpy().astype(np.float64)
    _, poses = CO.rollout(so, oracle_params(params[e]), a64, 1.0, shared_vector(env, name, params[e], act_keys[e]),
                          dtype=np.float64, want_poses=True)
    check_rows(b.fan[e], N, K, None, b._cost[e], poses, f"batched {name} instance {e}")
    assert b.core.device_status() == 0
    b.core.close()


# ------------------------------------------------------------------------------------------ 4: the episode log
def _episode_fan_log_single():
    """run_episode for 6 steps in two segments (4 + 2): read_fan() row k is what a Python loop of __call__ + env step collects, rows
    beyond n_steps stay untouched, and the env log and the trace are those of the same episode without the fan."""
    import covo_mpc_amd as cm
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    K, N, name = 8, 256, "mppi"
    got = {}
    for mode in ("fused", "hand", "nofan"):
        controller, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV, compute_info=False, compute_plan=True,
                                               compute_fan=None if mode == "nofan" else K)
        controller.alias_outputs = True
        core = controller.core
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (core.lib, core.h), DEV)
        cp = controller.reset(ep.state0, params, controller.init_control_params, cr.PRNGKey(42))
        rng = cr.PRNGKey(43)
        if mode == "hand":
            rows = []
            for _ in range(6):
                rng, rng_act, rng_step, _c = cr.split(rng, 4)
                u, cp, cinfo = controller(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                rows.append(core.fan[0].clone())
                ep.step(rng_step, u)
                rng, _c = cr.split(rng)
            with pytest.raises(RuntimeError):
                ep.read_fan()  # no run_episode segment: no fan log
            got["hand"] = torch.stack(rows).cpu().numpy()
        else:
            cp, rng = controller.run_episode(ep, params, cp, rng, 4)
            cp, rng = controller.run_episode(ep, params, cp, rng, 2)
            got[mode] = (ep.read_log(), ep.read_trace())
            if mode == "fused":
                got["fan"] = ep.read_fan()
                got["raw"] = ep.fanlog.cpu().numpy()
        core.close()
    fan, hand = got["fan"], got["hand"]
    assert fan["pos"].shape == (6, K, H, 3) and fan["cost"].shape == (6, K) and fan["idx"].shape == (6, K) and fan["idx"].dtype == np.int32
    assert got["raw"][:6].tobytes() == hand.tobytes()
    assert np.all(got["raw"][6:] == 0.0)
    assert np.array_equal(fan["idx"], np.broadcast_to(want_idx(N, K), (6, K)))
    assert np.array_equal(got["fused"][0], got["nofan"][0])
    for k in got["fused"][1]:
        assert got["fused"][1][k].tobytes() == got["nofan"][1][k].tobytes(), k


def _episode_fan_log_batched(name):
    """The same for E = 2 instances through covo_run_episode_batched[_mode]."""
    import covo_mpc_amd as cm
    N, E, K = 256, 2, 8
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    rngs0 = np.stack([np.asarray(cr.PRNGKey(60 + e)) for e in range(E)])
    c0, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    cp0 = c0.init_control_params
    c0.core.close()
    got = {}
    for mode in ("fused", "hand", "nofan"):
        b = batched_controller(env, name, cp0, E, N, 0.01, compute_plan=True, compute_fan=None if mode == "nofan" else K)
        ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
        if mode == "hand":
            b.bind_episode(ep)
            rngs = [rngs0[e] for e in range(E)]
            rows = []
            for _ in range(6):
                sp = [cr.split(r, 4) for r in rngs]
                b(None, np.stack([np.asarray(x[1]) for x in sp]))
                rows.append(b.fan.clone())
                ep.step(np.stack([np.asarray(x[2]) for x in sp]), b.a_mean)
                rngs = [cr.split(x[0])[0] for x in sp]
            got["hand"] = torch.stack(rows, dim=1).cpu().numpy()  # [E, 6, K, 100]
        else:
            keys = b.run_episode(ep, rngs0.copy(), 4)
            b.run_episode(ep, keys, 2)
            got[mode] = (ep.read_log(), ep.read_trace())
            if mode == "fused":
                got["fan"] = ep.read_fan()
                got["raw"] = ep.fanlog.cpu().numpy()
        assert b.core.device_status() == 0
        b.core.close()
    fan = got["fan"]
    assert fan["pos"].shape == (E, 6, K, H, 3) and fan["cost"].shape == (E, 6, K) and fan["idx"].shape == (E, 6, K)
    assert np.ascontiguousarray(got["raw"][:, :6]).tobytes() == got["hand"].tobytes()
    assert np.all(got["raw"][:, 6:] == 0.0)
    assert np.array_equal(got["fused"][0], got["nofan"][0])
    for k in got["fused"][1]:
        assert got["fused"][1][k].tobytes() == got["nofan"][1][k].tobytes(), k


@pytest.mark.parametrize("which", ["single", "batched-covo-online", "batched-mppi"])
def test_episode_fan_log(which):
    """Single (covo_run_episode) and batched, E = 2 (covo_run_episode_batched / _mode)."""
    if which == "single":
        _episode_fan_log_single()
    else:
        _episode_fan_log_batched(which[len("batched-"):])


def test_eval_env_batched_fan_shapes():
    import covo_mpc_amd as cm
    env = quad_env(task="tracking", randomizer=True)
    err, fan = cm.envs.quadrotor.eval_env_batched(env, 2, "N256_H32_lam0.01", n_steps=3, device=DEV, verbose=False, fan=4)
    assert err.shape == (2,) and fan["pos"].shape == (2, 3, 4, H, 3) and fan["cost"].shape == (2, 3, 4) and fan["idx"].shape == (2, 3, 4)
    assert np.all(np.isfinite(fan["pos"])) and np.all(np.isfinite(fan["cost"]))


def test_render_env_carries_the_fan(tmp_path, monkeypatch):
    """--mode render --fan 16 (the CLI's main): every entry of the pickled state sequence carries fan_pos (16, 32, 3)."""
    import pickle
    from covo_mpc_amd.envs import quadrotor as q
    monkeypatch.chdir(tmp_path)
    seq = q.main(q.Args(mode="render", controller="mppi", controller_params="N256_H32_lam0.01", task="tracking_zigzag", noDR=True,
                        name="fan", fan=16))
    with open(tmp_path / "results" / "state_seq_fan.pkl", "rb") as f:
        loaded = pickle.load(f)
    assert len(loaded) == len(seq) > 0
    for e in loaded:
        assert e["fan_pos"].shape == (16, H, 3) and e["fan_cost"].shape == (16,) and e["fan_idx"].shape == (16,)
        assert e["fan_idx"].dtype == np.int32 and np.array_equal(e["fan_idx"], want_idx(256, 16))
        assert np.all(np.isfinite(e["fan_pos"])) and e["pos_plan"].shape == (H, 3)


# ------------------------------------------------------------------------------------------ 5: refusals
def test_fan_refusals_leave_the_handle_usable():
    """Every refusal at the C boundary, matched on its message, nothing launched; afterwards the status is clean and a normal step
    is finite."""
    import covo_mpc_amd as cm
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    N, K = 256, 8
    c, _ = cm.envs.get_controller(env, "mppi", f"N{N}_H32_lam0.01", device=DEV, compute_info=False, compute_fan=K)
    core = c.core
    lib, h = core.lib, core.h
    obs, info, state = env.reset(cr.PRNGKey(1), params)
    dstate = as_device_state(info["noisy_state"], DEV)
    cp = c.init_control_params
    pc = c._params_c(params)
    big = torch.zeros((2, 64, FF), dtype=torch.float32, device=DEV)
    # (a) K outside [1, 64]
    for bad in (0, 65, -1):
        with pytest.raises(CovoError, match=r"outside \[1, 64\]"):
            check(lib.covo_set_step_fan(h, ptr(big), None, bad, 1), "covo_set_step_fan")
        with pytest.raises(CovoError, match=r"outside \[1, 64\]"):
            check(lib.covo_rollout_fan(h, ptr(dstate.packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj), dstate.T, C.byref(pc), None,
                                       None, ptr(core.a), N, None, bad, ptr(big), core.stream()), "covo_rollout_fan")
    # (b) K > n_samples: at the stand-alone entry, at attach time (a handle of 32 samples) and at step time (a 32-sample step)
    with pytest.raises(CovoError, match="K=64 > n_samples=32"):
        check(lib.covo_rollout_fan(h, ptr(dstate.packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj), dstate.T, C.byref(pc), None,
                                   None, ptr(core.a), 32, None, 64, ptr(big), core.stream()), "covo_rollout_fan")
    small = SamplingCore(32, H, 0.01, 1.0, device=DEV, compute_info=False)
    with pytest.raises(CovoError, match="K=64 > n_samples"):
        check(small.lib.covo_set_step_fan(small.h, ptr(big), None, 64, 1), "covo_set_step_fan")
    small.close()
    args, am, _, _ = core._prepare_step(_lib.MODE_MPPI, dstate, cp.a_mean, a_cov=cp.a_cov, gamma_mean=1.0, sample_sigma=0.5,
                                        derive_keys=True, rollout_deterministic=False)
    core.cost.fill_(-7.0)
    core.fan.fill_(-7.0)
    check(lib.covo_set_step_fan(h, ptr(big), None, 64, 1), "covo_set_step_fan")
    args.n_samples = 32
    with pytest.raises(CovoError, match="K=64 > n_samples=32"):
        check(lib.covo_mpc_step(h, C.byref(pc), C.byref(args), 1, 2, None, core.stream()), "covo_mpc_step")
    args.n_samples = N
    check(lib.covo_set_step_fan(h, ptr(core.fan), ptr(core.fan_idx), K, 1), "covo_set_step_fan")
    # (c) a sample-sharded step
    core.partial.fill_(-7.0)
    args.partial_out = core.partial.data_ptr()
    with pytest.raises(CovoError, match="sample fan.*sample-sharded"):
        check(lib.covo_mpc_step(h, C.byref(pc), C.byref(args), 1, 2, None, core.stream()), "covo_mpc_step")
    args.partial_out = None
    torch.cuda.synchronize()
    assert bool((core.cost == -7.0).all()) and bool((core.partial == -7.0).all()) and bool((core.fan == -7.0).all())
    # (d) an episode segment that would leave the log
    c.alias_outputs = True
    ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (lib, h), DEV)
    cpe = c.reset(ep.state0, params, cp, cr.PRNGKey(42))
    attach = core.attach_log
    core.attach_log = lambda name, episode, rows_left: attach(name, episode, 5 if name == "fanlog" else rows_left)
    before = ep.true.clone()
    with pytest.raises(CovoError, match="episode fan log"):
        c.run_episode(ep, params, cpe, cr.PRNGKey(43), 6)
    torch.cuda.synchronize()
    assert torch.equal(ep.true, before) and bool((ep.fanlog == 0).all())
    del core.attach_log
    check(lib.covo_set_episode_fan(h, None, 0), "covo_set_episode_fan")
    # the log needs a fan size
    fresh = SamplingCore(N, H, 0.01, 1.0, device=DEV, compute_info=False)
    with pytest.raises(CovoError, match="covo_set_step_fan"):
        check(fresh.lib.covo_set_episode_fan(fresh.h, ptr(big), 4), "covo_set_episode_fan")
    fresh.close()
    # the handle is usable: a normal step with the fan
    assert core.device_status() == 0
    u, cp2, cinfo = c(obs, state, params, cr.PRNGKey(9), cp, info)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(cinfo["fan_pos"]).all()) and bool(torch.isfinite(cinfo["fan_cost"]).all())
    assert core.device_status() == 0
    core.close()
    # (e) a batched step with more instances than n_inst
    E = 3
    envr = quad_env(task="tracking", randomizer=True)
    c0, _ = cm.envs.get_controller(envr, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False)
    cp0 = c0.init_control_params
    c0.core.close()
    for name in ("covo-online", "mppi"):
        b = batched_controller(envr, name, cp0, E, N, 0.01, compute_fan=K)
        check(b.core.lib.covo_set_step_fan(b.core.h, ptr(b.fan), ptr(b.core.fan_idx), K, 2), "covo_set_step_fan")
        ps = [envr.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
        ep = cm.envs.BatchedDeviceEpisode(envr, [cr.PRNGKey(50 + e) for e in range(E)], ps, (b.core.lib, b.core.h), DEV)
        keys = np.stack([np.asarray(cr.PRNGKey(60 + e)) for e in range(E)])
        b.bind_episode(ep)
        b._cost.fill_(-7.0)
        with pytest.raises(CovoError, match="fan buffer"):
            b(None, keys)
        before = ep.true.clone()
        with pytest.raises(CovoError, match="fan buffer"):
            b.run_episode(ep, keys, 2)
        torch.cuda.synchronize()
        assert torch.equal(ep.true, before) and bool((b._cost == -7.0).all())
        check(b.core.lib.covo_set_step_fan(b.core.h, ptr(b.fan), ptr(b.core.fan_idx), K, E), "covo_set_step_fan")
        assert b.core.device_status() == 0
        u = b(None, keys)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(b.fan).all())
        b.core.close()
