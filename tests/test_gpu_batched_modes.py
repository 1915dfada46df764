"""GPU tests (-m gpu) of the env-batched MPPI and covo-offline steps (covo_mpc_step_batched_mode, csrc/step_small.hip with the
instance as a grid dimension; controllers/batched.py: BatchedMPPIController, BatchedCoVOController(mode="offline")):
  * instance e of a batched step == the single controller on instance e alone, bit for bit (same device functions, one ticket
    and one record set per instance);
  * against oracle/ directly: per-sample costs (C fp64 rollout with the instance's own parameters, 1e-5) and the new mean
    (ref_np.softmax_update, 1e-4 unless the two best costs are closer than 1e-3 * lam / 0.01) -- the bars of
    tests/gpu_cases.py::_oracle_check_of_a_fused_step, including its cap of max(2, N // 4096) samples per call that may
    use the widened bar (1.5 x what the fp32 C oracle loses against the fp64 one on the same samples);
  * whole episodes (control step + env step on the device) against per-instance episodes;
  * refusals: argument checks that return before any launch.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from tests.gpu_cases import CASES, _mode_step_equals_replicas  # noqa: E402
from tests.gpu_support import DEV, ST_TIME, batched_controller, instances, quad_env  # noqa: E402
from tests.oracle_support import oracle_params, oracle_state, rel_err  # noqa: E402
from tests.update_oracle import check_update  # noqa: E402


@pytest.mark.parametrize("name,N,lam,rollover", CASES)
@pytest.mark.parametrize("E", [1, 5, 32])
@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_batched_mode_step_equals_replicas(name, N, lam, rollover, E, graph, monkeypatch):
    _mode_step_equals_replicas(name, N, lam, rollover, E, graph, monkeypatch)


@pytest.mark.parametrize("name", ["covo-online", "mppi"])
def test_batched_graph_caches_are_dropped_by_growth_new_buffers_and_debug_setters(name, monkeypatch):
    """The env-batched twin of tests/test_gpu_parity.py::test_workspace_growth_drops_the_captured_step_graph, for both batched graph
    caches (covo-online: covo_mpc_step_batched; MPPI: the fused launch of covo_mpc_step_batched_mode).  A graph-replaying handle and
    a COVO_FLAG_NO_GRAPH handle step the same 3 instances side by side for 8 steps; a_mean and a_cov are torch.equal after every
    step.  The graph handle captures at step 1 and then meets, each time two steps later (eager call, re-capture), every event that
    must invalidate its caches:
      after step 1: covo_sigma and covo_hessian on a larger batch (both workspaces the captured launches point into are re-allocated);
      after step 3: a new a_mean buffer (the argument block, which is the cache key, changes);
      after step 5: a covo_debug_set_* switch flipped and restored (the handle's epoch moves on)."""
    import covo_mpc_amd as cm
    N, lam, E, B = 1024, "0.01", 3, 5
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, name, N, lam, E)
    cp0 = inst[0]["cp"]

    def build():
        if name == "mppi":
            return batched_controller(env, name, inst, len(inst), N, lam, check_cov=True)
        return cm.controllers.BatchedCoVOController(env, E, N, 32, float(lam), discount=cp0.discount, gamma_mean=cp0.gamma_mean,
                                                    sample_sigma=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=DEV)
    monkeypatch.setenv("COVO_GRAPH", "1")
    bg = build()
    monkeypatch.delenv("COVO_GRAPH")
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    be = build()
    assert bg.core.uses_graph and not be.core.uses_graph
    for b in (bg, be):
        b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    rng = np.random.default_rng(1)
    for step in range(8):
        k_acts = []
        for i in inst:
            i["key"], k_act, i["k_step"] = cr.split(i["key"], 3)
            k_acts.append(np.asarray(k_act))
        noisy = [i["info"]["noisy_state"] for i in inst]
        bg(noisy, np.stack(k_acts))
        u = be(noisy, np.stack(k_acts)).clone()
        assert torch.equal(bg.a_mean, be.a_mean) and torch.equal(bg.a_cov, be.a_cov), (name, step)
        if step == 1:
            A = rng.normal(size=(B, 128, 128))
            S, L = bg.core.sigma(torch.from_numpy(0.05 * (A + np.transpose(A, (0, 2, 1)))).to(DEV), 0.5, batch=B)
            assert torch.isfinite(S).all()
            ds = noisy[0].to_device(DEV)
            Hs = bg.core.hessian(ds.packed.repeat(B), ds, bg._params[0], bg.a_mean[0].repeat(B), batch=B)
            assert torch.isfinite(Hs).all()
        if step == 3:
            bg.a_mean = bg.a_mean.clone()  # (in/out: a stale graph would go on updating the old buffer)
            bg._args = bg._make_args(bg._states_buf, *bg._traj)
        if step == 5:  # (1 is the default of a handle created without COVO_NS_MERGED in the environment)
            _lib.check(bg.core.lib.covo_debug_set_ns_merged(bg.core.h, 0), "ns_merged")
            _lib.check(bg.core.lib.covo_debug_set_ns_merged(bg.core.h, 1), "ns_merged")
        for e, i in enumerate(inst):
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u[e].cpu().numpy(), i["params"])
    assert bg.core.device_status() == 0 and be.core.device_status() == 0 and torch.isfinite(bg.a_mean).all()
    assert (bg.a_mean[0] - bg.a_mean[1]).abs().max() > 1e-4  # different plants, different plans


def _oracle_check_instance(name, env, params, ns, a_mean_before, k_act, a_dev_t, cost_dev_t, a_mean_new_t, lam, rollover=False):
    """The checks and bars of tests/gpu_cases.py::_oracle_check_of_a_fused_step for one instance of a batch, with the
    instance's own parameters.  -> how many samples used the widened bar (at most max(2, N // 4096) may)."""
    N = a_dev_t.shape[1]
    so, po = oracle_state(ns), oracle_params(params)
    am = R.shift_mean(np.asarray(a_mean_before, dtype=np.float64).reshape(32, 4))
    fs = np.zeros(3)
    if name == "mppi":  # mppi.py:69,74: one shared non-deterministic draw for every sample and step
        _, step_key = cr.split(cr.split(k_act)[0])
        fs = np.asarray(env.rollout_disturbance(step_key, params, deterministic=False), dtype=np.float64)
    a_dev = a_dev_t.permute(1, 0, 2).contiguous().cpu().numpy().astype(np.float64)
    cost_dev = cost_dev_t.cpu().numpy()
    cost_ref = CO.rollout(so, po, a_dev, 1.0, fs, dtype=np.float64, rollover=rollover)
    rel = rel_err(cost_dev, cost_ref)
    bar, used = 1e-5, 0
    if rel.max() >= bar:
        c32 = CO.rollout(so.astype(np.float32), po, a_dev.astype(np.float32), 1.0, fs.astype(np.float32), dtype=np.float32,
                         rollover=rollover)
        bar = max(bar, 1.5 * rel_err(c32, cost_ref).max())
        used = int((rel >= 1e-5).sum())
        print(f"  {name} N={N}: {used} samples beyond 1e-5 (max {rel.max():.3e}; fp32 oracle vs fp64 {rel_err(c32, cost_ref).max():.3e})")
        assert used <= max(2, N // 4096), (name, N, used)
    assert rel.max() < bar, (name, N, rel.max(), bar)
    a_ref, _ = R.softmax_update(cost_ref, a_dev, float(lam), 1.0, am)
    gap = np.diff(np.sort(cost_ref)[:2])[0]
    err = np.abs(a_mean_new_t.cpu().numpy().reshape(32, 4) - a_ref).max()
    print(f"  {name} N={N}: max rel cost err {rel.max():.3e}, mean err {err:.3e}, top-2 gap {gap:.3e}")
    print(f"  batched {name} N={N} lam {lam}: mean vs oracle costs: err {err:.3e}, gap {gap:.3e}, passed by {'err' if err < 1e-4 else 'gap'}")
    assert err < 1e-4 or gap < 1e-3 * float(lam) / 0.01, (name, N, err, gap)
    check_update((cost_dev_t, a_dev_t), a_mean_before, 1.0, float(lam), a_mean_new_t, where=f"batched {name} N={N}")  # own costs: no hatch
    return used


@pytest.mark.parametrize("name,N", [("mppi", 1024), ("covo-offline", 4096)])
def test_batched_mode_step_against_the_oracle(name, N):
    """One batch of 6 instances per mode against oracle/ directly (not only against the sibling path): every instance's costs
    against the C fp64 rollout with that instance's parameters, state and -- MPPI -- shared disturbance draw, and its new mean
    against ref_np.softmax_update of the oracle's costs.  covo-offline builds its tables through the batched controller's own
    reset()."""
    lam, E = "0.01", 6
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, name, N, lam, E, seed=7)
    b = batched_controller(env, name, inst, len(inst), N, lam, check_cov=True)
    b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    if name == "covo-offline":
        b.reset([i["state"] for i in inst], [i["params"] for i in inst], [i["reset_key"] for i in inst])
    total = 0
    for step in range(2):
        k_acts = []
        for i in inst:
            i["key"], k_act, i["k_step"] = cr.split(i["key"], 3)
            k_acts.append(np.asarray(k_act))
        am_before = b.a_mean.cpu().numpy().copy()
        noisy = [i["info"]["noisy_state"] for i in inst]
        u_b = b(noisy, np.stack(k_acts)).clone()
        torch.cuda.synchronize()
        for e, i in enumerate(inst):
            total += _oracle_check_instance(name, env, i["params"], noisy[e], am_before[e], k_acts[e], b._a[e], b._cost[e],
                                            b.a_mean[e], lam)
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u_b[e].cpu().numpy(), i["params"])
    print(f"{name}: {total} samples in all used the widened bar")


@pytest.mark.parametrize("name,N", [("mppi", 1024), ("covo-offline", 2048)])
def test_run_episode_batched_mode_equals_per_instance_episodes(name, N):
    """covo_run_episode_batched_mode, 40 steps on 8 instances in two segments, against 8 per-instance episodes of the single
    controller with the same keys: logs, means, final states, key chains (and MPPI's covariances) bit-identical.  Instance 3 starts
    at step 285 of its episode: it terminates and auto-resets inside the segment.  covo-offline: the batched reset()'s tables
    equal those of 8 single CoVOController.reset calls."""
    import covo_mpc_amd as cm
    E, n, lam = 8, 40, "0.01"
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, name, N, lam, E, seed=50, warm=False)
    params = [i["params"] for i in inst]
    b = batched_controller(env, name, inst, len(inst), N, lam, check_cov=True)
    reset_keys = [cr.PRNGKey(150 + e) for e in range(E)]
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    late = torch.tensor([285], dtype=torch.int32, device=DEV).view(torch.float32)
    ep.true[3, ST_TIME:ST_TIME + 1] = late
    ep.noisy[3, ST_TIME:ST_TIME + 1] = late
    table_keys = [cr.PRNGKey(250 + e) for e in range(E)]
    if name == "covo-offline":
        with pytest.raises(RuntimeError, match="call controller.reset"):
            b.run_episode(ep, np.zeros((E, 2), dtype=np.uint32), 1)
        b.reset(ep.states0, params, table_keys)
    rngs0 = np.stack([np.asarray(cr.PRNGKey(160 + e)) for e in range(E)])
    rngs = b.run_episode(ep, rngs0, n // 2)
    rngs = b.run_episode(ep, rngs, n - n // 2)
    log = ep.read_log()
    assert log.shape == (E, n, 4)
    assert log[3, :, 3].sum() >= 1 and log[0, :, 3].sum() == 0  # instance 3 finished its episode inside the segment
    for e, i in enumerate(inst):
        c = i["c"]
        c.alias_outputs = True
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        if e == 3:
            se.true[ST_TIME:ST_TIME + 1] = late
            se.noisy[ST_TIME:ST_TIME + 1] = late
        cp = c.reset(se.state0, params[e], c.init_control_params, table_keys[e])
        if name == "covo-offline":
            assert torch.equal(cp.a_cov_offline, b.a_cov_offline[e]) and torch.equal(cp.a_chol_offline, b.a_chol_offline[e]), e
        cp, rng = c.run_episode(se, params[e], cp, rngs0[e], n)
        assert np.array_equal(se.read_log(), log[e]), e
        assert torch.equal(cp.a_mean.reshape(-1), b.a_mean[e]) and torch.equal(se.true, ep.true[e]), e
        if name == "mppi":
            assert torch.equal(cp.a_cov, b.a_cov[e]), e
        assert np.array_equal(np.asarray(rng, dtype=np.uint32), rngs[e]), e


def test_batched_mode_refusals_name_the_condition_and_leave_the_handle_usable():
    """What the batched fused launch does not take is refused by argument checks, before any launch, with a message that names the
    condition; the handle works afterwards."""
    import covo_mpc_amd as cm
    from covo_mpc_amd.dynamics import utils
    N, lam, E = 256, "0.01", 2

    def build(env, name="mppi", n=N, **kw):
        inst = instances(env, name, n, lam, E, warm=False)
        cp0 = inst[0]["cp"]
        if name == "mppi":
            b = cm.controllers.BatchedMPPIController(env, E, n, 32, 0.01, sigmas=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=DEV, **kw)
        else:
            b = cm.controllers.BatchedCoVOController(env, E, n, 32, 0.01, a_mean_init=cp0.a_mean, device=DEV, mode="offline")
        b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
        return b, inst

    keys = np.arange(2 * E, dtype=np.uint32).reshape(E, 2) + 1
    # gamma_sigma != 0: the constructor, and the C boundary for a caller that sets the field itself
    with pytest.raises(NotImplementedError, match="gamma_sigma"):
        cm.controllers.BatchedMPPIController(quad_env(task="tracking", randomizer=True), E, N, 32, 0.01, gamma_sigma=0.2, device=DEV)
    b, inst = build(quad_env(task="tracking", randomizer=True))
    noisy = [i["info"]["noisy_state"] for i in inst]
    b._args.gamma_sigma = 0.2
    with pytest.raises(_lib.CovoError, match="gamma_sigma != 0"):
        b(noisy, keys)
    b._args.gamma_sigma = 0.0
    # more instances than COVO_MAX_ENVS
    with pytest.raises(ValueError, match="n_envs"):
        cm.controllers.BatchedMPPIController(quad_env(task="tracking", randomizer=True), _lib.COVO_MAX_ENVS + 1, N, 32, 0.01, device=DEV)
    b._args.base.n_envs = _lib.COVO_MAX_ENVS + 1
    with pytest.raises(_lib.CovoError, match="n_envs=65"):
        b(noisy, keys)
    b._args.base.n_envs = E
    # ... and the handle still works: the refused calls launched nothing and left nothing behind
    u = b(noisy, keys).clone()
    assert torch.isfinite(u).all() and b.core.device_status() == 0
    # the realworld reward
    env_r = quad_env(task="tracking", randomizer=True)
    env_r.reward_fn = utils.tracking_realworld_reward_fn
    br, inst_r = build(env_r)
    with pytest.raises(_lib.CovoError, match="realworld reward"):
        br([i["info"]["noisy_state"] for i in inst_r], keys)
    # a disturbance model with per-step tables
    bp, inst_p = build(quad_env(task="tracking", randomizer=True, disturb="periodic"))
    with pytest.raises(_lib.CovoError, match="per-step tables"):
        bp([i["info"]["noisy_state"] for i in inst_p], keys)
    # N > 16 384
    bn, inst_n = build(quad_env(task="tracking", randomizer=True), n=16384 + 64)
    with pytest.raises(_lib.CovoError, match="16384"):
        bn([i["info"]["noisy_state"] for i in inst_n], keys)
    # covo-offline without a table: the controller, and the C boundary
    bo, inst_o = build(quad_env(task="tracking", randomizer=True), name="covo-offline")
    with pytest.raises(RuntimeError, match="a_cov_offline table missing"):
        bo([i["info"]["noisy_state"] for i in inst_o], keys)
    bo.a_chol_offline = torch.zeros(1, device=DEV)  # (past the controller's own check; the argument block still has no table)
    with pytest.raises(_lib.CovoError, match="table is missing"):
        bo([i["info"]["noisy_state"] for i in inst_o], keys)
    # covo_debug_time_batched replays covo-online's launch groups only
    with pytest.raises(_lib.CovoError, match="covo_mpc_step_batched first"):
        b.time_phases(16)
    for c in (b, br, bp, bn, bo):
        assert c.core.device_status() == 0
    u2 = b(noisy, keys)
    assert torch.isfinite(u2).all()


# (step_mask, hess_mask, sigma_stages) of every CovoCore.time_phases call in bench.py and scripts/phase_times.py, the whole step last
SINGLE_MASKS = [(4,), (4 | 8,), (4 | 8 | 16,), (2 | 4,), (8 | 16 | 32,), (8,), (8 | 16,),                     # bench.py
                (63,), (2,), (2, 1), (2, 2), (2, 8), (4, 15, 1), (4, 15, 2), (4, 15, 3), (16,), (32,), (0,),  # scripts/phase_times.py
                (24,), (56,), (48,), (63,)]
BATCHED_MASKS = [2 | 4 | 8 | 16 | 32, 2, 4, 8, 16, 32, 63]  # bench.py --config envs; 63


@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_masked_launch_groups_of_the_phase_timers(graph, monkeypatch):
    """covo-online, N = 256 single and E = 2 x N = 256 env-batched, on a graph-replaying and on an eager handle: after one full step,
    covo_debug_time_step / covo_debug_time_batched with every mask bench.py and scripts/phase_times.py use (bench.py's two with the
    GEMM as a launch of its own included) and with 63 return a finite positive time and leave device_status() 0; a following
    ordinary step then gives the same a_mean, bit for bit, as on a fresh controller with the same keys that never ran the timers.
    No timing is asserted: the masked forms of the step's launch sequence must be something the runtime accepts, and must leave the
    handle (scratch, graph caches, keys) as a step expects it.
    The update group (mask 32) writes the caller's a_mean by definition, mask 63 of the batched timer also runs the begin launch,
    which shifts the in/out mean once more per copy, and on an eager handle covo_debug_time_step refills the step's scratch with
    the key derived from (0, 0): the mean the timers leave in the CALLER's buffer is not the step's.  Both controllers therefore
    start the following step from the mean the first step returned (saved before the timers); everything the handle owns is left
    as the timers left it."""
    import covo_mpc_amd as cm
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    N, lam, E = 256, "0.01", 2
    env = quad_env(task="tracking", randomizer=True)

    def timed_ok(us, what):
        assert np.isfinite(us) and us > 0.0, (graph, what, us)

    # ---- single: two identical controllers on instance 0, the first one runs the timers between its two steps
    runs = [instances(env, "covo-online", N, lam, 1)[0] for _ in range(2)]
    assert runs[0]["c"].core.uses_graph == (graph == "graph")
    for step in range(2):
        for r, i in enumerate(runs):
            i["key"], k_act, i["k_step"] = cr.split(i["key"], 3)
            u, i["cp"], _ = i["c"](i["obs"], i["state"], i["params"], k_act, i["cp"], i["info"])
            if step == 0 and r == 0:
                saved = i["cp"].a_mean.clone()
                core = i["c"].core
                for m in SINGLE_MASKS:
                    timed_ok(core.time_phases(*m, reps=4), ("single", m))
                _lib.check(core.lib.covo_debug_set_stream_gemm(core.h, 0), "stream_gemm")
                for m in ((4,), (4 | 8,)):
                    timed_ok(core.time_phases(*m, reps=4), ("single, stream_gemm=0", m))
                _lib.check(core.lib.covo_debug_set_stream_gemm(core.h, 1), "stream_gemm")
                timed_ok(core.time_phases(63, reps=4), ("single", 63))
                assert core.device_status() == 0
                i["cp"] = i["cp"].replace(a_mean=saved)
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u.cpu().numpy(), i["params"])
        print(f"{graph} single step {step}: max |a_mean difference| {(runs[0]['cp'].a_mean - runs[1]['cp'].a_mean).abs().max():.3g}")
        assert torch.equal(runs[0]["cp"].a_mean, runs[1]["cp"].a_mean), (graph, "single", step)
    assert all(i["c"].core.device_status() == 0 for i in runs)

    # ---- env-batched: two identical controllers on E instances
    inst = instances(env, "covo-online", N, lam, E)
    cp0 = inst[0]["cp"]
    bs = [cm.controllers.BatchedCoVOController(env, E, N, 32, float(lam), discount=cp0.discount, gamma_mean=cp0.gamma_mean,
                                               sample_sigma=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=DEV) for _ in range(2)]
    for b in bs:
        b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    assert bs[0].core.uses_graph == (graph == "graph")
    for step in range(2):
        k_acts = []
        for i in inst:
            i["key"], k_act, i["k_step"] = cr.split(i["key"], 3)
            k_acts.append(np.asarray(k_act))
        noisy = [i["info"]["noisy_state"] for i in inst]
        for r, b in enumerate(bs):
            u = b(noisy, np.stack(k_acts)).clone()
            if step == 0 and r == 0:
                saved = b.a_mean.clone()
                for m in BATCHED_MASKS:
                    timed_ok(b.time_phases(m, reps=4), ("batched", m))
                assert b.core.device_status() == 0
                b.a_mean.copy_(saved)
        print(f"{graph} batched step {step}: max |a_mean difference| {(bs[0].a_mean - bs[1].a_mean).abs().max():.3g}")
        assert torch.equal(bs[0].a_mean, bs[1].a_mean), (graph, "batched", step)
        for e, i in enumerate(inst):
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u[e].cpu().numpy(), i["params"])
    assert all(b.core.device_status() == 0 for b in bs) and torch.isfinite(bs[0].a_mean).all()
