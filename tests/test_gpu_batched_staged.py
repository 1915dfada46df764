"""GPU tests (-m gpu) of the STAGED env-batched MPPI and covo-offline steps (covo_set_step_batched_staged, csrc/step.hip:
covo_step_batched_staged_impl; staged=True of BatchedMPPIController / BatchedCoVOController(mode="offline")).

The bar throughout: instance e of a staged batched step == the single controller stepped on instance e alone with the same
configuration, bit for bit (torch.equal on a_mean, the action buffer, the costs, a_cov, the first action and every attachment
row) -- and therefore, for a configuration the fused launch takes, == the fused batched step.  Every case: E = 3 (2 at the large
N) domain-randomised instances that differ in state, trajectory, parameters and key, 3 consecutive steps (eager, capture,
replay) and the same three once more on a COVO_NO_GRAPH handle.  The instances, tables and oracle helpers are those of
tests/test_gpu_batched_modes.py.
  1. staged == fused batched, on the ragged and full shapes of that file's CASES;
  2. staged == single replicas on every refusal of the fused launch that is lifted: the four table-driven disturbance models, the
     realworld reward, N = 16 384 + 64, MPPI's covariance adaptation (with and without diagnostics), shared / per-instance tables;
  3. every attachment row: elite, ess_min, compute_post_cov, iters=2 with update="guarded", compute_plan + compute_fan under periodic;
  4. against oracle/ directly (bars and cap of tests/test_gpu_batched_modes.py's docstring: 1e-5, 1e-4, max(2, N // 4096) widened);
  5. an 8-step episode with an auto-reset inside against per-instance DeviceEpisodes;
  6. the refusals that remain under staged, each leaving the handle usable.
     For gamma_sigma = 0.2 the new mean and a_cov against ref_np.softmax_update + ref_np.mppi_cov_update in fp64, at the bars of the
     single controller's covariance-adaptation test, tests/test_gpu_models.py::test_mppi_covariance_adaptation_vs_oracle: 1e-5 on
     the mean and 1e-5 on a_cov;
  7. eval_env_batched(controller="mppi" | "covo-offline", staged=True): the driver reaches the baselines;
  8. one handle stepped alternately through covo_mpc_step_batched and the staged covo_mpc_step_batched_mode == two handles.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers.batched import CORE_BUFFERS  # noqa: E402
from covo_mpc_amd.dynamics.dataclass import as_device_state  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from tests.gpu_support import DEV, ST_TIME, batched_controller, disturb_key, instances, offline_tables, quad_env  # noqa: E402
from tests.oracle_support import oracle_params, oracle_state, rel_err  # noqa: E402
from tests.update_oracle import check_update  # noqa: E402

GRAPHS = ["graph", "eager"]


def _bits(t):
    return t.contiguous().view(torch.int32).reshape(-1)


def _tables(env, name, inst, bs, shared=False):
    """covo-offline: every instance's table (one set for the whole file: both sides of a comparison read the same factors, whatever
    they were built from); shared: all instances read instance 0's through L_table_stride = 0."""
    if name != "covo-offline":
        return
    Sig, L = offline_tables(env, inst, "staged")
    for b in bs:
        b.set_tables(Sig, L)
        if shared:
            b._args.L_table_stride = 0
    if shared:
        for i in inst:
            i["cp"] = i["cp"].replace(a_cov_offline=Sig[0], a_chol_offline=L[0])


def _same_as_single(b, e, i, u_b, u, name, where):
    assert torch.equal(b.a_mean[e].view(32, 4), i["cp"].a_mean), where
    assert torch.equal(b._a[e], i["c"].core.a), where
    assert torch.equal(b._cost[e], i["c"].core.cost), where
    assert torch.equal(u_b[e], u), where
    if name == "mppi":
        assert torch.equal(b.a_cov[e], i["cp"].a_cov), where
    for mine, cores in CORE_BUFFERS:  # every [E, ...] attachment row against the single core's one row
        rows = getattr(b, mine)
        if rows is not None:
            assert torch.equal(_bits(rows[e]), _bits(getattr(i["c"].core, cores)[0])), where + (mine,)


def _steps(env, name, inst, b, others=(), n_steps=3, where=()):
    """n_steps closed-loop steps of the staged batched controller b, of `others` (batched twins that must agree with it bit for bit)
    and of the instances' single controllers."""
    E = len(inst)
    for step in range(n_steps):
        k_acts = []
        for i in inst:
            i["key"], k_act, i["k_step"] = cr.split(i["key"], 3)
            k_acts.append(np.asarray(k_act))
        noisy = [i["info"]["noisy_state"] for i in inst]
        u_b = b(noisy, np.stack(k_acts)).clone()
        for o in others:
            u_o = o(noisy, np.stack(k_acts)).clone()
            for x, y in ((b.a_mean, o.a_mean), (b._a, o._a), (b._cost, o._cost), (b.a_cov, o.a_cov), (u_b, u_o)):
                assert torch.equal(x, y), where + (step, "twin")
        for e, i in enumerate(inst):
            u, i["cp"], _ = i["c"](i["obs"], i["state"], i["params"], k_acts[e], i["cp"], i["info"])
            _same_as_single(b, e, i, u_b, u, name, where + (step, e))
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u.cpu().numpy(), i["params"])
    assert b.core.device_status() == 0 and torch.isfinite(b.a_mean).all(), where
    if E > 1:
        assert (b.a_mean[0] - b.a_mean[1]).abs().max() > 1e-4, where  # different plants, different plans


def _close(inst, *bs):
    for b in bs:
        b.core.close()
    for i in inst:
        i["c"].core.close()


def _case(name, N, lam, graph, monkeypatch, E=3, disturb="gaussian", rollover=False, task="tracking", gamma_sigma=0.0, shared=False,
          fused_twin=False, **opts):
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    env = quad_env(task=task, randomizer=True, rollover=rollover, disturb=disturb)
    inst = instances(env, name, N, lam, E, gamma_sigma=gamma_sigma, **opts)
    b = batched_controller(env, name, inst, len(inst), N, lam, set_instances=True, staged=True, gamma_sigma=gamma_sigma, **opts)
    assert b.staged and b.core.uses_graph == (graph == "graph")
    twins = []
    if fused_twin:
        twins = [batched_controller(env, name, inst, len(inst), N, lam, set_instances=True, staged=False, gamma_sigma=0.0)]
    _tables(env, name, inst, [b] + twins, shared)
    _steps(env, name, inst, b, twins, where=(name, N, graph, disturb, task))
    if gamma_sigma:
        # adapted, and still symmetric: entries (i, j) and (j, i) are the same four terms -- S2, m1_i e_j, e_i m1_j, e_i e_j, each at
        # most 4 in magnitude (|a - mu| <= 2) -- summed in another order: they differ by at most 4 roundings of 2^-24 * 4
        asym = (b.a_cov - b.a_cov.transpose(-1, -2)).abs().max().item()
        assert asym <= 4 * 4 * 2.0 ** -24, asym
        assert (b.a_cov[0] - b.a_cov[1]).abs().max() > 0
    _close(inst, b, *twins)


# ---- 1. staged == fused batched (== single replicas) ------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("name,N,lam,rollover", [("mppi", 100, "5.0", True), ("mppi", 1024, "0.01", False),
                                                 ("covo-offline", 40, "0.01", True)])
def test_staged_equals_fused(name, N, lam, rollover, graph, monkeypatch):
    _case(name, N, lam, graph, monkeypatch, rollover=rollover, fused_twin=True)


# ---- 2. staged == single replicas on each refusal lifted --------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("name,N", [("mppi", 100), ("covo-offline", 40)])
@pytest.mark.parametrize("disturb", ["periodic", "sin", "drag", "mixed"])
def test_disturbance_models_with_tables(disturb, name, N, graph, monkeypatch):
    _case(name, N, "0.01", graph, monkeypatch, disturb=disturb)


@pytest.mark.parametrize("graph", GRAPHS)
def test_realworld_reward(graph, monkeypatch):
    _case("mppi", 256, "0.01", graph, monkeypatch, task="tracking_slow")


@pytest.mark.parametrize("graph", GRAPHS)
def test_first_sample_count_the_fused_launch_refuses(graph, monkeypatch):
    _case("mppi", 16384 + 64, "0.01", graph, monkeypatch, E=2)


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("diag", [False, True])
@pytest.mark.parametrize("N,lam", [(100, "5.0"), (1024, "0.01")])
def test_mppi_covariance_adaptation(N, lam, diag, graph, monkeypatch):
    _case("mppi", N, lam, graph, monkeypatch, gamma_sigma=0.2, compute_diag=diag)


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("shared", [True, False])
def test_offline_shared_and_per_instance_tables(shared, graph, monkeypatch):
    _case("covo-offline", 64, "0.01", graph, monkeypatch, shared=shared)


# ---- 3. attachments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("name,N", [("mppi", 256), ("covo-offline", 64)])
@pytest.mark.parametrize("opts", [dict(elite=8), dict(ess_min=8), dict(compute_post_cov=True), dict(iters=2, update="guarded"),
                                  dict(compute_plan=True, compute_fan=4, disturb="periodic")],
                         ids=["elite", "ess_min", "post_cov", "iters_guarded", "plan_fan_periodic"])
def test_attachment_rows(opts, name, N, graph, monkeypatch):
    opts = dict(opts)
    _case(name, N, "0.01", graph, monkeypatch, disturb=opts.pop("disturb", "gaussian"), **opts)


# ---- 4. against oracle/ directly --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,disturb", [("mppi", "periodic"), ("covo-offline", "drag")])
def test_staged_step_against_the_oracle(name, disturb):
    """Per-sample costs against the C fp64 rollout with the instance's parameters, state and disturbance draw (1e-5; at most
    max(2, N // 4096) samples per instance may use the widened bar, 1.5 x what the fp32 C oracle loses against the fp64 one), the new
    mean against ref_np.softmax_update of the oracle's costs (1e-4 unless the two best costs are closer than 1e-3 * lam / 0.01)."""
    N, lam, E = 1024, "0.01", 3
    env = quad_env(task="tracking", randomizer=True, disturb=disturb)
    inst = instances(env, name, N, lam, E, seed=7)
    b = batched_controller(env, name, inst, len(inst), N, lam, set_instances=True, staged=True, gamma_sigma=0.0)
    _tables(env, name, inst, [b])
    k_acts = [np.asarray(cr.split(i["key"], 3)[1]) for i in inst]
    am_before = b.a_mean.cpu().numpy().copy()
    noisy = [i["info"]["noisy_state"] for i in inst]
    b(noisy, np.stack(k_acts))
    torch.cuda.synchronize()
    for e, i in enumerate(inst):
        p = i["params"]
        so = oracle_state(noisy[e])
        po = oracle_params(p).replace(disturb_period=int(p.disturb_period), disturb_scale=float(p.disturb_scale))
        step_key = cr.split(cr.split(k_acts[e])[0])[1]
        draw = cr.uniform(disturb_key(step_key), (3,), -po.disturb_scale, po.disturb_scale).astype(np.float64)
        d = R.Disturb(disturb, draw, name != "mppi")
        a_dev = b._a[e].permute(1, 0, 2).contiguous().cpu().numpy().astype(np.float64)
        cost_dev = b._cost[e].cpu().numpy()
        cost_ref = CO.rollout(so, po, a_dev, 1.0, dtype=np.float64, disturb=d)
        rel = rel_err(cost_dev, cost_ref)
        bar = 1e-5
        if rel.max() >= bar:
            c32 = CO.rollout(so.astype(np.float32), po, a_dev.astype(np.float32), 1.0, dtype=np.float32, disturb=d)
            bar = max(bar, 1.5 * rel_err(c32, cost_ref).max())
            used = int((rel >= 1e-5).sum())
            print(f"  {name} {disturb} instance {e}: {used} samples beyond 1e-5 (max {rel.max():.3e})")
            assert used <= max(2, N // 4096), (name, e, used)
        assert rel.max() < bar, (name, e, rel.max(), bar)
        am = R.shift_mean(am_before[e].astype(np.float64).reshape(32, 4))
        a_ref, _ = R.softmax_update(cost_ref, a_dev, float(lam), 1.0, am)
        gap = np.diff(np.sort(cost_ref)[:2])[0]
        err = np.abs(b.a_mean[e].cpu().numpy().reshape(32, 4) - a_ref).max()
        print(f"  {name} {disturb} instance {e}: max rel cost err {rel.max():.3e}, mean err {err:.3e}, top-2 gap {gap:.3e}")
        print(f"  batched staged {name} {disturb} instance {e}: mean vs oracle costs: err {err:.3e}, gap {gap:.3e}, "
              f"passed by {'err' if err < 1e-4 else 'gap'}")
        assert err < 1e-4 or gap < 1e-3 * float(lam) / 0.01, (name, e, err, gap)
        check_update((b._cost[e], b._a[e]), am_before[e], 1.0, float(lam), b.a_mean[e],
                     where=f"batched staged {name} {disturb} instance {e}")  # the same mean on the step's own costs: no hatch
    _close(inst, b)


@pytest.mark.parametrize("N,lam", [(100, "5.0"), (1024, "0.01")])
def test_staged_covariance_adaptation_against_the_oracle(N, lam):
    """MPPI with gamma_sigma = 0.2 on the batch, two steps (the second adapts covariances the first has already moved): per instance
    the new mean and a_cov[e] against ref_np.softmax_update + ref_np.mppi_cov_update in fp64 on the device's costs and samples, the
    covariances about the NEW mean and blended into the SHIFTED old ones (mppi.py:43-49, 109-125) -- the reference, the inputs and
    the bars (1e-5 and 1e-5) of tests/test_gpu_models.py::test_mppi_covariance_adaptation_vs_oracle."""
    E, gs = 3, 0.2
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "mppi", N, lam, E, seed=11, gamma_sigma=gs)
    b = batched_controller(env, "mppi", inst, len(inst), N, lam, set_instances=True, staged=True, gamma_sigma=gs)
    moved = 0.0
    for step in range(2):
        k_acts = []
        for i in inst:
            i["key"], k_act, i["k_step"] = cr.split(i["key"], 3)
            k_acts.append(np.asarray(k_act))
        am_before = b.a_mean.cpu().numpy().astype(np.float64)
        cov_before = b.a_cov.cpu().numpy().astype(np.float64)
        u_b = b([i["info"]["noisy_state"] for i in inst], np.stack(k_acts)).clone()
        torch.cuda.synchronize()
        for e, i in enumerate(inst):
            a_dev = b._a[e].permute(1, 0, 2).contiguous().cpu().numpy().astype(np.float64)
            cost = b._cost[e].cpu().numpy().astype(np.float64)
            a_new, w = R.softmax_update(cost, a_dev, float(lam), float(inst[0]["cp"].gamma_mean), R.shift_mean(am_before[e].reshape(32, 4)))
            cov_old = R.shift_mean(cov_before[e])
            cov_ref = R.mppi_cov_update(w, a_dev, a_new, cov_old, gs)
            e_mean = np.abs(b.a_mean[e].cpu().numpy().reshape(32, 4) - a_new).max()
            e_cov = np.abs(b.a_cov[e].cpu().numpy() - cov_ref).max()
            moved = max(moved, np.abs(cov_ref - cov_old).max())
            print(f"  N={N} step {step} instance {e}: mean err {e_mean:.3e}, a_cov err {e_cov:.3e}")
            assert e_mean < 1e-5, (N, step, e, e_mean)
            assert e_cov < 1e-5, (N, step, e, e_cov)
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u_b[e].cpu().numpy(), i["params"])
    assert moved > 1e-3  # the adaptation moved the covariances
    assert b.core.device_status() == 0
    _close(inst, b)


# ---- 5. episode -------------------------------------------------------------------------------------------------------------------
def test_run_episode_staged_equals_per_instance_episodes():
    """covo_run_episode_batched_mode under staged, MPPI-periodic with elite = 8, 8 steps in two segments on 3 instances, against 3
    per-instance DeviceEpisodes of the single controller with the same keys: env logs, elite logs, means, covariances, final states
    and key chains bit-identical.  Instance 1 starts at max_steps - 3: it terminates and auto-resets inside the segment."""
    E, n, N, lam, name = 3, 8, 256, "0.01", "mppi"
    env = quad_env(task="tracking", randomizer=True, disturb="periodic")
    inst = instances(env, name, N, lam, E, seed=50, warm=False, elite=8)
    params = [i["params"] for i in inst]
    b = batched_controller(env, name, inst, len(inst), N, lam, set_instances=True, staged=True, gamma_sigma=0.0, elite=8)
    reset_keys = [cr.PRNGKey(150 + e) for e in range(E)]
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    late = torch.tensor([int(params[1].max_steps_in_episode) - 3], dtype=torch.int32, device=DEV).view(torch.float32)
    ep.true[1, ST_TIME:ST_TIME + 1] = late
    ep.noisy[1, ST_TIME:ST_TIME + 1] = late
    rngs0 = np.stack([np.asarray(cr.PRNGKey(160 + e)) for e in range(E)])
    rngs = b.run_episode(ep, rngs0, n // 2)
    rngs = b.run_episode(ep, rngs, n - n // 2)
    log = ep.read_log()
    assert log.shape == (E, n, 4) and log[1, :, 3].sum() >= 1 and log[0, :, 3].sum() == 0
    elite = ep.read_elite()
    assert np.all(elite["K"] == 8.0) and elite["K"].shape == (E, n)
    for e, i in enumerate(inst):
        c = i["c"]
        c.alias_outputs = True
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        if e == 1:
            se.true[ST_TIME:ST_TIME + 1] = late
            se.noisy[ST_TIME:ST_TIME + 1] = late
        cp = c.reset(se.state0, params[e], c.init_control_params, cr.PRNGKey(250 + e))
        cp, rng = c.run_episode(se, params[e], cp, rngs0[e], n)
        assert np.array_equal(se.read_log(), log[e]), e
        assert torch.equal(_bits(se.elitelog[:n]), _bits(ep.elitelog[e, :n])), e
        rows = se.read_elite()  # the per-step rows of the single controller, field by field
        assert set(rows) == set(elite)
        for f in rows:
            assert rows[f].shape == (n,) and np.array_equal(elite[f][e], rows[f]), (e, f)
        assert torch.equal(cp.a_mean.reshape(-1), b.a_mean[e]) and torch.equal(cp.a_cov, b.a_cov[e]), e
        assert torch.equal(se.true, ep.true[e]), e
        assert np.array_equal(np.asarray(rng, dtype=np.uint32), rngs[e]), e
    assert b.core.device_status() == 0
    _close(inst, b)


# ---- 6. refusals under staged -----------------------------------------------------------------------------------------------------
def test_staged_refusals_name_the_condition_and_leave_the_handle_usable():
    N, lam, E = 256, "0.01", 2
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "mppi", N, lam, E, warm=False)
    noisy = [i["info"]["noisy_state"] for i in inst]
    keys = np.arange(2 * E, dtype=np.uint32).reshape(E, 2) + 1
    b = batched_controller(env, "mppi", inst, len(inst), N, lam, set_instances=True, staged=True, gamma_sigma=0.2)
    assert b._args.gamma_sigma == np.float32(0.2)
    # the update reads the per-wave minima
    gm = b._args.base.groupmin
    b._args.base.groupmin = None
    with pytest.raises(_lib.CovoError, match="groupmin"):
        b(noisy, keys)
    b._args.base.groupmin = gm
    assert torch.isfinite(b(noisy, keys)).all() and b.core.device_status() == 0
    # gamma_sigma next to an elite set attached through the C setter
    rows = torch.zeros((E, _lib.COVO_ELITE_FLOATS), dtype=torch.float32, device=DEV)
    _lib.check(b.core.lib.covo_set_step_elite(b.core.h, 8, _lib.ptr(rows), E), "covo_set_step_elite")
    with pytest.raises(_lib.CovoError, match="gamma_sigma != 0 together with the elite-set update"):
        b(noisy, keys)
    _lib.check(b.core.lib.covo_set_step_elite(b.core.h, 0, None, 0), "covo_set_step_elite")
    assert torch.isfinite(b(noisy, keys)).all() and b.core.device_status() == 0
    # gamma_sigma is MPPI's
    inst_o = instances(env, "covo-offline", 64, lam, E, warm=False)
    bo = batched_controller(env, "covo-offline", inst_o, len(inst_o), 64, lam, set_instances=True, staged=True, gamma_sigma=0.0)
    _tables(env, "covo-offline", inst_o, [bo])
    noisy_o = [i["info"]["noisy_state"] for i in inst_o]
    bo._args.gamma_sigma = 0.2
    with pytest.raises(_lib.CovoError, match="gamma_sigma != 0 is MPPI's covariance adaptation"):
        bo(noisy_o, keys)
    bo._args.gamma_sigma = 0.0
    assert torch.isfinite(bo(noisy_o, keys)).all() and bo.core.device_status() == 0
    # the phase timer replays covo-online's launch groups only, as after a fused step
    with pytest.raises(_lib.CovoError, match="covo_mpc_step_batched first"):
        b.time_phases(16)
    # switching the handle back to the fused launch: today's refusal, and its step once the cause is gone
    _lib.check(b.core.lib.covo_set_step_batched_staged(b.core.h, 0), "covo_set_step_batched_staged")
    with pytest.raises(_lib.CovoError, match="gamma_sigma != 0"):
        b(noisy, keys)
    b._args.gamma_sigma = 0.0
    assert torch.isfinite(b(noisy, keys)).all() and b.core.device_status() == 0
    _close(inst + inst_o, b, bo)


# ---- 7. the driver ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("controller,opts", [("mppi", dict(elite=8)), ("covo-offline", dict(iters=2, update="guarded"))])
def test_eval_env_batched_runs_the_baselines_staged(controller, opts):
    """eval_env_batched on the two baseline controllers under the periodic disturbance with an option the fused launch refuses: it runs
    under staged=True (finite errors, the rows of the option come back) and is refused without it, as the controllers are."""
    env = quad_env(task="tracking", randomizer=True, disturb="periodic")
    run = lambda **kw: cm.envs.quadrotor.eval_env_batched(env, 2, "N256_H32_lam0.01", n_steps=4, device=DEV, verbose=False,
                                                          controller=controller, rows=True, **opts, **kw)
    with pytest.raises(NotImplementedError, match="staged=True"):
        run()
    err, rows = run(staged=True)
    assert err.shape == (2,) and np.all(np.isfinite(err))
    if "elite" in opts:
        assert rows["elite"]["K"].shape == (2, 4) and np.all(rows["elite"]["K"] == 8.0)
    else:
        assert rows["iters"].shape == (2, 4, 2) and np.all(np.isfinite(rows["iters"]))
    with pytest.raises(ValueError, match='staged=True with mode="online"'):
        cm.envs.quadrotor.eval_env_batched(env, 2, "N256_H32_lam0.01", n_steps=1, device=DEV, verbose=False, staged=True)


# ---- 8. one handle, both batched entry points -------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma_period", [1, 2])
def test_one_handle_through_both_batched_entry_points(sigma_period, monkeypatch):
    """The covo-online batch and the staged MPPI batch keep separate scratch, keys and graphs on one handle.  A: the covo-online batch,
    E = 3, N = 256; B: the staged MPPI batch, E = 2, N = 100 (another instance count: a scratch the two shared would be re-allocated by
    every call).  Reference: four steps of each on its own handle (eager, capture, two replays), open loop on the instances' states,
    a_mean / the action buffer / the costs / a_cov and A's sigma_age recorded after every step.  Then both are rebuilt from the same
    initial state and both argument blocks are driven through A's handle alternately, with the same keys: every recorded tensor is
    torch.equal to the two-handle run, step by step.

    sigma_period = 1: both entries run.  After every MPPI step the factors covo-online left in its scratch (covo_debug_sigma_factor)
    are still those of the two-handle run: the other entry has neither freed nor rewritten them.
    sigma_period = 2 on A: check_step_attachments refuses an MPPI / covo-offline step on a handle that carries a Sigma period ("belongs
    to covo-online steps") before anything is launched, so B's half of the alternation cannot run there; every B call must be refused
    with that message, and A's steps between the refused calls go on through refresh and reuse -- sigma_age 0, 1, 0, 1 -- equal to A
    alone."""
    monkeypatch.setenv("COVO_GRAPH", "1")
    env = quad_env(task="tracking", randomizer=True)
    inst_a = instances(env, "covo-online", 256, "0.01", 3, seed=20)
    inst_b = instances(env, "mppi", 100, "0.01", 2, seed=30)  # (lam and the discount are the handle's: one value for both)
    _close(inst_a + inst_b)  # (only the instances' states, parameters and keys are used)
    keys = {}
    for tag, inst in (("A", inst_a), ("B", inst_b)):
        keys[tag] = []
        for step in range(4):
            row = []
            for i in inst:
                i["key"], k_act, _ = cr.split(i["key"], 3)
                row.append(np.asarray(k_act))
            keys[tag].append(np.ascontiguousarray(np.stack(row), dtype=np.uint32))
    noisy = {"A": [i["info"]["noisy_state"] for i in inst_a], "B": [i["info"]["noisy_state"] for i in inst_b]}

    def build():
        cp0 = inst_a[0]["cp"]
        A = cm.controllers.BatchedCoVOController(env, 3, 256, 32, 0.01, discount=cp0.discount, gamma_mean=cp0.gamma_mean,
                                                 sample_sigma=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=DEV,
                                                 sigma_period=sigma_period)
        A.set_instances([i["state"] for i in inst_a], [i["params"] for i in inst_a])
        B = batched_controller(env, "mppi", inst_b, len(inst_b), 100, "0.01", set_instances=True, staged=True, gamma_sigma=0.0)
        assert A.core.uses_graph and B.core.uses_graph and B.staged
        return A, B

    def record(c):
        return dict(a_mean=c.a_mean.clone(), a=c._a.clone(), cost=c._cost.clone(), a_cov=c.a_cov.clone())

    A, B = build()
    ref = {"A": [], "B": [], "age": [], "L": []}
    for step in range(4):
        A(noisy["A"], keys["A"][step])
        ref["A"].append(record(A))
        ref["age"].append(A.sigma_age)
        ref["L"].append(A.core.sigma_factor(3))
        if sigma_period == 1:
            B(noisy["B"], keys["B"][step])
            ref["B"].append(record(B))
    assert ref["age"] == [step % sigma_period for step in range(4)]
    assert A.core.device_status() == 0 and B.core.device_status() == 0
    _close([], A, B)

    A, B = build()
    lib, h = A.core.lib, A.core.h
    _lib.check(lib.covo_set_step_batched_staged(h, 1), "covo_set_step_batched_staged")
    for step in range(4):
        for tag, c in (("A", A), ("B", B)):
            torch.stack([as_device_state(s, DEV).packed for s in noisy[tag]], out=c._states_buf)
            k = keys[tag][step].ctypes.data_as(C.POINTER(C.c_uint32))
            if tag == "A":
                _lib.check(lib.covo_mpc_step_batched(h, C.byref(A._args.base), A._params, k, A.core.stream()), "covo_mpc_step_batched")
                assert A.sigma_age == ref["age"][step], step
            elif sigma_period == 1:
                _lib.check(lib.covo_mpc_step_batched_mode(h, C.byref(B._args), B._params, k, A.core.stream()), "covo_mpc_step_batched_mode")
                assert torch.equal(A.core.sigma_factor(3), ref["L"][step]), step
            else:
                with pytest.raises(_lib.CovoError, match="the Sigma period .* belongs to covo-online steps"):
                    _lib.check(lib.covo_mpc_step_batched_mode(h, C.byref(B._args), B._params, k, A.core.stream()), "covo_mpc_step_batched_mode")
                continue
            for name, t in record(c).items():
                assert torch.equal(t, ref[tag][step][name]), (tag, step, name)
    assert A.core.device_status() == 0
    _close([], A, B)
