"""GPU (-m gpu): iterations per control step (covo_set_step_iters; iters= of the controllers).

The definition the code is held to: a step with raw key rng_act and iters = k runs k passes on its one state; pass 0 is today's step;
pass j >= 1 is today's step without the shift, from the mean pass j - 1 committed, with the raw key
key_j = split(split(key_{j-1})[0])[0] and the gamma_mean blend against its own starting mean.

Bars.  Actions, costs, a_cov (covo-online's Sigma, MPPI's shifted blocks) and iter_cost_min: torch.equal.  The mean of a fused pass
against the kernel-by-kernel composition: <= 5e-6 absolute, the bar of tests/test_gpu_parity.py::
test_fused_step_ragged_sizes_and_warm_lambda (the fused step forms the softmax from per-workgroup records shifted by their local cost
minimum, the stand-alone update shifts by the global minimum) -- so the composition cannot be chained bit for bit through k passes.
It is chained through the fused controllers themselves: a controller built with iters = j returns the mean after pass j - 1, and the
reference's pass j starts from that tensor (as the one-pass test re-seeds its twin with the fused mean after every step).  MPPI's
adapted covariances (gamma_sigma = 0.2) are a function of that mean: the same 5e-6."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.dynamics.dataclass import as_device_state  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from tests import iters_oracle as IO  # noqa: E402
from tests.gpu_cases import _batched_iters_case, _definition_case, _run_episode_case, iters_controller, iters_start  # noqa: E402
from tests.gpu_support import DEV, batched_controller, instances, quad_env  # noqa: E402
from tests.oracle_support import rel_err  # noqa: E402

MEAN_BAR = 5e-6  # test_fused_step_ragged_sizes_and_warm_lambda's (ragged sizes)
MEAN_BAR_4096 = 2e-6  # test_fused_step_equals_kernel_by_kernel's, which runs at N = 4096
SIZES = [("mppi", 100), ("mppi", 1024), ("covo-offline", 40), ("covo-offline", 4096), ("covo-online", 256)]


@pytest.mark.parametrize("graph", ["graph", "eager"])
@pytest.mark.parametrize("name,N", SIZES)
def test_iters_1_is_todays_step(name, N, graph, monkeypatch):
    """A controller built with iters=1 against one built without the argument, 3 consecutive steps: everything torch.equal."""
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    env = quad_env(task="hovering" if name == "mppi" else "tracking_zigzag")
    ca, cb = iters_controller(env, name, N, iters=1), iters_controller(env, name, N)
    assert ca.core.iter_cost_min is None and ca.core.uses_graph == (graph == "graph")
    cp, obs, info, state, params = iters_start(env, cb, name)
    cpa = cpb = cp
    key = cr.PRNGKey(6)
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        ua, cpa, ia = ca(obs, state, params, k_act, cpa, info)
        ub, cpb, ib = cb(obs, state, params, k_act, cpb, info)
        where = (name, N, graph, step)
        assert "iter_cost_min" not in ia and "iter_cost_min" not in ib
        assert torch.equal(cpa.a_mean, cpb.a_mean) and torch.equal(ua, ub), where
        assert torch.equal(ca.core.a, cb.core.a) and torch.equal(ca.core.cost, cb.core.cost), where
        assert torch.equal(cpa.a_cov, cpb.a_cov), where
        obs, state, _, _, info = env.step(k_step, state, ua.cpu().numpy(), params)
    assert ca.core.device_status() == 0
    ca.core.close(), cb.core.close()


@pytest.mark.parametrize("graph", ["graph", "eager"])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("name,N", SIZES)
def test_k_pass_step_equals_its_definition(name, N, k, graph, monkeypatch):
    _definition_case(name, N, k, graph, monkeypatch)


@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_k_pass_step_under_the_periodic_disturbance(graph, monkeypatch):
    """The key chain reaches the per-step tables: the Hessian's (raw key) and the rollouts' (step key) are rebuilt in every pass."""
    _definition_case("covo-online", 256, 2, graph, monkeypatch, disturb="periodic")


@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_k_pass_step_adapts_mppi_covariances_in_every_pass(graph, monkeypatch):
    _definition_case("mppi", 100, 2, graph, monkeypatch, gamma_sigma=0.2)


@pytest.mark.parametrize("E", [1, 5])
@pytest.mark.parametrize("name,N", [("mppi", 100), ("covo-offline", 40), ("covo-online", 256)])
def test_batched_iters_equal_replicas(name, N, E):
    _batched_iters_case(name, N, E, 2)


def test_run_episode_with_iters_equals_the_python_loop():
    _run_episode_case(2, 8)


def test_run_episode_batched_with_iters_equals_per_instance_loops():
    """covo_run_episode_batched_mode, 8 steps of MPPI N = 256 on E = 2 instances with iters=2, against per-instance Python loops of
    the single controller with iters=2 and the same keys: logs, final means, states and key chains bit-identical."""
    E, n, N = 2, 8, 256
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "mppi", N, "0.01", E, iters=2)
    params = [i["params"] for i in inst]
    b = batched_controller(env, "mppi", inst, len(inst), N, 0.01, iters=2)
    reset_keys = [cr.PRNGKey(150 + e) for e in range(E)]
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    rngs0 = np.stack([np.asarray(cr.PRNGKey(160 + e)) for e in range(E)])
    rngs = b.run_episode(ep, rngs0, n)
    log = ep.read_log()
    assert log.shape == (E, n, 4)
    for e, i in enumerate(inst):
        c = i["c"]
        c.alias_outputs = True
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        cp = c.reset(se.state0, params[e], c.init_control_params, cr.PRNGKey(250 + e))
        rng = rngs0[e]
        for _ in range(n):
            rng, rng_act, rng_step, rng_control = cr.split(rng, 4)
            u, cp, _ = c(None, None, params[e], rng_act, cp, {"noisy_state": se.noisy_state})
            se.step(rng_step, u)
            rng, rng_control = cr.split(rng)
        assert np.array_equal(se.read_log(), log[e]), e
        assert torch.equal(cp.a_mean.reshape(-1), b.a_mean[e]) and torch.equal(se.true, ep.true[e]), e
        assert torch.equal(cp.a_cov, b.a_cov[e]), e
        assert np.array_equal(np.asarray(rng, dtype=np.uint32), rngs[e]), e
        c.core.close()
    b.core.close()


@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_iters_next_to_the_other_options(graph, monkeypatch):
    """k = 2, covo-online N = 256, update="guarded", ess_min=16, diagnostics, plan and a fan of 4 all on: the rows describe the last
    pass, whose nominal is the mean pass 0 committed."""
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    name, N = "covo-online", 256
    env = quad_env(task="hovering" if name == "mppi" else "tracking_zigzag")
    opts = dict(update="guarded", ess_min=16.0, compute_diag=True, compute_plan=True, compute_fan=4)
    c2, c1 = iters_controller(env, name, N, iters=2, **opts), iters_controller(env, name, N, iters=1, **opts)
    cp, obs, info, state, params = iters_start(env, c1, name)
    key = cr.PRNGKey(6)
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        dstate = as_device_state(info["noisy_state"], DEV)
        u1, cp1, i1 = c1(obs, state, params, k_act, cp, info)  # pass 0 alone: its committed mean is pass 1's starting mean
        u2, cp2, i2 = c2(obs, state, params, k_act, cp, info)
        torch.cuda.synchronize()
        core, where = c2.core, (graph, step)
        start1 = cp1.a_mean.reshape(-1).contiguous().clone()
        pc = c2._params_c(params)
        row = core.arbitrate(dstate, pc, start1, cp2.a_mean.reshape(-1).contiguous().clone(), mask=0b010)
        arb = i2["arb_cost"]
        print(f"{where}: arb_cost {arb.tolist()} chosen {float(i2['arb_cost_chosen']):.6g} nominal recomputed {float(row[1]):.6g} "
              f"iter_cost_min {i2['iter_cost_min'].tolist()}")
        assert torch.equal(arb[1], row[1]), where  # the nominal candidate IS pass 1's starting mean
        assert float(i2["arb_cost_chosen"]) <= float(row[1]), where
        idx = i2["fan_idx"].long()
        assert torch.equal(i2["fan_cost"], core.cost[idx]), where
        prow = core.arbitrate(dstate, pc, start1, cp2.a_mean.reshape(-1).contiguous().clone(), mask=0b001)
        assert torch.equal(i2["cost_plan"], prow[0]), where  # the plan is the returned mean's
        assert torch.equal(i2["iter_cost_min"][1], core.cost.min()), where
        assert torch.equal(i2["iter_cost_min"][0], c1.core.cost.min()), where
        assert torch.equal(i2["cost_min"], core.cost.min()), where  # the diagnostics row is the last pass's
        assert core.device_status() == 0
        cp = cp2.replace(a_mean=cp2.a_mean.clone(), a_cov=cp2.a_cov.clone())
        obs, state, _, _, info = env.step(k_step, state, u2.cpu().numpy(), params)
    c1.core.close(), c2.core.close()


def test_refusals_name_the_condition_and_leave_the_handle_usable():
    env = quad_env(task="hovering")
    c = iters_controller(env, "mppi", 256, iters=2)
    lib, h = c.core.lib, c.core.h
    for bad in (0, 17, -3):
        assert lib.covo_set_step_iters(h, bad, _lib.ptr(c.core.iter_cost_min), 1) != 0
        assert b"outside [1, 16]" in lib.covo_last_error()
    cp, obs, info, state, params = iters_start(env, c, "mppi")
    u, cp, i = c(obs, state, params, cr.PRNGKey(9), cp, info)
    with pytest.raises(_lib.CovoError, match="covo_set_step_iters"):
        c.core.time_phases()
    assert lib.covo_set_step_iters(h, 1, None, 0) == 0  # off
    c.core.time_phases()
    assert c.core.device_status() == 0
    c.core.close()


@pytest.mark.parametrize("name", list(IO.CASES))
def test_two_pass_step_against_the_oracle(name):
    """k = 2, mppi N = 1 024 and covo-offline N = 2 048, gamma_mean = 0.8 (so that the blend against a pass's OWN starting mean
    shows), against the definition composed from oracle/ref_np.py in tests/iters_oracle.py: shift_mean once, then per pass
    sample_actions_* on the Philox normals of the pass's act_key (oracle/rng_np.py), the C fp64 rollout, softmax_update; keys by
    split(split(key)[0])[0].  Nothing of csrc/ is in the reference.  covo-offline samples from a fixed SPD table row known without a
    device.  The device's pass 0 is a controller with iters=1, its pass 1 the controller with iters=2.
    Bars, those of test_gpu_batched_modes.py::test_batched_mode_step_against_the_oracle: every cost within 1e-5 relative of the fp64
    rollout of the device's own actions (at most max(2, N // 4096) samples up to 1.5 x what the fp32 oracle loses), the new mean within
    1e-4 of the oracle chain's -- without that test's excuse for a small top-2 gap: the seeds are ones for which the fp32 and fp64
    oracle agree on the best sample of both passes (tests/test_iters_oracle_seeds.py, CPU; gaps printed below).  The actions against
    sample_actions_*: the device's normals differ from libm's by <= 2e-5 (test_randn_matches_philox_oracle...), which a row of L
    scales by its absolute sum; + 5e-6 for two 128-term fp32 sums; + in pass 1 the 1e-4 the starting means may differ by."""
    case = IO.CASES[name]
    N = case["N"]
    env = IO.make_env(name, DEV)
    obs, info, state, key = IO.problem(env, case["seed"])
    ns, params = info["noisy_state"], env.default_params
    c1, c2 = iters_controller(env, name, N, iters=1), iters_controller(env, name, N, iters=2)
    cp = c1.init_control_params.replace(gamma_mean=IO.GAMMA)
    assert np.array_equal(cp.a_mean.cpu().numpy(), IO.hover_mean(env)) and float(cp.sample_sigma) == IO.SIGMA
    if name == "covo-offline":
        S = IO.offline_sigma()
        L = np.linalg.cholesky(S.astype(np.float64)).astype(np.float32)
        cp = cp.replace(a_cov_offline=torch.from_numpy(np.stack([S, S])).to(DEV), a_chol_offline=torch.from_numpy(np.stack([L, L])).to(DEV))
        lsum = float(np.abs(L).sum(axis=1).max())
    else:
        lsum = IO.SIGMA
    a_bar = 2e-5 * lsum + 5e-6
    ref = IO.oracle_chain(name, env, ns, cp.a_mean.cpu().numpy(), key, 2, np.float64)
    so, po = IO.oracle_state(ns), R.Params().fp32()
    outs = [c(obs, state, params, key, cp, info) for c in (c1, c2)]
    torch.cuda.synchronize()
    assert ns.time == 0
    for j, (c, (u, cpj, ij)) in enumerate(zip((c1, c2), outs)):
        a_ref, cost_ref, mean_ref = ref[j]
        a_dev = c.core.a.permute(1, 0, 2).contiguous().cpu().numpy().astype(np.float64)
        cost_dev = c.core.cost.cpu().numpy()
        aerr = float(np.abs(a_dev - a_ref).max())
        _, fs = IO.pass_inputs(name, env, key if j == 0 else IO.next_raw_key(key), N)
        cost_own = CO.rollout(so, po, a_dev, 1.0, fs, dtype=np.float64)
        rel = rel_err(cost_dev, cost_own)
        bar = 1e-5
        if rel.max() >= bar:
            c32 = CO.rollout(so.astype(np.float32), po, a_dev.astype(np.float32), 1.0, fs.astype(np.float32), dtype=np.float32)
            bar = max(bar, 1.5 * rel_err(c32, cost_own).max())
            assert int((rel >= 1e-5).sum()) <= max(2, N // 4096), (name, j, int((rel >= 1e-5).sum()))
        gap = float(np.diff(np.sort(cost_ref)[:2])[0])
        merr = float(np.abs(cpj.a_mean.cpu().numpy() - mean_ref).max())
        print(f"{name} N={N} pass {j}: |a - oracle| {aerr:.3e} (bar {a_bar + 1e-4 * j:.3e}), max rel cost err {rel.max():.3e}, "
              f"mean err {merr:.3e}, top-2 gap {gap:.3e}, best sample device {int(np.argmin(cost_dev))} oracle {int(np.argmin(cost_ref))}")
        assert aerr <= a_bar + 1e-4 * j, (name, j, aerr)
        assert rel.max() < bar, (name, j, rel.max(), bar)
        assert int(np.argmin(cost_dev)) == int(np.argmin(cost_ref)), (name, j)
        assert merr < 1e-4, (name, j, merr, gap)
        assert torch.equal(u, cpj.a_mean[0])
    icm = outs[1][2]["iter_cost_min"].cpu().numpy()
    assert rel_err(icm, np.array([ref[0][1].min(), ref[1][1].min()])).max() < 1e-5, icm
    # the passes are distinguishable: pass 1 did not shift (its start is pass 0's mean) and drew from the advanced key
    assert np.abs(ref[1][2] - ref[0][2]).max() > 1e-3 and np.abs(ref[0][0] - ref[1][0]).max() > 0.1
    c1.core.close(), c2.core.close()


def test_sharded_step_is_refused_by_the_library():
    """covo_mpc_step on a handle with iterations attached and partial_out != NULL (a sample-sharded step): COVO_E_BADARG naming the
    condition, before any launch; the handle steps on once the log is detached."""
    env = quad_env(task="hovering")
    c = iters_controller(env, "mppi", 256, iters=2)
    cp, obs, info, state, params = iters_start(env, c, "mppi")
    c(obs, state, params, cr.PRNGKey(9), cp, info)
    pc, args = c.core._last_step
    import ctypes as C
    args.partial_out = c.core.partial.data_ptr()
    rc = c.core.lib.covo_mpc_step(c.core.h, C.byref(pc), C.byref(args), 1, 2, None, c.core.stream())
    assert rc != 0 and b"not available for sample-sharded steps" in c.core.lib.covo_last_error()
    args.partial_out = None
    assert c.core.lib.covo_mpc_step(c.core.h, C.byref(pc), C.byref(args), 1, 2, None, c.core.stream()) == 0
    torch.cuda.synchronize()
    assert c.core.device_status() == 0
    c.core.close()
