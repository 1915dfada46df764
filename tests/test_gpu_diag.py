"""GPU tests (-m gpu) of the per-step sampling diagnostics (covo_set_step_diag / covo_set_episode_diag_log; `compute_diag`):
{ess, cost_min, cost_weighted, cost_mean, weight_sum, n_samples, 0, 0} per control step and instance, formed by the softmax
update's own launches (csrc/rollout_common.hpp: rollout_record, csrc/reduce.hip, csrc/softmax_merge.hpp: merge_body).

Bars of the comparison against numpy fp64 on the device's own fp32 costs: cost_min exact; cost_weighted, cost_mean, weight_sum
1e-5 relative (the project's bar for the softmax update; relative as everywhere in this suite: |x - ref| / max(|ref|, 1));
ess 3e-5 (s^2 / s2: twice the error of s plus that of s2).  lambda reaches the kernels as the float 1 / lam: the reference uses
the same float.
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
from tests.gpu_support import DEV, batched_controller, instances, quad_env, set_time, single_controller  # noqa: E402
from tests.oracle_support import rel_err_scalar  # noqa: E402

BARS = {"ess": 3e-5, "cost_weighted": 1e-5, "cost_mean": 1e-5, "weight_sum": 1e-5}


def _reference(cost_f32, lam):
    """The four quantities and weight_sum in numpy fp64 from exactly the fp32 costs of the step."""
    inv = np.float64(np.float32(1.0) / np.float32(lam))
    c = cost_f32.astype(np.float64)
    m = c.min()
    w = np.exp(-(c - m) * inv)
    s = w.sum()
    return dict(ess=s * s / (w * w).sum(), cost_min=m, cost_weighted=(w * c).sum() / s, cost_mean=c.mean(), weight_sum=s)


def _check_against_fp64(diag_row, cost, lam, where):
    d = diag_row.cpu().numpy()
    c = cost.cpu().numpy()
    ref = _reference(c, lam)
    got = dict(zip(_lib.DIAG_FIELDS, d[:6]))
    errs = {k: rel_err_scalar(got[k], ref[k]) for k in BARS}
    print(f"  {where}: ess {got['ess']:.6g} (ref {ref['ess']:.6g}) errs " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert np.float32(ref["cost_min"]) == got["cost_min"], (where, got["cost_min"], ref["cost_min"])
    for k, bar in BARS.items():
        assert errs[k] <= bar, (where, k, errs[k], bar, got[k], ref[k])
    assert got["n_samples"] == float(c.size) and d[6] == 0.0 and d[7] == 0.0, (where, d)
    return errs


SIZES = {"mppi": [40, 1024, 8192, 65536], "covo-offline": [40, 1024, 8192, 65536], "covo-online": [40, 1024, 8192, 65536]}
CASES = [(n, N) for n in ("mppi", "covo-offline", "covo-online") for N in SIZES[n]]


@pytest.mark.parametrize("name,N", CASES)
@pytest.mark.parametrize("lam", ["0.01", "5.0"])
@pytest.mark.parametrize("rollover", [False, True])
@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_diag_against_fp64_on_the_device_costs(name, N, lam, rollover, graph, monkeypatch):
    """Three closed-loop steps (eager first call, capture, replay -- or three eager calls); after each, the step's cost buffer is
    read back and the diagnostics compared with numpy fp64 on exactly those costs.  N = 40 .. 8 192: the fused small step (MPPI,
    covo-offline) and the record-leaving rollout (covo-online); N = 65 536: the record-leaving rollout for all three.  The
    stand-alone stage 1 (more workgroups than records) is test_diag_standalone_stage1.  Measured maxima: DESIGN 4.7."""
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag", rollover=rollover)
    c, cp, obs, info, state, params = single_controller(env, name, N, lam=lam, compute_diag=True)
    key = cr.PRNGKey(3)
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        u, cp, cinfo = c(obs, state, params, k_act, cp, info)
        torch.cuda.synchronize()
        assert set(cinfo) >= {"ess", "cost_min", "cost_weighted", "cost_mean"} and cinfo["ess"].dim() == 0
        assert cinfo["ess"].data_ptr() == c.core.diag.data_ptr()  # a view: no copy
        _check_against_fp64(c.core.diag[0], c.core.cost, lam, (name, N, lam, rollover, graph, step))
        obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
    assert c.core.device_status() == 0
    c.core.close()


@pytest.mark.parametrize("name", ["mppi", "covo-online"])
@pytest.mark.parametrize("lam", ["0.01", "5.0"])
def test_diag_standalone_stage1(name, lam, monkeypatch):
    """N = 300 000: the rollout has more workgroups than the merge takes records, so the stand-alone stage-1 kernel
    (reduce.hip: softmax_partial_diag_kernel) forms the sums."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    N = 300000
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, name, N, lam=lam, compute_diag=True)
    key = cr.PRNGKey(5)
    for step in range(2):
        key, k_act, k_step = cr.split(key, 3)
        u, cp, _ = c(obs, state, params, k_act, cp, info)
        torch.cuda.synchronize()
        _check_against_fp64(c.core.diag[0], c.core.cost, lam, (name, N, lam, "standalone", step))
        obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
    c.core.close()


def test_diag_mppi_covariance_adaptation(monkeypatch):
    """MPPI with gamma_sigma != 0 runs its own stage 1 and merge (second moments): the diagnostics come from the same records."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, "mppi", 4096, compute_diag=True)
    cp = cp.replace(gamma_sigma=0.1)
    u, cp, _ = c(obs, state, params, cr.PRNGKey(9), cp, info)
    torch.cuda.synchronize()
    _check_against_fp64(c.core.diag[0], c.core.cost, "0.01", ("mppi", 4096, "gamma_sigma"))
    c.core.close()


@pytest.mark.parametrize("name,N", [("mppi", 1024), ("covo-offline", 4096), ("covo-online", 65536), ("covo-online", 300000)])
def test_known_answer_frozen_rewards(name, N, monkeypatch):
    """A state outside the 3 m box: every rollout terminates at step 0, every reward is frozen, all costs are equal --
    ess == N, weight_sum == N (sums of ones, exact below 2^24), cost_min == cost_weighted == cost_mean, exactly."""
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, name, N, compute_diag=True)
    ns = info["noisy_state"]
    info = dict(info, noisy_state=ns.replace(pos=np.array([5.0, 0.0, 0.0], dtype=np.float32)))
    c(obs, state, params, cr.PRNGKey(4), cp, info)
    torch.cuda.synchronize()
    cost = c.core.cost.cpu().numpy()
    assert (cost == cost[0]).all()
    d = c.core.diag[0].cpu().numpy()
    assert d[0] == float(N) and d[4] == float(N) and d[5] == float(N), d
    assert d[1] == d[2] == d[3] == cost[0], d
    assert d[6] == 0.0 and d[7] == 0.0
    c.core.close()


@pytest.mark.parametrize("name", ["mppi", "covo-offline", "covo-online"])
def test_known_answer_one_sample(name, monkeypatch):
    monkeypatch.setenv("COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    c, cp, obs, info, state, params = single_controller(env, name, 1, compute_diag=True)
    c(obs, state, params, cr.PRNGKey(4), cp, info)
    torch.cuda.synchronize()
    d = c.core.diag[0].cpu().numpy()
    cost = c.core.cost.cpu().numpy()
    assert d[0] == 1.0 and d[4] == 1.0 and d[5] == 1.0 and d[1] == d[2] == d[3] == cost[0], d
    c.core.close()


@pytest.mark.parametrize("name,N", [("mppi", 1024), ("covo-offline", 1024), ("covo-online", 2048), ("covo-online", 65536)])
@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_nothing_else_moves(name, N, graph, monkeypatch):
    """Two controllers on the same inputs, one with compute_diag: a_mean, the actions, the costs and a_cov are torch.equal over
    three consecutive steps."""
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    A = single_controller(env, name, N, compute_diag=True)
    B = single_controller(env, name, N)
    ca, cpa, obs, info, state, params = A
    cb, cpb = B[0], B[1]
    key = cr.PRNGKey(11)
    for step in range(3):
        key, k_act, k_step = cr.split(key, 3)
        ua, cpa, ia = ca(obs, state, params, k_act, cpa, info)
        ub, cpb, ib = cb(obs, state, params, k_act, cpb, info)
        torch.cuda.synchronize()
        where = (name, N, graph, step)
        assert "ess" in ia and "ess" not in ib
        assert torch.equal(cpa.a_mean, cpb.a_mean) and torch.equal(ua, ub), where
        assert torch.equal(ca.core.a, cb.core.a) and torch.equal(ca.core.cost, cb.core.cost), where
        assert torch.equal(cpa.a_cov, cpb.a_cov), where
        obs, state, _, _, info = env.step(k_step, state, ua.cpu().numpy(), params)
    assert ca.core.device_status() == 0
    ca.core.close()
    cb.core.close()


_TABLES = {}


def _offline_tables(inst, E):
    out = []
    for e, i in enumerate(inst):
        if e not in _TABLES:
            cp = i["c"].reset(i["state"], i["params"], i["c"].init_control_params, i["reset_key"])
            _TABLES[e] = (cp.a_cov_offline, cp.a_chol_offline)
        out.append(_TABLES[e])
        i["cp"] = i["cp"].replace(a_cov_offline=out[-1][0], a_chol_offline=out[-1][1])
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


@pytest.mark.parametrize("name,N", [("mppi", 1024), ("covo-offline", 1024), ("covo-online", 1024)])
@pytest.mark.parametrize("E", [1, 5, 32])
def test_batched_diag_equals_single(name, N, E):
    """Row e of the batched controller's `diag` is torch.equal to the single controller's diagnostics on instance e alone, over
    three steps (eager call, capture, replay)."""
    lam = "0.01"
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, name, N, lam, E, compute_diag=True)
    b = batched_controller(env, name, inst, len(inst), N, lam, compute_diag=True)
    b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    if name == "covo-offline":
        b.set_tables(*_offline_tables(inst, E))
    assert tuple(b.diag.shape) == (E, 8)
    for step in range(3):
        k_acts = []
        for i in inst:
            i["key"], k_act, i["k_step"] = cr.split(i["key"], 3)
            k_acts.append(np.asarray(k_act))
        b([i["info"]["noisy_state"] for i in inst], np.stack(k_acts))
        for e, i in enumerate(inst):
            u, i["cp"], _ = i["c"](i["obs"], i["state"], i["params"], k_acts[e], i["cp"], i["info"])
            where = (name, N, E, step, e)
            assert torch.equal(b._cost[e], i["c"].core.cost), where
            assert torch.equal(b.diag[e], i["c"].core.diag[0]), (where, b.diag[e], i["c"].core.diag[0])
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u.cpu().numpy(), i["params"])
    _check_against_fp64(b.diag[E - 1], b._cost[E - 1], lam, (name, N, E, "batched"))
    assert b.core.device_status() == 0
    for i in inst:
        i["c"].core.close()
    b.core.close()


@pytest.mark.parametrize("name", ["covo-online", "mppi"])
def test_closed_loop_batched_diag_log(name):
    """run_episode for 40 steps on 3 instances, instance 1 starting at step 285 (frozen-reward tail from `time + k >= 300`, then
    an auto-reset inside the segment): read_diag() has one row per step and instance, bit-equal to step-by-step __call__ +
    episode.step with the same keys; the [.., 4] log equals the log of the same episode without diagnostics.  Expected from the
    reward freeze: the late instance's ESS grows through the tail and falls back after the reset -- asserted as: its largest ESS
    lies in a row before its reset row and exceeds the ESS of its first row after the reset.
    Which row is "the reset row": control step k runs BEFORE env step k, and the env step whose pre-step state is terminal
    (log row k: done = 1) is the one that resets.  The first control step that plans from the reset state is therefore row
    k + 1 -- that is the reset row here; row k itself still plans from the terminal state (time = 300).  Observed on the MI355X
    (covo-online, N = 1 024, lambda = 0.01, start at step 285): ESS 1.8, 3.2, 23.0, 172.8 in rows 11-14, exactly N = 1 024 in
    row 15 (done = 1: every reward frozen, the blind-controller signature), 1.0 in row 16.  With the log's done row taken as
    the reset row instead, the maximum would lie IN that row, not before it: the finding is recorded in DESIGN 4.7."""
    from covo_mpc_amd.envs.quadrotor import BatchedDeviceEpisode
    E, N, lam, T = 3, 1024, "0.01", 40
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, name, N, lam, E, seed=3, compute_diag=True)
    for i in inst:
        i["c"].core.close()
    keys = np.stack([np.asarray(cr.PRNGKey(50 + e)) for e in range(E)])
    rngs = np.stack([np.asarray(cr.PRNGKey(70 + e)) for e in range(E)])
    params = [i["params"] for i in inst]
    out = {}
    for kind in ("episode", "steps", "plain"):
        b = batched_controller(env, name, inst, len(inst), N, lam, compute_diag=kind != "plain")
        ep = BatchedDeviceEpisode(env, keys, params, (b.core.lib, b.core.h), b.core.device)
        set_time(ep, 1, 285)
        if kind == "steps":
            b.bind_episode(ep)
            ks, rows = rngs.copy(), []
            for t in range(T):
                nxt, acts, stepk = [], [], []
                for e in range(E):  # run_one_step's key threading (quadrotor.py:520-538)
                    k4 = cr.split(ks[e], 4)
                    acts.append(np.asarray(k4[1]))
                    stepk.append(np.asarray(k4[2]))
                    nxt.append(np.asarray(cr.split(k4[0])[0]))
                b(None, np.stack(acts))
                rows.append(b.diag.clone())
                ep.step(np.stack(stepk), b.a_mean)
                ks = np.stack(nxt)
            out[kind] = (torch.stack(rows, dim=1).cpu().numpy(), ep.read_log())
        else:
            b.run_episode(ep, rngs.copy(), T // 2)
            b.run_episode(ep, rngs_after(rngs, T // 2), T - T // 2)
            log = ep.read_log()
            out[kind] = (ep.read_diag() if kind == "episode" else None, log)
        assert b.core.device_status() == 0
        b.core.close()
    d_ep, log_ep = out["episode"]
    d_st, log_st = out["steps"]
    assert d_ep.shape == (E, T, 8)
    assert np.array_equal(log_ep, out["plain"][1]) and np.array_equal(log_ep, log_st)
    assert np.array_equal(d_ep, d_st)
    done = log_ep[1, :, 3]
    done_row = int(np.argmax(done > 0))
    assert done[done_row] > 0 and 0 < done_row < T - 1, done
    reset_row = done_row + 1  # the first control step that plans from the reset state (see the docstring)
    ess = d_ep[1, :, 0]
    print(f"  {name}: late instance: done in row {done_row}; ess rows: " + " ".join(f"{v:.1f}" for v in ess))
    assert int(np.argmax(ess)) < reset_row and ess.max() > ess[reset_row], (reset_row, ess)


def rngs_after(rngs, n):
    """the instances' chain keys after n steps of run_one_step (rng = split(split(rng, 4)[0])[0])."""
    out = []
    for k in rngs:
        for _ in range(n):
            k = np.asarray(cr.split(cr.split(k, 4)[0])[0])
        out.append(k)
    return np.stack(out)


def test_closed_loop_single_diag_log(monkeypatch):
    """covo_run_episode under a single controller with diagnostics, in two segments: one row per step, bit-equal to step-by-step
    __call__ + episode.step; the [.., 4] log equals the log without diagnostics."""
    from covo_mpc_amd.envs.quadrotor import DeviceEpisode
    monkeypatch.setenv("COVO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    T, N = 40, 2048
    out = {}
    for kind in ("episode", "steps", "plain"):
        c, cp, _, _, _, params = single_controller(env, "covo-online", N, compute_diag=kind != "plain")
        c.alias_outputs = True
        ep = DeviceEpisode(env, cr.PRNGKey(21), params, (c.core.lib, c.core.h), c.core.device)
        cp = c.reset(ep.state0, params, cp, cr.PRNGKey(22))
        rng = cr.PRNGKey(23)
        if kind == "steps":
            rows = []
            for _ in range(T):
                rng, rng_act, rng_step, _ = cr.split(rng, 4)
                u, cp, ci = c(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                rows.append(c.core.diag[0].clone())
                ep.step(rng_step, u)
                rng, _ = cr.split(rng)
            out[kind] = (torch.stack(rows).cpu().numpy(), ep.read_log())
        else:
            cp, rng = c.run_episode(ep, params, cp, rng, 15)
            cp, rng = c.run_episode(ep, params, cp, rng, T - 15)
            log = ep.read_log()
            out[kind] = (ep.read_diag() if kind == "episode" else None, log)
        assert c.core.device_status() == 0
        c.core.close()
    assert out["episode"][0].shape == (T, 8)
    assert np.array_equal(out["episode"][1], out["plain"][1]) and np.array_equal(out["episode"][1], out["steps"][1])
    assert np.array_equal(out["episode"][0], out["steps"][0])


@pytest.mark.parametrize("name,N", [("covo-offline", 1024), ("covo-online", 4096)])
def test_attach_detach(name, N, monkeypatch):
    """Diagnostics turned on after the graph was captured, off again, on with another buffer: every call returns correct values,
    the device status stays 0, the outputs stay bit-identical to a handle that never had them."""
    monkeypatch.setenv("COVO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    ca, cpa, obs, info, state, params = single_controller(env, name, N)
    cb, cpb = single_controller(env, name, N)[:2]
    lib, h = ca.core.lib, ca.core.h
    bufs = [torch.full((1, 8), -1.0, device=DEV), torch.full((1, 8), -1.0, device=DEV)]
    # steps 0-2 off (eager, capture, replay), 3-4 on (buffer 0), 5-6 off, 7-9 on (buffer 1)
    plan = {3: bufs[0], 5: None, 7: bufs[1]}
    cur = None
    key = cr.PRNGKey(31)
    for step in range(10):
        if step in plan:
            cur = plan[step]
            _lib.check(lib.covo_set_step_diag(h, _lib.ptr(cur), 1), "covo_set_step_diag")
            for t in bufs:
                t.fill_(-1.0)
        key, k_act, k_step = cr.split(key, 3)
        ua, cpa, _ = ca(obs, state, params, k_act, cpa, info)
        ub, cpb, _ = cb(obs, state, params, k_act, cpb, info)
        torch.cuda.synchronize()
        where = (name, N, step)
        assert torch.equal(cpa.a_mean, cpb.a_mean) and torch.equal(ca.core.cost, cb.core.cost), where
        assert torch.equal(ca.core.a, cb.core.a), where
        for t in bufs:
            if t is cur:
                _check_against_fp64(t[0], ca.core.cost, "0.01", where)
            else:
                assert (t == -1.0).all(), where  # a detached buffer is never written
        assert ca.core.device_status() == 0, where
        obs, state, _, _, info = env.step(k_step, state, ua.cpu().numpy(), params)
    ca.core.close()
    cb.core.close()


def test_sharded_step_with_diag_is_refused():
    """partial_out != NULL with diagnostics attached: an error that names sample-sharded steps; the handle works afterwards."""
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.dynamics.dataclass import as_device_state
    core = SamplingCore(4096, 32, 0.01, 1.0, device=DEV, use_graph=False, compute_diag=True)
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(3), params)
    dstate = as_device_state(info["noisy_state"], DEV)
    pc = params.to_c()
    g = torch.Generator().manual_seed(0)
    A = torch.randn(3, 128, 128, generator=g, dtype=torch.float64)
    L = torch.linalg.cholesky(0.05 * A @ A.transpose(1, 2) + 0.2 * torch.eye(128, dtype=torch.float64)).float().to(DEV).contiguous()
    a_mean = (0.1 * torch.randn(128, generator=g)).to(DEV)
    args, am, am_shift, _ = core._prepare_step(_lib.MODE_COVO_OFFLINE, dstate, a_mean, L_table=L, derive_keys=True)
    rec = torch.zeros(_lib.COVO_PARTIAL_FLOATS, device=DEV)
    args.partial_out = rec.data_ptr()
    rc = core.lib.covo_mpc_step(core.h, C.byref(pc), C.byref(args), 7, 9, None, core.stream())
    assert rc != 0 and b"sample-sharded" in core.lib.covo_last_error()
    args.partial_out = None
    _lib.check(core.lib.covo_mpc_step(core.h, C.byref(pc), C.byref(args), 7, 9, None, core.stream()), "covo_mpc_step")
    torch.cuda.synchronize()
    _check_against_fp64(core.diag[0], core.cost, "0.01", "after the refusal")
    assert core.device_status() == 0
    core.close()
