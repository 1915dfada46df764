"""GPU tests (-m gpu) of the episode logs of the step attachments' rows (covo_set_episode_rows, csrc/episode_rows.hip):
`lamlog`, `elitelog`, `iterlog`, `sigmalog`, `postlog` and `postcovlog` of an episode run by covo_run_episode, covo_run_episode_batched
and covo_run_episode_batched_mode.

The logs are copies: every comparison is np.array_equal on uint32 views, against the rows cloned from the core's own buffers after every
step of a Python loop that threads the keys as the drivers do (tests/test_gpu_sigma_adapt.py::test_run_episode_equals_the_python_loop).
Shapes: N <= 256, at most 8 steps, tracking_zigzag under the gaussian disturbance.  Section 7: all ten logs of the handle's one table
at once -- the four with setters of their own (`diag_log`, `trace`, `fanlog`, `arblog`) next to the six -- at N = 1 024, 5 steps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd._lib import CovoError, check, ptr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from tests.gpu_support import DEV, H, bits, quad_env  # noqa: E402


def same_bits(got, want, where):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (where, g.shape, w.shape)
    assert np.array_equal(g, w), (where, int((g != w).sum()), "words differ")


def sigma_row(age, adapt_row):
    """the Sigma log's row of a step that ran at `age` and left Sigma adapt's row `adapt_row` (device tensor [4], or None)"""
    rest = adapt_row[:3].detach().cpu().numpy() if adapt_row is not None else np.array([0.0, 1.0, 0.0], dtype=np.float32)
    return np.concatenate([np.array([float(age)], dtype=np.float32), rest.astype(np.float32)])


def _single(env, name, N, **kw):
    c, _ = cm.envs.get_controller(env, name, f"N{N}_H32_lam0.01", device=DEV, compute_info=False, **kw)
    c.alias_outputs = True
    return c, c.init_control_params, env.default_params


def _run_single(env, name, N, segments, rows_of, opts, log_post_cov=False):
    """-> (the episode of the driver's run, its core (still open: the episode's read_* ask the handle for its status; the caller closes
    it), the Python loop's rows per step, both env logs)"""
    T = sum(segments)
    out = {}
    for kind in ("episode", "steps"):
        c, cp, params = _single(env, name, N, **opts)
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(21), params, (c.core.lib, c.core.h), c.core.device, log_post_cov=log_post_cov)
        cp = c.reset(ep.state0, params, cp, cr.PRNGKey(22))
        rng = cr.PRNGKey(23)
        if kind == "steps":
            rows = []
            for t in range(T):
                rng, rng_act, rng_step, _ = cr.split(rng, 4)
                u, cp, ci = c(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                rows.append(rows_of(c.core, dict(ci, episode=ep, u=u)))  # (the trace row holds the states entering the env step and u)
                ep.step(rng_step, u)
                rng, _ = cr.split(rng)
            out[kind] = (rows, ep.read_log())
            assert c.core.device_status() == 0
            c.core.close()
        else:
            for n in segments:
                cp, rng = c.run_episode(ep, params, cp, rng, n)
            out[kind] = (ep, ep.read_log(), c.core)
    return out["episode"][0], out["episode"][2], out["steps"][0], out["episode"][1], out["steps"][1]


# ---- 1. single covo-online: every kind but the elite set's, two segments, both step paths ----------------------------------------------
@pytest.mark.parametrize("graph", ["graph", "eager"])
def test_single_covo_online_logs_equal_the_python_loop(graph, monkeypatch):
    """N = 256, ess_min = 8, iters = 3, m = 3, gamma = 0.2, the matrix log on; 7 steps as 2 + 5.  The second segment's iteration log
    starts 2 x 3 floats into the buffer: 24 bytes, the float-by-float path at an address that is not 16-byte aligned."""
    monkeypatch.setenv("COVO_GRAPH" if graph == "graph" else "COVO_NO_GRAPH", "1")
    env = quad_env(task="tracking_zigzag")
    m, T = 3, 7

    def rows_of(core, ci):
        return dict(lam=core.lam_eff[0].clone(), iters=core.iter_cost_min[0].clone(), age=int(ci["sigma_age"]),
                    adapt=core.sigma_adapt_rows[0].clone(), aux=core.post_aux[0].clone(), cov=core.post_cov[0].clone())

    ep, core, rows, log_ep, log_steps = _run_single(env, "covo-online", 256, (2, 5), rows_of,
                                                    dict(ess_min=8, iters=3, sigma_period=m, sigma_adapt=0.2), log_post_cov=True)
    assert np.array_equal(log_ep, log_steps)
    assert tuple(ep.iterlog.shape) == (ep.log.shape[0], 3) and tuple(ep.postcovlog.shape) == (ep.log.shape[0], 128 * 128)
    assert (ep.iterlog[2:].data_ptr() % 16) == 8  # the scalar path's unaligned segment
    assert ep.elitelog is None
    assert [r["age"] for r in rows] == [t % m for t in range(T)]
    same_bits(ep.lamlog[:T], torch.stack([r["lam"] for r in rows]), "lamlog")
    same_bits(ep.iterlog[:T], torch.stack([r["iters"] for r in rows]), "iterlog")
    same_bits(ep.sigmalog[:T], np.stack([sigma_row(r["age"], r["adapt"]) for r in rows]), "sigmalog")
    same_bits(ep.postlog[:T], torch.stack([r["aux"] for r in rows]), "postlog")
    same_bits(ep.postcovlog[:T].view(T, 128, 128), torch.stack([r["cov"] for r in rows]), "postcovlog")
    for name in ("lamlog", "iterlog", "sigmalog", "postlog", "postcovlog"):
        assert not bits(getattr(ep, name)[T:]).any(), name  # rows 7 .. were never written
    sg, post = ep.read_sigma(), ep.read_post()
    assert sg["age"].dtype == np.int32 and sg["age"].tolist() == [t % m for t in range(T)]
    assert np.all(sg["scale"][[0, 3, 6]] == 1.0) and np.all(sg["scale"][[1, 2, 4, 5]] != 1.0)  # refresh steps do not adapt
    assert post["cov"].shape == (T, 128, 128) and post["shift"].shape == (T, 128) and post["weight"].shape == (T,)
    cov = bits(post["cov"])
    assert np.array_equal(cov, cov.transpose(0, 2, 1))  # symmetric bit for bit
    lam = ep.read_lam()
    assert tuple(lam) == _lib.LAM_FIELDS and lam["lam_eff"].shape == (T,) and np.all(lam["lam_eff"] > 0.0)
    assert ep.read_iters().shape == (T, 3)
    with pytest.raises(RuntimeError, match="elite"):
        ep.read_elite()
    assert core.device_status() == 0
    core.close()


def test_single_episode_without_log_post_cov_keeps_the_side_row_only():
    env = quad_env(task="tracking_zigzag")
    c, cp, params = _single(env, "covo-online", 256, compute_post_cov=True)
    ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(21), params, (c.core.lib, c.core.h), c.core.device)
    cp = c.reset(ep.state0, params, cp, cr.PRNGKey(22))
    c.run_episode(ep, params, cp, cr.PRNGKey(23), 2)
    post = ep.read_post()
    assert sorted(post) == ["shift", "weight"] and ep.postcovlog is None and post["shift"].shape == (2, 128)
    same_bits(ep.postlog[1], c.core.post_aux[0], "the last step's side row")
    with pytest.raises(RuntimeError, match="sigma_period"):
        ep.read_sigma()
    assert c.core.device_status() == 0
    c.core.close()


# ---- 2. single MPPI: a ragged N, the elite set, width 5 ----------------------------------------------------------------------------
def test_single_mppi_elite_and_iteration_logs_equal_the_python_loop():
    env = quad_env(task="tracking_zigzag")
    T = 5

    def rows_of(core, ci):
        return dict(elite=core.elite_rows[0].clone(), iters=core.iter_cost_min[0].clone())

    ep, core, rows, log_ep, log_steps = _run_single(env, "mppi", 100, (T,), rows_of, dict(elite=16, iters=5))
    assert np.array_equal(log_ep, log_steps)
    assert tuple(ep.iterlog.shape) == (ep.log.shape[0], 5) and ep.lamlog is None and ep.sigmalog is None and ep.postlog is None
    same_bits(ep.elitelog[:T], torch.stack([r["elite"] for r in rows]), "elitelog")
    same_bits(ep.iterlog[:T], torch.stack([r["iters"] for r in rows]), "iterlog")
    assert not bits(ep.elitelog[T:]).any() and not bits(ep.iterlog[T:]).any()
    el = ep.read_elite()
    assert el["threshold_index_word"].dtype == np.uint32 and np.all(el["threshold_index_word"] < 100) and np.all(el["K"] == 16.0)
    assert np.all(el["cost_min"] <= el["cost_kth"])
    assert core.device_status() == 0
    core.close()


# ---- 3. batched covo-online ----------------------------------------------------------------------------------------------------------
def _batch_setup(E):
    env = quad_env(task="tracking_zigzag", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    rngs0 = np.stack([np.asarray(cr.PRNGKey(60 + e)) for e in range(E)])
    c0, _ = cm.envs.get_controller(env, "covo-online", "N256_H32_lam0.01", device=DEV, compute_info=False)
    cp0 = c0.init_control_params
    c0.core.close()
    return env, params, reset_keys, rngs0, cp0


def _run_batched(make, env, params, reset_keys, rngs0, segments, rows_of):
    E, T = len(params), sum(segments)
    out = {}
    for kind in ("episode", "steps"):
        b = make()
        ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
        if kind == "steps":
            b.bind_episode(ep)
            rngs, rows = [rngs0[e] for e in range(E)], []
            for _ in range(T):
                sp = [cr.split(r, 4) for r in rngs]
                b(None, np.stack([np.asarray(x[1]) for x in sp]))
                rows.append(rows_of(b))
                ep.step(np.stack([np.asarray(x[2]) for x in sp]), b.a_mean)
                rngs = [cr.split(x[0])[0] for x in sp]
            out[kind] = (rows, ep.read_log())
            assert b.core.device_status() == 0
            b.core.close()
        else:
            keys = rngs0.copy()
            for n in segments:
                keys = b.run_episode(ep, keys, n)
            out[kind] = (ep, ep.read_log(), b.core)
    return out["episode"][0], out["episode"][2], out["steps"][0], out["episode"][1], out["steps"][1]


def test_batched_covo_online_logs_equal_the_python_loop():
    """E = 3 domain-randomised instances, N = 256, elite = 32, m = 2, gamma = 0.2, 6 steps as 4 + 2 of a log of T + 1 rows per instance:
    a copy that confused the instance stride with the steps run would land in another row."""
    E, T, m = 3, 6, 2
    env, params, reset_keys, rngs0, cp0 = _batch_setup(E)

    def make():
        return cm.controllers.BatchedCoVOController(env, E, 256, H, 0.01, discount=cp0.discount, gamma_mean=cp0.gamma_mean,
                                                    sample_sigma=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=DEV, elite=32,
                                                    sigma_period=m, sigma_adapt=0.2)

    def rows_of(b):
        return dict(elite=b.elite.clone(), age=b.sigma_age, adapt=b.sigma_adapt_rows.clone(), aux=b.post_aux.clone())

    ep, core, rows, log_ep, log_steps = _run_batched(make, env, params, reset_keys, rngs0, (4, 2), rows_of)
    assert np.array_equal(log_ep, log_steps)
    n_rows = int(ep.log.shape[1])
    assert n_rows > T and tuple(ep.elitelog.shape) == (E, n_rows, 8) and tuple(ep.sigmalog.shape) == (E, n_rows, 4)
    assert ep.postcovlog is None and ep.lamlog is None and ep.iterlog is None
    same_bits(ep.elitelog[:, :T], torch.stack([r["elite"] for r in rows], dim=1), "elitelog")
    same_bits(ep.postlog[:, :T], torch.stack([r["aux"] for r in rows], dim=1), "postlog")
    want = np.stack([np.stack([sigma_row(r["age"], r["adapt"][e]) for r in rows]) for e in range(E)])
    same_bits(ep.sigmalog[:, :T], want, "sigmalog")
    for name in ("elitelog", "postlog", "sigmalog"):
        assert not bits(getattr(ep, name)[:, T:]).any(), name
    sg = ep.read_sigma()
    assert sg["age"].shape == (E, T) and np.all(sg["age"] == np.arange(T) % m)
    assert np.all(sg["scale"][:, 0::2] == 1.0) and np.all(sg["scale"][:, 1::2] != 1.0)
    assert ep.read_post()["weight"].shape == (E, T) and np.all(ep.read_elite()["K"] == 32.0)
    assert core.device_status() == 0
    core.close()


# ---- 4. batched MPPI: the fused step ---------------------------------------------------------------------------------------------------
def test_batched_mppi_fused_step_iteration_log():
    E, T = 3, 4
    env, params, reset_keys, rngs0, cp0 = _batch_setup(E)

    def make():
        return cm.controllers.BatchedMPPIController(env, E, 128, H, 0.01, sigmas=cp0.sample_sigma, discount=cp0.discount,
                                                    gamma_mean=cp0.gamma_mean, a_mean_init=cp0.a_mean, device=DEV, iters=2)

    ep, core, rows, log_ep, log_steps = _run_batched(make, env, params, reset_keys, rngs0, (3, 1), lambda b: b.iter_cost_min.clone())
    assert np.array_equal(log_ep, log_steps)
    assert tuple(ep.iterlog.shape) == (E, int(ep.log.shape[1]), 2)
    same_bits(ep.iterlog[:, :T], torch.stack(rows, dim=1), "iterlog")
    assert not bits(ep.iterlog[:, T:]).any()
    assert ep.read_iters().shape == (E, T, 2) and np.all(np.isfinite(ep.read_iters()))
    assert core.device_status() == 0
    core.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_condition_and_a_detached_log_stays_untouched():
    rows = torch.zeros((8, 128 * 128), dtype=torch.float32, device=DEV)
    fresh = SamplingCore(256, H, 0.01, 1.0, device=DEV, compute_info=False)
    lib, h = fresh.lib, fresh.h
    firsts = ("covo_set_step_ess_floor", "covo_set_step_elite", "covo_set_step_iters", "covo_set_step_sigma_period",
              "covo_set_step_post_cov", "covo_set_step_post_cov")
    for kind, first in enumerate(firsts):  # a kind whose attachment is off
        with pytest.raises(CovoError, match=rf"kind={kind}: no .*call {first}"):
            check(lib.covo_set_episode_rows(h, kind, ptr(rows), 8), "covo_set_episode_rows")
        check(lib.covo_set_episode_rows(h, kind, None, 0), "covo_set_episode_rows")  # detaching nothing is fine
    for bad in (6, -1):
        with pytest.raises(CovoError, match=rf"kind={bad} outside \[0, 6\)"):
            check(lib.covo_set_episode_rows(h, bad, ptr(rows), 8), "covo_set_episode_rows")
    check(lib.covo_set_step_sigma_period(h, 2), "covo_set_step_sigma_period")
    with pytest.raises(CovoError, match="stride=0"):
        check(lib.covo_set_episode_rows(h, _lib.COVO_EPLOG_SIGMA, ptr(rows), 0), "covo_set_episode_rows")
    check(lib.covo_set_episode_rows(h, _lib.COVO_EPLOG_SIGMA, ptr(rows), 8), "covo_set_episode_rows")
    fresh.close()

    env = quad_env(task="tracking_zigzag")
    c, cp, params = _single(env, "mppi", 128, elite=8, iters=3)
    core = c.core
    lib, h = core.lib, core.h
    ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(21), params, (lib, h), DEV)
    cp = c.reset(ep.state0, params, cp, cr.PRNGKey(22))
    # a segment that overruns a log: nothing is launched
    attach = core.attach_log
    core.attach_log = lambda name, episode, rows_left: attach(name, episode, 5 if name == "iterlog" else rows_left)
    before = ep.true.clone()
    with pytest.raises(CovoError, match=r"episode iteration log rows \[0, 6\) outside \[0, 5\)"):
        c.run_episode(ep, params, cp, cr.PRNGKey(23), 6)
    torch.cuda.synchronize()
    assert torch.equal(ep.true, before) and not bits(ep.iterlog).any() and not bits(ep.elitelog).any()
    del core.attach_log
    # two steps with both logs, then the iteration log detached: a further segment fills the elite log only
    cp, rng = c.run_episode(ep, params, cp, cr.PRNGKey(23), 2)
    ep.read_log()
    kept = bits(ep.iterlog).copy()
    assert kept[:2].any() and not kept[2:].any()
    skip = lambda name, episode, rows_left: None if name == "iterlog" else attach(name, episode, rows_left)
    check(lib.covo_set_episode_rows(h, _lib.COVO_EPLOG_ITERS, None, 0), "covo_set_episode_rows")
    core.attach_log = skip
    cp, rng = c.run_episode(ep, params, cp, rng, 2)
    ep.read_log()
    assert np.array_equal(bits(ep.iterlog), kept) and bits(ep.elitelog[2:4]).any(axis=1).all() and not bits(ep.elitelog[4:]).any()
    # covo_set_step_iters with another width drops the log it finds attached
    check(lib.covo_set_episode_rows(h, _lib.COVO_EPLOG_ITERS, ptr(ep.iterlog[ep.n_steps:]), 4), "covo_set_episode_rows")
    two = torch.zeros((1, 2), dtype=torch.float32, device=DEV)
    check(lib.covo_set_step_iters(h, 2, ptr(two), 1), "covo_set_step_iters")
    cp, rng = c.run_episode(ep, params, cp, rng, 1)
    ep.read_log()
    assert np.array_equal(bits(ep.iterlog), kept) and bits(two).all() and bits(ep.elitelog[4]).any()
    # ... and so does turning the attachment off
    check(lib.covo_set_step_elite(h, 0, None, 0), "covo_set_step_elite")
    with pytest.raises(CovoError, match="kind=1: no elite-set update attached"):
        check(lib.covo_set_episode_rows(h, _lib.COVO_EPLOG_ELITE, ptr(ep.elitelog), 4), "covo_set_episode_rows")
    assert core.device_status() == 0
    core.close()


# ---- 6. the batched driver function ------------------------------------------------------------------------------------------------------
def test_eval_env_batched_returns_the_rows():
    env = quad_env(task="tracking_zigzag", randomizer=True)
    err, rows = cm.envs.quadrotor.eval_env_batched(env, 2, "N256_H32_lam0.01", n_steps=5, device=DEV, verbose=False, sigma_period=2,
                                                   sigma_adapt=0.1, iters=2, rows=True)
    assert err.shape == (2,) and sorted(rows) == ["iters", "post", "sigma"]
    assert rows["iters"].shape == (2, 5, 2) and np.all(np.isfinite(rows["iters"]))
    assert rows["sigma"]["age"].shape == (2, 5) and np.all(rows["sigma"]["age"] == np.array([0, 1, 0, 1, 0]))
    assert rows["sigma"]["fallback"].shape == (2, 5) and rows["sigma"]["logdet"].shape == (2, 5)
    assert rows["post"]["shift"].shape == (2, 5, 128) and rows["post"]["weight"].shape == (2, 5) and "cov" not in rows["post"]
    plain = cm.envs.quadrotor.eval_env_batched(env, 2, "N256_H32_lam0.01", n_steps=5, device=DEV, verbose=False, sigma_period=2,
                                               sigma_adapt=0.1, iters=2)
    assert np.array_equal(plain, err)  # the logs change nothing the episode computes


# ---- 7. every log at once: the ten logs of one table (DESIGN.md 4.19 "One table") ---------------------------------------------------
EVERY = dict(compute_diag=True, compute_plan=True, compute_fan=4, update="guarded", iters=2, sigma_period=2, sigma_adapt=0.25,
             compute_post_cov=True)
NINE = ("diag_log", "trace", "fanlog", "arblog", "elitelog", "iterlog", "sigmalog", "postlog", "postcovlog")  # (elite=K; ess_min: lamlog)


def _every_row(core, ci):
    """the row of every log a single step has just left, as the episode drivers would write it (the Sigma row: sigma_row)"""
    ep, u = ci["episode"], ci["u"]
    out = dict(diag_log=core.diag[0], trace=torch.cat([ep.true, ep.noisy, u.reshape(-1)[:4], core.plan[0]]), fanlog=core.fan[0],
               arblog=core.arbiter[0], iterlog=core.iter_cost_min[0], postlog=core.post_aux[0], postcovlog=core.post_cov[0].reshape(-1))
    if core.elite_rows is not None:
        out["elitelog"] = core.elite_rows[0]
    if core.lam_eff is not None:
        out["lamlog"] = core.lam_eff[0]
    out = {k: v.clone() for k, v in out.items()}
    out["sigmalog"] = torch.from_numpy(sigma_row(int(ci["sigma_age"]), core.sigma_adapt_rows[0])).to(DEV)
    return out


def test_single_every_log_at_once_equals_the_python_loop():
    """N = 1 024, 5 steps of covo_run_episode with all nine logs of `elite` attached (the diagnostic log now rides in the one copy launch,
    behind the after-step frame), then 3 steps with `ess_min` in place of `elite` for the temperature log: every row, bit for bit, is
    what a Python loop of controller(...) / episode.step reads from the step buffers after each step."""
    env = quad_env(task="tracking_zigzag")
    with_lam = tuple("lamlog" if name == "elitelog" else name for name in NINE)
    for weights, names, T in ((dict(elite=64), NINE, 5), (dict(ess_min=16), with_lam, 3)):
        ep, core, rows, log_ep, log_steps = _run_single(env, "covo-online", 1024, (T,), _every_row, dict(EVERY, **weights),
                                                        log_post_cov=True)
        assert np.array_equal(log_ep, log_steps)
        assert (ep.lamlog is None) == ("elite" in weights) and (ep.elitelog is None) == ("ess_min" in weights)
        for name in names:
            log = getattr(ep, name)
            same_bits(log[:T], torch.stack([r[name] for r in rows]), name)
            assert not bits(log[T:]).any(), name  # rows T .. were never written
        assert core.device_status() == 0
        core.close()


def test_batched_every_log_at_once_at_a_row_offset_equals_the_single_episodes():
    """The same nine logs through covo_run_episode_batched: E = 3 domain-randomised instances, 5 steps at log_index = 2 into logs of
    stride 8 that start out filled with a pattern.  Rows [2, 7) of instance e are the rows of covo_run_episode on instance e alone;
    rows 0, 1 and 7 keep the pattern."""
    E, T, first, stride, fill = 3, 5, 2, 8, -7.5
    env, params, reset_keys, rngs0, cp0 = _batch_setup(E)
    opts = dict(EVERY, elite=64)
    singles = []
    for e in range(E):
        c, cp, _ = _single(env, "covo-online", 1024, **opts)
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV, log_post_cov=True)
        cp = c.reset(se.state0, params[e], cp, cr.PRNGKey(2))
        c.run_episode(se, params[e], cp, rngs0[e], T)
        env_log = se.read_log()
        singles.append(dict({name: getattr(se, name)[:T].clone() for name in NINE}, log=env_log))
        assert c.core.device_status() == 0
        c.core.close()
    b = cm.controllers.BatchedCoVOController(env, E, 1024, H, 0.01, discount=cp0.discount, gamma_mean=cp0.gamma_mean,
                                             sample_sigma=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=DEV, **opts)
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV, log_post_cov=True)
    ep.log = torch.full((E, stride, 4), fill, dtype=torch.float32, device=DEV)  # the segment starts at row 2 of 8-row logs
    ep.n_steps = first
    for name in NINE:
        ep.alloc_log(name, *({"fanlog": (4,), "iterlog": (2,)}.get(name, ())))
        getattr(ep, name).fill_(fill)
        assert tuple(getattr(ep, name).shape[:2]) == (E, stride)
    b.run_episode(ep, rngs0.copy(), T)
    torch.cuda.synchronize()
    assert b.core.device_status() == 0
    pattern = bits(torch.full((1,), fill))[0]
    for name in NINE + ("log",):
        log = getattr(ep, name)
        for e in range(E):
            same_bits(log[e, first:first + T], singles[e][name], (name, e))
        untouched = bits(torch.cat([log[:, :first], log[:, first + T:]], dim=1))
        assert (untouched == pattern).all(), name
    b.core.close()


def test_diag_log_at_a_base_4_bytes_off_alignment():
    """covo_set_episode_diag_log with a base one float into a larger tensor: the 8-float rows take the copy kernel's float-by-float
    path, which the Python surface (16-byte aligned allocations, 32-byte rows) never reaches.  Same rows as the aligned run, bit for
    bit; the float in front of the log and the rows behind the segment stay untouched."""
    env = quad_env(task="tracking_zigzag")
    T, got = 5, {}
    for kind in ("aligned", "off"):
        c, cp, params = _single(env, "mppi", 1024, compute_diag=True)
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(21), params, (c.core.lib, c.core.h), DEV)
        if kind == "off":
            rows = int(ep.log.shape[0])
            big = torch.full((4 + rows * 8,), -7.5, dtype=torch.float32, device=DEV)
            ep.diag_log = big[1:1 + rows * 8].view(rows, 8)  # attach_log binds what it finds
            assert ep.diag_log.data_ptr() % 16 == 4
        cp = c.reset(ep.state0, params, cp, cr.PRNGKey(22))
        c.run_episode(ep, params, cp, cr.PRNGKey(23), T)
        got[kind] = (ep.read_diag(), ep.read_log())
        if kind == "off":
            assert bool((big[:1] == -7.5).all()) and bool((big[1 + T * 8:] == -7.5).all())
        assert c.core.device_status() == 0
        c.core.close()
    assert got["aligned"][0].shape == (T, 8) and np.isfinite(got["aligned"][0]).all()
    assert np.array_equal(bits(got["aligned"][0]), bits(got["off"][0])) and np.array_equal(got["aligned"][1], got["off"][1])
