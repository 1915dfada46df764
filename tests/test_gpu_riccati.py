"""GPU tests (-m gpu) of the Riccati refinement (covo_riccati / covo_riccati_refine / covo_set_step_riccati; `riccati=` of every
sampling controller; csrc/riccati.hip, csrc/newton_refine.hip with the direction supplied).

1. the stand-alone sweep against numpy on the device's own inputs: R = core.hessian, g = core.cost_gradient at make_problem(seed=17,
   time=37), hover + 0.3 noise (the clip is live).  The ladder must be decidable on the device's R (|lam_min + mu_j| >= 0.05 |lam_min|
   for every rung); then rung == the first j at which numpy's Cholesky of R + mu_j I succeeds, the normwise backward error of d is
   below 1e-9 (the project's Hessian bar), |d - d_np| <= 4 cond2(R + mu I) 1e-9 |d_np|, g.d < 0.  K, kff and x against the fp64
   oracle's sweep (tests/riccati_oracle.py) at the same bar, relative to the largest entry; the oracle's A, B under the device's K,
   kff reproduce the device's d.  The drag case is the 16-state build and gets the d checks only.
2. a batch of 3 equals three singles bit for bit; reg0 = 1e-9 finds no positive-definite rung (flag bit 3, d = 0, the mean stays); a
   NaN in the plan sets the flags and leaves the mean.
3. it descends from a poor mean on an MPPI handle (far_fast, hover + 0.3 noise, seed 1001 picked on the CPU: the fp64 oracle's
   candidates fall from 36.6 to 27.7, rung 5); g = 0 exactly -- every action of the plan beyond the clip, so B = 0 -- keeps the mean.
4. the production step against a twin without the switch (same key): MPPI, covo-offline, covo-online, and covo-online under
   sigma_period=4, whose second step is a reuse step; MPPI once more under the periodic disturbance, where the refinement forms the
   Hessian's table itself from the raw key.  The base cost is covo_arbitrate's candidate-0 cost of the twin's mean bit for
   bit; the committed mean is fp32(clip(b + alpha d)) with d = core.riccati(b), within 1.2e-7 (one fp32 rounding at |x| <= 1).
5. batched (E = 3) equals three singles bit for bit; iters=2 leaves the last pass's row; a 12-step run_episode equals 12 host calls.
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
from tests import riccati_oracle as RO  # noqa: E402
from tests.conftest import make_problem  # noqa: E402
from tests.gpu_support import DEV, DP, H, batched_controller, dev_state, params_c, quad_env, single_controller, step_inputs  # noqa: E402
from tests.state_atlas import atlas_state  # noqa: E402

RF = _lib.COVO_RICCATI_FLOATS
NC = _lib.COVO_REFINE_CANDIDATES
RUNGS = _lib.COVO_RICCATI_RUNGS
MUS = _lib.COVO_RICCATI_REG0 * 4.0 ** np.arange(RUNGS)
HESS_BAR = 1e-9
MEAN_BAR = 1.2e-7
KEY = cr.PRNGKey(5)


def split_row(row):
    """riccati row [8] (device tensor) -> (cost_base, cost_chosen, choice, alpha, |g|, g.d, mu, flags, rung)"""
    r = row.detach().cpu().numpy()
    i = np.ascontiguousarray(r).view(np.int32)
    return r[0], r[1], int(i[2]), r[3], r[4], r[5], r[6], int(i[7]) & 0xFF, int(i[7]) >> 8


def bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _core():
    return SamplingCore(256, H, 0.01, 1.0, device=DEV, compute_info=False)


@functools.lru_cache(maxsize=None)
def _problem():
    s, p, rng = make_problem(seed=17, time=37)
    p = p.replace(disturb_params=DP)
    b = (R.hover_action(p, 32, np.float64) + 0.3 * rng.normal(size=(32, 4))).astype(np.float32).reshape(-1)
    assert np.abs(b).max() > 1.0  # the clip has something to do
    return s, p, b


def _hessian_table(core, pc, ds, kind):
    if kind == "none":
        return None
    return core.disturb_table(pc, ds.packed, key=KEY, key_mode=_lib.DISTURB_KEYS_HESSIAN, deterministic=True)


def first_cholesky_rung(Rm):
    for j, mu in enumerate(MUS):
        try:
            np.linalg.cholesky(Rm + mu * np.eye(Rm.shape[0]))
            return j
        except np.linalg.LinAlgError:
            pass
    return RUNGS


# ------------------------------------------------------------------------------------------ 1: stand-alone against numpy
@pytest.mark.parametrize("kind,reward", [("none", "penyaw"), ("periodic", "realworld"), ("drag", "penyaw")])
def test_sweep_vs_numpy_on_the_devices_inputs(kind, reward):
    s, p, b = _problem()
    core = _core()
    ds = dev_state(s)
    pc = params_c(p, kind, reward)
    tab = _hessian_table(core, pc, ds, kind)
    bd = torch.from_numpy(b).to(DEV)
    Rm = core.hessian(ds.packed, ds, pc, bd, f_steps=tab)[0].cpu().numpy()
    Rm = (Rm + Rm.T) / 2.0
    g = core.cost_gradient(ds, pc, bd, f_steps=tab)[0].cpu().numpy()
    out = core.riccati(ds, pc, bd, f_steps=tab)
    torch.cuda.synchronize()
    assert core.device_status() == 0
    d = out["d"][0].cpu().numpy()
    mu, rung, piv, flags = out["rows"][0].cpu().numpy()
    lam = np.linalg.eigvalsh(Rm)
    where = f"{kind} {reward}: lam_min {lam.min():.4f} rung {rung} mu {mu} smallest pivot {piv:.3e} flags {flags}"
    print("  " + where)
    # the ladder is decidable on this R
    assert np.all(np.abs(lam.min() + MUS) >= 0.05 * abs(lam.min())), where
    want_rung = first_cholesky_rung(Rm)
    assert want_rung < RUNGS and int(rung) == want_rung and mu == MUS[want_rung] and flags == 0.0 and piv > 0.0, (where, want_rung)
    Rmu = Rm + mu * np.eye(128)
    berr = np.linalg.norm(Rmu @ d + g) / (np.linalg.norm(Rmu, 2) * np.linalg.norm(d) + np.linalg.norm(g))
    d_np = -np.linalg.solve(Rmu, g)
    cond = np.linalg.cond(Rmu, 2)
    ferr = np.linalg.norm(d - d_np) / np.linalg.norm(d_np)
    print(f"    backward error {berr:.3e}; |d - d_np| / |d_np| {ferr:.3e}, cond {cond:.3e}; g.d {g @ d:.4e}")
    assert berr <= HESS_BAR, (where, berr)
    assert ferr <= 4.0 * cond * HESS_BAR, (where, ferr)
    assert g @ d < 0.0, where
    assert np.all(d[124:] == 0.0), where               # action 31 reaches no reward
    assert np.all(d[np.abs(b) > 1.0] == 0.0), where    # a saturated component: B's column is zero
    K, kff, x = (out[n][0].cpu().numpy() for n in ("K", "kff", "x"))
    assert np.all(K[31] == 0.0) and np.isfinite(K).all() and np.isfinite(kff).all() and np.isfinite(x).all(), where
    if kind == "drag":
        return
    # the oracle's sweep on the same objective: periodic from the rows the device was fed
    assert np.all(K[:, :, RO.NX:] == 0.0) and np.all(x[:, RO.NX:] == 0.0), where
    forces = RO.step_forces(s, p, "none") if tab is None else RO.forces_from_table(s, tab[0].cpu().numpy())
    blk = RO.stage_blocks(s, p, b.astype(np.float64), reward, forces)
    r = RO.sweep(blk, float(mu))
    assert r["ok"], where
    bar = 4.0 * cond * HESS_BAR
    for name, got, ref in (("K", K[:, :, :RO.NX], r["K"]), ("kff", kff, r["kff"]), ("x", x[:, :RO.NX], blk["x"])):
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"    {name}: max err / max |{name}| {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (where, name, err)
    # the gains are a controller: the oracle's linearisation under the device's K, kff gives the device's d
    d_fb, _ = RO.forward(blk["A"], blk["B"], K[:, :, :RO.NX], kff)
    err = np.linalg.norm(d_fb - d) / np.linalg.norm(d)
    print(f"    forward pass of the oracle's A, B under the device's gains vs d: {err:.3e}")
    assert err <= bar, (where, err)


# ------------------------------------------------------------------------------------------ 2: batches, an empty ladder, NaN
def test_batch_equals_singles_and_the_ladder_can_fail():
    s, p, b = _problem()
    core = _core()
    ds = dev_state(s)
    pc = params_c(p, "none", "penyaw")
    rng = np.random.default_rng(3)
    plans = np.stack([b, (b + 0.05 * rng.normal(size=128)).astype(np.float32), (0.5 * b).astype(np.float32)])
    pd = torch.from_numpy(plans).to(DEV)
    batch = core.riccati(ds, pc, pd)
    for e in range(3):
        one = core.riccati(ds, pc, pd[e])
        for name in ("d", "K", "kff", "x", "rows"):
            assert torch.equal(batch[name][e].view(torch.int64), one[name][0].view(torch.int64)), (e, name)
    assert len({batch["d"][e].cpu().numpy().tobytes() for e in range(3)}) == 3  # three different directions
    assert core.device_status() == 0
    # reg0 = 1e-9: the highest rung is 1.6e-5, far below -lam_min(R) = 1.07 -- no rung is positive definite
    none = core.riccati(ds, pc, pd[0], reg0=1e-9)
    mu, rung, piv, flags = none["rows"][0].cpu().numpy()
    assert int(flags) == 8 and int(rung) == RUNGS and mu == 0.0, (mu, rung, piv, flags)
    assert not none["d"].any() and not none["K"].any() and not none["kff"].any()
    am = pd[0].clone()
    row, costs = core.riccati_refine(ds, pc, am, reg0=1e-9)
    base, chosen, choice, alpha, gnorm, slope, w6, fl, rg = split_row(row)
    assert fl == 8 and rg == RUNGS and choice == 0 and alpha == 0.0 and w6 == 0.0 and slope == 0.0 and gnorm > 0.0
    assert torch.equal(bits32(am), bits32(pd[0])) and chosen.tobytes() == base.tobytes()
    # a NaN in the plan: its gradient entry is not finite, no candidate is formed, the mean stays as it is
    bad = pd[0].clone()
    bad[5] = float("nan")
    amn = bad.clone()
    rown, _ = core.riccati_refine(ds, pc, amn)
    rn = split_row(rown)
    print(f"  NaN plan: flags {rn[7]} rung {rn[8]} choice {rn[2]}")
    assert rn[7] != 0 and (rn[7] & 1) == 1 and rn[2] == 0 and rn[3] == 0.0, rn
    assert torch.equal(bits32(amn), bits32(bad))
    side = core.riccati(ds, pc, bad)["rows"][0].cpu().numpy()
    assert (int(side[3]) & 1) == 1, side
    torch.cuda.synchronize()
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ 3: it descends
def test_riccati_refine_descends_on_an_mppi_handle():
    s, p, _ = atlas_state("far_fast")
    b = (R.hover_action(p, 32, np.float64) + 0.3 * np.random.default_rng(1001).normal(size=(32, 4))).astype(np.float32).reshape(-1)
    env = quad_env(task="tracking_zigzag")
    c, _, _, _, _, _ = single_controller(env, "mppi", 256, riccati=True)
    core = c.core
    ds = dev_state(s)
    pc = params_c(p, "none", "penyaw")
    bd = torch.from_numpy(b).to(DEV)
    am = bd.clone()
    row, costs = core.riccati_refine(ds, pc, am)
    base, chosen, choice, alpha, gnorm, slope, mu, flags, rung = split_row(row)
    print(f"  device costs {costs.cpu().numpy()}, choice {choice}, rung {rung}, mu {mu}, g.d {slope}")
    assert flags == 0 and choice >= 1 and chosen < base and slope < 0.0 and not torch.equal(am, bd)
    assert mu == np.float32(MUS[rung]) and alpha == 2.0 ** (3 - choice)
    assert torch.equal(am, am.clamp(-1, 1))  # the candidate as it was rolled out
    c_host = np.where(np.isnan(costs.cpu().numpy()), np.inf, costs.cpu().numpy().astype(np.float64))
    assert choice == int(np.argmin(c_host)) and base.tobytes() == costs[0].cpu().numpy().tobytes()
    # g = 0 exactly: every action of the plan lies beyond the clip, B = 0 at every stage -- d = 0, every candidate is clip(b), equal
    # costs go to the lowest candidate and the mean is not written
    sat = torch.full((128,), 1.5, dtype=torch.float32, device=DEV)
    am0 = sat.clone()
    row0, costs0 = core.riccati_refine(ds, pc, am0)
    r0 = split_row(row0)
    assert r0[2] == 0 and r0[7] == 0 and r0[3] == 0.0 and r0[4] == 0.0 and r0[5] == 0.0, r0
    assert torch.equal(am0, sat)  # untouched
    assert len(set(costs0.cpu().numpy().tobytes()[4 * j:4 * j + 4] for j in range(NC))) == 1
    assert core.device_status() == 0
    core.close()


# ------------------------------------------------------------------------------------------ 4: the production step
@pytest.mark.parametrize("name,kw,disturb", [("mppi", {}, "gaussian"), ("covo-offline", {}, "gaussian"), ("covo-online", {}, "gaussian"),
                                             ("covo-online", dict(sigma_period=4), "gaussian"), ("mppi", {}, "periodic")],
                         ids=["mppi", "covo-offline", "covo-online", "covo-online-period4", "mppi-periodic"])
def test_production_step_against_a_twin_without_the_switch(name, kw, disturb):
    """(mppi-periodic: a step that builds no Hessian table of its own -- the refinement forms it from the raw key)"""
    N = 256
    env = quad_env(task="tracking_zigzag", disturb=disturb)
    ca, cp, obs, info, state, params = single_controller(env, name, N, riccati=True, **kw)
    cb, _, _, _, _, _ = single_controller(env, name, N, **kw)
    if disturb != "gaussian":
        params = params.replace(disturb_params=np.asarray(DP, dtype=np.float32))
    assert cb.core.riccati_rows is None and tuple(ca.core.riccati_rows.shape) == (1, RF)
    key = cr.PRNGKey(11)
    for step in range(2):
        key, k_act, k_step = cr.split(key, 3)
        dstate = as_device_state(info["noisy_state"], DEV)
        ua, cpa, ia = ca(obs, state, params, k_act, cp, info)
        ub, cpb, ib = cb(obs, state, params, k_act, cp, info)
        torch.cuda.synchronize()
        core = ca.core
        base, chosen, choice, alpha, gnorm, slope, mu, flags, rung = split_row(core.riccati_rows[0])
        where = f"{name} {kw} {disturb} step {step}: base {base} chosen {chosen} choice {choice} alpha {alpha} mu {mu} rung {rung} flags {flags}"
        print("  " + where)
        if kw.get("sigma_period", 1) > 1:
            assert int(ia["sigma_age"]) == step, where  # step 1 is a reuse step
        assert not any(k.startswith("riccati_") for k in ib)
        assert ia["riccati_cost"].data_ptr() == core.riccati_rows[0, 1:2].data_ptr() and ia["riccati_choice"].dtype == torch.int32
        assert int(ia["riccati_choice"]) == choice and float(ia["riccati_alpha"]) == float(alpha), where
        assert int(ia["riccati_rung"]) == rung and float(ia["riccati_reg"]) == float(mu), where
        # nothing of the step itself changes
        assert torch.equal(core.a, cb.core.a) and torch.equal(core.cost, cb.core.cost), where
        # the base is the cost of the twin's mean under the step's own sampling objective: the arbiter's candidate 0
        pc = ca._params_c(params)
        f_shared, tab_r = step_inputs(env, cb, name, params, k_act, dstate, cb.core)
        mean_b = cpb.a_mean.reshape(-1).contiguous()
        arb = cb.core.arbitrate(dstate, pc, mean_b.clone(), mean_b.clone(), 1, f_shared=f_shared, f_steps=tab_r)
        assert torch.equal(core.riccati_rows[0, 0:1], arb[0:1]), (where, float(arb[0]))
        assert flags == 0 and rung < RUNGS and chosen <= base, where
        assert mu == np.float32(MUS[rung]) and alpha == (2.0 ** (3 - choice) if choice else 0.0), where
        if choice == 0:
            assert torch.equal(cpa.a_mean, cpb.a_mean), where
        else:
            # the committed mean is fp32(clip(b + alpha d)), d the stand-alone sweep's direction at b
            tab_h = None
            if pc.disturb_kind in _lib.TABLE_DISTURB_KINDS:
                tab_h = cb.core.disturb_table(pc, dstate.packed, key=k_act, key_mode=_lib.DISTURB_KEYS_HESSIAN, deterministic=True)
            d = cb.core.riccati(dstate, pc, mean_b, f_steps=tab_h)["d"][0].cpu().numpy()
            b64 = mean_b.cpu().numpy().astype(np.float64)
            want = np.clip(b64 + float(alpha) * d, -1.0, 1.0).astype(np.float32).astype(np.float64)
            err = np.abs(cpa.a_mean.reshape(-1).cpu().numpy().astype(np.float64) - want).max()
            print(f"    committed mean vs fp32(clip(b + alpha d)): {err:.3e}; |d|max {np.abs(d).max():.3e}")
            assert err <= MEAN_BAR, (where, err)
            assert not torch.equal(cpa.a_mean, cpb.a_mean) and torch.equal(cpa.a_mean, cpa.a_mean.clamp(-1, 1)), where
        cp = cpa
        obs, state, _, _, info = env.step(k_step, state, ua.cpu().numpy(), params)
    assert ca.core.device_status() == 0 and cb.core.device_status() == 0
    ca.core.close()
    cb.core.close()


# ------------------------------------------------------------------------------------------ 5: batched, iterated, closed loop
def _controller(env, N, riccati, **kw):
    import covo_mpc_amd as cm
    c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False, riccati=riccati, **kw)
    return c, c.init_control_params


def test_batched_riccati_equals_singles():
    import covo_mpc_amd as cm
    N, E = 256, 3
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    act = [np.stack([np.asarray(cr.PRNGKey(60 + 10 * k + e)) for e in range(E)]) for k in range(2)]
    rows, means = [], []
    for e in range(E):
        c, _ = _controller(env, N, True)
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        cp = c.reset(se.state0, params[e], c.init_control_params, cr.PRNGKey(2))
        r, m = [], []
        for k in range(2):
            _, cp, _ = c(None, None, params[e], act[k][e], cp, {"noisy_state": se.noisy_state})
            torch.cuda.synchronize()
            r.append(c.core.riccati_rows[0].clone())
            m.append(cp.a_mean.reshape(-1).clone())
        rows.append(r)
        means.append(m)
        cp0 = c.init_control_params
        c.core.close()
    b = batched_controller(env, "covo-online", cp0, E, N, 0.01, riccati=True)
    assert tuple(b.riccati.shape) == (E, RF)
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    b.bind_episode(ep)
    for k in range(2):
        b(None, act[k])
        torch.cuda.synchronize()
        for e in range(E):
            assert torch.equal(bits32(b.riccati[e]), bits32(rows[e][k])), (k, e, b.riccati[e], rows[e][k])
            assert torch.equal(b.a_mean[e].reshape(-1), means[e][k]), (k, e)
    print(f"  choices {[[split_row(rows[e][k])[2] for k in range(2)] for e in range(E)]}")
    assert b.core.device_status() == 0
    b.core.close()


def test_iterated_step_leaves_the_last_passes_row():
    """iters=2: every pass runs the refinement; the row is the last pass's -- its chosen cost is the plan's, which follows the last pass"""
    from tests.gpu_support import start_episode
    env = quad_env(task="tracking_zigzag")
    c, cp0 = _controller(env, 256, True, iters=2, compute_plan=True)
    cp, obs, info, state, params = start_episode(env, c, cp0, "covo-online")
    u, cp1, i1 = c(obs, state, params, cr.PRNGKey(11), cp, info)
    torch.cuda.synchronize()
    base, chosen, choice, _, _, _, _, flags, rung = split_row(c.core.riccati_rows[0])
    print(f"  base {base} chosen {chosen} choice {choice} rung {rung}; pass minima {i1['iter_cost_min'].cpu().numpy()}")
    assert flags == 0 and chosen <= base
    assert torch.equal(i1["cost_plan"].reshape(1), c.core.riccati_rows[0, 1:2])
    assert bool(torch.isfinite(i1["iter_cost_min"]).all())
    assert c.core.device_status() == 0
    c.core.close()


def test_run_episode_equals_host_calls():
    import covo_mpc_amd as cm
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    T = 12
    got = {}
    for mode in ("fused", "hand"):
        c, _ = _controller(env, 256, True, compute_plan=True)
        c.alias_outputs = True
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (c.core.lib, c.core.h), DEV)
        cp = c.reset(ep.state0, params, c.init_control_params, cr.PRNGKey(42))
        rng = cr.PRNGKey(43)
        if mode == "hand":
            us, ch = [], []
            for _ in range(T):
                rng, rng_act, rng_step, _c = cr.split(rng, 4)
                u, cp, _ = c(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                us.append(u.clone())
                ch.append(c.core.riccati_rows[0].clone())
                ep.step(rng_step, u)
                rng, _c = cr.split(rng)
            got["hand"] = (torch.stack(us).cpu().numpy(), ep.read_log(), [split_row(r)[2] for r in ch])
        else:
            cp, rng = c.run_episode(ep, params, cp, rng, 7)
            cp, rng = c.run_episode(ep, params, cp, rng, T - 7)
            got["fused"] = (ep.read_trace()["u"][:T].copy(), ep.read_log())
        assert c.core.device_status() == 0
        c.core.close()
    print(f"  choices of the 12 steps: {got['hand'][2]}")
    assert got["fused"][0].shape == (T, 4) and got["fused"][0].tobytes() == got["hand"][0].tobytes()
    assert np.array_equal(got["fused"][1], got["hand"][1])
