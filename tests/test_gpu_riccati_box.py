"""GPU tests (-m gpu) of the Riccati box (covo_riccati_box / covo_riccati_refine_box / covo_set_step_riccati_box; `riccati_box=` of
every controller that takes riccati=; csrc/riccati.hip, the BOX instantiations) against the fp64 oracle of
tests/riccati_box_oracle.py, on the named inputs tests/test_riccati_box_oracle.py guards (A yaw_quarter, B make_problem(17, 37) at
reg0 = 1e-4, C double_cover; each with the hover plan).

1. cases A and B on the device's inputs: same rung and mu as ladder_box, the masks equal at all 32 stages, d, K, kff within
   4 cond2(R + mu I) 1e-9 relative (the systems solved are principal sub-blocks and Schur complements of R + mu I, whose condition it
   bounds), x as tests/test_gpu_riccati.py holds it, |clip(b) + kff| <= 1 with no tolerance, clamped entries of kff the bound bit for
   bit, clamped rows of K exactly 0, g.d < 0.
2. case C: d, K, kff, x, rows equal core.riccati(box=False) bit for bit, the masks are 0.
3. the raw plan of tests/test_gpu_riccati.py (entries beyond the clip: B's column there is zero): d == 0 there, the masks compared on
   the coordinates with |b| < 1, d, K, kff at the bar of 1.
4. a batch of the three cases equals the three singles bit for bit; reg0 = 1e-9 gives flag bit 3 with d = 0, K = 0 and masks 0.
5. the stateless line search over the box sweep, with and without the closed-loop candidates, on case A.
6. production steps from case A's state with the switch on: MPPI, covo-online and BatchedCoVOController(mode="online") with 2
   instances; a twin with the switch off equals a controller built without the keyword.
7. iLQR, k = 3, riccati_box=True, from case A's state: the costs chain, ilqr_box_count, the hold step, a 6-step run_episode.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from tests import riccati_box_oracle as BO  # noqa: E402
from tests import riccati_oracle as RO  # noqa: E402
from tests.conftest import make_problem  # noqa: E402
from tests.gpu_support import DEV, H, batched_controller, dev_state, params_c, quad_env, single_controller  # noqa: E402

RUNGS = _lib.COVO_RICCATI_RUNGS
NC, NCF = _lib.COVO_REFINE_CANDIDATES, _lib.COVO_FEEDBACK_CANDIDATES
HESS_BAR = 1e-9
MEAN_BAR = 1.2e-7
KEY = cr.PRNGKey(5)
SWEEP_OUT = ("d", "K", "kff", "x", "rows")


def bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def bits64(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def split_row(row):
    """riccati row [8] (device tensor) -> (cost_base, cost_chosen, choice, alpha, |g|, g.d, mu, flags, rung)"""
    r = row.detach().cpu().numpy()
    i = np.ascontiguousarray(r).view(np.int32)
    return r[0], r[1], int(i[2]), r[3], r[4], r[5], r[6], int(i[7]) & 0xFF, int(i[7]) >> 8


def clamped(masks):
    """masks [..., 32] (numpy int) -> bool [..., 32, 4]: coordinate i of stage k is clamped (at either bound)"""
    m = np.asarray(masks)[..., None]
    i = np.arange(4)
    return (((m >> i) | (m >> (4 + i))) & 1).astype(bool)


@functools.lru_cache(maxsize=None)
def _core():
    return SamplingCore(256, H, 0.01, 1.0, device=DEV, compute_info=False)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(s, p, b float32 [128], reg0, the oracle's stage blocks at b, ladder_box's (rung, mu, result)); "raw": the plan of
    tests/test_gpu_riccati.py, hover + 0.3 noise, whose entries reach beyond the clip"""
    if name == "raw":
        s, p, rng = make_problem(seed=17, time=37)
        b = (R.hover_action(p, 32, np.float64) + 0.3 * rng.normal(size=(32, 4))).astype(np.float32).reshape(-1)
        assert np.abs(b).max() > 1.0
        reg0 = _lib.COVO_RICCATI_REG0
    else:
        s, p, b, reg0 = BO.named_case(name)
    blk = RO.stage_blocks(s, p, b.astype(np.float64), "penyaw", RO.step_forces(s, p, "none"))
    return s, p, b, reg0, blk, BO.ladder_box(blk, b, reg0)


def _sweep(name, box=True):
    s, p, b, reg0, _, _ = _case(name)
    out = _core().riccati(dev_state(s), params_c(p, "none", "penyaw"), torch.from_numpy(b).to(DEV), reg0=reg0, box=box)
    torch.cuda.synchronize()
    assert _core().device_status() == 0
    return out


def _against_the_oracle(name, live_only=False):
    """the box sweep of case `name` against ladder_box on the device's inputs -> (out, numpy masks, the oracle's result)"""
    s, p, b, reg0, blk, (j, mu_o, r) = _case(name)
    core, ds, pc = _core(), dev_state(s), params_c(p, "none", "penyaw")
    bd = torch.from_numpy(b).to(DEV)
    Rm = core.hessian(ds.packed, ds, pc, bd)[0].cpu().numpy()
    Rm = (Rm + Rm.T) / 2.0
    g = core.cost_gradient(ds, pc, bd)[0].cpu().numpy()
    out = _sweep(name)
    d, K, kff, x = (out[n][0].cpu().numpy() for n in ("d", "K", "kff", "x"))
    masks = out["box"][0].cpu().numpy()
    mu, rung, piv, flags = out["rows"][0].cpu().numpy()
    where = f"case {name}: rung {rung} mu {mu} smallest pivot {piv:.3e} flags {flags}; oracle rung {j}, margin {r['margin'].min():.3e}"
    print("  " + where)
    assert j < RUNGS and int(rung) == j and mu == mu_o and flags == 0.0 and piv > 0.0, where
    live = (np.abs(b) < 1.0).reshape(H, 4)
    got_c, want_c = clamped(masks), clamped(r["masks"])
    if live_only:
        assert np.array_equal(got_c & live, want_c & live), (where, masks, r["masks"])
        lo_bit = lambda m: ((np.asarray(m)[:, None] >> np.arange(4)) & 1).astype(bool)
        assert np.array_equal(lo_bit(masks) & live, lo_bit(r["masks"]) & live), where
    else:
        assert np.array_equal(masks, r["masks"]), (where, masks, r["masks"])
    print(f"    masks {[hex(int(m)) for m in masks if m]} ({BO.clamp_count(masks)} clamped coordinates)")
    cond = np.linalg.cond(Rm + mu * np.eye(128), 2)
    bar = 4.0 * cond * HESS_BAR
    ferr = np.linalg.norm(d - r["d"]) / np.linalg.norm(r["d"])
    print(f"    |d - d_oracle| / |d_oracle| {ferr:.3e}, cond {cond:.3e} (bar {bar:.3e}); g.d {g @ d:.4e}")
    assert ferr <= bar, (where, ferr)
    assert np.all(K[:, :, RO.NX:] == 0.0) and np.all(x[:, RO.NX:] == 0.0), where
    for nm, got, ref in (("K", K[:, :, :RO.NX], r["K"]), ("kff", kff, r["kff"]), ("x", x[:, :RO.NX], blk["x"])):
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"    {nm}: max err / max |{nm}| {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (where, nm, err)
    assert g @ d < 0.0, where
    assert np.all(d[124:] == 0.0) and np.all(K[31] == 0.0), where
    # the box holds without a tolerance; a clamped entry is the fp64 bound itself, its row of K exactly zero
    bc = np.clip(b.astype(np.float64), -1.0, 1.0).reshape(H, 4)
    assert np.all(np.abs(bc + kff) <= 1.0), (where, np.abs(bc + kff).max())
    lo_b, hi_b = -1.0 - bc, 1.0 - bc
    at_lo = ((masks[:, None] >> np.arange(4)) & 1).astype(bool)
    at_hi = ((masks[:, None] >> (4 + np.arange(4))) & 1).astype(bool)
    assert not (at_lo & at_hi).any()
    assert kff[at_lo].tobytes() == lo_b[at_lo].tobytes() and kff[at_hi].tobytes() == hi_b[at_hi].tobytes(), where
    assert not K[at_lo | at_hi].any(), where
    # the gains are a controller: the oracle's linearisation under the device's K, kff gives the device's d
    d_fb, _ = RO.forward(blk["A"], blk["B"], K[:, :, :RO.NX], kff)
    assert np.linalg.norm(d_fb - d) / np.linalg.norm(d) <= bar, where
    return out, masks, r


# ------------------------------------------------------------------------------------------ 1: the clamped cases against the oracle
@pytest.mark.parametrize("name", ["A", "B"])
def test_box_sweep_vs_the_oracle_on_the_devices_inputs(name):
    out, masks, r = _against_the_oracle(name)
    assert BO.clamp_count(masks) >= 3
    if name == "A":  # a lower and an upper clamp in one stage
        assert any((m & 0x0F) and (m & 0xF0) for m in masks), masks
    # the unconstrained sweep of the same inputs is another step
    free = _sweep(name, box=False)
    assert "box" not in free and not torch.equal(free["d"], out["d"])
    _, _, b, _, _, _ = _case(name)
    bc = np.clip(b.astype(np.float64), -1.0, 1.0).reshape(H, 4)
    assert np.abs(bc + free["kff"][0].cpu().numpy()).max() > 1.0


# ------------------------------------------------------------------------------------------ 2: no clamp: today's arithmetic
def test_a_feasible_sweep_is_the_unconstrained_one_bit_for_bit():
    box, free = _sweep("C"), _sweep("C", box=False)
    for n in SWEEP_OUT:
        assert torch.equal(bits64(box[n]), bits64(free[n])), n
    assert not box["box"].any() and tuple(box["box"].shape) == (1, H) and box["box"].dtype == torch.int32
    _, _, _, _, _, (j, mu, r) = _case("C")
    assert int(box["rows"][0, 1]) == j and not r["masks"].any()


# ------------------------------------------------------------------------------------------ 3: a plan with saturated entries
def test_raw_plan_with_saturated_entries():
    out, masks, r = _against_the_oracle("raw", live_only=True)
    _, _, b, _, _, _ = _case("raw")
    d = out["d"][0].cpu().numpy()
    assert np.all(d[np.abs(b) > 1.0] == 0.0)  # B's column is zero there, as today


# ------------------------------------------------------------------------------------------ 4: batches, an empty ladder
def test_batch_equals_singles_and_the_ladder_can_fail():
    core = _core()
    cases = [_case(n) for n in "ABC"]
    packed = torch.stack([dev_state(c[0]).packed for c in cases])
    plans = torch.from_numpy(np.stack([c[2] for c in cases])).to(DEV)
    # (one reg0 and one trajectory per call: A's; B and C are then other problems than the named ones, which is all a batch test needs)
    sA, pA = cases[0][0], cases[0][1]
    ds, pc = dev_state(sA), params_c(pA, "none", "penyaw")
    batch = core.riccati(ds, pc, plans, packed=packed, box=True)
    for e in range(3):
        one = core.riccati(ds, pc, plans[e], packed=packed[e:e + 1].contiguous(), box=True)
        for n in SWEEP_OUT:
            assert torch.equal(bits64(batch[n][e]), bits64(one[n][0])), (e, n)
        assert torch.equal(batch["box"][e], one["box"][0]), e
    assert batch["box"][0].any()
    assert len({batch["d"][e].cpu().numpy().tobytes() for e in range(3)}) == 3
    # reg0 = 1e-9: the highest rung is 1.6e-5 -- no rung is positive definite
    none = core.riccati(ds, pc, plans[0], reg0=1e-9, box=True)
    mu, rung, piv, flags = none["rows"][0].cpu().numpy()
    assert int(flags) == 8 and int(rung) == RUNGS and mu == 0.0, (mu, rung, piv, flags)
    assert not none["d"].any() and not none["K"].any() and not none["kff"].any() and not none["box"].any()
    torch.cuda.synchronize()
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ 5: the stateless line search
@pytest.mark.parametrize("feedback", [False, True])
def test_stateless_line_search_over_the_box_sweep(feedback):
    s, p, b, reg0, _, _ = _case("A")
    core, ds, pc = _core(), dev_state(s), params_c(p, "none", "penyaw")
    bd = torch.from_numpy(b).to(DEV)
    am, am0 = bd.clone(), bd.clone()
    got = core.riccati_refine(ds, pc, am, reg0=reg0, feedback=feedback, box=True)
    ref = core.riccati_refine(ds, pc, am0, reg0=reg0, feedback=feedback)
    torch.cuda.synchronize()
    row, costs, masks = got[0], got[1], got[-1]
    assert len(got) == (4 if feedback else 3) and tuple(costs.shape) == (NCF if feedback else NC,)
    base, chosen, choice, alpha, gnorm, slope, mu, flags, rung = split_row(row)
    print(f"  feedback {feedback}: base {base} chosen {chosen} choice {choice} alpha {alpha} rung {rung}; unboxed choice {split_row(ref[0])[2]}")
    sweep = _sweep("A")
    assert torch.equal(masks, sweep["box"][0]) and masks.any()
    assert flags == 0 and chosen <= base and slope < 0.0
    # candidate 0 is clip(b) either way
    assert torch.equal(bits32(costs[0:1]), bits32(ref[1][0:1])) and torch.equal(bits32(row[0:1]), bits32(ref[0][0:1]))
    # candidates 1 .. 16: fp32(clip(b + alpha d_box)) -- the committed one is in a_mean
    c_host = np.where(np.isnan(costs.cpu().numpy()), np.inf, costs.cpu().numpy().astype(np.float64))
    assert choice == int(np.argmin(c_host))
    d = sweep["d"][0].cpu().numpy()
    want = RO.candidates(b, d)
    if 1 <= choice <= 16:
        err = np.abs(am.cpu().numpy().astype(np.float64) - want[choice]).max()
        print(f"    committed mean vs fp32(clip(b + alpha d_box)): {err:.3e}")
        assert err <= MEAN_BAR and alpha == 2.0 ** (3 - choice)
    # every open-loop candidate's cost is the cost of that sequence: the unboxed search, started at it with d = anything, has it as
    # its candidate 0
    for jc in (1, 4, 16):
        probe = torch.from_numpy(want[jc].astype(np.float32)).to(DEV)
        r0 = core.riccati_refine(ds, pc, probe, reg0=reg0)
        rel = abs(float(r0[1][0]) - float(costs[jc])) / max(1.0, abs(float(costs[jc])))
        print(f"    candidate {jc}: cost {float(costs[jc]):.6f}, the rollout of fp32(clip(b + alpha d_box)) {float(r0[1][0]):.6f}")
        assert rel <= 1e-5, (jc, rel)  # a rollout cost's bar; the sequences differ by at most one fp32 rounding
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ 6: the production steps
def _check_committed(core_prim, ds, pc, mean_b, mean_a, row, masks, where):
    """the committed mean of a step whose sweep ran at mean_b, against the stand-alone box sweep there"""
    base, chosen, choice, alpha, gnorm, slope, mu, flags, rung = split_row(row)
    prim = core_prim.riccati(ds, pc, mean_b, box=True)
    torch.cuda.synchronize()
    assert torch.equal(masks.reshape(-1), prim["box"][0]), (where, masks, prim["box"][0])
    assert flags == 0 and rung < RUNGS and chosen <= base, where
    assert int(prim["rows"][0, 1]) == rung, where
    if choice == 0:
        assert torch.equal(bits32(mean_a), bits32(mean_b)), where
        return choice
    assert 1 <= choice <= 16, where
    d = prim["d"][0].cpu().numpy()
    want = np.clip(mean_b.cpu().numpy().astype(np.float64) + float(alpha) * d, -1.0, 1.0).astype(np.float32).astype(np.float64)
    err = np.abs(mean_a.cpu().numpy().astype(np.float64) - want).max()
    print(f"    {where}: choice {choice}, committed mean vs fp32(clip(b + alpha d_box)): {err:.3e}; masks {int(masks.ne(0).sum())} stages")
    assert err <= MEAN_BAR, (where, err)
    return choice


@pytest.mark.parametrize("name", ["mppi", "covo-online"])
def test_production_step_with_the_switch_on(name):
    s, _, _, _, _, _ = _case("A")
    ds = dev_state(s)
    env = quad_env(task="tracking_zigzag")
    ca, cp, _, _, _, params = single_controller(env, name, 256, riccati=True, riccati_box=True)
    cb, _, _, _, _, _ = single_controller(env, name, 256)
    coff, _, _, _, _, _ = single_controller(env, name, 256, riccati=True, riccati_box=False)
    cold, _, _, _, _, _ = single_controller(env, name, 256, riccati=True)
    assert tuple(ca.core.riccati_box_masks.shape) == (1, H) and coff.core.riccati_box_masks is None
    info = {"noisy_state": ds}
    ua, cpa, ia = ca(None, None, params, KEY, cp, info)
    ub, cpb, ib = cb(None, None, params, KEY, cp, info)
    uf, cpf, if_ = coff(None, None, params, KEY, cp, info)
    uo, cpo, io = cold(None, None, params, KEY, cp, info)
    torch.cuda.synchronize()
    assert ia["riccati_box_mask"].data_ptr() == ca.core.riccati_box_masks.data_ptr() and ia["riccati_box_mask"].dtype == torch.int32
    assert int(ia["riccati_box_count"]) == BO.clamp_count(ia["riccati_box_mask"].cpu().numpy())
    assert not any(k.startswith("riccati_box") for k in io) and not any(k.startswith("riccati_box") for k in if_)
    # the switch off is the controller without the keyword
    assert torch.equal(bits32(cpf.a_mean), bits32(cpo.a_mean)) and torch.equal(bits32(coff.core.riccati_rows), bits32(cold.core.riccati_rows))
    # nothing of the step itself changes; the sweep runs at the twin's mean
    assert torch.equal(ca.core.a, cb.core.a) and torch.equal(ca.core.cost, cb.core.cost)
    pc = ca._params_c(params)
    mean_b = cpb.a_mean.reshape(-1).contiguous()
    _check_committed(cb.core, ds, pc, mean_b, cpa.a_mean.reshape(-1), ca.core.riccati_rows[0], ia["riccati_box_mask"], name)
    for c in (ca, cb, coff, cold):
        assert c.core.device_status() == 0
        c.core.close()


def test_batched_production_step_with_the_switch_on():
    E, N = 2, 256
    s, _, _, _, _, _ = _case("A")
    ds = dev_state(s)
    env = quad_env(task="tracking_zigzag")
    c0, cp0, _, _, _, params = single_controller(env, "covo-online", N)
    keys = np.stack([np.asarray(cr.PRNGKey(70 + e)) for e in range(E)])
    packed = torch.stack([ds.packed] * E)
    steps = {}
    for tag, kw in (("box", dict(riccati=True, riccati_box=True)), ("plain", {}), ("off", dict(riccati=True, riccati_box=False)),
                    ("old", dict(riccati=True))):
        b = batched_controller(env, "covo-online", cp0, E, N, 0.01, **kw)
        b.set_instances([ds] * E, [params] * E)
        b(packed, keys)
        torch.cuda.synchronize()
        assert b.core.device_status() == 0
        steps[tag] = (b.a_mean.clone(), None if b.riccati is None else b.riccati.clone(),
                      None if b.riccati_box is None else b.riccati_box.clone())
        b.core.close()
    assert steps["off"][2] is None and tuple(steps["box"][2].shape) == (E, H)
    assert torch.equal(bits32(steps["off"][0]), bits32(steps["old"][0])) and torch.equal(bits32(steps["off"][1]), bits32(steps["old"][1]))
    pc = c0._params_c(params)
    for e in range(E):
        _check_committed(c0.core, ds, pc, steps["plain"][0][e].contiguous(), steps["box"][0][e], steps["box"][1][e], steps["box"][2][e],
                         f"batched instance {e}")
    c0.core.close()


# ------------------------------------------------------------------------------------------ 7: iLQR
def _ilqr(env, k, mean, **kw):
    cp = cm.controllers.ILQRParams(a_mean=torch.from_numpy(np.ascontiguousarray(mean, dtype=np.float32).reshape(H, 4)).to(DEV))
    return cm.controllers.ILQRBoxController(env, cp, H, iters=k, device=DEV, **kw), cp


def test_ilqr_iterations_over_the_box_sweep():
    s, p, b, _, _, _ = _case("A")
    ds = dev_state(s)
    env = quad_env(task="tracking_zigzag", disturb="none")
    params = env.default_params
    k = 3
    c, cp = _ilqr(env, k, b, plan_hold=2)
    u0, cp1, info = c(None, None, params, KEY, cp, {"noisy_state": ds})
    torch.cuda.synchronize()
    rows = info["ilqr_rows"].cpu().numpy()
    counts = info["ilqr_box_count"].cpu().numpy()
    print(f"  costs {rows[:, 0].tolist()} -> {rows[:, 1].tolist()}; clamped coordinates per iteration {counts.tolist()}")
    assert info["plan_age"] == 0 and tuple(counts.shape) == (k,) and info["ilqr_box_count"].dtype == torch.int32
    for j in range(k - 1):  # one objective per step: the costs chain as words
        assert rows[j + 1, 0].tobytes() == rows[j, 1].tobytes(), j
    assert counts[0] > 0
    assert int(counts[k - 1]) == int(info["riccati_box_count"]) == BO.clamp_count(info["riccati_box_mask"].cpu().numpy())
    # the first iteration's sweep ran at the shifted plan: the stand-alone box sweep there has its masks' count
    b0 = _core().shift_mean(torch.from_numpy(b).to(DEV).clone())
    prim = _core().riccati(ds, c._params_c(params), b0, box=True)
    assert BO.clamp_count(prim["box"][0].cpu().numpy()) == int(counts[0])
    # the hold step: the primitive on the handle's latch -- the last iteration's box gains
    latch = c.core.plan_latch()
    ric = c.core.riccati_rows[0].clone()
    s1 = s.replace(time=int(s.time) + 1, pos=s.pos + 0.01, vel=s.vel - 0.02)
    ds1 = dev_state(s1)
    mean1 = cp1.a_mean.reshape(-1).clone()
    u1, cp2, info1 = c(None, None, params, cr.PRNGKey(6), cp1, {"noisy_state": ds1})
    torch.cuda.synchronize()
    assert info1["plan_age"] == 1
    flags = int(np.ascontiguousarray(ric.cpu().numpy()).view(np.int32)[7]) & 0xFF
    side = torch.tensor([[0.0, 0.0, 0.0, float(flags)]], dtype=torch.float64, device=DEV)
    am = mean1.clone().reshape(1, -1)
    up, rp = c.core.plan_hold(ds1.packed, latch["b"], latch["K"], latch["kff"], latch["x"], ric[3:4].clone(), 1, t_plan=latch["t"],
                              a_mean=am, rows=side)
    torch.cuda.synchronize()
    assert torch.equal(bits32(u1), bits32(up[0])) and torch.equal(bits32(cp2.a_mean.reshape(-1)), bits32(am[0]))
    # ... which are box gains: the rows of K the last sweep clamped are zero in the latch
    cl = clamped(info["riccati_box_mask"].cpu().numpy())
    assert not latch["K"][0].cpu().numpy()[cl].any()
    assert c.core.device_status() == 0
    c.core.close()


def test_ilqr_run_episode_equals_host_calls_under_the_box():
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    T = 6
    got = {}
    for mode in ("fused", "hand"):
        c, _ = cm.envs.get_controller(env, "ilqr", "N64_H32_lam0.01", device=DEV, iters=3, compute_plan=True, riccati_box=True)
        c.alias_outputs = True
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (c.core.lib, c.core.h), DEV)
        cp = c.reset(ep.state0, params, c.init_control_params, cr.PRNGKey(42))
        rng = cr.PRNGKey(43)
        if mode == "hand":
            us, counts = [], []
            for _ in range(T):
                rng, rng_act, rng_step, _c = cr.split(rng, 4)
                u, cp, info = c(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                us.append(u.clone())
                counts.append(info["ilqr_box_count"].clone())
                ep.step(rng_step, u)
                rng, _c = cr.split(rng)
            got["hand"] = (torch.stack(us).cpu().numpy(), ep.read_log())
            print(f"  clamped coordinates per step and iteration {torch.stack(counts).cpu().numpy().tolist()}")
        else:
            cp, rng = c.run_episode(ep, params, cp, rng, 4)
            cp, rng = c.run_episode(ep, params, cp, rng, T - 4)
            got["fused"] = (ep.read_trace()["u"][:T].copy(), ep.read_log())
        got[mode + "_mean"] = cp.a_mean.cpu().numpy().copy()
        got[mode + "_masks"] = c.core.riccati_box_masks.cpu().numpy().copy()
        assert c.core.device_status() == 0
        c.core.close()
    assert got["fused"][0].shape == (T, 4) and got["fused"][0].tobytes() == got["hand"][0].tobytes()
    assert np.array_equal(got["fused"][1], got["hand"][1])
    assert got["fused_mean"].tobytes() == got["hand_mean"].tobytes() and np.array_equal(got["fused_masks"], got["hand_masks"])
