"""GPU tests (-m gpu) of Riccati feedback (covo_feedback_rollout / covo_riccati_refine_feedback / covo_set_step_riccati_feedback;
`riccati_feedback=` on top of `riccati=`; csrc/feedback_rollout.hip, csrc/newton_refine.hip with the closed-loop family).  N = 256
samples and at most 3 instances throughout.

1. the generator against the oracle (tests/feedback_oracle.py) on the device's own sweep (core.riccati at make_problem(seed=17,
   time=37), hover + 0.1 noise), cases (none, penyaw) and (periodic, realworld): the ladder's 16 step sizes from xb_0, and alpha = 0
   with the true kff from a start state moved by +0.05 m / +0.1 m/s.  The device's actions are held against the fp64 loop; the bar is
   twice what the float32 restatement loses on that case plus 2^-23 (the state atlas's convention: the kernel's reciprocals are 1-ulp
   hardware operations where the restatement's are correctly rounded).  At least 8 of the 16 sequences differ from their open-loop
   twin by >= 1e-4, so ignoring K cannot pass.
2. zero gains: bit-equal to fp32(clip(fma(alpha, kff, b))).
3. shapes: n_alpha = 1 and 64; a batch of 3 different states equals its singles bit for bit; the clipped count equals the oracle's
   on hover + 0.3 noise, where the clip is live at every step size.
4. the stand-alone refine with feedback: costs[:17] bit-equal to plain riccati_refine's, choice = the first minimum (NaN / inf never
   win), a closed-loop choice commits the generator's sequence bit for bit, cost_chosen <= plain's, the feedback row agrees with the 33
   costs.
5. invalid input is data: a NaN in K of instance 1 of 2 (covo_debug_feedback_gain) flags its closed-loop candidates -- cost +inf,
   never chosen, the open-loop result is plain refine's; instance 0 is bit-equal to running alone.
6. the production step (mppi, covo-offline, covo-online under sigma_period=4) against a twin with riccati=True alone, same key,
   first step; iters=2 leaves the last pass's rows.
7. batched (E = 3) equals three singles bit for bit in u, a_mean and both rows; 5 steps of run_episode equal 5 host calls, for the
   single controller and for the batched one.
8. refusals, each with its message and before any launch.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd._lib import ptr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from oracle import ref_np as R  # noqa: E402
from tests import feedback_oracle as FO  # noqa: E402
from tests import riccati_oracle as RO  # noqa: E402
from tests.conftest import make_problem  # noqa: E402
from tests.gpu_support import DEV, DP, H, batched_controller, dev_state, params_c, quad_env, single_controller, start_episode  # noqa: E402

RF, FF = _lib.COVO_RICCATI_FLOATS, _lib.COVO_FEEDBACK_FLOATS
NC, NCF = _lib.COVO_REFINE_CANDIDATES, _lib.COVO_FEEDBACK_CANDIDATES
KEY = cr.PRNGKey(5)
LADDER = np.asarray(_lib.FEEDBACK_LADDER)


def bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def ints(t):
    """float32 device tensor -> its int32 words (numpy)"""
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.int32)


def split_row(row):
    """riccati row [8] -> (cost_base, cost_chosen, choice, alpha, flags)"""
    r = row.detach().cpu().numpy()
    i = np.ascontiguousarray(r).view(np.int32)
    return r[0], r[1], int(i[2]), r[3], int(i[7]) & 0xFF


def split_fb(row):
    """feedback row [8] -> (cost_open, cost_closed, index open, index closed, gain, clipped, invalid mask)"""
    r = row.detach().cpu().numpy()
    i = np.ascontiguousarray(r).view(np.int32)
    return r[0], r[1], int(i[2]), int(i[3]), r[4], int(i[5]), int(i[6])


@functools.lru_cache(maxsize=None)
def _core():
    return SamplingCore(256, H, 0.01, 1.0, device=DEV, compute_info=False)


@functools.lru_cache(maxsize=None)
def _problem(noise):
    s, p, rng = make_problem(seed=17, time=37)
    p = p.replace(disturb_params=DP)
    b = (R.hover_action(p, 32, np.float64) + noise * rng.normal(size=(32, 4))).astype(np.float32).reshape(-1)
    return s, p, b


@functools.lru_cache(maxsize=None)
def _sweep(kind, reward, noise):
    """the device's own sweep at the case's plan: (s, p, b, ds, pc, table or None, forces [H, 3], K, kff, x as device tensors)"""
    s, p, b = _problem(noise)
    core = _core()
    ds = dev_state(s)
    pc = params_c(p, kind, reward)
    tab = None if kind == "none" else core.disturb_table(pc, ds.packed, key=KEY, key_mode=_lib.DISTURB_KEYS_HESSIAN, deterministic=True)
    out = core.riccati(ds, pc, torch.from_numpy(b).to(DEV), f_steps=tab)
    torch.cuda.synchronize()
    assert core.device_status() == 0 and out["rows"][0, 3].item() == 0.0
    forces = RO.step_forces(s, p, "none") if tab is None else RO.forces_from_table(s, tab[0].cpu().numpy())
    return s, p, b, ds, pc, tab, forces, out["K"], out["kff"], out["x"]


def _np(t):
    return t[0].cpu().numpy()


# ------------------------------------------------------------------------------------------ 1: the generator against the oracle
@pytest.mark.parametrize("kind,reward", [("none", "penyaw"), ("periodic", "realworld")])
def test_generator_against_the_oracle(kind, reward):
    s, p, b, ds, pc, tab, forces, K, kff, x = _sweep(kind, reward, 0.1)
    core = _core()
    bd = torch.from_numpy(b).to(DEV)
    a_out, aux = core.feedback_rollout(ds, pc, bd, K, kff, x, f_steps=tab)
    torch.cuda.synchronize()
    assert core.device_status() == 0 and tuple(a_out.shape) == (1, 16, 128) and tuple(aux.shape) == (1, 16, 4)
    dev = a_out[0].cpu().numpy().astype(np.float64).reshape(16, H, 4)
    ref64 = FO.closed_loop(s, p, b, _np(K), _np(kff), _np(x), forces)
    ref32 = FO.closed_loop(s, p, b, _np(K), _np(kff), _np(x), forces, dtype=np.float32)
    loss = np.abs(ref32["u"] - ref64["u"]).max()
    err = np.abs(dev - ref64["u"]).max()
    bar = 2.0 * loss + 2.0 ** -23
    print(f"  {kind} {reward}: device vs fp64 {err:.3e}; the float32 restatement loses {loss:.3e}; bar {bar:.3e}; "
          f"|K|max {np.abs(_np(K)).max():.3f}")
    assert np.all(ints(aux[0])[:, 2] == -1) and np.all(ref64["bad"] == -1)
    assert err <= bar, (kind, reward, err, loss)
    # K matters: the open-loop twin along kff is somewhere else
    twin = FO.open_loop(b, _np(kff))
    apart = np.abs(dev - twin).reshape(16, -1).max(axis=1)
    print(f"    max |closed - open twin| per step size: {apart}")
    assert (apart >= 1e-4).sum() >= 8, apart
    g = aux[0, :, 0].cpu().numpy()
    assert np.abs(g - ref64["gain"]).max() <= 1e-5 and np.all(ints(aux[0])[:, 3] == 0)
    # alpha = 0 with the true kff from a moved start state: pure feedback, the tube-MPC use
    packed = ds.packed.clone().reshape(1, -1)
    packed[0, 0:3] += 0.05
    packed[0, 3:6] += 0.1
    x0 = packed[0, :13].cpu().numpy().astype(np.float64)
    a0, aux0 = core.feedback_rollout(ds, pc, bd, K, kff, x, alphas=[0.0], f_steps=tab, packed=packed)
    dev0 = a0[0, 0].cpu().numpy().astype(np.float64).reshape(H, 4)
    m64 = FO.closed_loop(s, p, b, _np(K), _np(kff), _np(x), forces, alphas=[0.0], x0=x0)
    m32 = FO.closed_loop(s, p, b, _np(K), _np(kff), _np(x), forces, alphas=[0.0], x0=x0, dtype=np.float32)
    loss0 = np.abs(m32["u"] - m64["u"]).max()
    err0 = np.abs(dev0 - m64["u"][0]).max()
    moved = np.abs(dev0 - np.clip(b.astype(np.float64), -1, 1).reshape(H, 4)).max()
    print(f"    moved start, alpha = 0: device vs fp64 {err0:.3e}; restatement loses {loss0:.3e}; the feedback moves the plan by {moved:.3e}")
    assert err0 <= 2.0 * loss0 + 2.0 ** -23, (err0, loss0)
    assert moved >= 1e-3 and ints(aux0[0])[0, 2] == -1


# ------------------------------------------------------------------------------------------ 2: zero gains
def test_zero_gains_are_the_open_loop_candidates_bit_for_bit():
    s, p, b, ds, pc, tab, forces, K, kff, x = _sweep("none", "penyaw", 0.3)
    core = _core()
    bd = torch.from_numpy(b).to(DEV)
    a_out, aux = core.feedback_rollout(ds, pc, bd, torch.zeros_like(K), kff, x)
    want = RO.candidates(b, _np(kff).reshape(-1))[1:].astype(np.float32)
    assert a_out[0].cpu().numpy().tobytes() == want.tobytes()
    assert not aux[0, :, 0].any() and np.all(ints(aux[0])[:, 2] == -1)
    # the clipped count is then the open-loop candidates' own
    v = b.astype(np.float64)[None] + LADDER[:, None] * _np(kff).reshape(1, -1)
    assert np.array_equal(ints(aux[0])[:, 1], (np.abs(v) > 1.0).sum(axis=1))
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ 3: shapes
def test_step_size_counts_batches_and_the_clipped_count():
    s, p, b, ds, pc, tab, forces, K, kff, x = _sweep("none", "penyaw", 0.3)
    core = _core()
    bd = torch.from_numpy(b).to(DEV)
    ladder, aux_l = core.feedback_rollout(ds, pc, bd, K, kff, x)
    al64 = np.concatenate([LADDER, np.linspace(0.05, 3.0, 48)])
    a64, aux64 = core.feedback_rollout(ds, pc, bd, K, kff, x, alphas=al64)
    assert tuple(a64.shape) == (1, 64, 128) and tuple(aux64.shape) == (1, 64, 4)
    assert torch.equal(bits32(a64[0, :16]), bits32(ladder[0])) and torch.equal(bits32(aux64[0, :16]), bits32(aux_l[0]))
    for j in (0, 7, 40, 63):  # a lane does not depend on its neighbours
        a1, aux1 = core.feedback_rollout(ds, pc, bd, K, kff, x, alphas=[al64[j]])
        assert tuple(a1.shape) == (1, 1, 128)
        assert torch.equal(bits32(a1[0, 0]), bits32(a64[0, j])) and torch.equal(bits32(aux1[0, 0]), bits32(aux64[0, j])), j
    assert len({a64[0, j].cpu().numpy().tobytes() for j in range(64)}) == 64
    # the clip is live on this case: the counts are the oracle's
    ref = FO.closed_loop(s, p, b, _np(K), _np(kff), _np(x), forces, dtype=np.float32)
    got = ints(aux_l[0])[:, 1]
    print(f"  clipped components per step size: device {got}, oracle {ref['clipped']}")
    assert np.array_equal(got, ref["clipped"]) and np.all(got >= 1) and got[0] == 14
    # a batch of 3 different states and plans equals its singles
    rng = np.random.default_rng(3)
    plans = np.stack([b, (b + 0.05 * rng.normal(size=128)).astype(np.float32), (0.5 * b).astype(np.float32)])
    pd = torch.from_numpy(plans).to(DEV)
    packed = ds.packed.reshape(1, -1).repeat(3, 1)
    packed[1, 0:3] += 0.05
    packed[2, 3:6] -= 0.1
    sw = core.riccati(ds, pc, pd, packed=packed)
    ab, auxb = core.feedback_rollout(ds, pc, pd, sw["K"], sw["kff"], sw["x"], packed=packed)
    for e in range(3):
        a1, aux1 = core.feedback_rollout(ds, pc, pd[e], sw["K"][e:e + 1], sw["kff"][e:e + 1], sw["x"][e:e + 1], packed=packed[e:e + 1])
        assert torch.equal(bits32(ab[e]), bits32(a1[0])) and torch.equal(bits32(auxb[e]), bits32(aux1[0])), e
    assert len({ab[e].cpu().numpy().tobytes() for e in range(3)}) == 3
    torch.cuda.synchronize()
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ 4: the stand-alone refine with feedback
def _check_rows(row, fb, costs, aux):
    """the riccati row and the feedback row against the 33 costs (numpy) and the generator's aux rows"""
    base, chosen, choice, alpha, flags = split_row(row)
    co, cc, io, ic, gain, clipped, mask = split_fb(fb)
    c = np.where(np.isfinite(costs), costs.astype(np.float64), np.inf)
    assert flags == 0 and choice == int(np.argmin(c)) and np.isfinite(c[choice])
    assert base.tobytes() == costs[0].tobytes() and chosen.tobytes() == costs[choice].tobytes()
    j = choice if choice < NC else choice - (NC - 1)
    assert alpha == (2.0 ** (3 - j) if choice else 0.0)
    assert io == int(np.argmin(c[:NC])) and co.tobytes() == costs[io].tobytes()
    a = ints(aux)
    assert mask == sum(1 << q for q in range(16) if a[q, 2] >= 0)
    if np.isfinite(c[NC:]).any():
        assert ic == NC + int(np.argmin(c[NC:])) and cc.tobytes() == costs[ic].tobytes()
        assert gain.tobytes() == aux[ic - NC, 0].cpu().numpy().tobytes() and clipped == a[ic - NC, 1]
    else:
        assert ic == 0 and cc == np.inf and gain == 0.0 and clipped == 0
    assert chosen == min(co, cc) and (choice >= NC) == (cc < co)
    return choice, ic


@pytest.mark.parametrize("noise", [0.1, 0.3])
def test_standalone_refine_with_feedback(noise):
    s, p, b, ds, pc, tab, forces, K, kff, x = _sweep("none", "penyaw", noise)
    core = _core()
    bd = torch.from_numpy(b).to(DEV)
    plain = bd.clone()
    row_p, costs_p = core.riccati_refine(ds, pc, plain)
    am = bd.clone()
    row, costs, fb = core.riccati_refine(ds, pc, am, feedback=True)
    a_out, aux = core.feedback_rollout(ds, pc, bd, K, kff, x)
    torch.cuda.synchronize()
    assert core.device_status() == 0 and tuple(costs.shape) == (NCF,) and tuple(costs_p.shape) == (NC,) and tuple(fb.shape) == (FF,)
    cn = costs.cpu().numpy()
    print(f"  noise {noise}: open {cn[:NC]}\n    closed {cn[NC:]}\n    row {split_row(row)} feedback row {split_fb(fb)}")
    assert torch.equal(bits32(costs[:NC]), bits32(costs_p))
    choice, ic = _check_rows(row, fb, cn, aux[0])
    assert np.isfinite(cn).all() and split_fb(fb)[6] == 0
    assert float(row[1]) <= float(row_p[1])
    assert torch.equal(bits32(row[4:]), bits32(row_p[4:]))  # |g|, g.d, mu, flags | rung: the sweep's, unchanged
    if choice >= NC:
        assert torch.equal(bits32(am), bits32(a_out[0, choice - NC]))
    elif choice >= 1:
        assert torch.equal(bits32(am), bits32(plain)) and int(bits32(row_p[2:3])) == choice
    else:
        assert torch.equal(bits32(am), bits32(bd))
    # every closed-loop cost is the cost of the generator's sequence under the line search's own judge: candidate 16 + j rolled out
    # as a plan of its own is that plan's candidate 0
    for j in (1, 9):
        seq = a_out[0, j - 1].clone()
        _, cj = core.riccati_refine(ds, pc, seq)
        assert torch.equal(bits32(cj[0:1]), bits32(costs[NC - 1 + j:NC + j])), j


# ------------------------------------------------------------------------------------------ 5: invalid input
def _refine_feedback_raw(core, ds, pc, states, means, poke=None):
    """covo_riccati_refine_feedback on n_inst instances through the C ABI -> (rows, costs, feedback rows, means)"""
    n = int(means.shape[0])
    rows = torch.zeros((n, RF), dtype=torch.float32, device=DEV)
    costs = torch.zeros((n, NCF), dtype=torch.float32, device=DEV)
    fbs = torch.zeros((n, FF), dtype=torch.float32, device=DEV)
    am = means.clone()
    if poke is not None:
        _lib.check(core.lib.covo_debug_feedback_gain(core.h, *poke), "covo_debug_feedback_gain")
    with torch.cuda.device(core.device):
        _lib.check(core.lib.covo_riccati_refine_feedback(core.h, ptr(states), ptr(ds.pos_traj), ptr(ds.vel_traj), ds.T, C.byref(pc), None,
                                                         None, None, ptr(am), _lib.COVO_RICCATI_REG0, n, ptr(rows), ptr(costs), ptr(fbs),
                                                         core.stream()), "covo_riccati_refine_feedback")
    torch.cuda.synchronize()
    return rows, costs, fbs, am


def test_a_nan_gain_is_data():
    s, p, b, ds, pc, tab, forces, K, kff, x = _sweep("none", "penyaw", 0.1)
    core = _core()
    rng = np.random.default_rng(4)
    plans = torch.from_numpy(np.stack([b, (b + 0.05 * rng.normal(size=128)).astype(np.float32)])).to(DEV)
    states = ds.packed.reshape(1, -1).repeat(2, 1).contiguous()
    alone = _refine_feedback_raw(core, ds, pc, states[:1], plans[:1])
    clean = _refine_feedback_raw(core, ds, pc, states, plans)
    # K[stage 3][row 1][column 2] of instance 1 becomes NaN between the sweep and the generator
    dirty = _refine_feedback_raw(core, ds, pc, states, plans, poke=(1, 3 * 64 + 1 * 16 + 2, float("nan")))
    assert core.device_status() == 0
    for got in (clean, dirty):  # instance 0 is what it is alone
        for t, t1 in zip(got, alone):
            assert torch.equal(bits32(t[0]), bits32(t1[0]))
    rows, costs, fbs, am = dirty
    co, cc, io, ic, gain, clipped, mask = split_fb(fbs[1])
    base, chosen, choice, alpha, flags = split_row(rows[1])
    print(f"  instance 1 with a NaN gain: choice {choice}, feedback row {split_fb(fbs[1])}; clean: {split_row(clean[0][1])} {split_fb(clean[2][1])}")
    assert mask == 0xFFFF and ic == 0 and cc == np.inf and gain == 0.0 and clipped == 0
    assert bool(torch.isinf(costs[1, NC:]).all()) and bool((costs[1, NC:] > 0).all())
    assert flags == 0 and choice < NC and choice == io
    # its open-loop result is plain refine's
    plain = plans[1].clone()
    row_p, costs_p = core.riccati_refine(ds, pc, plain)
    assert torch.equal(bits32(rows[1]), bits32(row_p)) and torch.equal(bits32(costs[1, :NC]), bits32(costs_p))
    assert torch.equal(bits32(am[1]), bits32(plain))
    again = _refine_feedback_raw(core, ds, pc, states, plans)  # the hook fired once
    for t, t1 in zip(again, clean):
        assert torch.equal(bits32(t), bits32(t1))
    assert split_fb(clean[2][1])[6] == 0
    # the generator alone: flagged at stage 3, clip(b) from there on, nothing undefined in memory
    Kn = K.clone()
    Kn[0, 3, 1, 2] = float("nan")
    a_bad, aux_bad = core.feedback_rollout(ds, pc, plans[0], Kn, kff, x)
    a_ok, _ = core.feedback_rollout(ds, pc, plans[0], K, kff, x)
    assert np.all(ints(aux_bad[0])[:, 2] == 3) and bool(torch.isfinite(a_bad).all()) and bool(torch.isfinite(aux_bad[0, :, 0]).all())
    assert torch.equal(bits32(a_bad[0, :, :12]), bits32(a_ok[0, :, :12]))
    assert torch.equal(a_bad[0, :, 12:], plans[0].clamp(-1, 1)[12:].reshape(1, -1).expand(16, -1))
    torch.cuda.synchronize()
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ 6: the production step
@pytest.mark.parametrize("name,kw", [("mppi", {}), ("covo-offline", {}), ("covo-online", dict(sigma_period=4))],
                         ids=["mppi", "covo-offline", "covo-online-period4"])
def test_production_step_against_a_twin_with_riccati_alone(name, kw):
    N = 256
    env = quad_env(task="tracking_zigzag")
    ca, cp, obs, info, state, params = single_controller(env, name, N, riccati=True, riccati_feedback=True, compute_plan=True, **kw)
    cb, _, _, _, _, _ = single_controller(env, name, N, riccati=True, compute_plan=True, **kw)
    assert cb.core.riccati_feedback_rows is None and tuple(ca.core.riccati_feedback_rows.shape) == (1, FF)
    k_act = cr.split(cr.PRNGKey(11), 3)[1]
    ua, cpa, ia = ca(obs, state, params, k_act, cp, info)
    ub, cpb, ib = cb(obs, state, params, k_act, cp, info)
    torch.cuda.synchronize()
    core = ca.core
    base, chosen, choice, alpha, flags = split_row(core.riccati_rows[0])
    co, cc, io, ic, gain, clipped, mask = split_fb(core.riccati_feedback_rows[0])
    tb = split_row(cb.core.riccati_rows[0])
    print(f"  {name} {kw}: base {base} open {co} (index {io}) closed {cc} (index {ic}, gain {gain}, clipped {clipped}) choice {choice}; "
          f"twin chose {tb[2]} at {tb[1]}")
    assert not any(k in ib for k in ("riccati_closed", "riccati_cost_open", "riccati_cost_closed", "riccati_gain_max"))
    assert ia["riccati_cost_open"].data_ptr() == core.riccati_feedback_rows[0, 0:1].data_ptr()
    assert ia["riccati_closed"].dtype == torch.bool and ia["riccati_closed"].dim() == 0 and bool(ia["riccati_closed"]) == (choice >= NC)
    assert float(ia["riccati_cost_closed"]) == float(cc) and float(ia["riccati_gain_max"]) == float(gain)
    # nothing of the step itself changes, and candidates 0 .. 16 are the twin's
    assert torch.equal(core.a, cb.core.a) and torch.equal(core.cost, cb.core.cost)
    assert torch.equal(bits32(ia["riccati_cost_base"].reshape(1)), bits32(ib["riccati_cost_base"].reshape(1)))
    assert torch.equal(bits32(ia["riccati_cost_open"].reshape(1)), bits32(ib["riccati_cost"].reshape(1)))
    assert io == tb[2] and flags == 0 and mask == 0
    assert float(ia["riccati_cost"]) <= float(ib["riccati_cost"]) and chosen == min(co, cc) and (choice >= NC) == (cc < co)
    assert torch.equal(bits32(ia["cost_plan"].reshape(1)), bits32(ia["riccati_cost"].reshape(1)))
    if choice < NC:
        assert choice == tb[2] and torch.equal(cpa.a_mean, cpb.a_mean) and torch.equal(ua, ub)
    else:
        assert not torch.equal(cpa.a_mean, cpb.a_mean) and torch.equal(cpa.a_mean, cpa.a_mean.clamp(-1, 1))
    assert ca.core.device_status() == 0 and cb.core.device_status() == 0
    ca.core.close()
    cb.core.close()


def _controller(env, N, **kw):
    import covo_mpc_amd as cm
    c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device=DEV, compute_info=False, riccati=True,
                                  riccati_feedback=True, **kw)
    return c, c.init_control_params


def test_iterated_step_leaves_the_last_passes_rows():
    env = quad_env(task="tracking_zigzag")
    c, cp0 = _controller(env, 256, iters=2, compute_plan=True)
    cp, obs, info, state, params = start_episode(env, c, cp0, "covo-online")
    u, cp1, i1 = c(obs, state, params, cr.PRNGKey(11), cp, info)
    torch.cuda.synchronize()
    base, chosen, choice, _, flags = split_row(c.core.riccati_rows[0])
    co, cc, io, ic, gain, clipped, mask = split_fb(c.core.riccati_feedback_rows[0])
    print(f"  base {base} chosen {chosen} choice {choice}; open {co} closed {cc}; pass minima {i1['iter_cost_min'].cpu().numpy()}")
    assert flags == 0 and chosen <= base and chosen == min(co, cc) and mask == 0
    # both rows are the last pass's: its chosen cost is the plan's, which follows the last pass
    assert torch.equal(bits32(i1["cost_plan"].reshape(1)), bits32(c.core.riccati_rows[0, 1:2]))
    assert c.core.device_status() == 0
    c.core.close()


# ------------------------------------------------------------------------------------------ 7: batched, closed loop
def test_batched_feedback_equals_singles():
    import covo_mpc_amd as cm
    N, E = 256, 3
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    act = [np.stack([np.asarray(cr.PRNGKey(60 + 10 * k + e)) for e in range(E)]) for k in range(2)]
    rows, fbs, means, us = [], [], [], []
    for e in range(E):
        c, _ = _controller(env, N)
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        cp = c.reset(se.state0, params[e], c.init_control_params, cr.PRNGKey(2))
        r, f, m, uu = [], [], [], []
        for k in range(2):
            u, cp, _ = c(None, None, params[e], act[k][e], cp, {"noisy_state": se.noisy_state})
            torch.cuda.synchronize()
            r.append(c.core.riccati_rows[0].clone())
            f.append(c.core.riccati_feedback_rows[0].clone())
            m.append(cp.a_mean.reshape(-1).clone())
            uu.append(u.reshape(-1).clone())
        rows.append(r), fbs.append(f), means.append(m), us.append(uu)
        cp0 = c.init_control_params
        c.core.close()
    b = batched_controller(env, "covo-online", cp0, E, N, 0.01, riccati=True, riccati_feedback=True)
    assert tuple(b.riccati.shape) == (E, RF) and tuple(b.riccati_feedback.shape) == (E, FF)
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    b.bind_episode(ep)
    for k in range(2):
        u = b(None, act[k])
        torch.cuda.synchronize()
        for e in range(E):
            assert torch.equal(bits32(b.riccati[e]), bits32(rows[e][k])), (k, e, b.riccati[e], rows[e][k])
            assert torch.equal(bits32(b.riccati_feedback[e]), bits32(fbs[e][k])), (k, e, b.riccati_feedback[e], fbs[e][k])
            assert torch.equal(bits32(b.a_mean[e].reshape(-1)), bits32(means[e][k])), (k, e)
            assert torch.equal(bits32(u[e].reshape(-1)), bits32(us[e][k])), (k, e)
    print(f"  choices {[[split_row(rows[e][k])[2] for k in range(2)] for e in range(E)]}; "
          f"closed-loop bests {[[split_fb(fbs[e][k])[3] for k in range(2)] for e in range(E)]}")
    assert b.core.device_status() == 0
    b.core.close()


def test_run_episode_equals_host_calls():
    import covo_mpc_amd as cm
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    T = 5
    got = {}
    for mode in ("fused", "hand"):
        c, _ = _controller(env, 256, compute_plan=True)
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
                ch.append(split_row(c.core.riccati_rows[0])[2])
                ep.step(rng_step, u)
                rng, _c = cr.split(rng)
            got["hand"] = (torch.stack(us).cpu().numpy(), ep.read_log(), ch)
        else:
            cp, rng = c.run_episode(ep, params, cp, rng, 3)
            cp, rng = c.run_episode(ep, params, cp, rng, T - 3)
            got["fused"] = (ep.read_trace()["u"][:T].copy(), ep.read_log())
        assert c.core.device_status() == 0
        c.core.close()
    print(f"  choices of the 5 steps: {got['hand'][2]}")
    assert got["fused"][0].shape == (T, 4) and got["fused"][0].tobytes() == got["hand"][0].tobytes()
    assert np.array_equal(got["fused"][1], got["hand"][1])


def test_batched_run_episode_equals_host_calls():
    """covo_run_episode_batched for 5 steps in two segments on E = 3 instances equals the hand-stepped loop of __call__ +
    episode.step bit for bit: the env log, and what the last step leaves in the means and in both rows"""
    import covo_mpc_amd as cm
    N, E, T = 256, 3, 5
    env = quad_env(task="tracking", randomizer=True)
    params = [env.sample_params(cr.PRNGKey(40 + e)) for e in range(E)]
    reset_keys = [cr.PRNGKey(50 + e) for e in range(E)]
    rngs0 = np.stack([np.asarray(cr.PRNGKey(60 + e)) for e in range(E)])
    c0, cp0 = _controller(env, N)
    c0.core.close()
    got = {}
    for mode in ("fused", "hand"):
        b = batched_controller(env, "covo-online", cp0, E, N, 0.01, riccati=True, riccati_feedback=True)
        ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
        if mode == "hand":
            b.bind_episode(ep)
            rngs = [rngs0[e] for e in range(E)]
            for _ in range(T):
                sp = [cr.split(r, 4) for r in rngs]
                b(None, np.stack([np.asarray(x[1]) for x in sp]))
                ep.step(np.stack([np.asarray(x[2]) for x in sp]), b.a_mean)
                rngs = [cr.split(x[0])[0] for x in sp]
        else:
            keys = b.run_episode(ep, rngs0.copy(), 3)
            b.run_episode(ep, keys, T - 3)
        got[mode] = (ep.read_log(), b.a_mean.clone(), b.riccati.clone(), b.riccati_feedback.clone())
        assert b.core.device_status() == 0
        b.core.close()
    assert np.array_equal(got["fused"][0], got["hand"][0])
    for f, h in zip(got["fused"][1:], got["hand"][1:]):
        assert torch.equal(bits32(f), bits32(h))
    print(f"  last step: choices {[split_row(r)[2] for r in got['hand'][2]]}, closed-loop bests {[split_fb(r)[3] for r in got['hand'][3]]}")


# ------------------------------------------------------------------------------------------ 8: refusals
def test_refusals_name_their_condition_before_any_launch():
    env = quad_env(task="tracking_zigzag")
    fb_rows = torch.zeros((3, FF), dtype=torch.float32, device=DEV)

    def step_refused(c, cp, obs, info, state, params, match):
        c.core.a.fill_(7.0)
        before = cp.a_mean.clone()
        with pytest.raises(_lib.CovoError, match=match):
            c(obs, state, params, cr.PRNGKey(11), cp, info)
        torch.cuda.synchronize()
        assert bool((c.core.a == 7.0).all()) and torch.equal(cp.a_mean, before) and not fb_rows.any()  # nothing ran
        assert c.core.device_status() == 0

    # attached without the Riccati refinement: at the setter ...
    c, cp, obs, info, state, params = single_controller(env, "mppi", 256)
    assert c.core.lib.covo_set_step_riccati_feedback(c.core.h, ptr(fb_rows), 1) != 0
    assert b"needs the Riccati refinement attached" in c.core.lib.covo_last_error()
    c.core.close()
    # ... and at the step, when the refinement is detached under it; more rows than the refinement has
    c, cp, obs, info, state, params = single_controller(env, "mppi", 256, riccati=True, riccati_feedback=True)
    assert c.core.lib.covo_set_step_riccati_feedback(c.core.h, ptr(fb_rows), 2) != 0
    assert b"at least as many instances" in c.core.lib.covo_last_error()
    _lib.check(c.core.lib.covo_set_step_riccati_feedback(c.core.h, ptr(fb_rows), 1), "covo_set_step_riccati_feedback")
    _lib.check(c.core.lib.covo_set_step_riccati(c.core.h, None, 0), "covo_set_step_riccati")
    step_refused(c, cp, obs, info, state, params, "without the Riccati refinement")
    c.core.close()
    # drag at the step (the Python surface refuses it at construction; the rows are attached by hand)
    drag = quad_env(task="tracking_zigzag", disturb="drag")
    with pytest.raises(NotImplementedError, match="16-state plants"):
        single_controller(drag, "mppi", 256, riccati=True, riccati_feedback=True)
    c, cp, obs, info, state, params = single_controller(drag, "mppi", 256, riccati=True)
    _lib.check(c.core.lib.covo_set_step_riccati_feedback(c.core.h, ptr(fb_rows), 1), "covo_set_step_riccati_feedback")
    step_refused(c, cp, obs, info, state, params, "drag / mixed")
    # ... and in the stand-alone calls
    s, p, b = _problem(0.1)
    ds, pcd = dev_state(s), params_c(p, "drag", "penyaw")
    tabd = c.core.disturb_table(pcd, ds.packed, key=KEY, key_mode=_lib.DISTURB_KEYS_HESSIAN, deterministic=True)
    bd = torch.from_numpy(b).to(DEV)
    with pytest.raises(NotImplementedError, match="16-state plant"):
        c.core.riccati_refine(ds, pcd, bd.clone(), f_steps=tabd, f_steps_hessian=tabd, feedback=True)
    z = torch.zeros(1, dtype=torch.float64, device=DEV)
    with pytest.raises(NotImplementedError, match="16-state plant"):
        c.core.feedback_rollout(ds, pcd, bd, z.expand(32 * 64), z.expand(32 * 4), z.expand(32 * 16), f_steps=tabd)
    am = bd.clone()
    rc = c.core.lib.covo_riccati_refine_feedback(c.core.h, ptr(ds.packed), ptr(ds.pos_traj), ptr(ds.vel_traj), ds.T, C.byref(pcd), None,
                                                 ptr(tabd), ptr(tabd), ptr(am), 1e-2, 1, ptr(fb_rows), None, ptr(fb_rows), c.core.stream())
    assert rc != 0 and b"16-state plant" in c.core.lib.covo_last_error()
    torch.cuda.synchronize()
    assert torch.equal(am, bd) and not fb_rows.any()
    c.core.close()
    # more instances than rows
    bc = batched_controller(quad_env(task="tracking", randomizer=True), "covo-online", cp, 3, 256, 0.01, riccati=True, riccati_feedback=True)
    _lib.check(bc.core.lib.covo_set_step_riccati_feedback(bc.core.h, ptr(fb_rows), 2), "covo_set_step_riccati_feedback")
    import covo_mpc_amd as cm
    renv = quad_env(task="tracking", randomizer=True)
    ps = [renv.sample_params(cr.PRNGKey(40 + e)) for e in range(3)]
    ep = cm.envs.BatchedDeviceEpisode(renv, [cr.PRNGKey(50 + e) for e in range(3)], ps, (bc.core.lib, bc.core.h), DEV)
    bc.bind_episode(ep)
    before = bc.a_mean.clone()
    with pytest.raises(_lib.CovoError, match=r"3 instances, the feedback buffer \(covo_set_step_riccati_feedback\) has n_inst=2"):
        bc(None, np.stack([np.asarray(cr.PRNGKey(60 + e)) for e in range(3)]))
    torch.cuda.synchronize()
    assert torch.equal(bc.a_mean, before) and not fb_rows.any() and bc.core.device_status() == 0
    bc.core.close()
