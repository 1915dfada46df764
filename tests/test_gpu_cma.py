"""GPU: the CMA controller -- csrc/cma_path.hip against tests/cma_oracle.py, and the step, the batch and the episode
drivers against the stand-alone kernels.

Bars.  The kernel's p and log s: 1e-10 relative (max |dp| / max |p|; |d log s| / max(|log s|, 1)) against the fp64 oracle -- the forward
substitution's own bound is n u cond(L) ~ 1.4e-12 at cond(Sigma) = 1e4; the measured worst is printed with its conditioning.  The row is
fp32: every entry within one fp32 ulp of the fp32 rounding of the oracle's fp64 value (a 1e-10 difference can only flip the rounding),
the flag word exact.  L' and Sigma': within one fp32 ulp of fp32(s_oracle L_hat') and fp32(s_oracle^2 Sigma_hat'); zeros and symmetry
exact.  Everything the step, the batch and the episode drivers are held to is torch.equal against the stand-alone launches on the
recorded inputs."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

pytestmark = pytest.mark.gpu

import covo_mpc_amd as cm  # noqa: E402
from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd import random as cr  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from tests import cma_oracle as CO  # noqa: E402
from tests import contract_support as CS  # noqa: E402
from tests import update_oracle as UO  # noqa: E402
from tests.gpu_support import DEV, H, instances, quad_env, ulps  # noqa: E402
from tests.sigma_shift_oracle import random_spd  # noqa: E402

N_A, SIG0, N, LAM = 128, 0.5, 256, 0.01
CONDS = (1e0, 1e2, 1e4)
D_SCALES = (1e-3, 3e-2, 0.5)
ESSES = (1.0, 7.3, float(N))
BAR = 1e-10
ST_TIME = 25
f64 = dict(dtype=torch.float64, device=DEV)
f32 = dict(dtype=torch.float32, device=DEV)


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device=DEV, dtype=dtype).contiguous()


# ---- 1. the stand-alone kernel ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core():
    c = SamplingCore(N, H, LAM, 1.0, device=DEV, use_graph=False, compute_info=False)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(core):
    """Every (L, d, ess): L = sigma0 I and the fp32 factors of random SPD matrices at cond 1e0, 1e2, 1e4; d random at three scales and
    d = 0; ess in {1, 7.3, N} -- 48 instances, each with its own start p (random) and log s (in [-0.5, 0.5]), its own posterior
    covariance C (a rank-40 cloud) and the shape covo_sigma_adapt gives for it.  The oracle's answers, computed once."""
    rng = np.random.default_rng(11)
    Ls = [(SIG0 * np.eye(N_A)).astype(np.float32)] + [np.linalg.cholesky(random_spd(rng, c)).astype(np.float32) for c in CONDS]
    conds = [1.0] + list(CONDS)
    rows = []
    for li, L in enumerate(Ls):
        for ds in D_SCALES + (0.0,):
            for ess in ESSES:
                X = rng.normal(size=(40, N_A)) * 0.2
                rows.append(dict(L=L, cond=conds[li], d=(ds * rng.normal(size=N_A)).astype(np.float32), ess=np.float32(ess), W=np.float32(1.7),
                                 p=rng.normal(size=N_A) * 0.7, ls=rng.uniform(-0.5, 0.5), C=(X.T @ X / 40.0).astype(np.float32)))
    Lb, Cb = dev(np.stack([r["L"] for r in rows])), dev(np.stack([r["C"] for r in rows]))
    Sh, Lh, srows = core.sigma_adapt(Lb, Cb, 0.2, SIG0)
    torch.cuda.synchronize()
    assert not bool(srows[:, 0].any())
    for i, r in enumerate(rows):
        r["Lh"], r["Sh"] = Lh[i].cpu().numpy(), Sh[i].cpu().numpy()
        r["ref"] = CO.step_size(r["L"], r["d"], r["W"], r["ess"], r["p"], r["ls"], N)
    return rows, Lb, Lh.contiguous(), Sh.contiguous(), srows.contiguous()


def run_kernel(core, rows, idx, Lb, Lh, Sh, srows=None, **kw):
    """covo_cma_path on the instances idx as one batch -> (L', Sigma', rows, p, log s) as numpy"""
    idx = list(idx)
    p = dev(np.stack([rows[i]["p"] for i in idx]), torch.float64)
    ls = dev(np.array([rows[i]["ls"] for i in idx]), torch.float64)
    d = dev(np.stack([rows[i]["d"] for i in idx]))
    ess = dev(np.array([rows[i]["ess"] for i in idx], dtype=np.float32))
    W = dev(np.array([rows[i]["W"] for i in idx], dtype=np.float32))
    sel = torch.tensor(idx, device=DEV)
    Lo, So, out = core.cma_path(Lb[sel].contiguous(), d, ess, p, ls, Lh[sel].contiguous(), Sh[sel].contiguous(), W=W,
                                shape_rows=None if srows is None else srows[sel].contiguous(), **kw)
    torch.cuda.synchronize()
    return Lo.cpu().numpy(), So.cpu().numpy(), out.cpu().numpy(), p.cpu().numpy(), ls.cpu().numpy()


def check_against_oracle(r, Lo, So, row, p, ls, where):
    p_ref, ls_ref, row_ref = r["ref"]
    e_p = np.abs(p - p_ref).max() / max(np.abs(p_ref).max(), 1e-300)
    e_ls = abs(ls - ls_ref) / max(abs(ls_ref), 1.0)
    assert e_p <= BAR and e_ls <= BAR, (where, e_p, e_ls, r["cond"])
    assert row[7] == row_ref[7], (where, row, row_ref)
    assert ulps(row[:7], row_ref[:7].astype(np.float32)) <= 1.0, (where, row, row_ref)
    Lr, Sr = CO.scale(np.exp(ls_ref), r["Lh"], r["Sh"])
    assert ulps(Lo, Lr) <= 1.0 and ulps(So, Sr) <= 1.0, where
    assert not np.triu(Lo, 1).any() and np.array_equal(So.view(np.uint32), So.T.copy().view(np.uint32)), where
    assert np.isfinite(Lo).all() and (np.diag(Lo) > 0).all(), where
    return e_p, e_ls


def test_kernel_against_the_oracle_in_batches_of_three_and_alone(core, cases):
    rows, Lb, Lh, Sh, srows = cases
    worst = {}
    order = np.random.default_rng(2).permutation(len(rows))  # every batch mixes factors, scales and ess
    for k in range(0, len(rows), 3):
        idx = [int(i) for i in order[k:k + 3]]
        Lo, So, out, p, ls = run_kernel(core, rows, idx, Lb, Lh, Sh, srows)
        for j, i in enumerate(idx):
            e = check_against_oracle(rows[i], Lo[j], So[j], out[j], p[j], ls[j], i)
            c = rows[i]["cond"]
            worst[c] = np.maximum(worst.get(c, np.zeros(2)), e)
        if k % 12 == 0:  # a third of the instances alone: the bits of their batch row
            i = idx[1]
            L1, S1, o1, p1, l1 = run_kernel(core, rows, [i], Lb, Lh, Sh, srows)
            for a, b in ((L1[0], Lo[1]), (S1[0], So[1]), (o1[0], out[1]), (p1[0], p[1]), (l1[0], ls[1])):
                assert np.array_equal(np.asarray(a), np.asarray(b)), i
    for c, e in sorted(worst.items()):
        print(f"  cond(Sigma) {c:g}: worst p error {e[0]:.2e}, log s {e[1]:.2e} (bar {BAR:g}; substitution bound n u cond(L) = "
              f"{N_A * 2.0 ** -53 * np.sqrt(c):.1e})")
    # the three ess give three different mu_eff, and N caps it
    mus = {float(r["ref"][2][4]) for r in rows}
    assert mus == {1.0, float(np.float32(7.3)), float(N)}


def test_step_size_off_only_copies(core, cases):
    rows, Lb, Lh, Sh, srows = cases
    idx = [5, 20, 40]
    Lo, So, out, p, ls = run_kernel(core, rows, idx, Lb, Lh, Sh, srows, step_size=False)
    for j, i in enumerate(idx):
        assert np.array_equal(Lo[j], rows[i]["Lh"]) and np.array_equal(So[j], rows[i]["Sh"]), i
        assert np.array_equal(out[j], CO.NEUTRAL_ROW.astype(np.float32)), i
        assert np.array_equal(p[j], rows[i]["p"]) and ls[j] == rows[i]["ls"], i


def test_in_place_and_run_to_run(core, cases):
    rows, Lb, Lh, Sh, srows = cases
    idx = [7, 19, 46]
    a = run_kernel(core, rows, idx, Lb, Lh, Sh, srows)
    b = run_kernel(core, rows, idx, Lb, Lh, Sh, srows)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    sel = torch.tensor(idx, device=DEV)
    Lio, Sio = Lb[sel].clone(), Sh[sel].clone()  # as the step does it: L' over L, Sigma' over the shape's Sigma
    c = run_kernel(core, rows, idx, Lb, Lh, Sh, srows)  # (fresh p / log s)
    p = dev(np.stack([rows[i]["p"] for i in idx]), torch.float64)
    ls = dev(np.array([rows[i]["ls"] for i in idx]), torch.float64)
    Lo, So, out = core.cma_path(Lio, dev(np.stack([rows[i]["d"] for i in idx])), dev(np.array([rows[i]["ess"] for i in idx], dtype=np.float32)),
                                p, ls, Lh[sel].contiguous(), Sio, W=dev(np.array([rows[i]["W"] for i in idx], dtype=np.float32)),
                                shape_rows=srows[sel].contiguous(), L_out=Lio, Sigma_out=Sio)
    torch.cuda.synchronize()
    assert Lo is Lio and So is Sio
    assert np.array_equal(Lio.cpu().numpy(), c[0]) and np.array_equal(Sio.cpu().numpy(), c[1]) and np.array_equal(out.cpu().numpy(), c[2])
    assert np.array_equal(p.cpu().numpy(), c[3])


@pytest.mark.parametrize("fault", ["W=0", "nan in d", "zero pivot", "inf ess", "clamp", "shape fell back"])
def test_fall_backs_flag_one_instance_and_leave_its_neighbours_alone(core, cases, fault):
    """A batch of three whose middle instance is faulty: its flag, its unchanged p and log s, a finite L'; the neighbours' outputs are
    the bits of the same batch without the fault.  Finite work throughout: the checks are arithmetic, the launch completes normally."""
    rows, Lb, Lh, Sh, srows = cases
    idx = [13, 27, 38]
    clean = run_kernel(core, rows, idx, Lb, Lh, Sh, srows)
    mid = dict(rows[idx[1]])
    Lb2, srows2, kw, want = Lb.clone(), srows.clone(), {}, CO.FLAG_KEPT
    if fault == "W=0":
        mid["W"] = np.float32(0.0)
    elif fault == "nan in d":
        mid["d"] = mid["d"].copy()
        mid["d"][77] = np.nan
    elif fault == "zero pivot":
        Lb2[idx[1], 50, 50] = 0.0
    elif fault == "inf ess":
        mid["ess"] = np.float32(np.inf)
    elif fault == "clamp":  # a displacement of 40 sigma along every axis: log s leaves [log s_min, log s_max] at once
        mid["d"] = (40.0 * (mid["L"].astype(np.float64) @ np.ones(N_A))).astype(np.float32)
        kw, want = dict(s_max=1.05), CO.FLAG_CLAMP
        clean = run_kernel(core, rows, idx, Lb, Lh, Sh, srows, **kw)
    else:
        srows2[idx[1], 0] = 1.0
        want = CO.FLAG_SHAPE
    rows2 = list(rows)
    rows2[idx[1]] = mid
    Lo, So, out, p, ls = run_kernel(core, rows2, idx, Lb2, Lh, Sh, srows2, **kw)
    assert int(out[1, 7]) == want, out[1]
    assert np.isfinite(Lo).all() and np.isfinite(So).all() and (np.diagonal(Lo, axis1=1, axis2=2) > 0).all()
    if want == CO.FLAG_KEPT:
        assert np.array_equal(p[1], mid["p"]) and ls[1] == mid["ls"]
        assert ulps(out[1, :3], np.array([np.exp(mid["ls"]), mid["ls"], np.linalg.norm(mid["p"])], dtype=np.float32)) <= 1.0, out[1]
        assert not out[1, 3:7].any()
        Lr, Sr = CO.scale(np.exp(mid["ls"]), mid["Lh"], mid["Sh"])
        assert ulps(Lo[1], Lr) <= 1.0 and ulps(So[1], Sr) <= 1.0
    elif want == CO.FLAG_CLAMP:
        assert ls[1] == np.log(float(np.float32(1.05))) and not np.array_equal(p[1], mid["p"])
    else:
        assert np.array_equal(p[1], clean[3][1]) and ls[1] == clean[4][1] and np.array_equal(Lo[1], clean[0][1])
    for j in (0, 2):
        for x, y in zip((Lo, So, out, p, ls), clean):
            assert np.array_equal(x[j], y[j]), (fault, j)
    assert core.device_status() == 0


def test_a_state_handed_over_broken_is_mended_before_it_is_used(core, cases):
    """The stand-alone entry takes p and log s from the caller.  A log s of 800 on an instance that falls back (W = 0) is held at
    log s_max, so exp() does not overflow into L'; a NaN in p makes that path count as 0, so it does not stay NaN for ever; a NaN
    log s counts as 0.  Each against the oracle, which states the same rule; the stored state is the mended one."""
    rows, Lb, Lh, Sh, srows = cases
    idx = [16, 28, 41]
    rows2 = list(rows)
    a, b, c = (dict(rows[i]) for i in idx)
    a["ls"], a["W"] = 800.0, np.float32(0.0)
    b["p"] = b["p"].copy()
    b["p"][5] = np.nan
    c["ls"] = np.nan
    for i, r in zip(idx, (a, b, c)):
        r["ref"] = CO.step_size(r["L"], r["d"], r["W"], r["ess"], r["p"], r["ls"], N)
        rows2[i] = r
    Lo, So, out, p, ls = run_kernel(core, rows2, idx, Lb, Lh, Sh, srows)
    assert np.isfinite(Lo).all() and np.isfinite(So).all() and np.isfinite(p).all() and np.isfinite(ls).all()
    for j, i in enumerate(idx):
        check_against_oracle(rows2[i], Lo[j], So[j], out[j], p[j], ls[j], i)
    assert ls[0] == np.log(float(np.float32(4.0))) and int(out[0, 7]) == CO.FLAG_KEPT and out[0, 0] == np.float32(4.0)
    assert int(out[1, 7]) in (0, CO.FLAG_CLAMP) and int(out[2, 7]) in (0, CO.FLAG_CLAMP)
    # what a path of exactly 0 and a log s of exactly 0 give, bit for bit
    b0, c0 = dict(rows[idx[1]]), dict(rows[idx[2]])
    b0["p"], c0["ls"] = np.zeros(N_A), 0.0
    rows3 = list(rows)
    rows3[idx[1]], rows3[idx[2]] = b0, c0
    L3, S3, o3, p3, l3 = run_kernel(core, rows3, idx, Lb, Lh, Sh, srows)
    for j in (1, 2):
        for x, y in ((Lo, L3), (So, S3), (out, o3), (p, p3), (ls, l3)):
            assert np.array_equal(x[j], y[j]), j
    assert core.device_status() == 0


def _raw_call(core, T, E, stream=None):
    return core.lib.covo_cma_path(core.h, _lib.ptr(T["L"]), _lib.ptr(T["aux"]), _lib.COVO_POST_AUX_FLOATS, _lib.ptr(T["ess"]), 1,
                                  _lib.ptr(T["Lh"]), _lib.ptr(T["Sh"]), _lib.ptr(T["srows"]), E, N, 1, 1.0, 0.1, 4.0, _lib.ptr(T["p"]),
                                  _lib.ptr(T["ls"]), _lib.ptr(T["Lo"]), _lib.ptr(T["So"]), _lib.ptr(T["rows"]),
                                  core.stream() if stream is None else stream)


def _raw_inputs(rows, idx, Lb, Lh, Sh, srows):
    sel = torch.tensor(idx, device=DEV)
    aux = np.zeros((len(idx), _lib.COVO_POST_AUX_FLOATS), dtype=np.float32)
    for j, i in enumerate(idx):
        aux[j, :N_A], aux[j, N_A] = rows[i]["d"], rows[i]["W"]
    return dict(L=Lb[sel].cpu().numpy(), aux=aux, ess=np.array([rows[i]["ess"] for i in idx], dtype=np.float32), Lh=Lh[sel].cpu().numpy(),
                Sh=Sh[sel].cpu().numpy(), srows=srows[sel].cpu().numpy(), p=np.stack([rows[i]["p"] for i in idx]),
                ls=np.array([rows[i]["ls"] for i in idx]))


@pytest.mark.parametrize("poison", CS.POISONS)
def test_extents_guard_bands_around_every_buffer_stay_unwritten(core, cases, poison):
    """Every buffer of a batch-of-3 call inside guard bands, outputs poison-filled: no band loses a word, every output element is
    written, the inputs keep their bits, and the results are those of the plain call whatever the poison."""
    rows, Lb, Lh, Sh, srows = cases
    idx = [2, 30, 45]
    X = _raw_inputs(rows, idx, Lb, Lh, Sh, srows)
    al = {k: CS.banded(v, poison, device=DEV, name=k) for k, v in X.items()}
    al["Lo"] = CS.banded_empty((3, N_A, N_A), torch.float32, poison, device=DEV, name="Lo")
    al["So"] = CS.banded_empty((3, N_A, N_A), torch.float32, poison, device=DEV, name="So")
    al["rows"] = CS.banded_empty((3, 8), torch.float32, poison, device=DEV, name="rows")
    torch.cuda.synchronize()
    assert _raw_call(core, {k: a.view for k, a in al.items()}, 3) == 0
    torch.cuda.synchronize()
    for k, a in al.items():
        assert CS.bands_intact(a) is None, CS.bands_intact(a)
    for k in ("Lo", "So", "rows"):
        assert CS.unwritten(al[k]).size == 0, k
    for k in ("L", "aux", "ess", "Lh", "Sh", "srows"):
        assert np.array_equal(al[k].view.cpu().numpy().view(np.uint32), np.ascontiguousarray(X[k]).view(np.uint32)), k
    want = run_kernel(core, rows, idx, Lb, Lh, Sh, srows)
    got = [al[k].view.cpu().numpy() for k in ("Lo", "So", "rows", "p", "ls")]
    for x, y in zip(got, want):
        assert np.array_equal(x, y)


def test_the_launch_runs_on_the_callers_stream(core, cases):
    """The inputs hold NaN; a side stream sleeps, then copies the real values in, then the call follows on it and the inputs are
    spoiled again behind it: work on another stream would read NaN (flag 1, p unchanged) -- the outputs must be the default stream's."""
    rows, Lb, Lh, Sh, srows = cases
    idx = [9, 22, 35]
    X = _raw_inputs(rows, idx, Lb, Lh, Sh, srows)
    want = run_kernel(core, rows, idx, Lb, Lh, Sh, srows)
    stage = {k: dev(v, torch.float64 if v.dtype == np.float64 else torch.float32) for k, v in X.items()}
    T = {k: torch.full_like(v, float("nan")) for k, v in stage.items()}
    T.update(Lo=torch.zeros((3, N_A, N_A), **f32), So=torch.zeros((3, N_A, N_A), **f32), rows=torch.zeros((3, 8), **f32))
    bad = {k: torch.full_like(v, float("nan")) for k, v in stage.items()}
    side = torch.cuda.Stream()
    per_ms = CS.sleep_cycles_per_ms(torch)
    torch.cuda.synchronize()
    const = ("L", "aux", "ess", "Lh", "Sh", "srows")
    rc, slept = CS.delayed(side, [(T[k], stage[k]) for k in stage], cycles=int(per_ms * 10.0), call=lambda: _raw_call(core, T, 3),
                           spoil=[(T[k], bad[k]) for k in const])
    torch.cuda.synchronize()
    assert rc == 0 and slept >= 5.0, slept
    got = [T[k].cpu().numpy() for k in ("Lo", "So", "rows", "p", "ls")]
    for x, y in zip(got, want):
        assert np.array_equal(x, y)


# ---- 2. the step --------------------------------------------------------------------------------------------------------------------
def build(env, n=N, **kw):
    dp = env.default_params
    th = (dp.m * dp.g / dp.max_thrust) * 2.0 - 1.0
    cp = cm.controllers.CMAParams(gamma_mean=1.0, discount=1.0, sample_sigma=SIG0,
                                  a_mean=torch.tensor([th, 0.0, 0.0, 0.0], **f32).repeat(H, 1), a_cov=torch.eye(N_A, **f32) * SIG0 ** 2)
    return cm.controllers.CMAController(env, cp, n, H, LAM, device=DEV, compute_info=False, **kw)


def walk(c, env, n, seed=1):
    """n closed-loop steps from reset() -> one record per step: what the step returned and what it left on the handle."""
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(seed), params)
    cp = c.reset(state, params, c.init_control_params, cr.PRNGKey(seed + 1))
    key, recs, core = cr.PRNGKey(seed + 2), [], c.core
    for t in range(n):
        key, k_act, k_step = cr.split(key, 3)
        before = cp.a_mean.clone()
        u, cp, out = c(obs, state, params, k_act, cp, info)
        recs.append(dict(before=before, mean=cp.a_mean.clone(), a_cov=cp.a_cov.clone(), L=core.sigma_factor(), rows=core.cma_rows.clone(),
                         path=core.cma_p.clone(), C=core.post_cov.clone(), aux=core.post_aux.clone(), diag=core.diag.clone(),
                         cost=core.cost.clone(), a=core.a.clone(), info={k: v.clone() for k, v in out.items() if k.startswith("cma_")},
                         ess=out["ess"].clone(), k_act=np.asarray(k_act), around=core._bufs["a_mean_shift"].clone()))
        obs, state, _, _, info = env.step(k_step, state, u.cpu().numpy(), params)
    torch.cuda.synchronize()
    assert core.device_status() == 0
    return recs


def replay(core, recs, gamma=0.2, n_samples=N, **kw):
    """The stand-alone covo_sigma_adapt followed by covo_cma_path on every step's recorded factor, C, d, W and ess, the path and log s
    carried from the reset state -> [(L', Sigma', rows, p)] for steps 1 .. n - 1"""
    p, ls = torch.zeros((1, N_A), **f64), torch.zeros((1,), **f64)
    out = []
    for prev in recs[:-1]:
        Sh, Lh, srows = core.sigma_adapt(prev["L"].reshape(1, N_A, N_A), prev["C"].reshape(1, N_A, N_A).contiguous(), gamma, SIG0)
        Lo, So, rows = core.cma_path(prev["L"], prev["aux"][:, :N_A].contiguous(), prev["diag"][:, 0].contiguous(), p, ls, Lh, Sh,
                                     W=prev["aux"][:, N_A].contiguous(), shape_rows=srows, n_samples=n_samples, **kw)
        out.append((Lo[0].clone(), So[0].clone(), rows.clone(), p.clone()))
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_four_steps_equal_the_stand_alone_kernels_on_the_recorded_inputs(core, graph):
    env = quad_env(task="tracking_zigzag")
    c = build(env, use_graph=graph)
    recs = walk(c, env, 4)
    first = recs[0]
    assert np.abs(first["a_cov"].cpu().numpy() - SIG0 ** 2 * np.eye(N_A)).max() <= 1e-6
    assert torch.equal(first["L"], SIG0 * torch.eye(N_A, **f32))
    assert np.array_equal(first["rows"].cpu().numpy()[0], CO.NEUTRAL_ROW.astype(np.float32)) and not bool(first["path"].any())
    for t, (Lo, So, rows, p) in enumerate(replay(core, recs), start=1):
        r = recs[t]
        assert torch.equal(r["L"], Lo) and torch.equal(r["a_cov"], So), t
        assert torch.equal(r["rows"], rows) and torch.equal(r["path"], p), t
        row = rows[0].cpu().numpy()
        assert row[7] == 0 and row[0] != 1.0 and row[4] == np.float32(min(max(float(recs[t - 1]["diag"][0, 0]), 1.0), N)), (t, row)
        assert torch.equal(r["info"]["cma_scale"], rows[0, 0]) and torch.equal(r["info"]["cma_rows"], rows[0]), t
        assert torch.equal(r["info"]["cma_path_norm"], rows[0, 2]) and torch.equal(r["info"]["cma_mu_eff"], rows[0, 4]), t
        # the oracle on the same recorded inputs (fp64 from the recorded fp32 factor): the step size of the step
        prev = recs[t - 1]
        ref = CO.step_size(prev["L"].cpu().numpy(), prev["aux"][0, :N_A].cpu().numpy(), float(prev["aux"][0, N_A]), float(prev["diag"][0, 0]),
                           recs[t - 1]["path"][0].cpu().numpy(), np.float64(recs[t - 1]["rows"][0, 1].item()) if t == 1 else ls_prev, N)
        ls_prev = ref[1]
        assert abs(float(row[1]) - ref[1]) <= 1e-6 * max(abs(ref[1]), 1.0), (t, row, ref[2])
    for t, r in enumerate(recs):
        UO.check_update((r["cost"], r["a"]), r["before"], 1.0, LAM, r["mean"], where=f"cma step {t}")
        # the step sampled clip(shift(mu) + L' eps) with its own Philox draw: the stand-alone sampler on the recorded factor
        assert torch.equal(core.noise_gemm_philox(r["L"], r["around"], cr.split(r["k_act"])[1]), r["a"]), t
        Lh = r["L"].cpu().numpy()
        assert np.isfinite(Lh).all() and not np.triu(Lh, 1).any() and (np.diag(Lh) > 0).all(), t
    # reset() starts over: the next step is a first step again
    again = walk(c, env, 2)
    for k in ("a_cov", "L", "rows", "path", "mean", "cost"):
        assert torch.equal(again[0][k], recs[0][k]) and torch.equal(again[1][k], recs[1][k]), k
    c.core.close()


def test_graph_replay_equals_eager_launches():
    env = quad_env(task="tracking_zigzag")
    outs = []
    for graph in (False, True):
        c = build(env, use_graph=graph)
        outs.append(walk(c, env, 5))  # (the reuse graph is captured by the third step and replayed from the fourth)
        c.core.close()
    for t, (a, b) in enumerate(zip(*outs)):
        for k in ("mean", "a_cov", "L", "rows", "path", "C", "aux", "diag", "cost", "a"):
            assert torch.equal(a[k], b[k]), (t, k)


def test_no_step_size_and_no_blend_keep_sigma0_squared_identity():
    env = quad_env(task="tracking_zigzag")
    c = build(env, gamma=0.0, step_size=False)
    for t, r in enumerate(walk(c, env, 4)):
        assert np.abs(r["a_cov"].cpu().numpy() - SIG0 ** 2 * np.eye(N_A)).max() <= 1e-6, t
        row = r["rows"].cpu().numpy()[0]
        assert row[0] == 1.0 and row[1] == 0.0 and not row[2:].any() and not bool(r["path"].any()), (t, row)
    c.core.close()


def test_two_passes_share_the_factor_and_the_next_step_reads_the_last_pass(core):
    env = quad_env(task="tracking_zigzag")
    c = build(env, iters=2)
    recs = walk(c, env, 3)
    # (the recorded C, d and ess are what the last pass left: replaying on them reproduces the next step's factor)
    for t, (Lo, So, rows, p) in enumerate(replay(core, recs), start=1):
        assert torch.equal(recs[t]["L"], Lo) and torch.equal(recs[t]["a_cov"], So) and torch.equal(recs[t]["rows"], rows), t
    # the second pass sampled from the step's one L': its samples are the stand-alone sampler's on that factor, around the mean the
    # first pass committed, with the walked key split(split(key)[0])[0] -- and not those of the factor before the step
    for t in (1, 2):
        r = recs[t]
        act_key = cr.split(cr.split(cr.split(r["k_act"])[0])[0])[1]
        assert torch.equal(core.noise_gemm_philox(r["L"], r["around"], act_key), r["a"]), t
        assert not torch.equal(core.noise_gemm_philox(recs[t - 1]["L"], r["around"], act_key), r["a"]), t
        assert not torch.equal(r["around"].view(H, 4), torch.cat([r["before"][1:], r["before"][-1:]])), t  # (the first pass moved it)
    c.core.close()


@pytest.mark.parametrize("kw,ess", [(dict(elite=16), 16.0), (dict(ess_min=8.0), None)])
def test_elite_and_ess_floor_feed_their_ess_into_mu_eff(kw, ess):
    env = quad_env(task="tracking_zigzag")
    c = build(env, **kw)
    recs = walk(c, env, 3)
    for t in (1, 2):
        prev = float(recs[t - 1]["ess"])
        assert float(recs[t]["rows"][0, 4]) == np.float32(min(max(prev, 1.0), N)), (t, prev)
        if ess is not None:
            assert prev == ess
        else:
            assert prev >= 8.0 * (1 - 1e-3)
        assert int(recs[t]["rows"][0, 7]) in (0, CO.FLAG_CLAMP)
    c.core.close()


def test_a_step_without_its_targets_is_refused_before_any_launch():
    env = quad_env(task="tracking_zigzag")
    c = build(env)
    core = c.core
    params = env.default_params
    obs, info, state = env.reset(cr.PRNGKey(1), params)
    cp = c.reset(state, params, c.init_control_params, cr.PRNGKey(2))
    mean0 = cp.a_mean.clone()
    for setter, args, word in (("covo_set_step_diag", (None, 0), "diagnostics target"),
                               ("covo_set_step_post_cov", (None, None, 0), "posterior covariance target"),
                               ("covo_set_step_cma", (0.2, 1, 1.0, 0.1, 4.0, None, None, 0), "without covo_set_step_cma")):
        assert getattr(core.lib, setter)(core.h, *args) == 0
        with pytest.raises(_lib.CovoError, match=word):
            c(obs, state, params, cr.PRNGKey(3), cp, info)
        # re-attach
        if setter == "covo_set_step_diag":
            assert core.lib.covo_set_step_diag(core.h, _lib.ptr(core.diag), 1) == 0
        elif setter == "covo_set_step_post_cov":
            assert core.lib.covo_set_step_post_cov(core.h, _lib.ptr(core.post_cov), _lib.ptr(core.post_aux), 1) == 0
        else:
            core.attach_cma(c.cma)
    assert core.lib.covo_set_step_sigma_period(core.h, 4) == 0
    with pytest.raises(_lib.CovoError, match="Sigma period"):
        c(obs, state, params, cr.PRNGKey(3), cp, info)
    assert core.lib.covo_set_step_sigma_period(core.h, 1) == 0
    u, cp2, _ = c(obs, state, params, cr.PRNGKey(3), cp, info)  # the handle is usable
    torch.cuda.synchronize()
    assert torch.isfinite(cp2.a_mean).all() and not torch.equal(cp2.a_mean, mean0) and core.device_status() == 0
    core.close()


# ---- 3. the batch and the episode drivers -------------------------------------------------------------------------------------------
def batched(env, inst, E, **kw):
    cp0 = inst[0]["cp"]
    b = cm.controllers.BatchedCMAController(env, E, N, H, LAM, discount=cp0.discount, gamma_mean=cp0.gamma_mean,
                                            sample_sigma=cp0.sample_sigma, a_mean_init=cp0.a_mean, device=DEV, **kw)
    return b


def test_batched_step_equals_the_single_controller_per_instance():
    E = 3  # E ceil(N / 64) = 12 < 1024
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "cma", N, str(LAM), E, seed=3)
    b = batched(env, inst, E)
    b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    b.reset()
    for i in inst:
        i["cp"] = i["c"].reset(i["state"], i["params"], i["cp"], None)
    for step in range(4):
        k_acts = []
        for i in inst:
            i["key"], k_act, i["k_step"] = cr.split(i["key"], 3)
            k_acts.append(np.asarray(k_act))
        u_b = b.step([i["info"]["noisy_state"] for i in inst], np.stack(k_acts)).clone()
        Lb = b.core.sigma_factor(n_envs=E)
        for e, i in enumerate(inst):
            u, i["cp"], info = i["c"](i["obs"], i["state"], i["params"], k_acts[e], i["cp"], i["info"])
            where = (step, e)
            assert torch.equal(b.a_mean[e].view(H, 4), i["cp"].a_mean) and torch.equal(u_b[e], u), where
            assert torch.equal(b._a[e], i["c"].core.a) and torch.equal(b._cost[e], i["c"].core.cost), where
            assert torch.equal(b.a_cov[e], i["cp"].a_cov) and torch.equal(Lb[e], i["c"].core.sigma_factor()), where
            assert torch.equal(b.cma_rows[e], info["cma_rows"]) and torch.equal(b.cma_path[e], i["c"].core.cma_p[0]), where
            assert torch.equal(b.post_cov[e], i["c"].core.post_cov[0]) and torch.equal(b.diag[e], i["c"].core.diag[0]), where
            i["obs"], i["state"], _, _, i["info"] = env.step(i["k_step"], i["state"], u.cpu().numpy(), i["params"])
    rows = b.cma_rows.cpu().numpy()
    assert tuple(rows.shape) == (E, 8) and tuple(b.cma_path.shape) == (E, N_A) and (rows[:, 0] != 1.0).all()
    assert len({float(x) for x in rows[:, 0]}) == E  # every instance has its own step size
    # the phase timers replay copies of a step: each would adapt (or reset) the covariance -- refused, and nothing on the device moves
    keep = [t.clone() for t in (b.cma_rows, b.cma_path, b.a_cov, b.core.sigma_factor(n_envs=E))]
    with pytest.raises(_lib.CovoError, match="phase timers replay a step without its state"):
        b.time_phases(63, reps=2)
    torch.cuda.synchronize()
    for t, k in zip((b.cma_rows, b.cma_path, b.a_cov, b.core.sigma_factor(n_envs=E)), keep):
        assert torch.equal(t, k)
    assert b.core.device_status() == 0
    b.core.close()
    for i in inst:
        i["c"].core.close()


def test_a_batch_larger_than_the_attached_rows_is_refused_before_any_launch():
    """Attach rows for 3 instances, then attach other, smaller buffers for 1: a batched step of 3 must be refused -- it would write
    rows and paths 1 .. 2 past the new buffers -- and nothing moves.  The capacity of the handle's own second factor buffer (which
    only grows) is not what the step is held to."""
    E = 3
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "cma", N, str(LAM), E, seed=9, controllers=False)
    dp = env.default_params
    a0 = torch.tensor([(dp.m * dp.g / dp.max_thrust) * 2.0 - 1.0, 0.0, 0.0, 0.0], **f32).repeat(H, 1)
    b = cm.controllers.BatchedCMAController(env, E, N, H, LAM, a_mean_init=a0, device=DEV)
    b.set_instances([i["state"] for i in inst], [i["params"] for i in inst])
    noisy = [i["info"]["noisy_state"] for i in inst]
    keys = np.stack([np.asarray(cr.PRNGKey(70 + e)) for e in range(E)])
    core = b.core
    # small buffers of their own, each inside a larger one whose rest holds a sentinel
    rows1, path1 = torch.full((E, 8), 7.0, **f32), torch.full((E, N_A), 7.0, **f64)
    assert core.lib.covo_set_step_cma(core.h, 0.2, 1, 1.0, 0.1, 4.0, _lib.ptr(rows1), _lib.ptr(path1), 1) == 0
    mean0 = b.a_mean.clone()
    with pytest.raises(_lib.CovoError, match=r"3 instances, the CMA rows \(covo_set_step_cma\) have n_inst=1"):
        b.step(noisy, keys)
    torch.cuda.synchronize()
    assert bool((rows1 == 7.0).all()) and bool((path1 == 7.0).all()) and torch.equal(b.a_mean, mean0)
    # detached: refused by name; attached for 3 again: the step runs and fills all three rows
    assert core.lib.covo_set_step_cma(core.h, 0.2, 1, 1.0, 0.1, 4.0, None, None, 0) == 0
    with pytest.raises(_lib.CovoError, match="without covo_set_step_cma"):
        b.step(noisy, keys)
    assert core.lib.covo_set_step_cma(core.h, 0.2, 1, 1.0, 0.1, 4.0, _lib.ptr(rows1), _lib.ptr(path1), E) == 0
    b.step(noisy, keys)
    torch.cuda.synchronize()
    assert torch.equal(rows1, torch.tensor(CO.NEUTRAL_ROW, **f32).repeat(E, 1)) and not bool(path1.any())
    assert not torch.equal(b.a_mean, mean0) and core.device_status() == 0
    core.close()


def test_run_episode_equals_the_python_loop():
    n = 4
    env = quad_env(task="tracking_zigzag")
    params = env.default_params
    outs = []
    for fused in (False, True):
        c = build(env)
        c.alias_outputs = True
        ep = cm.envs.DeviceEpisode(env, cr.PRNGKey(41), params, (c.core.lib, c.core.h), DEV)
        cp = c.reset(ep.state0, params, c.init_control_params, cr.PRNGKey(42))
        rng = cr.PRNGKey(43)
        if fused:
            cp, rng = c.run_episode(ep, params, cp, rng, n)
        else:
            for _ in range(n):  # eval_env's run_one_step (quadrotor.py:520-538)
                rng, rng_act, rng_step, rng_control = cr.split(rng, 4)
                u, cp, info = c(None, None, params, rng_act, cp, {"noisy_state": ep.noisy_state})
                ep.step(rng_step, u)
                rng, rng_control = cr.split(rng)
        torch.cuda.synchronize()
        outs.append((ep.read_log().copy(), cp.a_mean.cpu().numpy().copy(), cp.a_cov.cpu().numpy().copy(), ep.true.cpu().numpy().copy(),
                     np.asarray(rng).copy(), c.core.cma_rows.cpu().numpy().copy(), c.core.cma_p.cpu().numpy().copy(),
                     c.core.sigma_factor().cpu().numpy().copy()))
        assert c.core.device_status() == 0
        c.core.close()
    for k, (x, y) in enumerate(zip(outs[0], outs[1])):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), k
    assert outs[0][0].shape == (n, 4) and outs[0][5][0, 0] != 1.0


def test_the_drivers_take_the_name():
    """get_controller(env, "cma", ...) and eval_env_batched(controller="cma") at the defaults: 4 steps, finite errors, a row per instance."""
    env = quad_env(task="tracking", randomizer=True)
    c, cp = cm.envs.get_controller(env, "cma", f"N{N}_H32_lam{LAM}", device=DEV, compute_info=False)
    assert isinstance(c, cm.controllers.CMAController) and c.cma.gamma == 0.2 and c.core.diag is not None and c.core.post_cov is not None
    c.core.close()
    err, found = cm.envs.quadrotor.eval_env_batched(env, 2, f"N{N}_H32_lam{LAM}", n_steps=4, device=DEV, verbose=False, controller="cma",
                                                    rows=True)
    assert err.shape == (2,) and np.isfinite(err).all() and found["cma"].shape == (2, 8) and (found["cma"][:, 0] > 0).all()
    with pytest.raises(ValueError, match="sigma_period=2"):
        cm.envs.quadrotor.eval_env_batched(env, 2, f"N{N}_H32_lam{LAM}", n_steps=4, device=DEV, controller="cma", sigma_period=2)


def test_run_episode_batched_equals_per_instance_loops_through_an_auto_reset():
    """Instance 1 starts two steps before its episode's end: the device env step resets it inside the segment; its factor stays a valid
    one (finite, lower, positive diagonal) and the batch still equals the per-instance loops."""
    E, n = 3, 4
    env = quad_env(task="tracking", randomizer=True)
    inst = instances(env, "cma", N, str(LAM), E, seed=50, warm=False)
    params = [i["params"] for i in inst]
    b = batched(env, inst, E)
    reset_keys = [cr.PRNGKey(150 + e) for e in range(E)]
    ep = cm.envs.BatchedDeviceEpisode(env, reset_keys, params, (b.core.lib, b.core.h), DEV)
    late = torch.tensor([params[1].max_steps_in_episode - 2], dtype=torch.int32, device=DEV).view(torch.float32)
    ep.true[1, ST_TIME:ST_TIME + 1] = late
    ep.noisy[1, ST_TIME:ST_TIME + 1] = late
    b.reset()
    rngs0 = np.stack([np.asarray(cr.PRNGKey(160 + e)) for e in range(E)])
    rngs = b.run_episode(ep, rngs0, n)
    log = ep.read_log()
    assert log.shape == (E, n, 4) and log[1, :, 3].sum() >= 1 and log[0, :, 3].sum() == 0
    Lb = b.core.sigma_factor(n_envs=E)
    Lh = Lb.cpu().numpy()
    assert np.isfinite(Lh).all() and not np.triu(Lh, 1).any() and (np.diagonal(Lh, axis1=1, axis2=2) > 0).all()
    for e, i in enumerate(inst):
        c = i["c"]
        c.alias_outputs = True
        se = cm.envs.DeviceEpisode(env, reset_keys[e], params[e], (c.core.lib, c.core.h), DEV)
        if e == 1:
            se.true[ST_TIME:ST_TIME + 1] = late
            se.noisy[ST_TIME:ST_TIME + 1] = late
        cp = c.reset(se.state0, params[e], c.init_control_params, None)
        rng = rngs0[e]
        for _ in range(n):
            rng, rng_act, rng_step, rng_control = cr.split(rng, 4)
            u, cp, info = c(None, None, params[e], rng_act, cp, {"noisy_state": se.noisy_state})
            se.step(rng_step, u)
            rng, rng_control = cr.split(rng)
        assert np.array_equal(se.read_log().view(np.uint32), log[e].view(np.uint32)), e
        assert torch.equal(cp.a_mean.reshape(-1), b.a_mean[e]) and torch.equal(se.true, ep.true[e]) and torch.equal(cp.a_cov, b.a_cov[e]), e
        assert torch.equal(c.core.sigma_factor(), Lb[e]) and torch.equal(c.core.cma_rows[0], b.cma_rows[e]), e
        assert torch.equal(c.core.cma_p[0], b.cma_path[e]), e
        assert np.array_equal(np.asarray(rng, dtype=np.uint32), rngs[e]), e
        c.core.close()
    assert b.core.device_status() == 0
    b.core.close()
