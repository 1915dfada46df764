"""GPU tests (-m gpu) of the weighted update's kernels on crafted inputs, through the C ABI, against tests/update_oracle.py (numpy
fp64 on the same fp32 inputs; the inputs' properties are asserted in tests/test_update_oracle.py).

Stage 1 + merge (csrc/softmax_stage1.hpp, csrc/softmax_merge.hpp; covo_softmax_update, covo_softmax_update_cov, covo_softmax_reduce):
sizes around a wave, a workgroup and the capped grid (65 600 / 65 570 samples: 1 025 groups over 1 024 waves, so one wave strides),
seven cost patterns at three temperatures, with the caller's per-wave minima and with the library's own.
Merge alone (covo_merge, covo_merge_ranks, covo_merge_ranks_wide, covo_merge_ranks_cov): G up to MG_MAXG = 1 024 records (merge_body's
tail loop runs from G > 256), empty records (m = +inf; with garbage in v; with a stale finite m, where s = 0 alone marks them), scales
that underflow, equal minima, both rank strides.
Bars: mean and covariance 1e-5 absolute; record m exact, s and v 1e-5 max(1, s); G records against the same records
padded with empty ones 2e-6 (test_gpu_parity.py::test_merge_shard_invariance_on_device).  The merged-record output of the merge is
reached through covo_softmax_reduce only (G <= 256 stage-1 records): the ABI has no entry that merges caller records into a record.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs the MI355X", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from covo_mpc_amd.controllers._core import SamplingCore  # noqa: E402
from tests import update_oracle as U  # noqa: E402
from tests.gpu_support import DEV, to_stripes  # noqa: E402

N_MAX = max(U.EDGE_SIZES)
GAMMA_SIGMA = 0.3
COVO_E_BADARG = -1


@functools.lru_cache(maxsize=None)
def _core(lam):
    """One handle per temperature (lambda is the handle's)."""
    return SamplingCore(N_MAX, 32, lam, 1.0, device=DEV, use_graph=False)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


@functools.lru_cache(maxsize=2)
def _inputs(N):
    a, mean, cov = U.actions(N)
    return dict(a=a, a64=a.astype(np.float64), mean=mean, cov=cov, a_dev=to_stripes(a), mean_dev=_dev(mean.reshape(-1)),
                cov_dev=_dev(cov.reshape(-1)))


def _run_stage1(core, x, cost, N, gamma, with_minima):
    """covo_softmax_update, covo_softmax_update_cov and covo_softmax_reduce on the same inputs -> (mean, mean_cov, cov, record)."""
    lib, h, s = core.lib, core.h, core.stream()
    cost_dev = _dev(cost)
    gm = _dev(np.minimum.reduceat(cost, np.arange(0, N, 64))) if with_minima else None
    assert gm is None or gm.numel() == (N + 63) // 64
    mean, mean_c, cov, rec = (torch.full((n,), float("nan"), device=DEV) for n in (128, 128, 512, 132))
    _lib.check(lib.covo_softmax_update(h, _lib.ptr(cost_dev), _lib.ptr(x["a_dev"]), N, _lib.ptr(gm), _lib.ptr(x["mean_dev"]), gamma,
                                       _lib.ptr(mean), s), "covo_softmax_update")
    _lib.check(lib.covo_softmax_update_cov(h, _lib.ptr(cost_dev), _lib.ptr(x["a_dev"]), N, _lib.ptr(gm), _lib.ptr(x["mean_dev"]), gamma,
                                           _lib.ptr(x["cov_dev"]), GAMMA_SIGMA, _lib.ptr(mean_c), _lib.ptr(cov), s),
               "covo_softmax_update_cov")
    _lib.check(lib.covo_softmax_reduce(h, _lib.ptr(cost_dev), _lib.ptr(x["a_dev"]), N, _lib.ptr(gm), _lib.ptr(rec), s),
               "covo_softmax_reduce")
    torch.cuda.synchronize()
    return (mean.cpu().numpy().reshape(32, 4), mean_c.cpu().numpy().reshape(32, 4), cov.cpu().numpy().reshape(32, 4, 4),
            rec.cpu().numpy())


@pytest.mark.parametrize("lam", U.EDGE_LAMS)
@pytest.mark.parametrize("N", U.EDGE_SIZES)
def test_stage1_and_merge_on_crafted_costs(N, lam):
    core, x = _core(lam), _inputs(N)
    worst = dict(mean=0.0, cov=0.0, s=0.0, v=0.0)
    for pattern in U.PATTERNS:
        cost = U.cost_pattern(pattern, N, lam)
        live = U.n_live(cost, lam)
        rec64 = U.record64(cost, x["a64"], lam)
        for gamma in (1.0, 0.7):
            ref, w = U.mean64(cost, x["a64"], lam, gamma, x["mean"])
            ref_cov = U.cov64(w, x["a64"], ref, x["cov"], GAMMA_SIGMA)
            mean, mean_c, cov, rec = _run_stage1(core, x, cost, N, gamma, with_minima=True)
            where = (pattern, N, lam, gamma)
            errs = dict(mean=np.abs(mean - ref).max(), mean_cov=np.abs(mean_c - ref).max(), cov=np.abs(cov - ref_cov).max(),
                        s=abs(rec[1] - rec64["s"]) / max(1.0, rec64["s"]), v=np.abs(rec[2:130] - rec64["v"]).max() / max(1.0, rec64["s"]))
            print(f"  {pattern:12s} N {N:6d} lam {lam:g} gamma {gamma}: n_live {live:6d} ess {U.ess64(w):9.2f} " +
                  " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
            assert errs["mean"] <= U.BAR and errs["mean_cov"] <= U.BAR and errs["cov"] <= U.BAR, (where, errs)
            assert rec[0] == np.float32(rec64["m"]) == cost.min(), (where, rec[0], rec64["m"])
            assert errs["s"] <= 1e-5 and errs["v"] <= 1e-5, (where, errs)
            worst = {k: max(worst[k], errs[k], errs["mean_cov"] if k == "mean" else 0.0) for k in worst}
            if pattern == "equal":  # every weight is exactly 1: s == N (sums of ones are exact), the mean is the plain average
                assert rec[1] == float(N), (where, rec[1])
                assert np.abs(mean - (gamma * x["a64"].mean(axis=0) + (1 - gamma) * x["mean"])).max() <= U.BAR, where
            if live == 1 and gamma == 1.0:  # one weight is 1, every other one exactly 0: that sample's actions, bit for bit
                i = int(np.argmin(cost))
                assert rec[1] == 1.0 and np.array_equal(rec[2:130], x["a"][i].reshape(-1)), where
                assert np.array_equal(mean, x["a"][i]) and np.array_equal(mean_c, x["a"][i]), where
            if gamma == 1.0:  # groupmin = NULL: the library forms the minima itself -- the same minima, the same bits
                again = _run_stage1(core, x, cost, N, gamma, with_minima=False)
                for got, want in zip(again, (mean, mean_c, cov, rec[:130])):
                    assert np.array_equal(got[:130] if got.ndim == 1 else got, want), where
        if pattern in ("winner", "winner_last") and lam == 0.01:
            assert live == 1
    print(f"  worst N {N} lam {lam:g}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert core.device_status() == 0


# ------------------------------------------------------------------------------------------ the merge alone
def _merge(core, fn, rows, gamma, mean_dev, cov_dev=None):
    """One of the four merge entry points on rows [G, stride] -> (mean [32, 4], cov [32, 4, 4] or None)."""
    lib, h, s = core.lib, core.h, core.stream()
    G, stride = rows.shape
    recs = _dev(rows)
    out = torch.full((128,), float("nan"), device=DEV)
    cov = None
    if fn == "covo_merge":
        assert stride == _lib.COVO_PARTIAL_FLOATS
        rc = lib.covo_merge(h, _lib.ptr(recs), G, _lib.ptr(mean_dev), gamma, _lib.ptr(out), s)
    elif fn == "covo_merge_ranks":
        assert stride == _lib.COVO_RANK_RECORD_FLOATS
        rc = lib.covo_merge_ranks(h, _lib.ptr(recs), G, _lib.ptr(mean_dev), gamma, _lib.ptr(out), None, s)
    elif fn == "covo_merge_ranks_wide":
        rc = lib.covo_merge_ranks_wide(h, _lib.ptr(recs), G, stride, _lib.ptr(mean_dev), gamma, _lib.ptr(out), None, s)
    else:
        assert stride == _lib.COVO_RANK_RECORD_COV_FLOATS
        cov = torch.full((512,), float("nan"), device=DEV)
        rc = lib.covo_merge_ranks_cov(h, _lib.ptr(recs), G, _lib.ptr(mean_dev), gamma, _lib.ptr(cov_dev), GAMMA_SIGMA, _lib.ptr(out),
                                      _lib.ptr(cov), None, s)
    _lib.check(rc, fn)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(32, 4), None if cov is None else cov.cpu().numpy().reshape(32, 4, 4)


MERGE_CASES = [(v, lam) for v in U.MERGE_VARIANTS for lam in ((0.01,) if v == "underflow" else (0.01, 1.0))]


@pytest.mark.parametrize("variant,lam", MERGE_CASES)
def test_merge_of_crafted_records(variant, lam):
    """covo_merge (FINAL) over G records: G = 1 .. 1 024 -- one virtual wave, several, the 32 preloaded records per slice
    (G <= 256) and the tail loop behind them (G > 256)."""
    core = _core(lam)
    worst, worst_pad = 0.0, 0.0
    for k, G in enumerate(U.MERGE_GS):
        rows, mu = U.shard_records(G, lam, variant, seed=G)
        outs = {}
        for gamma in (1.0, 0.7):
            ref = U.merge64(rows, lam, gamma, mu)["mean"]
            out, _ = _merge(core, "covo_merge", rows, gamma, _dev(mu.reshape(-1)))
            err = np.abs(out - ref).max()
            worst = max(worst, err)
            assert err <= U.BAR, (variant, lam, G, gamma, err)
            outs[gamma] = out
        if k + 1 < len(U.MERGE_GS):  # the same records followed by empty ones up to the next G
            padded, _ = _merge(core, "covo_merge", U.pad_rows(rows, U.MERGE_GS[k + 1]), 0.7, _dev(mu.reshape(-1)))
            d = np.abs(padded - outs[0.7]).max()
            worst_pad = max(worst_pad, d)
            assert d <= 2e-6, (variant, lam, G, U.MERGE_GS[k + 1], d)
    print(f"  covo_merge {variant} lam {lam:g}: worst err {worst:.2e}, worst padded-vs-plain {worst_pad:.2e}")
    assert core.device_status() == 0


@pytest.mark.parametrize("variant,lam", MERGE_CASES)
def test_merge_of_crafted_rank_records(variant, lam):
    """covo_merge_ranks, covo_merge_ranks_wide at both rank strides and covo_merge_ranks_cov (mean and covariance; merge_cov_body
    beyond one wave of records) over G = 1, 8, 65, 257 rank records."""
    core = _core(lam)
    _, _, cov_old = U.actions(1)
    cov_dev = _dev(cov_old.reshape(-1))
    worst = dict(mean=0.0, cov=0.0, pad=0.0)
    for k, G in enumerate(U.RANK_GS):
        wide, mu = U.shard_records(G, lam, variant, seed=G, floats=_lib.COVO_RANK_RECORD_COV_FLOATS, with_cov=True)
        narrow = np.zeros((G, _lib.COVO_RANK_RECORD_FLOATS), dtype=np.float32)
        narrow[:, :132] = wide[:, :132]
        mu_dev = _dev(mu.reshape(-1))
        calls = [("covo_merge_ranks", narrow), ("covo_merge_ranks_wide", narrow), ("covo_merge_ranks_wide", wide),
                 ("covo_merge_ranks_cov", wide)]
        last = {}
        for gamma in (1.0, 0.7):
            ref = U.merge64(wide, lam, gamma, mu, cov_old, GAMMA_SIGMA)
            for fn, rows in calls:
                out, cov = _merge(core, fn, rows, gamma, mu_dev, cov_dev)
                err = np.abs(out - ref["mean"]).max()
                worst["mean"] = max(worst["mean"], err)
                assert err <= U.BAR, (fn, rows.shape, variant, lam, G, gamma, err)
                if cov is not None:
                    err = np.abs(cov - ref["cov"]).max()
                    worst["cov"] = max(worst["cov"], err)
                    assert err <= U.BAR, (fn, variant, lam, G, gamma, err)
                last[(fn, rows.shape[1])] = (out, cov)
        if k + 1 < len(U.RANK_GS):
            for fn, rows in calls:
                out, cov = _merge(core, fn, U.pad_rows(rows, U.RANK_GS[k + 1]), 0.7, mu_dev, cov_dev)
                d = np.abs(out - last[(fn, rows.shape[1])][0]).max()
                if cov is not None:
                    d = max(d, np.abs(cov - last[(fn, rows.shape[1])][1]).max())
                worst["pad"] = max(worst["pad"], d)
                assert d <= 2e-6, (fn, variant, lam, G, d)
    print(f"  rank merges {variant} lam {lam:g}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert core.device_status() == 0


def test_merge_refuses_more_records_than_it_holds():
    """G = MG_MAXG + 1 = 1 025 is refused with COVO_E_BADARG by every merge entry point, so is a record width that is neither rank
    stride; the handle stays usable."""
    core = _core(0.01)
    lib, h, s = core.lib, core.h, core.stream()
    rows, mu = U.shard_records(8, 0.01, "as_is")
    mu_dev, out = _dev(mu.reshape(-1)), torch.zeros(128, device=DEV)
    big = torch.zeros((1025, _lib.COVO_RANK_RECORD_COV_FLOATS), device=DEV)
    big[:, 0] = 5.0
    big[:, 1] = 1.0
    cov = torch.zeros(512, device=DEV)
    assert lib.covo_merge(h, _lib.ptr(big), 1025, _lib.ptr(mu_dev), 1.0, _lib.ptr(out), s) == COVO_E_BADARG
    assert b"1025" in lib.covo_last_error()
    assert lib.covo_merge_ranks(h, _lib.ptr(big), 1025, _lib.ptr(mu_dev), 1.0, _lib.ptr(out), None, s) == COVO_E_BADARG
    assert lib.covo_merge_ranks_wide(h, _lib.ptr(big), 1025, _lib.COVO_RANK_RECORD_FLOATS, _lib.ptr(mu_dev), 1.0, _lib.ptr(out), None,
                                     s) == COVO_E_BADARG
    assert lib.covo_merge_ranks_cov(h, _lib.ptr(big), 1025, _lib.ptr(mu_dev), 1.0, _lib.ptr(cov), 0.3, _lib.ptr(out), _lib.ptr(cov),
                                    None, s) == COVO_E_BADARG
    assert lib.covo_merge_ranks_wide(h, _lib.ptr(big), 8, _lib.COVO_PARTIAL_FLOATS, _lib.ptr(mu_dev), 1.0, _lib.ptr(out), None,
                                     s) == COVO_E_BADARG
    torch.cuda.synchronize()
    assert not out.any() and core.device_status() == 0  # nothing was launched
    got, _ = _merge(core, "covo_merge", rows, 1.0, mu_dev)
    assert np.abs(got - U.merge64(rows, 0.01, 1.0, mu)["mean"]).max() <= U.BAR
