"""GPU: every entry of the C ABI does all its work on the caller's stream -- per case of tests/contract_cases.py, on a non-blocking
side stream (one per test, nothing else in flight):

  inputs start spoiled (NaN; integer inputs hold the harmless out-of-range value the row names); the side stream gets an event, a
  sleep, an event and the device-to-device copies that give the inputs their real values; the wrapper call follows and picks the side
  stream up as torch's current stream; every const input is spoiled again right behind it; only then the stream is synchronised.

Library work that runs on another stream, or is ordered only against the null stream, reads the spoiled inputs or loses its inputs
early: the outputs then differ from the same case on the default stream, which is what each case asserts (bit-equal; an atomics row
within its bar).  The sleep was real: between the two events at least 5 ms and at least 10 x the case's own call-plus-sync time on the
default stream passed -- a case whose sleep falls short fails, it is not skipped.  The sleep is torch.cuda._sleep, calibrated once per
module with events (printed, with every case's ratio).

These tests never run two handles side by side: they only move ONE handle's work off the null stream.

The negative control makes the call with the default stream's pointer while the side stream sleeps: it reads the NaNs, and the
comparison must notice."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import contract_cases as CC  # noqa: E402
from tests import contract_support as CS  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = CC.all_cases()
MIN_MS, RATIO = 5.0, 10.0
MARGIN = 2.0  # the delay asked for is MARGIN x max(MIN_MS, RATIO x the call): clock changes and timer noise do not eat the bound
_CAL = {}


def cycles_for(ms):
    """torch.cuda._sleep cycles for `ms` milliseconds, from the module's one calibration"""
    if "per_ms" not in _CAL:
        _CAL["per_ms"] = CS.sleep_cycles_per_ms(torch)
        print(f"\n  sleep calibration: {_CAL['per_ms']:.0f} cycles per ms")
    return int(_CAL["per_ms"] * ms)


def side_stream(must=False):
    """A new non-blocking stream on which work demonstrably runs beside the null stream's (a 3 ms sleep on it does not hold a null-stream
    launch back): the runtime maps streams to a few hardware queues, and a stream that shares the null stream's queue would order a
    launch on the wrong stream by accident.  Up to 8 candidates; must=False: the last one if none qualifies (the case then still
    checks values, with less power), must=True: none is a failure."""
    for _ in range(8):
        s = torch.cuda.Stream()
        if CS.runs_beside_the_null_stream(torch, s, cycles_for(3.0)):
            return s
    assert not must, "none of 8 new streams ran beside the null stream"
    print("  (no stream ran beside the null stream: taking the last candidate)")
    return s


def reference(row, core, sz, X):
    """the case on the default stream -> (outputs, its call-plus-sync milliseconds: the faster of two runs behind a warm-up)"""
    ref, _ = CC.run_tight(row, core, sz, X)
    best = np.inf
    for _ in range(2):
        t0 = time.perf_counter()
        CC.run_tight(row, core, sz, X)
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return ref, best


def on_side_stream(row, core, sz, X, side, call_ms, call=None, info=None, margin=MARGIN):
    """the case behind a delay on `side` -> (outputs, the sleep's ms)"""
    dev = lambda v: CC._to_dev(torch, v)
    names = [k for k in X if not k.startswith("_")]
    stage = {k: dev(X[k]) for k in names}
    bad = {k: dev(CC.spoiled(row, k, np.ascontiguousarray(X[k]))) for k in names}
    T = {k: (bad[k].clone() if k in bad else v) for k, v in X.items()}
    torch.cuda.synchronize()
    ms = max(MIN_MS, RATIO * call_ms) * margin
    res = {}

    def go():
        with CC.Swap(core, sz, **{attr: T[key] for attr, key in row.core_in.items()}):
            res["outs"] = (call or row.run)(core, T, sz)

    _, slept = CS.delayed(side, [(T[k], stage[k]) for k in names], cycles=cycles_for(ms), call=go,
                          spoil=[(T[k], bad[k]) for k in names if k not in row.inout], info=info)
    torch.cuda.synchronize()
    return {k: CC._words(v) for k, v in res["outs"].items()}, slept


@pytest.mark.parametrize("row,sz", CASES, ids=[CC.Row.case_id(r, s) for r, s in CASES])
def test_entry_works_on_the_callers_stream(row, sz):
    X = row.build(sz)
    core = row.new_core(sz)
    ref, call_ms = reference(row, core, sz, X)
    if row.fresh_core:  # a twin handle makes the same calls on the side stream
        core.close()
        core = row.new_core(sz)
    side = side_stream()
    got, slept = on_side_stream(row, core, sz, X, side, call_ms)
    print(f"  {CC.Row.case_id(row, sz)}: call+sync {call_ms:.3f} ms, slept {slept:.2f} ms, ratio {slept / call_ms:.1f}")
    assert slept >= MIN_MS and slept >= RATIO * call_ms, f"the sleep of {slept:.2f} ms does not cover the call ({call_ms:.3f} ms)"
    differ = CC.same(row, ref, got, sz, X)
    assert not differ, f"on a side stream behind a {slept:.1f} ms delay the outputs differ from the default stream's: {differ}"
    assert core.device_status() == 0
    if row.fresh_core:
        core.close()


def test_negative_control_a_call_on_the_wrong_stream_is_noticed():
    """covo_shift_mean (pure arithmetic, no data-dependent loop) with its input produced by the delayed copies on the side stream, but
    called with the DEFAULT stream's pointer while the side stream sleeps: it reads the NaN the input still holds."""
    row = CC.ROWS_BY_ENTRY["covo_shift_mean"][0]
    sz = {}
    X = row.build(sz)
    core = CC.get_core(**row.core_kw(sz))
    ref, call_ms = reference(row, core, sz, X)
    default = torch.cuda.default_stream()

    def wrong(core, T, sz):
        with torch.cuda.stream(default):  # the call leaves the side stream: core.stream() is the null stream's pointer
            assert core.stream().value in (None, 0)
            out = row.run(core, T, sz)
            default.synchronize()         # it has run: while the side stream still sleeps, if the attempt is to count
        return out

    # The control needs the wrong call to have RUN while the side stream slept.  Two things outside the library can prevent that: the
    # host was held up between enqueueing the sleep and making the call, or the runtime put the two streams on one hardware queue.
    # Both are visible (the sleep's end event has fired when the call returns), so such an attempt is made again on another stream
    # with a sleep twice as long; an attempt that did run beside the sleep is judged, whatever it shows.
    for attempt in range(6):
        side, info = side_stream(must=True), {}
        got, slept = on_side_stream(row, core, sz, X, side, call_ms, call=wrong, info=info, margin=MARGIN * 2 ** attempt)
        print(f"  attempt {attempt}: slept {slept:.2f} ms, asleep when the wrong call had run: {info['asleep_after_call']}")
        if info["asleep_after_call"]:
            break
    assert info["asleep_after_call"], "in 6 attempts the call on the null stream never ran while the side stream slept"
    assert slept >= MIN_MS
    assert CC.same(row, ref, got, sz, X) == ["out"], "a call on the wrong stream went unnoticed"
    assert np.isnan(got["out"].view(np.float32)).all() and np.isfinite(ref["out"].view(np.float32)).all()


# ---------------------------------------------------------------------------------------------- the fused step, call by call
STEP_ROW = CC.ROWS_BY_ENTRY["covo_mpc_step"][0]
STEP_SIZES = [sz for sz in STEP_ROW.sizes if sz.get("graph", 1)]
PLANS = {"a-all-on-side": "ssss", "b-replay-moves-to-side": "dddss", "c-workspace-grows-on-side": "dddGs"}


def _grow(core, batch=5):
    """a larger-batch covo_sigma on the handle: the Sigma workspace is re-allocated under the captured step graph
    (tests/test_gpu_parity.py: test_workspace_growth_drops_the_captured_step_graph)"""
    Rb = torch.from_numpy(CC._sym(np.random.default_rng(5), batch)).to(CC.DEV)
    S, L = core.sigma(Rb, 0.5, batch=batch)
    return S


def _walk(sz, X, plan, side, call_ms):
    """the calls of `plan` on a handle of their own (d: default stream; s: side stream behind its own delay; G: on the side stream,
    behind the delay, a workspace growth and then the call) -> ([every call's mean, the last call's stripes, costs, covariance],
    the shortest sleep)"""
    core = CC.get_core(fresh=True, **STEP_ROW.core_kw(sz))
    dev = lambda v: CC._to_dev(torch, v)
    names = [k for k in X if not k.startswith("_")]
    stage = {k: dev(X[k]) for k in names}
    bad = {k: dev(CC.spoiled(STEP_ROW, k, np.ascontiguousarray(X[k]))) for k in names}
    T = {key: (stage[key].clone() if key in stage else v) for key, v in X.items()}  # one set of input tensors for every call
    outs, slept = [], []
    for k, where in enumerate(plan):
        on_side = side is not None and where != "d"
        for key in names:
            T[key].copy_(bad[key] if on_side else stage[key])
        torch.cuda.synchronize()

        def go():
            if where == "G":
                _grow(core)
            return CC.step_call(core, T, sz, k)

        if on_side:
            (am, cov), ms = CS.delayed(side, [(T[key], stage[key]) for key in names], cycles=cycles_for(max(MIN_MS, RATIO * call_ms) * MARGIN),
                                       call=go, spoil=[(T[key], bad[key]) for key in names])
            slept.append(ms)
        else:
            am, cov = go()
        torch.cuda.synchronize()
        outs.append(CC._words(am))
    # (not core.blockmin: the step's groupmin is a work area the header promises no contents for)
    outs += [CC._words(t) for t in (core.a, core.cost)] + ([CC._words(cov)] if cov is not None else [])
    assert core.device_status() == 0
    core.close()
    return outs, min(slept) if slept else 0.0


# (c) grows the Sigma chain's workspace: the covo-online step alone has launches that hold its address
WALKS = [(sz, p) for sz in STEP_SIZES for p in PLANS if not p.startswith("c") or sz["mode"] == "online"]


@pytest.mark.parametrize("sz,plan", WALKS, ids=[CC.Row.case_id(STEP_ROW, s) + "-" + p for s, p in WALKS])
def test_step_calls_move_between_streams(sz, plan):
    """(a) every call on the side stream behind its own delay; (b) three calls on the default stream, then the captured graph is
    replayed on the side stream; (c) the same, with the Sigma workspace growing on the side stream under the captured graph -- each
    against a twin handle that made the same calls with the same keys on the default stream."""
    plan_calls = PLANS[plan]
    X = STEP_ROW.build(sz)
    probe = CC.get_core(fresh=True, **STEP_ROW.core_kw(sz))
    _, call_ms = reference(STEP_ROW, probe, sz, X)
    probe.close()
    # (call_ms is the time of the row's four calls together: every single call's delay covers it with room to spare)
    want, _ = _walk(sz, X, plan_calls, None, call_ms)
    side = side_stream()
    got, slept = _walk(sz, X, plan_calls, side, call_ms)
    print(f"  {CC.Row.case_id(STEP_ROW, sz)} {plan}: four calls {call_ms:.3f} ms, shortest sleep {slept:.2f} ms")
    assert slept >= MIN_MS and slept >= RATIO * call_ms
    differ = [i for i, (a, b) in enumerate(zip(want, got)) if not np.array_equal(a, b)]
    assert not differ, f"plan {plan_calls}: results {differ} differ from the twin's on the default stream"
