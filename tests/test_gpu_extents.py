"""GPU: every entry of the C ABI writes all of the extent include/covo_hip.h states for its outputs and nothing outside it, and reads
nothing outside its inputs that reaches a result -- per case of tests/contract_cases.py:

  1. two runs on tight, ordinary allocations are bit-equal (an atomics row: within its bar);
  2. with every input, every output and every core buffer between guard bands (tests/contract_support.py), all bands are intact;
  3. no payload element of an `empty`-allocated output still holds the poison, under the NaN and under the finite poison word --
     except the elements a row's mask names, each mask citing the header line that leaves them unwritten;
  4. the outputs under bands are bit-equal to the tight run's;
  5. the outputs with NaN-poisoned input bands are bit-equal to those with finite-poisoned input bands;
  6. inputs the header marks const are bit-unchanged;
  7. (three entries) a refused call returns non-zero and leaves every output payload all poison.

What step 5 cannot see: a read past the end of an input that never reaches a result.  The only other way to see such a read is a
fault, which these tests do not provoke.  Out of scope: library-owned workspaces, the attachment rows a core registers at
construction, misaligned pointers, two handles side by side.

The negative control writes one sample more than a banded buffer expects -- into the band, memory the test owns -- and the harness
must report it at the right offset."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from covo_mpc_amd import _lib  # noqa: E402
from tests import contract_cases as CC  # noqa: E402
from tests import contract_support as CS  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = CC.all_cases()


@pytest.mark.parametrize("row,sz", CASES, ids=[CC.Row.case_id(r, s) for r, s in CASES])
def test_entry_writes_its_extent_and_nothing_else(row, sz):
    t0 = time.perf_counter()
    X = row.build(sz)
    cores = []

    def core_for_a_run():  # the shared core of the case's (N, options); a row with fresh_core gets a new one for every run
        if not cores or row.fresh_core:
            cores.append(row.new_core(sz))
        return cores[-1]

    # 1: determinism on tight allocations
    first, _ = CC.run_tight(row, core_for_a_run(), sz, X)
    second, _ = CC.run_tight(row, core_for_a_run(), sz, X)
    differ = CC.same(row, first, second, sz, X)
    assert not differ, f"not reproducible on tight allocations: {differ}"
    res = {}
    for poison in CS.POISONS:
        outs, ins, bufs, proxy = CC.run_banded(row, core_for_a_run(), sz, X, poison)
        found = CC.check_banded(row, sz, X, outs, ins, bufs, proxy)          # 2, 3, 6
        assert not found, f"poison 0x{poison:08X}: " + "; ".join(found)
        res[poison] = {k: CC._words(v) for k, v in outs.items()}
        differ = CC.same(row, first, res[poison], sz, X)                            # 4
        assert not differ, f"poison 0x{poison:08X}: outputs under bands differ from the tight run: {differ}"
    differ = CC.same(row, res[CS.POISON_NAN], res[CS.POISON_FINITE], sz, X)         # 5
    assert not differ, f"outputs depend on what lies beyond the inputs: {differ}"
    assert all(c.device_status() == 0 for c in cores)
    n_out = sum(len(v) for v in first.values())
    print(f"  {CC.Row.case_id(row, sz)}: {len(first)} outputs, {n_out} bytes, {time.perf_counter() - t0:.2f} s")
    if row.fresh_core:
        for c in cores:
            c.close()


def _refusals():
    """(entry, a call it refuses) of the noise, update and Sigma families: callable(core, outs) -> return code"""
    P = _lib.ptr
    rng = np.random.default_rng(0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(CC.DEV)
    L, mu = t(CC._factor(rng)), t(np.zeros(128))
    cost, a = t(CC._costs(rng, (64,))), t(np.zeros((32, 64, 4)))
    keep = [L, mu, cost, a]
    return keep, [
        ("covo_noise_gemm_philox", [(32, 64, 4)],  # N = 0
         lambda core, o: core.lib.covo_noise_gemm_philox(core.h, P(L), P(mu), 1, 2, 0, 0, P(o[0]), core.stream())),
        ("covo_softmax_update", [(128,)],  # N = 0
         lambda core, o: core.lib.covo_softmax_update(core.h, P(cost), P(a), 0, None, P(mu), 1.0, P(o[0]), core.stream())),
        ("covo_sigma_shift", [(128, 128), (128, 128)],  # batch = 0
         lambda core, o: core.lib.covo_sigma_shift(core.h, P(L), 0, 0.5, P(o[0]), P(o[1]), core.stream())),
    ]


@pytest.mark.parametrize("k", range(3))
def test_a_refused_call_writes_nothing(k):
    keep, calls = _refusals()
    entry, shapes, call = calls[k]
    core = CC.get_core(N=64)
    for poison in CS.POISONS:
        outs = [CS.banded_empty(s, torch.float32, poison, CC.DEV, torch, name=f"{entry} out{i}") for i, s in enumerate(shapes)]
        rc = call(core, [o.view for o in outs])
        torch.cuda.synchronize()
        assert rc != 0, f"{entry} accepted the call"
        for o in outs:
            assert CS.all_poison(o) and CS.bands_intact(o) is None, f"{entry}: the refused call wrote to {o.name}"
    assert core.device_status() == 0


def test_negative_control_one_sample_too_many_is_reported_at_its_offset():
    """covo_noise_nodes_philox on a core with n_local = 65 whose core.a is banded as if n = 64: the kernel legitimately writes the
    stripes [32][65][4], 128 floats more than the payload [32][64][4] holds.  They land at the start of the back band: element
    8192 (stage 31, sample 33, component 0) to element 8319."""
    core = CC.get_core(N=65)
    row = CC.ROWS_BY_ENTRY["covo_noise_nodes_philox"][0]
    sz = dict(N=65, M=5)
    X = row.build(sz)
    T = {k: CC._to_dev(torch, v) for k, v in X.items()}
    short = CS.banded_empty((32, 64, 4), torch.float32, CS.POISON_NAN, CC.DEV, torch, name="core.a as if n = 64")
    with CC.Swap(core, sz, a=short.view):
        core.noise_nodes(T["basis"], T["mu"], CC.KEY)
        torch.cuda.synchronize()
    b = CS.bands_intact(short)
    print(f"  {b!r}")
    assert b is not None and b.side == "back"
    assert b.elem_offset == 32 * 64 * 4 and b.count == 128 and b.last_byte_offset == (32 * 65 * 4 - 1) * 4
    assert CS.unwritten(short).size == 0
    assert core.device_status() == 0
