"""CPU: the harness of the calling-contract tests bites, and their table is complete.

tests/contract_support.py is exercised on CPU tensors: a planted store one element in front of a payload and one behind it are
reported with their offsets, a planted unwritten element is reported, an `allowed` mask hides exactly its own elements, `zeros`
payloads are zero between poison bands, and every view is contiguous and 16-byte aligned.  tests/contract_cases.py is held against
include/covo_hip.h: every `int covo_*(...)` that takes a `void *stream` is a row of the table or a key of EXEMPT with a reason."""
import re

import numpy as np
import pytest

from tests import contract_cases as CC
from tests import contract_support as CS
from tests.abi_support import header_text

torch = pytest.importorskip("torch")

SHAPES = [((7,), "float32"), ((3, 5), "float64"), ((32, 65, 4), "float32"), ((2, 3), "int32"), ((20000,), "float32"), ((1,), "float64")]


def _allocs(poison):
    t = CS.BandedTorch(torch, poison)
    views = [t.empty(s, dtype=getattr(torch, d), device="cpu") for s, d in SHAPES]
    return t, views


@pytest.mark.parametrize("poison", CS.POISONS)
def test_views_are_contiguous_aligned_and_sized(poison):
    t, views = _allocs(poison)
    assert len(t.allocs) == len(SHAPES)
    for (shape, dtype), v, al in zip(SHAPES, views, t.allocs):
        assert tuple(v.shape) == shape and v.dtype == getattr(torch, dtype) and v.is_contiguous()
        assert v.data_ptr() % 16 == 0 and v.data_ptr() == al.view.data_ptr()
        band = max(64 * 1024, -(-al.pay_bytes // 256) * 256)
        assert al.front * 4 == band and al.back * 4 >= band and band % 256 == 0
        assert v.data_ptr() - al.flat.data_ptr() == band                       # the payload starts right behind the front band
        assert CS.bands_intact(al) is None
        assert CS.unwritten(al).size == v.numel()                              # an `empty` payload is all poison
        assert CS.all_poison(al)
    big = t.allocs[4]
    assert big.pay_bytes == 80000 and big.front * 4 == 80128                   # above 64 KiB the band follows the payload


def test_the_nan_poison_is_a_nan_in_both_widths_and_the_finite_one_is_finite():
    t, views = _allocs(CS.POISON_NAN)
    assert torch.isnan(views[0]).all() and torch.isnan(views[1]).all()
    assert int(views[1].view(torch.int64)[0, 0]) == 0x7FF8BEEF7FF8BEEF
    t, views = _allocs(CS.POISON_FINITE)
    assert torch.isfinite(views[0]).all() and torch.isfinite(views[1]).all()
    assert 1.4e16 < float(views[0][0]) < 1.6e16


@pytest.mark.parametrize("poison", CS.POISONS)
@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_a_store_one_element_outside_is_reported_with_its_offset(poison, k):
    for where in ("front", "back"):
        t, views = _allocs(poison)
        al, v = t.allocs[k], views[k]
        per = al.item // 4
        n = v.numel()
        word = al.front - per if where == "front" else al.front + n * per
        al.flat[word] = 12345
        b = CS.bands_intact(al)
        assert b is not None and b.side == where and b.count == 1 and b.word == 12345
        assert b.elem_offset == (-1 if where == "front" else n) and b.byte_offset == b.elem_offset * al.item
        assert all(CS.bands_intact(o) is None for o in t.allocs if o is not al)
        assert "altered" in repr(b)


def test_a_stride_doubling_store_still_lands_in_a_band():
    t = CS.BandedTorch(torch, CS.POISON_NAN)
    v = t.empty((20000,), dtype=torch.float32, device="cpu")
    al = t.allocs[0]
    al.flat[al.front + 2 * 20000 - 1] = 0                                     # the last element of a payload twice as long
    b = CS.bands_intact(al)
    assert b is not None and b.side == "back" and b.elem_offset == 39999 and v.numel() == 20000


@pytest.mark.parametrize("poison", CS.POISONS)
def test_an_unwritten_element_is_reported_and_a_mask_hides_only_its_own(poison):
    t, views = _allocs(poison)
    v, al = views[2], t.allocs[2]
    v.fill_(0.25)
    assert CS.unwritten(al).size == 0 and not CS.all_poison(al)
    al.payload_words()[[17, 4000]] = CS._i32(poison)                           # two elements the kernel "forgot"
    assert CS.unwritten(al).tolist() == [17, 4000]
    mask = np.zeros(v.shape, dtype=bool)
    mask.reshape(-1)[17] = True
    assert CS.unwritten(al, mask).tolist() == [4000]
    mask.reshape(-1)[[4000, 4001]] = True
    assert CS.unwritten(al, mask).size == 0
    d, ald = views[1], t.allocs[1]                                             # fp64: an element counts only if both its words are poison
    d.fill_(1.5)
    ald.payload_words()[[4, 5, 8]] = CS._i32(poison)
    assert CS.unwritten(ald).tolist() == [2]


@pytest.mark.parametrize("poison", CS.POISONS)
def test_zeros_full_and_like_payloads_between_poison_bands(poison):
    t = CS.BandedTorch(torch, poison)
    z = t.zeros((5, 8), dtype=torch.float32, device="cpu")
    f = t.full((6,), 0.5, dtype=torch.float32, device="cpu")
    zl, el = t.zeros_like(z), t.empty_like(torch.ones(3, 2, dtype=torch.float64))
    assert [a.kind for a in t.allocs] == ["zeros", "full", "zeros", "empty"]
    assert bool((z == 0).all()) and bool((f == 0.5).all()) and bool((zl == 0).all()) and zl.shape == z.shape
    assert el.dtype == torch.float64 and tuple(el.shape) == (3, 2) and CS.all_poison(t.allocs[3])
    for al in t.allocs:
        p = CS._i32(poison)
        assert bool((al.flat[:al.front] == p).all()) and bool((al.flat[al._back_start:] == p).all()) and CS.bands_intact(al) is None
    assert t.float32 is torch.float32 and t.is_tensor(z) and t.cuda is torch.cuda  # everything else is torch's own


def test_banded_inputs_hold_the_array_and_owner_finds_views():
    x = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    al = CS.banded(x, CS.POISON_FINITE)
    assert al.kind == "input" and np.array_equal(al.view.numpy(), x) and CS.bands_intact(al) is None and al.view.data_ptr() % 16 == 0
    k = CS.banded(np.array([[1, 2 ** 32 - 1]], dtype=np.uint32), CS.POISON_NAN)
    assert k.view.dtype == torch.int32 and k.view.tolist() == [[1, -1]]
    assert CS.owner([k, al], al.view[1, 2]) is al and CS.owner([k], al.view) is None
    e = CS.banded_empty((3, 4), torch.float32, CS.POISON_NAN)
    assert e.kind == "empty" and CS.all_poison(e)


# ---------------------------------------------------------------------------------------------- the table
def stream_entries():
    fs = re.findall(r"\bint\s+(covo_\w+)\s*\(([^;]*?)\)\s*;", header_text(), re.S)
    return [name for name, args in fs if re.search(r"void\s*\*\s*stream\b", args)]


def test_every_stream_taking_entry_has_a_row_or_a_reasoned_exemption():
    names = stream_entries()
    assert len(names) == 65 and len(set(names)) == 65
    rows = set(CC.ROWS_BY_ENTRY)
    missing = [n for n in names if n not in rows and n not in CC.EXEMPT]
    assert not missing, f"no contract row in tests/contract_cases.py and no EXEMPT reason: {missing}"
    assert not rows & set(CC.EXEMPT), "an entry is both a row and exempt"
    assert not (rows | set(CC.EXEMPT)) - set(names), "a row or an exemption names no stream-taking entry of the header"
    for n, why in CC.EXEMPT.items():
        assert isinstance(why, str) and len(why) > 20, n
    print(f"{len(names)} stream-taking entries: {len(rows)} rows ({len(CC.all_cases())} cases), {len(CC.EXEMPT)} exemptions")


def test_case_ids_are_unique_and_every_required_size_is_in_the_table():
    ids = [CC.Row.case_id(r, sz) for r, sz in CC.all_cases()]
    assert len(ids) == len(set(ids))
    sizes = lambda e, k: {sz[k] for r in CC.ROWS_BY_ENTRY.get(e, []) for sz in r.sizes if k in sz}
    for e in ("covo_randn", "covo_noise_gemm", "covo_noise_gemm_philox", "covo_noise_blockdiag_philox", "covo_rollout_cost",
              "covo_softmax_update", "covo_softmax_update_cov"):
        assert sizes(e, "N") >= {1, 63, 65, 1000}, e
    for e in ("covo_randn", "covo_noise_gemm_philox", "covo_noise_blockdiag_philox", "covo_noise_nodes_philox", "covo_noise_factor_philox"):
        assert any(sz.get("offset") and sz["N"] == 65 for r in CC.ROWS_BY_ENTRY[e] for sz in r.sizes), e
    assert sizes("covo_cholesky", "n") >= {1, 5, 8, 9, 24, 72, 127, 128}
    assert sizes("covo_sigma_nodes", "M") == {2, 3, 16} == sizes("covo_noise_factor_philox", "M")
    assert sizes("covo_noise_nodes_philox", "M") == {2, 5, 32}
    assert sizes("covo_rollout_fan", "K") == {1, 5}
    assert {(sz["N"], sz["K"]) for sz in CC.ROWS_BY_ENTRY["covo_elite_select"][0].sizes} >= {(1, 1), (65, 65), (1000, 1000), (1000, 1)}
    for e in ("covo_weighted_cov", "covo_sigma_adapt", "covo_sigma_shift"):
        assert e in CC.ROWS_BY_ENTRY
    for e in ("covo_hessian", "covo_sigma", "covo_riccati", "covo_cost_gradient", "covo_plan_hold"):
        assert sizes(e, "B") == {1, 3}, e
