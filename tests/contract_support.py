"""The harness of the calling-contract tests (tests/test_gpu_extents.py, tests/test_gpu_streams.py; checked on the CPU by
tests/test_contract_support.py): guard bands around every buffer an entry of include/covo_hip.h touches, and a delayed side stream.

Extents.  A banded buffer is a contiguous view into a larger flat allocation:

    | front band | payload | back band |          band = max(64 KiB, payload bytes rounded up to 256 B)

The bands hold a poison word; the payload holds it too where the allocation was an `empty`.  A band that lost a poison word is a store
outside the extent the header states; a payload word that kept it is an element the entry did not write.  Band sizes are multiples of
256 B, so the payload keeps the alignment the allocator gave the flat buffer (>= 64 B on the host, 512 B on the device).
Two poison words: POISON_NAN is a quiet NaN as an fp32 and, doubled, as an fp64 (0x7FF8BEEF7FF8BEEF: both halves recognisable);
POISON_FINITE is 0x5A5A5A5A, about 1.5e16 as an fp32 and about 2.9e127 as an fp64 -- finite, so a read that leaks into a result changes
it between the two runs instead of turning it into the same NaN twice.

torch is imported inside the functions only: the module imports on a machine without it."""
import numpy as np

POISON_NAN = 0x7FF8BEEF
POISON_FINITE = 0x5A5A5A5A
POISONS = (POISON_NAN, POISON_FINITE)
MIN_BAND = 64 * 1024


def _i32(word):
    """the poison word as the int32 a torch.int32 fill takes"""
    return int(np.uint32(word).astype(np.int32))


def band_bytes(payload_bytes):
    return max(MIN_BAND, -(-int(payload_bytes) // 256) * 256)


class Alloc:
    """One banded allocation: .flat (int32 words of the whole buffer), .view (the payload, shaped and typed), .kind ("empty" | "zeros"
    | "full" | "input"), .poison, .front / .back (band words) and .pay_bytes."""

    def __init__(self, torch, shape, dtype, device, poison, kind, name=""):
        self.poison, self.kind, self.name = int(poison), kind, name
        shape = tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        self.item = item
        self.pay_bytes = int(np.prod(shape, dtype=np.int64)) * item
        band = band_bytes(self.pay_bytes)
        pay_round = -(-self.pay_bytes // 256) * 256
        total = band + pay_round + band
        self.front = band // 4
        self.flat = torch.full((total // 4,), _i32(poison), dtype=torch.int32, device=device)
        self._back_start = (band + self.pay_bytes + 3) // 4  # the slack that rounds the payload up to 256 B belongs to the back band
        self.back = total // 4 - self._back_start
        raw = self.flat.view(torch.uint8)[band:band + self.pay_bytes]
        self.view = (raw.view(dtype) if self.pay_bytes else torch.empty((0,), dtype=dtype, device=device)).reshape(shape)

    def payload_words(self):
        """the payload as int32 words (whole words only: every dtype the ABI uses is 4 or 8 bytes wide)"""
        return self.flat[self.front:self.front + self.pay_bytes // 4]


class Breach:
    """What bands_intact found: side ("front" | "back"), byte_offset of the first altered band word relative to the payload's first
    byte (negative in the front band), elem_offset = byte_offset // itemsize (floor), the word found there, count of altered words in
    that band and last_byte_offset of the last one."""

    def __init__(self, side, byte_offset, item, word, count, last_byte_offset, name):
        self.side, self.byte_offset, self.word, self.count, self.last_byte_offset = side, byte_offset, word, count, last_byte_offset
        self.elem_offset, self.name = byte_offset // item, name

    def __repr__(self):
        return (f"<{self.name or 'buffer'}: {self.count} altered word(s) in the {self.side} band, the first at element "
                f"{self.elem_offset} (byte {self.byte_offset}) of the payload = 0x{self.word:08X}, the last at byte {self.last_byte_offset}>")


def bands_intact(alloc):
    """None while both bands of `alloc` hold their poison; else the Breach of the first altered word (front band first)."""
    p = _i32(alloc.poison)
    for side, words, start in (("front", alloc.flat[:alloc.front], 0), ("back", alloc.flat[alloc._back_start:], alloc._back_start)):
        bad = (words != p).nonzero()
        if bad.numel():
            i, j = int(bad[0, 0]), int(bad[-1, 0])
            off = lambda k: (start + k - alloc.front) * 4
            return Breach(side, off(i), alloc.item, int(words[i]) & 0xFFFFFFFF, int(bad.numel()), off(j), alloc.name)
    return None


def unwritten(alloc, allowed=None):
    """Flat indices (numpy int64) of the payload elements that still hold the poison pattern in every one of their words, minus those
    `allowed` (a boolean array of the payload's shape: True where the header says the entry does not write) marks."""
    w = alloc.payload_words() == _i32(alloc.poison)
    per = alloc.item // 4
    if per > 1:
        w = w.reshape(-1, per).all(dim=1)
    idx = w.nonzero().reshape(-1).cpu().numpy().astype(np.int64)
    if allowed is not None:
        allowed = np.asarray(allowed, dtype=bool).reshape(-1)
        assert allowed.size == w.numel(), f"allowed mask of {allowed.size} elements for a payload of {w.numel()}"
        idx = idx[~allowed[idx]]
    return idx


def all_poison(alloc):
    """Every payload word still holds the poison (a refused call wrote nothing)."""
    return bool((alloc.payload_words() == _i32(alloc.poison)).all())


def banded(array, poison, device="cpu", torch=None, name=""):
    """The banded layout around a copy of `array` (numpy) on `device` -> Alloc (kind "input"); .view is the tensor to hand on."""
    if torch is None:
        import torch
    array = np.ascontiguousarray(array)
    src = torch.from_numpy(array.view(np.int32) if array.dtype == np.uint32 else array)
    al = Alloc(torch, array.shape, src.dtype, device, poison, "input", name)
    if al.pay_bytes:
        al.view.copy_(src.reshape(array.shape))
    return al


def banded_empty(shape, dtype, poison, device="cpu", torch=None, name=""):
    """A banded, poison-filled buffer for an output the test allocates itself (core.a, core.cost, ...) -> Alloc (kind "empty")."""
    if torch is None:
        import torch
    return Alloc(torch, shape, dtype, device, poison, "empty", name)


class BandedTorch:
    """Stands in for SamplingCore.torch: every attribute is torch's own, except the allocators empty / empty_like / zeros / zeros_like /
    full, which return banded views and are recorded in .allocs (in call order)."""

    def __init__(self, torch, poison):
        self._torch, self.poison, self.allocs = torch, int(poison), []

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def _new(self, shape, dtype, device, kind, fill=None):
        t = self._torch
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, t.Size)):
            shape = tuple(shape[0])
        if dtype is None:
            dtype = t.get_default_dtype() if fill is None or isinstance(fill, float) else (t.bool if isinstance(fill, bool) else t.int64)
        al = Alloc(t, shape, dtype, device if device is not None else "cpu", self.poison, kind, f"{kind}#{len(self.allocs)}")
        if fill is not None and al.pay_bytes:
            al.view.fill_(fill)
        self.allocs.append(al)
        return al.view

    @staticmethod
    def _plain(kw):
        extra = set(kw) - {"dtype", "device", "requires_grad", "pin_memory", "memory_format", "layout"}
        assert not extra, f"BandedTorch: allocator keyword(s) {sorted(extra)} are not modelled"

    def empty(self, *shape, dtype=None, device=None, **kw):
        self._plain(kw)
        return self._new(shape, dtype, device, "empty")

    def zeros(self, *shape, dtype=None, device=None, **kw):
        self._plain(kw)
        return self._new(shape, dtype, device, "zeros", 0)

    def full(self, shape, fill_value, dtype=None, device=None, **kw):
        self._plain(kw)
        return self._new((shape,), dtype, device, "full", fill_value)

    def empty_like(self, t, dtype=None, device=None, **kw):
        self._plain(kw)
        return self._new((tuple(t.shape),), dtype or t.dtype, device or t.device, "empty")

    def zeros_like(self, t, dtype=None, device=None, **kw):
        self._plain(kw)
        return self._new((tuple(t.shape),), dtype or t.dtype, device or t.device, "zeros", 0)


def owner(allocs, tensor):
    """The Alloc of `allocs` whose payload holds `tensor`'s first byte, or None."""
    p = tensor.data_ptr()
    for al in allocs:
        q = al.view.data_ptr()
        if al.pay_bytes and q <= p < q + al.pay_bytes:
            return al
    return None


# ---------------------------------------------------------------------------------------------- the delayed side stream
def sleep_cycles_per_ms(torch, probe_cycles=20_000_000, probes=3):
    """torch.cuda._sleep's cycles per millisecond on the current device: the largest of `probes` event-timed sleeps of probe_cycles,
    behind one such sleep as a warm-up.  The sleep counts shader clocks, which follow the device's power state: the largest figure is
    the one at full clock, and a delay sized with it can only come out longer at a lower clock."""
    torch.cuda._sleep(probe_cycles)
    torch.cuda.synchronize()
    best = 0.0
    for _ in range(probes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(probe_cycles)
        e1.record()
        torch.cuda.synchronize()
        best = max(best, probe_cycles / max(e0.elapsed_time(e1), 1e-3))
    return best


def delayed(stream, fills, *, cycles, call, spoil=(), info=None):
    """The stream harness.  fills: [(input tensor, staging tensor)] -- the inputs hold their spoiled values (NaN; a named harmless value
    for integers), the staging tensors the real ones, and everything is synchronised before this is called.  Under
    torch.cuda.stream(stream): an event, a sleep of `cycles`, an event and the device-to-device copies that give the inputs their real
    values are enqueued; call() makes the wrapper call, which picks `stream` up as the current stream; every (tensor, spoiled tensor)
    of `spoil` is copied over again behind it; only then the stream is synchronised -> (what call() returned, the sleep's milliseconds).
    info (a dict, optional) receives "asleep_after_call": the sleep had not ended when call() returned."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        torch.cuda._sleep(int(cycles))
        e1.record()
        for dst, src in fills:
            dst.copy_(src, non_blocking=True)
        out = call()
        if info is not None:
            info["asleep_after_call"] = not e1.query()
        for dst, src in spoil:
            dst.copy_(src, non_blocking=True)
        stream.synchronize()
    return out, e0.elapsed_time(e1)


def runs_beside_the_null_stream(torch, stream, cycles):
    """Does work on the null stream finish while `stream` sleeps?  Streams that the runtime maps to one hardware queue run one
    behind the other, and on such a pair a launch on the wrong stream is ordered by accident."""
    end = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(cycles))
        end.record()
    default = torch.cuda.default_stream()
    with torch.cuda.stream(default):
        torch.zeros(1, device="cuda").add_(1.0)
        default.synchronize()
    beside = not end.query()
    stream.synchronize()
    return beside
