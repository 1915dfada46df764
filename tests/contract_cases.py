"""The table of the calling-contract tests: one Row per stream-taking entry of include/covo_hip.h, used by tests/test_gpu_extents.py
and tests/test_gpu_streams.py; tests/test_contract_support.py (CPU) checks that the table and EXEMPT together name every such entry.

A Row holds the entry's name, its sizes (one case each), a builder of the inputs as numpy arrays, and a body run(core, T, sz) that
makes the call through the SamplingCore wrapper (through core.lib with core.torch's allocators and core.stream() where the core has no
single-rank wrapper for the entry) and returns {name: output tensor}.  T maps the builder's names to device tensors; a key that
starts with "_" is a host-side value and is handed through as it is.  The rest of a Row says which inputs the entry also writes
(inout), what an integer input holds while it is spoiled (ints: out of range for a correct call, harmless for the kernel), which
attributes of the core the entry writes (core_out) or reads (core_in: attribute -> input name), which output elements the header
documents as not written (masks), which of the returned buffers are work areas whose contents the header does not promise (work:
their bands are checked, their contents are not) and whether the entry accumulates with floating-point atomics (atomics: (bar, note)).

torch and the package are imported inside the functions: the module imports on a machine without a GPU."""
import ctypes as C
import functools

import numpy as np

from tests import contract_support as CS
from tests.conftest import make_problem

H, NA = 32, 128
NS = (1, 63, 65, 1000)
DEV = "cuda:0"

# The stream-taking entries that have no row, each with its reason.
EXEMPT = {
    "covo_exchange_records": "multi-rank peer exchange: needs connected ranks; covered by the two-rank tests of tests/test_gpu_parity.py",
    "covo_exchange_records_cov": "multi-rank peer exchange: needs connected ranks; covered by the two-rank tests of tests/test_gpu_parity.py",
    "covo_debug_time_step": "synchronises and times by design: its only output is a host float",
    "covo_debug_time_batched": "synchronises and times by design: its only output is a host float",
    "covo_debug_time_rollout": "synchronises and times by design: its only outputs are two host floats",
    "covo_debug_raise_device_status": "test hook that raises a status bit from one thread: no caller buffer",
    "covo_sigma_profile": "only times: covo_sigma's chain with tick stamps, used by scripts/sigma_prof.py alone; covo_sigma has a row",
}


class Row:
    def __init__(self, entry, sizes, build, run, *, core=None, inout=(), ints=None, core_out=(), core_in=None, masks=None, atomics=None,
                 fresh_core=False, tag="", make=None, work=()):
        self.entry, self.sizes, self.build, self.run, self.make = entry, list(sizes), build, run, make
        self.core_kw = core or (lambda sz: dict(N=sz.get("N", 64)))
        self.inout, self.ints, self.core_out, self.core_in = tuple(inout), dict(ints or {}), tuple(core_out), dict(core_in or {})
        self.masks, self.atomics, self.fresh_core, self.tag, self.work = masks, atomics, fresh_core, tag, tuple(work)

    def new_core(self, sz):
        """the core a run of the case is made on: the shared one of its (N, options); a new one under fresh_core; make(sz)'s under make"""
        if self.make is not None:
            return self.make(sz)
        return get_core(fresh=self.fresh_core, **self.core_kw(sz))

    def cases(self):
        for sz in self.sizes:
            yield self, sz

    @staticmethod
    def case_id(row, sz):
        return "-".join([row.entry[5:] + row.tag] + [f"{k}{v}" for k, v in sz.items()])


# ---------------------------------------------------------------------------------------------- cores
_CORES = {}


def get_core(fresh=False, **kw):
    """One SamplingCore per (N, options), shared by every case of both GPU files; fresh=True: a core of the case's own (a step caches
    buffer addresses in its argument block)."""
    from covo_mpc_amd.controllers._core import SamplingCore
    kw = dict(kw)
    N = kw.pop("N")
    make = lambda: SamplingCore(N, H, 0.01, 1.0, device=DEV, compute_info=False, **kw)
    if fresh:
        return make()
    k = (N, tuple(sorted(kw.items())))
    if k not in _CORES:
        _CORES[k] = make()
    return _CORES[k]


# ---------------------------------------------------------------------------------------------- running a case
def spoiled(row, name, arr):
    """What input `name` holds before its real value arrives and after the call: NaN (a packed state keeps its time word, an int32
    whose NaN image would index far outside the trajectory), the row's named value for an integer input."""
    if arr.dtype.kind == "f":
        out = np.full_like(arr, np.nan)
        if name.startswith("packed"):
            out.reshape(-1, 32)[:, 25] = arr.reshape(-1, 32)[:, 25]
        return out
    return np.full_like(arr, row.ints[name])


def _to_dev(torch, v):
    v = np.ascontiguousarray(v)
    return torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(DEV)


def _words(t):
    """device tensor -> its bytes as a numpy uint8 array (bit comparisons; NaN payloads count)"""
    import torch
    t = t.detach().contiguous()
    return t.reshape(-1).view(torch.uint8).cpu().numpy().copy()


class Swap:
    """core attributes (and the shard's offset / global N) replaced for one call, restored afterwards"""

    def __init__(self, core, sz, **attrs):
        self.core, self.new = core, dict(attrs)
        for k, a in (("offset", "offset"), ("n_total", "N")):
            if k in sz:
                self.new[a] = sz[k]

    def __enter__(self):
        self.old = {k: getattr(self.core, k) for k in self.new}
        for k, v in self.new.items():
            setattr(self.core, k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(self.core, k, v)


def run_tight(row, core, sz, X, T=None):
    """The case on ordinary allocations and the current stream -> ({name: output bytes}, T).  T: device tensors of the inputs (made
    from X when None)."""
    import torch
    if T is None:
        T = {k: (v if k.startswith("_") else _to_dev(torch, v)) for k, v in X.items()}
    with Swap(core, sz, **{attr: T[key] for attr, key in row.core_in.items()}):
        outs = row.run(core, T, sz)
        torch.cuda.synchronize()
        res = {k: _words(v) for k, v in outs.items()}
    return res, T


def run_banded(row, core, sz, X, poison):
    """The case with every input, every output the wrapper allocates and every core buffer the entry touches between guard bands ->
    (outputs {name: tensor}, inputs {name: Alloc}, core buffers {attr: Alloc}, the BandedTorch proxy)."""
    import torch
    ins = {k: CS.banded(v, poison, DEV, torch, name=k) for k, v in X.items() if not k.startswith("_")}
    T = {k: (ins[k].view if k in ins else v) for k, v in X.items()}
    bufs = {}
    for attr in row.core_out:
        old = getattr(core, attr) if attr != "_eps" else core.eps
        bufs[attr] = CS.banded_empty(tuple(old.shape), old.dtype, poison, DEV, torch, name=f"core.{attr}")
    proxy = CS.BandedTorch(torch, poison)
    attrs = {attr: T[key] for attr, key in row.core_in.items()}
    attrs.update({attr: al.view for attr, al in bufs.items()}, torch=proxy)
    with Swap(core, sz, **attrs):
        outs = row.run(core, T, sz)
        torch.cuda.synchronize()
    return outs, ins, bufs, proxy


def check_banded(row, sz, X, outs, ins, bufs, proxy):
    """Steps 2, 3 and 6 on one banded run: every band intact, no `empty` payload element left unwritten outside the row's masks, every
    const input bit-unchanged -> list of findings (empty: the contract holds)."""
    found = []
    everything = list(ins.values()) + list(bufs.values()) + proxy.allocs
    for al in everything:
        b = CS.bands_intact(al)
        if b is not None:
            found.append(f"store outside the extent: {b!r}")
    masks = row.masks(sz, X) if row.masks else {}
    named = {}
    for name, m in masks.items():
        t = outs[name]
        al = CS.owner(list(bufs.values()) + proxy.allocs, t)
        assert al is not None and al.view.numel() == t.numel(), f"mask {name}: not a whole allocation"
        named[id(al)] = m
    scratch = {id(CS.owner(list(bufs.values()) + proxy.allocs, outs[name])) for name in row.work}
    for al in list(bufs.values()) + [a for a in proxy.allocs if a.kind == "empty"]:
        if id(al) in scratch:  # a work area: the header promises no contents, only its extent (the bands above)
            continue
        m = named.get(id(al))
        if m is not None:
            kept = np.zeros(al.view.numel(), dtype=bool)
            kept[CS.unwritten(al)] = True
            if not kept[np.asarray(m, dtype=bool).reshape(-1)].all():
                found.append(f"{al.name}: an element the header leaves unwritten was written")
        left = CS.unwritten(al, m)
        if left.size:
            found.append(f"{al.name} {tuple(al.view.shape)}: {left.size} element(s) not written, the first at flat index {left[:8].tolist()}")
    for k, al in ins.items():
        if k in row.inout:
            continue
        want = np.ascontiguousarray(X[k]).reshape(-1).view(np.uint8)
        if not np.array_equal(_words(al.view), want):
            found.append(f"const input {k} changed")
    return found


def same(row, a, b, sz=None, X=None):
    """two {name: bytes} results: bit-equal (outside the elements the row's masks name: nobody writes them), or within the bar of an
    atomics row -> list of the names that differ"""
    bad = []
    masks = row.masks(sz, X) if row.masks and sz is not None else {}
    for k in a:
        if k in row.work:
            continue
        if k in masks and a[k].size == b[k].size:
            m = np.asarray(masks[k], dtype=bool).reshape(-1)
            keep = np.repeat(~m, a[k].size // m.size)
            if np.array_equal(a[k][keep], b[k][keep]):
                continue
        if np.array_equal(a[k], b[k]):
            continue
        if row.atomics is not None and a[k].size % 8 == 0:
            x, y = a[k].view(np.float64), b[k].view(np.float64)
            if np.all(np.isfinite(x)) and np.abs(x - y).max() <= row.atomics[0] * max(np.abs(x).max(), 1e-300):
                continue
        bad.append(k)
    return bad


# ---------------------------------------------------------------------------------------------- inputs
def _pack(s):
    """the packed state float32 [32] of an oracle state (the layout of tests/gpu_support.py: dev_state)"""
    x = np.zeros(32, dtype=np.float32)
    x[0:3], x[3:6], x[6:10], x[10:13], x[13:16] = s.pos, s.vel, s.quat, s.omega, s.f_disturb
    x[16:19], x[19:22], x[22:25] = s.pos_tar, s.vel_tar, s.acc_tar
    x[25:26] = np.asarray([s.time], dtype=np.int32).view(np.float32)
    return x


@functools.lru_cache(maxsize=None)
def _problem(seed=0, B=1):
    """make_problem's state as arrays: packed [B, 32] (entry b moved by b cm), the trajectories, the parameters"""
    s, p, _ = make_problem(seed=seed, time=37)
    packed = np.stack([_pack(s.replace(pos=s.pos + 0.01 * b)) for b in range(B)])
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(packed=packed, pos_traj=f(s.pos_traj), vel_traj=f(s.vel_traj), acc_traj=f(s.acc_traj), _p=p)


def _state(seed=0, B=1, acc=False):
    st = dict(_problem(seed, B))
    if not acc:
        del st["acc_traj"]
    return st


def _stripes(p, rng, N, B=None):
    """sample_actions in the stripe layout [H, N, 4] ([B, H, N, 4])"""
    from oracle import ref_np as R
    n = N * (B or 1)
    a = np.clip(R.hover_action(p, H, np.float64)[None] + 0.5 * rng.normal(size=(n, H, 4)), -1, 1).astype(np.float32)
    a = a.reshape((B or 1), N, H, 4).transpose(0, 2, 1, 3)
    return np.ascontiguousarray(a if B else a[0])


def _mean(p, rng, B=1, scale=0.1):
    from oracle import ref_np as R
    return (R.hover_action(p, H, np.float64).reshape(-1)[None] + scale * rng.normal(size=(B, NA))).astype(np.float32)


def _factor(rng):
    A = rng.normal(size=(NA, NA))
    return np.linalg.cholesky(A @ A.T / NA + 0.05 * np.eye(NA)).astype(np.float32)


def _blocks(rng):
    return np.stack([np.linalg.cholesky((lambda B: B @ B.T + 0.1 * np.eye(4))(rng.normal(size=(4, 4)))) for _ in range(H)]).astype(np.float32)


def _costs(rng, shape):
    return (5.0 + 3.0 * rng.random(size=shape)).astype(np.float32)


def _groupmin(cost):
    n = cost.shape[-1]
    return np.stack([cost[..., i:i + 64].min(axis=-1) for i in range(0, n, 64)], axis=-1).astype(np.float32)


def _sym(rng, B):
    A = rng.normal(size=(B, NA, NA))
    return np.ascontiguousarray(0.5 * (A + A.transpose(0, 2, 1)) + np.stack([np.diag(rng.uniform(0, 30, NA)) for _ in range(B)]))


def _ds(T):
    from covo_mpc_amd.dynamics.dataclass import DeviceState
    return DeviceState(packed=T["packed"], pos_traj=T["pos_traj"], vel_traj=T["vel_traj"])


def _pc(T, kind="none"):
    from tests.gpu_support import DP, params_c
    p = T["_p"]
    return params_c(p.replace(disturb_params=np.asarray(DP)) if kind != "none" else p, kind=kind)


def _lib():
    from covo_mpc_amd import _lib
    return _lib


def _call(core, name, *args):
    L = _lib()
    L.check(getattr(core.lib, name)(core.h, *[L.ptr(a) if hasattr(a, "data_ptr") else a for a in args], core.stream()), name)


def _direct(name, outs, args):
    """the body of an entry the core has no single-rank wrapper for: outs(core, sz) -> {name: output tensor}, allocated through
    core.torch; args(core, T, sz, o) -> the entry's arguments between the handle and the stream"""
    def run(core, T, sz):
        o = outs(core, sz)
        _call(core, name, *args(core, T, sz, o))
        return o
    return run


def _mean_and_sums(core, sz):
    return {"mean": _f32(core, NA), "stats": _f64(core, _lib().COVO_POS_STATS_DOUBLES)}


def _f32(core, *shape):
    return core.torch.empty(shape, dtype=core.torch.float32, device=core.device)


def _f64(core, *shape):
    return core.torch.empty(shape, dtype=core.torch.float64, device=core.device)


def _pad_mask(n):
    """include/covo_hip.h, covo_softmax_reduce: "floats 130 and 131 (the pad) are not written" (the record is {m, s, v[128], pad[2]})"""
    def masks(sz, X):
        m = np.zeros(n(), dtype=bool)
        m[130:132] = True
        return {"rec": m}
    return masks


def _update_inputs(sz, cov=False):
    N = sz["N"]
    st = _state(3)
    rng = np.random.default_rng(100 + N)
    cost = _costs(rng, (N,))
    X = dict(a=_stripes(st["_p"], rng, N), cost=cost, blockmin=_groupmin(cost), a_mean=_mean(st["_p"], rng)[0])
    if cov:
        X["a_cov"] = np.stack([np.eye(4, dtype=np.float32) * 0.25 for _ in range(H)])
    return X


_UPD = dict(core_in={"a": "a", "cost": "cost", "blockmin": "blockmin"})
_sizesN = [dict(N=n) for n in NS]
_shard = dict(N=65, offset=3 * 65, n_total=4 * 65)
KEY = (77, 88)


def _records(sz, floats, cov=False):
    """G rank records {m, s, v[128], pad[2]} (+ 320 second moments) with the position sums at the end, the old mean (and covariances)"""
    L = _lib()
    G = sz["G"]
    rng = np.random.default_rng(200 + G + floats)
    rec = np.zeros((G, floats), dtype=np.float32)
    rec[:, 0] = _costs(rng, (G,))
    rec[:, 1] = 1.0 + rng.random(G)
    rec[:, 2:2 + NA] = 0.3 * rng.normal(size=(G, NA))
    if cov:
        rec[:, L.COVO_PARTIAL_FLOATS:L.COVO_PARTIAL_FLOATS + L.COVO_COV_FLOATS] = 0.1 * rng.random(size=(G, L.COVO_COV_FLOATS))
    if floats > L.COVO_PARTIAL_FLOATS:
        sums = rng.normal(size=(G, L.COVO_POS_STATS_DOUBLES))
        rec[:, floats - 2 * L.COVO_POS_STATS_DOUBLES:] = sums.view(np.float32)
    X = dict(records=rec, a_mean=(0.2 * rng.normal(size=NA)).astype(np.float32))
    if cov:
        X["a_cov"] = np.stack([np.eye(4, dtype=np.float32) * 0.25 for _ in range(H)])
    return X


# ---------------------------------------------------------------------------------------------- bodies
def _noise_inputs(sz, eps=None, what="L"):
    N = sz["N"]
    rng = np.random.default_rng(10 + N)
    st = _state(1)
    X = dict(mu=_mean(st["_p"], rng, scale=0.3)[0])
    if what == "L":
        X["L"] = _factor(rng) + np.triu(rng.normal(size=(NA, NA)).astype(np.float32), 1)  # above the diagonal: ignored
    elif what == "Ls":
        X["Ls"] = _blocks(rng)
    elif what == "basis":
        X["basis"] = (0.3 * rng.normal(size=(H, sz["M"]))).astype(np.float32)
    elif what == "G":
        X["G"] = (0.3 * rng.normal(size=(NA, 4 * sz["M"]))).astype(np.float32)
    if eps:
        X["eps"] = rng.normal(size=(N, NA)).astype(np.float32)
    return X


def _hess_inputs(sz):
    B = sz["B"]
    st = _state(5, B)
    st["a_mean"] = _mean(st["_p"], np.random.default_rng(300 + B), B)
    return st


def _run_hessian(method):
    def run(core, T, sz):
        return {"R": core.hessian(T["packed"].reshape(-1), _ds(T), _pc(T), T["a_mean"].reshape(-1), batch=sz["B"], method=method)}
    return run


def _run_sigma(method):
    def run(core, T, sz):
        S, Lf = core.sigma(T["R"], 0.5, batch=sz["B"], method=method)
        return {"Sigma": S, "L": Lf}
    return run


def _cost_rows(sz):
    rng = np.random.default_rng(400 + sz["N"] + sz["E"])
    return dict(cost=_costs(rng, (sz["E"], sz["N"])))


def _rollout_inputs(sz, extra=()):
    N = sz["N"]
    st = _state(7)
    rng = np.random.default_rng(500 + N)
    st["a"] = _stripes(st["_p"], rng, N)
    if "cost" in extra:
        st["cost"] = _costs(rng, (N,))
    if "idx" in extra:
        st["idx"] = rng.integers(0, N, size=sz["K"]).astype(np.int32)
    if "means" in extra:
        m = _mean(st["_p"], rng, 2)
        st["a_nominal"], st["a_mean"] = m[0], m[1]
    return st


@functools.lru_cache(maxsize=None)
def _sweep(B):
    """the device's own Riccati sweep at the plan of _plan_inputs(B): numpy K, kff, x, rows (inputs of the entries that take gains)"""
    import torch
    X = _plan_inputs(dict(B=B))
    core = get_core(N=64)
    T = {k: (v if k.startswith("_") else _to_dev(torch, v)) for k, v in X.items()}
    out = core.riccati(_ds(T), _pc(T), T["a_mean"], packed=T["packed"])
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in ("K", "kff", "x", "rows")}


def _plan_inputs(sz, gains=False, sigma=False):
    B = sz["B"]
    st = _state(17, B)
    rng = np.random.default_rng(600 + B)
    st["a_mean"] = _mean(st["_p"], rng, B)
    if gains:
        st.update({k: v for k, v in _sweep(B).items() if k != "rows"})
    if sigma:
        Lf = _factor(rng)
        st["Sigma"] = np.ascontiguousarray((Lf.astype(np.float64) @ Lf.T.astype(np.float64)).astype(np.float32))
        st["a_mean"] = st["a_mean"][0]
    return st


def _run_riccati(box):
    def run(core, T, sz):
        return core.riccati(_ds(T), _pc(T), T["a_mean"], packed=T["packed"], box=box)
    return run


def _run_refine(feedback, box):
    def run(core, T, sz):
        r = core.riccati_refine(_ds(T), _pc(T), T["a_mean"], feedback=feedback, box=box)
        out = {f"out{i}": t for i, t in enumerate(r)}
        out["a_mean"] = T["a_mean"]
        return out
    return run


def _run_feedback(core, T, sz):
    a_out, aux = core.feedback_rollout(_ds(T), _pc(T), T["a_mean"], T["K"], T["kff"], T["x"], alphas=[4.0, 1.0, 0.25][:sz["A"]],
                                       packed=T["packed"])
    return {"a_out": a_out, "aux": aux}


def _run_plan_hold(core, T, sz):
    u, rows = core.plan_hold(T["packed"], T["a_mean"], T["K"], T["kff"], T["x"], 0.5, 3, t_plan=T["t_plan"])
    return {"u": u, "rows": rows}


def _hold_inputs(sz):
    st = _plan_inputs(sz, gains=True)
    st["t_plan"] = np.full((sz["B"],), 37, dtype=np.int32)
    del st["pos_traj"], st["vel_traj"]
    return st


def _run_newton(core, T, sz):
    row, costs = core.newton_refine(_ds(T), _pc(T), T["a_mean"], T["Sigma"], 0.25)
    return {"row": row, "costs": costs, "a_mean": T["a_mean"]}


def _run_arbitrate(core, T, sz):
    row = core.arbitrate(_ds(T), _pc(T), T["a_nominal"], T["a_mean"], 0b111)
    return {"row": row, "a_mean": T["a_mean"]}


def _run_table(core, T, sz):
    L = _lib()
    kw = dict(keys_dev=T["keys"]) if "keys" in T else dict(key=KEY)
    return {"table": core.disturb_table(_pc(T, sz["kind"]), T["packed"], key_mode=L.DISTURB_KEYS_HESSIAN, deterministic=True,
                                        batch=sz["B"], **kw)}


def _table_inputs(sz):
    st = _state(9, sz["B"])
    del st["pos_traj"], st["vel_traj"]
    if sz.get("keys"):
        st["keys"] = np.random.default_rng(9).integers(0, 2 ** 32, size=(sz["B"], 2), dtype=np.uint64).astype(np.uint32)
    return st


def _run_ws_sigma(core, T, sz):
    S, Lf = core.sigma(T["R"], 0.5, batch=sz["B"])
    out = _f64(core, 4)  # SC_SHIFT, SC_LMIN, SC_DELTA, SC_SCALE of matrix 0 (csrc/sigma_ns.hip; the slots from 16 on hold clock stamps)
    _call(core, "covo_debug_sigma_workspace", out, C.c_int64(11 * sz["B"] * NA * NA), C.c_int64(4))
    return {"slots": out, "L": Lf}


def _run_ws_hess(core, T, sz):
    Rm = core.hessian(T["packed"].reshape(-1), _ds(T), _pc(T), T["a_mean"].reshape(-1), batch=sz["B"])
    out = _f64(core, 512)  # WS_X of batch entry 0: the 32 x 16 nominal states (csrc/hessian_adj_body.hpp)
    _call(core, "covo_debug_hess_workspace", out, C.c_int64(0), C.c_int64(512))
    return {"X": out, "R": Rm}


def _post_inputs(sz):
    N, B = sz["N"], 3
    st = _state(11)
    rng = np.random.default_rng(700 + N)
    return dict(a=_stripes(st["_p"], rng, N, B), cost=_costs(rng, (B, N)), mu=_mean(st["_p"], rng, B))


def _run_post(core, T, sz):
    cov, d, W = core.weighted_cov(T["a"], T["cost"], T["mu"], elite=sz.get("K"))
    return {"cov": cov, "d": d, "W": W}


def _chol(n):
    from tests.chol_cases import batch_cases
    return batch_cases(n, 3)


def _factors(sz):
    rng = np.random.default_rng(800)
    Ls = np.stack([_factor(rng) for _ in range(3)])
    Cs = np.stack([(lambda F: (F.astype(np.float64) @ F.T.astype(np.float64)).astype(np.float32))(_factor(rng)) for _ in range(3)])
    return dict(L=np.ascontiguousarray(np.tril(Ls)), C=Cs)


ROWS = [
    # ---- noise
    Row("covo_randn", _sizesN + [_shard], lambda sz: {}, lambda core, T, sz: {"eps": core.randn(KEY)}, core_out=("_eps",)),
    Row("covo_randn_jax", [dict(N=n, mppi=m) for n in NS for m in (0, 1)] + [dict(_shard, mppi=0)], lambda sz: {},
        lambda core, T, sz: {"eps": core.randn_jax(KEY, mppi=bool(sz["mppi"]))}, core_out=("_eps",)),
    Row("covo_noise_gemm", _sizesN, lambda sz: _noise_inputs(sz, eps=True),
        lambda core, T, sz: {"a": core.noise_gemm(T["L"], T["mu"], T["eps"])}, core_out=("a",)),
    Row("covo_noise_gemm_philox", _sizesN + [_shard], _noise_inputs,
        lambda core, T, sz: {"a": core.noise_gemm_philox(T["L"], T["mu"], KEY)}, core_out=("a",)),
    Row("covo_noise_blockdiag", _sizesN, lambda sz: _noise_inputs(sz, eps=True, what="Ls"),
        lambda core, T, sz: {"a": core.noise_blockdiag(T["Ls"], T["mu"], T["eps"])}, core_out=("a",)),
    Row("covo_noise_blockdiag_philox", _sizesN + [_shard], lambda sz: _noise_inputs(sz, what="Ls"),
        lambda core, T, sz: {"a": core.noise_blockdiag_philox(T["Ls"], T["mu"], KEY)}, core_out=("a",)),
    Row("covo_noise_nodes_philox", [dict(N=n, M=m) for n, m in ((1, 2), (63, 5), (65, 32), (1000, 5), (65, 2))] + [dict(_shard, M=5)],
        lambda sz: _noise_inputs(sz, what="basis"), lambda core, T, sz: {"a": core.noise_nodes(T["basis"], T["mu"], KEY)}, core_out=("a",)),
    Row("covo_noise_factor_philox", [dict(N=n, M=m) for n, m in ((1, 2), (63, 3), (65, 16), (1000, 3))] + [dict(_shard, M=3)],
        lambda sz: _noise_inputs(sz, what="G"), lambda core, T, sz: {"a": core.noise_factor(T["G"], T["mu"], KEY)}, core_out=("a",)),
    Row("covo_shift_mean", [dict()], lambda sz: dict(a_mean=_mean(_state(1)["_p"], np.random.default_rng(1))[0]),
        lambda core, T, sz: {"out": core.shift_mean(T["a_mean"])}),
    # ---- rollout and what reads its outputs
    Row("covo_rollout_cost", _sizesN, _rollout_inputs,
        lambda core, T, sz: {"cost": core.rollout(_ds(T), _pc(T), (0.01, -0.02, 0.03), True), "blockmin": core.blockmin,
                             "stats": core.stats.clone()}, core_in={"a": "a"}, core_out=("cost", "blockmin")),
    Row("covo_disturb_table", [dict(B=1, kind="periodic"), dict(B=3, kind="mixed"), dict(B=3, kind="periodic", keys=1)], _table_inputs,
        _run_table, ints={"keys": 0x0BAD0BAD}),
    Row("covo_pos_info", [dict()], lambda sz: dict(stats=np.abs(np.random.default_rng(2).normal(size=192)) * 64, packed=_state(1)["packed"][0]),
        lambda core, T, sz: core.info(_ds(dict(T, pos_traj=None, vel_traj=None))), core_in={"stats_total": "stats"}),
    Row("covo_rollout_fan", [dict(N=65, K=1), dict(N=65, K=5), dict(N=1000, K=5)], lambda sz: _rollout_inputs(sz, ("idx",)),
        lambda core, T, sz: {"rows": core.rollout_fan(_ds(T), _pc(T), T["idx"], f_shared=(0.01, -0.02, 0.03))},
        core_in={"a": "a"}, ints={"idx": 0x7FFFFFFF}),
    Row("covo_arbitrate", [dict(N=65), dict(N=1000)], lambda sz: _rollout_inputs(sz, ("cost", "means")), _run_arbitrate,
        core_in={"a": "a", "cost": "cost"}, inout=("a_mean",)),
    # ---- the update
    Row("covo_softmax_update", _sizesN, _update_inputs, lambda core, T, sz: {"mean": core.update(T["a_mean"], 0.8)}, **_UPD),
    Row("covo_softmax_update_cov", _sizesN, lambda sz: _update_inputs(sz, cov=True),
        lambda core, T, sz: dict(zip(("mean", "cov"), core.update_cov(T["a_mean"], 0.8, T["a_cov"], 0.5))), **_UPD),
    Row("covo_softmax_reduce", _sizesN, _update_inputs,
        _direct("covo_softmax_reduce", lambda core, sz: {"rec": _f32(core, _lib().COVO_PARTIAL_FLOATS)},
                lambda core, T, sz, o: (core.cost, core.a, sz["N"], core.blockmin, o["rec"])),
        masks=_pad_mask(lambda: _lib().COVO_PARTIAL_FLOATS), **_UPD),
    Row("covo_softmax_reduce_cov", _sizesN, _update_inputs,
        _direct("covo_softmax_reduce_cov", lambda core, sz: {"rec": _f32(core, _lib().COVO_PARTIAL_FLOATS + _lib().COVO_COV_FLOATS)},
                lambda core, T, sz, o: (core.cost, core.a, sz["N"], core.blockmin, T["a_mean"], o["rec"])),
        masks=_pad_mask(lambda: _lib().COVO_PARTIAL_FLOATS + _lib().COVO_COV_FLOATS), **_UPD),
    Row("covo_merge", [dict(G=1), dict(G=3)], lambda sz: _records(sz, _lib().COVO_PARTIAL_FLOATS),
        _direct("covo_merge", lambda core, sz: {"mean": _f32(core, NA)},
                lambda core, T, sz, o: (T["records"], sz["G"], T["a_mean"], C.c_float(0.8), o["mean"]))),
    Row("covo_merge_ranks", [dict(G=1), dict(G=3)], lambda sz: _records(sz, _lib().COVO_RANK_RECORD_FLOATS),
        _direct("covo_merge_ranks", _mean_and_sums,
                lambda core, T, sz, o: (T["records"], sz["G"], T["a_mean"], C.c_float(0.8), o["mean"], o["stats"]))),
    Row("covo_merge_ranks_wide", [dict(G=3, cov=0), dict(G=3, cov=1)],
        lambda sz: _records(sz, _lib().COVO_RANK_RECORD_COV_FLOATS if sz["cov"] else _lib().COVO_RANK_RECORD_FLOATS),
        _direct("covo_merge_ranks_wide", _mean_and_sums,
                lambda core, T, sz, o: (T["records"], sz["G"], int(T["records"].shape[1]), T["a_mean"], C.c_float(0.8), o["mean"], o["stats"]))),
    Row("covo_merge_ranks_cov", [dict(G=1), dict(G=3)], lambda sz: _records(sz, _lib().COVO_RANK_RECORD_COV_FLOATS, cov=True),
        _direct("covo_merge_ranks_cov", lambda core, sz: dict(_mean_and_sums(core, sz), cov=_f32(core, H, 4, 4)),
                lambda core, T, sz, o: (T["records"], sz["G"], T["a_mean"], C.c_float(0.8), T["a_cov"], C.c_float(0.5), o["mean"], o["cov"],
                                        o["stats"]))),
    Row("covo_ess_lambda", [dict(N=n, E=e) for n, e in ((63, 1), (65, 3), (1000, 3))], _cost_rows,
        _direct("covo_ess_lambda", lambda core, sz: {"rows": _f32(core, sz["E"], _lib().COVO_LAM_FLOATS)},
                lambda core, T, sz, o: (T["cost"], sz["N"], sz["E"], C.c_float(0.01), C.c_float(4.0), o["rows"]))),
    Row("covo_cost_standardise", [dict(N=n, E=e) for n, e in ((1, 1), (63, 1), (65, 3), (1000, 3))], _cost_rows,
        lambda core, T, sz: {"rows": core.cost_standardise(T["cost"], 0.5)}),
    Row("covo_elite_select", [dict(N=n, E=e, K=k) for n, e, k in ((1, 1, 1), (63, 3, 1), (65, 1, 65), (65, 3, 1), (1000, 3, 1000), (1000, 1, 1))],
        _cost_rows, lambda core, T, sz: {"rows": core.elite_select(T["cost"], sz["K"])}),
    Row("covo_weighted_cov", [dict(N=1), dict(N=63), dict(N=65), dict(N=1000), dict(N=65, K=65), dict(N=1000, K=1)], _post_inputs, _run_post),
    # ---- Hessian, gradient, Sigma
    Row("covo_hessian", [dict(B=1), dict(B=3)], _hess_inputs, _run_hessian("adjoint")),
    Row("covo_hessian_pairs", [dict(B=1), dict(B=3)], _hess_inputs, _run_hessian("pairs"),
        atomics=(1e-9, "csrc/hessian.hip zeroes R with a memset, then every pair's block accumulates with fp64 atomics: the order of the "
                       "additions is not fixed; 1e-9 of max |R| is the bar tests/test_gpu_parity.py holds it to against covo_hessian")),
    Row("covo_cost_gradient", [dict(B=1), dict(B=3)], _hess_inputs,
        lambda core, T, sz: {"g": core.cost_gradient(_ds(T), _pc(T), T["a_mean"], packed=T["packed"])}),
    Row("covo_sigma", [dict(B=1), dict(B=3)], lambda sz: dict(R=_sym(np.random.default_rng(3), sz["B"])), _run_sigma("ns")),
    Row("covo_sigma_jacobi", [dict(B=1), dict(B=3)], lambda sz: dict(R=_sym(np.random.default_rng(3), sz["B"])), _run_sigma("jacobi")),
    Row("covo_debug_sigma_workspace", [dict(B=1), dict(B=3)], lambda sz: dict(R=_sym(np.random.default_rng(3), sz["B"])), _run_ws_sigma),
    Row("covo_debug_hess_workspace", [dict(B=1)], _hess_inputs, _run_ws_hess),
    Row("covo_sigma_nodes", [dict(B=b, M=m) for b, m in ((1, 2), (3, 3), (3, 16))], lambda sz: dict(R=_sym(np.random.default_rng(4), sz["B"])),
        lambda core, T, sz: dict(zip(("SigM", "G", "Sigma", "rows"), core.sigma_nodes(T["R"], sz["M"])))),
    Row("covo_sigma_shift", [dict(B=3)], lambda sz: dict(L=_factors(sz)["L"]),
        lambda core, T, sz: dict(zip(("Sigma", "L"), core.sigma_shift(T["L"])))),
    Row("covo_sigma_adapt", [dict(B=3)], _factors,
        lambda core, T, sz: dict(zip(("Sigma", "L", "rows"), core.sigma_adapt(T["L"], T["C"], 0.3)))),
    Row("covo_cholesky", [dict(n=n) for n in (1, 5, 8, 9, 24, 72, 127, 128)],
        lambda sz: dict(A=_chol(sz["n"])),
        lambda core, T, sz: {"L": core.cholesky(T["A"], sz["n"], 3)}),
    # ---- Riccati, refinement, hold
    Row("covo_riccati", [dict(B=1), dict(B=3)], _plan_inputs, _run_riccati(False)),
    Row("covo_riccati_box", [dict(B=1), dict(B=3)], _plan_inputs, _run_riccati(True)),
    Row("covo_riccati_refine", [dict(B=1)], lambda sz: dict(_plan_inputs(sz), a_mean=_plan_inputs(sz)["a_mean"][0]),
        _run_refine(False, False), inout=("a_mean",)),
    Row("covo_riccati_refine_feedback", [dict(B=1)], lambda sz: dict(_plan_inputs(sz), a_mean=_plan_inputs(sz)["a_mean"][0]),
        _run_refine(True, False), inout=("a_mean",)),
    Row("covo_riccati_refine_box", [dict(B=1, fb=0), dict(B=1, fb=1)], lambda sz: dict(_plan_inputs(sz), a_mean=_plan_inputs(sz)["a_mean"][0]),
        lambda core, T, sz: _run_refine(bool(sz["fb"]), True)(core, T, sz), inout=("a_mean",)),
    Row("covo_feedback_rollout", [dict(B=1, A=1), dict(B=3, A=3)], lambda sz: _plan_inputs(sz, gains=True), _run_feedback),
    Row("covo_plan_hold", [dict(B=1), dict(B=3)], _hold_inputs, _run_plan_hold, ints={"t_plan": 0x7FFFFFF0}),
    Row("covo_newton_refine", [dict(B=1)], lambda sz: _plan_inputs(sz, sigma=True), _run_newton, inout=("a_mean",)),
]


# ---------------------------------------------------------------------------------------------- the fused step and its copy-outs
_MODES = {"mppi": "MODE_MPPI", "offline": "MODE_COVO_OFFLINE", "online": "MODE_COVO_ONLINE"}


def _step_inputs(sz):
    st = _state(21)
    rng = np.random.default_rng(900 + sz["N"])
    st["a_mean"] = _mean(st["_p"], rng)[0]
    if sz["mode"] == "mppi":
        st["a_cov"] = np.stack([np.eye(4, dtype=np.float32) * 0.25 for _ in range(H)])
    if sz["mode"] == "offline":  # 38 factors: the state's time 37 takes the table's last row (the index is clamped into the table)
        Lf = np.tril(_factor(rng))
        st["L_table"] = np.ascontiguousarray(np.stack([Lf * np.float32(1.0 + 0.01 * t) for t in range(38)]))
    return st


def step_call(core, T, sz, k):
    """call k of a case of the fused step: key (11 + k, 22); the first call reads the caller's mean where it lies, the later ones the
    handle's own buffer, as a controller's do -> (mean, covariance or None), views of the handle's persistent buffers"""
    L = _lib()
    mode = getattr(L, _MODES[sz["mode"]])
    kw = dict(derive_keys=True, sample_sigma=0.5, rollout_deterministic=sz["mode"] != "mppi")
    if sz["mode"] == "mppi":
        kw["a_cov"] = T["a_cov"] if k == 0 else core._bufs["a_cov_mppi"]
    if sz["mode"] == "offline":
        kw["L_table"] = T["L_table"]
    am = T["a_mean"] if k == 0 else core._bufs["a_mean"]
    return core.step(mode, _ds(T), _pc(T), am, (11 + k, 22), **kw)


def _run_step(core, T, sz, calls=4):
    """4 calls: a graph core (use_graph=True) runs its eager, capture and replay forms"""
    outs = {}
    for k in range(calls):
        am, cov = step_call(core, T, sz, k)
        outs[f"mean{k}"] = am.clone()
    outs.update(a=core.a, cost=core.cost, blockmin=core.blockmin)
    if cov is not None:
        outs["cov"] = cov
    return outs


def _step_core(sz):
    kw = dict(N=sz["N"], use_graph=bool(sz.get("graph", 1)))
    for k in ("riccati", "plan_hold", "sigma_nodes"):
        if k in sz:
            kw[k] = sz[k]
    return kw


def _run_sigma_factor(core, T, sz):
    outs = _run_step(core, T, sz, calls=2)
    outs["factor"] = core.sigma_factor()
    return outs


def _run_plan_latch(core, T, sz):
    outs = _run_step(core, T, sz, calls=1)
    outs.update({f"latch_{k}": v for k, v in core.plan_latch().items()})
    return outs


def _run_step_sigma_nodes(core, T, sz):
    outs = _run_step(core, T, sz, calls=2)
    G = _f32(core, 1, NA, 4 * sz["sigma_nodes"])
    outs.update(SigM=core.read_sigma_node_cov(G), G=G)
    return outs


# include/covo_hip.h, covo_step_args / covo_batch_args: "groupmin: work ... a step may leave it unwritten"
_STEP = dict(core=_step_core, core_out=("a", "cost", "blockmin"), fresh_core=True, work=("blockmin",))
ROWS += [
    Row("covo_mpc_step", [dict(mode="mppi", N=100), dict(mode="offline", N=1000), dict(mode="online", N=1000),
                          dict(mode="online", N=1000, graph=0)], _step_inputs, _run_step, **_STEP),
    Row("covo_debug_sigma_factor", [dict(mode="online", N=65)], _step_inputs, _run_sigma_factor, **_STEP),
    Row("covo_debug_plan_latch", [dict(mode="mppi", N=65, riccati=True, plan_hold=3)], _step_inputs, _run_plan_latch, **_STEP),
    Row("covo_step_sigma_nodes", [dict(mode="online", N=65, sigma_nodes=3)], _step_inputs, _run_step_sigma_nodes,
        core=_step_core, core_out=("a", "cost", "blockmin", "sigma_node_cov"), fresh_core=True, work=("blockmin",)),
]


# ---------------------------------------------------------------------------------------------- the device env and the nominal chain
STEP_KEY = (C.c_uint32 * 2)(5, 6)


def _env_inputs(sz):
    E = sz["E"]
    rng = np.random.default_rng(1000 + E)
    if E == 0:  # covo_env_step: one instance without the leading axis
        st = _state(25, 1, acc=True)
        st.update(packed=st["packed"][0], action=(0.3 * rng.normal(size=4)).astype(np.float32), log=np.zeros((4, 4), dtype=np.float32))
        return st
    st = _state(25, E, acc=True)
    st["log"] = np.zeros((E, 4, 4), dtype=np.float32)
    for k in ("pos_traj", "vel_traj", "acc_traj"):
        st[k] = np.ascontiguousarray(np.stack([st[k]] * E))
    st["a_mean"] = _mean(st["_p"], rng, E, scale=0.3)
    return st


def _run_env_step(core, T, sz):
    noisy = _f32(core, 32)
    pc = _pc(T)
    _call(core, "covo_env_step", T["packed"], noisy, T["pos_traj"], T["vel_traj"], T["acc_traj"], int(T["pos_traj"].shape[0]), C.byref(pc),
          T["action"], STEP_KEY, 1, C.c_float(0.01), T["log"], 2)
    return {"true": T["packed"], "noisy": noisy, "log": T["log"]}


def _run_env_step_batched(core, T, sz):
    L = _lib()
    E = sz["E"]
    noisy = _f32(core, E, 32)
    pcs = (L.EnvParamsC * E)(*[_pc(T) for _ in range(E)])
    keys = (C.c_uint32 * (2 * E))(*range(7, 7 + 2 * E))
    _call(core, "covo_env_step_batched", E, T["packed"], noisy, T["pos_traj"], T["vel_traj"], T["acc_traj"], int(T["pos_traj"].shape[1]), pcs,
          T["a_mean"], keys, 1, C.c_float(0.01), T["log"], 4, 2)
    return {"true": T["packed"], "noisy": noisy, "log": T["log"]}


def _run_pid_nominal(core, T, sz):
    n = sz["steps"]
    pc, pid_pc = _pc(T), _pc(T)
    states, means = _f32(core, n, 32), _f32(core, n, NA)
    keys = core.torch.empty((n, 2), dtype=core.torch.int32, device=core.device)
    _call(core, "covo_pid_nominal", T["packed"], T["pos_traj"], T["vel_traj"], T["acc_traj"], int(T["pos_traj"].shape[0]), C.byref(pc),
          C.byref(pid_pc), C.c_float(10.0), C.c_float(5.0), C.c_float(10.0), 3, 4, n, states, means, keys)
    return {"states": states, "means": means, "keys": keys}


ROWS += [
    Row("covo_env_step", [dict(E=0)], _env_inputs, _run_env_step, inout=("packed", "log")),
    Row("covo_env_step_batched", [dict(E=1), dict(E=3)], _env_inputs, _run_env_step_batched, inout=("packed", "log")),
    Row("covo_pid_nominal", [dict(steps=1), dict(steps=5)],
        lambda sz: (lambda st: dict(st, packed=st["packed"][0]))(_state(27, 1, acc=True)), _run_pid_nominal),
]


# ---------------------------------------------------------------------------------------------- env-batched steps, the episode drivers
_ENV = {}


def _env():
    from tests.gpu_support import quad_env
    if "e" not in _ENV:
        _ENV["e"] = quad_env(task="tracking_zigzag")
    return _ENV["e"]


def _make_batched(sz):
    """the core of an env-batched controller for E = 2 instances (the controller rides along as core.contract_b)"""
    import covo_mpc_amd as cm
    E, N = 2, sz["N"]
    if sz["mode"] == "mppi":
        b = cm.controllers.BatchedMPPIController(_env(), E, N, H, 0.01, device=DEV)
    else:
        b = cm.controllers.BatchedCoVOController(_env(), E, N, H, 0.01, device=DEV, mode="online")
    b.core.contract_b = b
    return b.core


def _batched_inputs(sz):
    E = 2
    st = _state(29, E, acc=True)
    rng = np.random.default_rng(1100 + sz["N"])
    for k in ("pos_traj", "vel_traj", "acc_traj"):
        st[k] = np.ascontiguousarray(np.stack([st[k]] * E))
    st["a_mean"] = _mean(st["_p"], rng, E)
    if sz["mode"] == "mppi":
        st["a_cov"] = np.ascontiguousarray(np.stack([[np.eye(4, dtype=np.float32) * 0.25] * H] * E))
    if sz.get("episode"):
        st["true"] = st["packed"].copy()
    else:
        del st["acc_traj"]
    return st


def _bind_batched(core, T, sz):
    """the controller's buffers through core.torch (banded under the proxy), its argument block over them and the case's inputs, and a
    diagnostics buffer of THREE rows for its two instances -> (controller, outputs so far)"""
    L = _lib()
    b, t, E, N = core.contract_b, core.torch, 2, sz["N"]
    f32 = dict(dtype=t.float32, device=core.device)
    b._a, b._cost, b._groupmin = t.empty((E, H, N, 4), **f32), t.empty((E, N), **f32), t.empty((E, (N + 63) // 64), **f32)
    b.a_mean = T["a_mean"]
    b.a_cov = T["a_cov"] if sz["mode"] == "mppi" else t.empty((E, NA, NA), **f32)
    b._params = (L.EnvParamsC * E)(*[_pc(T) for _ in range(E)])
    b._traj = (T["pos_traj"], T["vel_traj"], int(T["pos_traj"].shape[1]))
    b._args = b._make_args(T["packed"], *b._traj)
    b._states_buf, b._episode = T["packed"], None
    diag = t.empty((3, L.COVO_DIAG_FLOATS), **f32)
    L.check(core.lib.covo_set_step_diag(core.h, L.ptr(diag), 3), "covo_set_step_diag")
    core.contract_keep = (diag, T)
    return b, {"a_mean": b.a_mean, "a_cov": b.a_cov, "a": b._a, "cost": b._cost, "groupmin": b._groupmin, "diag": diag}


def _run_batched_step(core, T, sz):
    b, outs = _bind_batched(core, T, sz)
    for k in range(sz.get("calls", 4)):
        b(None, np.asarray([[31 + k, 32], [33 + k, 34]], dtype=np.uint32))
        outs[f"mean{k}"] = b.a_mean.clone()
    if sz.get("hessians"):  # instance 1's Hessian of the last step, to the host
        Rh = core.torch.empty((NA * NA,), dtype=core.torch.float64, device="cpu")
        _call(core, "covo_debug_batched_hessians", Rh, C.c_int64(NA * NA), C.c_int64(NA * NA))
        outs["R1"] = Rh
    return outs


class _Episode:
    """what SamplingCore.run_episode / BatchedCoVOController.run_episode read of an episode, over the case's tensors"""
    LOGS = ()

    def __init__(self, core, T, sz, batched):
        import types
        from covo_mpc_amd.dynamics.dataclass import DeviceState
        n = sz["episode"]
        self.env = types.SimpleNamespace(generate_noisy_state=True, default_params=types.SimpleNamespace(obs_noise_scale=0.01))
        self.true, self.noisy, self.acc_traj = T["true"], T["packed"], T["acc_traj"]
        self.pos_traj, self.vel_traj = T["pos_traj"], T["vel_traj"]
        self.params_c = _pc(T)
        self.n_steps = 0
        if batched:
            self.E, self.T = 2, int(T["pos_traj"].shape[1])
            self.params_c = (_lib().EnvParamsC * 2)(*[_pc(T) for _ in range(2)])
            self.log = core.torch.empty((2, n, 4), dtype=core.torch.float32, device=core.device)
        else:
            self.log = core.torch.empty((n, 4), dtype=core.torch.float32, device=core.device)
            self.noisy_state = DeviceState(packed=self.noisy, pos_traj=self.pos_traj, vel_traj=self.vel_traj)


def _run_batched_episode(core, T, sz):
    b, outs = _bind_batched(core, T, sz)
    ep = _Episode(core, T, sz, True)
    keys = b.run_episode(ep, np.asarray([[41, 42], [43, 44]], dtype=np.uint32), sz["episode"])
    outs.update(true=T["true"], noisy=T["packed"], log=ep.log, a_mean=b.a_mean)
    core.torch.cuda.synchronize()
    outs["keys"] = core.torch.from_numpy(keys.astype(np.int64))
    return outs


def _episode_inputs(sz):
    st = _state(31, 1, acc=True)
    st["true"] = st["packed"].copy()
    st["a_mean"] = _mean(st["_p"], np.random.default_rng(1200))[0]
    st["a_cov"] = np.stack([np.eye(4, dtype=np.float32) * 0.25 for _ in range(H)])
    return st


def _run_episode(core, T, sz):
    L = _lib()
    ep = _Episode(core, T, sz, False)
    am, cov, rng = core.run_episode(L.MODE_MPPI, ep, ep.params_c, T["a_mean"], (51, 52), sz["episode"], a_cov=T["a_cov"],
                                    sample_sigma=0.5, rollout_deterministic=False)
    core.torch.cuda.synchronize()
    return {"mean": am, "cov": cov, "rng": core.torch.from_numpy(rng.astype(np.int64)), "true": T["true"], "noisy": T["packed"],
            "log": ep.log, "a": core.a, "cost": core.cost, "blockmin": core.blockmin}


def _diag_mask(sz, X):
    """include/covo_hip.h, covo_set_step_diag: "row e = instance e of a batched step" -- two instances write rows 0 and 1 of three"""
    m = np.zeros((3, 8), dtype=bool)
    m[2] = True
    return {"diag": m}


_BATCHED = dict(make=_make_batched, fresh_core=True, masks=_diag_mask, work=("groupmin",))
ROWS += [
    Row("covo_mpc_step_batched", [dict(mode="online", N=65)], _batched_inputs, _run_batched_step, inout=("a_mean",), **_BATCHED),
    Row("covo_mpc_step_batched_mode", [dict(mode="mppi", N=100)], _batched_inputs, _run_batched_step, inout=("a_mean", "a_cov"), **_BATCHED),
    Row("covo_debug_batched_hessians", [dict(mode="online", N=65, calls=1, hessians=1)], _batched_inputs, _run_batched_step,
        inout=("a_mean",), **_BATCHED),
    Row("covo_run_episode_batched", [dict(mode="online", N=65, episode=5)], _batched_inputs, _run_batched_episode,
        inout=("a_mean", "packed", "true"), **_BATCHED),
    Row("covo_run_episode_batched_mode", [dict(mode="mppi", N=100, episode=5)], _batched_inputs, _run_batched_episode,
        inout=("a_mean", "a_cov", "packed", "true"), **_BATCHED),
    Row("covo_run_episode", [dict(N=100, episode=5)], _episode_inputs, _run_episode, core=lambda sz: dict(N=sz["N"], use_graph=True),
        core_out=("a", "cost", "blockmin"), fresh_core=True, inout=("packed", "true"), work=("blockmin",)),
]

ROWS_BY_ENTRY = {}
for _r in ROWS:
    ROWS_BY_ENTRY.setdefault(_r.entry, []).append(_r)


def all_cases():
    return [c for r in ROWS for c in r.cases()]
