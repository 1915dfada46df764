"""Shared device-side machinery of the sampling controllers (MPPI / CoVO).

Owns the libcovo_hip handle and the HBM buffers of one control step and issues the kernels of
include/covo_hip.h on torch's current stream.  When a torch.distributed process group with more
than one rank is given, the sample axis N is sharded: rank g owns global sample ids
[g*N/G, (g+1)*N/G), epsilon is keyed by global id, every rank reduces its shard to ONE rank record
(online-softmax partial + the position sums of covo.py:281 when they are wanted: 2 064 bytes) and ONE
exchange per control step makes all G records known to all ranks, which then merge identically
(SURVEY.md 5.8 / 8e).  The exchange is an all-gather (RCCL over xGMI under the nccl backend; the DEFAULT)
or -- opt-in: `exchange="peer"` / "auto", COVO_EXCHANGE=peer|auto -- direct peer writes into hipIpc-mapped buffers
(csrc/exchange.hip: no collective library and no host round trip, so whole sharded episodes can be enqueued from C).
The peer path has only ever run with ranks sharing ONE GPU (the build pool has single-GPU boxes): it stays opt-in
until it has been measured over xGMI.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .. import _lib
from .._lib import (COVO_COV_FLOATS, COVO_H, COVO_NA, COVO_PARTIAL_FLOATS, COVO_POS_STATS_DOUBLES, COVO_RANK_RECORD_COV_FLOATS,
                    COVO_RANK_RECORD_FLOATS, check, ptr)
from ._options import check_kernel_path, check_sigma_nodes, check_step_options, check_step_switches, sharded_refusal, take, take_switches

# the episode logs a core fills: the episode's attribute -> (the core attribute that turns it on, the C call that binds it, whether
# that attribute's value is the log's extra allocation argument: the fan's K, the iteration log's row width; covo_set_episode_rows' kind
# or None for a log with a setter of its own; the episode attribute that has to ask for the log, or None: every episode keeps it)
_ROWS = "covo_set_episode_rows"
EPISODE_LOGS = {"diag_log": ("compute_diag", "covo_set_episode_diag_log", False, None, None),
                "trace": ("compute_plan", "covo_set_episode_trace", False, None, None),
                "fanlog": ("compute_fan", "covo_set_episode_fan", True, None, None),
                "arblog": ("arb_mask", "covo_set_episode_arbiter_log", False, None, None),
                "lamlog": ("lam_logged", _ROWS, False, _lib.COVO_EPLOG_LAM, None),
                "elitelog": ("elite", _ROWS, False, _lib.COVO_EPLOG_ELITE, None),
                "iterlog": ("iters_logged", _ROWS, True, _lib.COVO_EPLOG_ITERS, None),
                "sigmalog": ("sigma_logged", _ROWS, False, _lib.COVO_EPLOG_SIGMA, None),
                "postlog": ("compute_post_cov", _ROWS, False, _lib.COVO_EPLOG_POST_AUX, None),
                "postcovlog": ("compute_post_cov", _ROWS, False, _lib.COVO_EPLOG_POST_COV, "log_post_cov")}


def shard_range(N: int, rank: int, world: int):
    """Global sample ids owned by `rank`: [offset, offset + n_local)."""
    if N % world != 0:
        raise ValueError(f"N={N} must be divisible by the number of ranks {world}")
    n_local = N // world
    return rank * n_local, n_local


def exchange_records(record, gathered_flat, process_group=None):
    """THE one collective of a sample-sharded control step: all-gather the per-rank online-softmax
    records (RCCL over xGMI under the nccl backend; gloo in the CPU tests).  `gathered_flat` is a flat
    (world * len(record)) tensor; returns it viewed as (world, len(record))."""
    import torch.distributed as dist
    if record.is_cuda and dist.get_backend(process_group) == "gloo":
        # gloo has no device all-gather: stage the 528-byte records through the host (multi-process runs that share
        # one GPU, e.g. tests/test_gpu_parity.py::test_two_ranks_one_gpu; the product backend is nccl = RCCL)
        import torch
        g = torch.empty(gathered_flat.shape, dtype=gathered_flat.dtype)
        dist.all_gather_into_tensor(g, record.cpu(), group=process_group)
        gathered_flat.copy_(g)
    else:
        dist.all_gather_into_tensor(gathered_flat, record, group=process_group)
    return gathered_flat.view(-1, record.numel())


def _mask_count(m):
    """The clamped coordinates of clamp masks (int32, any shape [..., 32]) -> int32 [...]: the set bits among bits 0-7, on the device"""
    bits = (m.unsqueeze(-1) >> m.new_tensor(list(range(8)))) & 1
    return bits.sum(dim=(-1, -2)).to(m.dtype)


class SamplingCore:
    def __init__(self, N: int, H: int, lam: float, discount: float, device=None, process_group=None,
                 compute_info: bool = True, trust_clipped: bool = False, use_graph=None, shared_device=None, exchange=None,
                 cov_records: bool = False, propagate_nan=None, compute_diag: bool = False, diag_rows: int = 1,
                 compute_plan: bool = False, ess_min=None, compute_fan=None, update: str = "softmax", iters: int = 1, elite=None,
                 sigma_period: int = 1, compute_post_cov: bool = False, sigma_adapt: float = 0.0, refine: bool = False,
                 riccati: bool = False, riccati_feedback: bool = False, plan_hold: int = 1, riccati_box: bool = False, anneal=None, *,
                 sigma_nodes=None, node_interp: str = "linear"):
        opts, switches = take(locals()), take_switches(locals())
        import torch
        sharded = False
        if process_group is not None:  # what sample-sharded ranks cannot have is refused before the device is looked for
            import torch.distributed as dist
            sharded = dist.get_world_size(process_group) > 1
        opt = check_step_options(N, "online", sharded=sharded, **opts)
        sw = check_step_switches("a sampling core", mode_what="online", riccati_what="a sampling core", sigma_period=opt.sigma_period,
                                 sharded=sharded, **switches)
        sn = check_sigma_nodes(sigma_nodes, node_interp, what="online", sigma_period=opt.sigma_period, sigma_adapt=opt.sigma_adapt,
                               refine=sw.refine, sharded=sharded)
        if anneal is not None and sharded:
            raise NotImplementedError("anneal= on sample-sharded ranks: a rank sees only its shard's costs (covo_set_step_anneal "
                                      "refuses sample-sharded steps)")
        if H != COVO_H:
            raise NotImplementedError(f"the fused kernels are built for H={COVO_H}, got H={H}")
        if not torch.cuda.is_available():
            raise _lib.CovoError("covo_mpc_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                                 "there is no CPU fallback")
        self.torch = torch
        self.lib = _lib.load_library()
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (
            lambda i: torch.cuda.current_stream(i).cuda_stream)
        self.N, self.H, self.lam, self.discount = int(N), int(H), float(lam), float(discount)
        self.compute_info = compute_info
        self.pg = process_group
        self.world, self.rank = 1, 0
        if process_group is not None:
            import torch.distributed as dist
            self.world, self.rank = dist.get_world_size(process_group), dist.get_rank(process_group)
        self.offset, self.n_local = shard_range(self.N, self.rank, self.world)
        # the action stripes this core rolls out always come from covo_noise_* (already clipped)
        # covo_mpc_step replays a captured hipGraph or issues its launches one by one (COVO_FLAG_NO_GRAPH).  Measured on the
        # MI355X box: every graph replay costs a ~8 us bubble on the GPU, an eager launch ~3.5 us of host
        # time; with one rank per node the host keeps ahead and eager is faster on every config (covo-online +3.4 %,
        # covo-offline / MPPI +18..25 %); a sample-sharded rank has less GPU work per step plus a collective to issue and is
        # better off with the graph's 40 us of host time.  COVO_GRAPH=1 / COVO_NO_GRAPH=1 force either.
        import os
        eager = self.world == 1
        if use_graph is not None:
            eager = not use_graph
        if os.environ.get("COVO_GRAPH") == "1":
            eager = False
        if os.environ.get("COVO_NO_GRAPH") == "1":
            eager = True
        self.uses_graph = not eager
        # shared_device (or COVO_SHARED_DEVICE=1): other processes / streams compete for this GPU, so no launch may rely on
        # its workgroups being co-resident -- the Sigma chain's two persistent launches (grid barriers) are replaced by one
        # launch per phase.  Without it a starved barrier times out after 0.2 s, that step's Sigma is NaN and the NEXT call
        # on the handle fails with COVO_E_DEVICE (covo_device_status).
        if shared_device is None:
            shared_device = os.environ.get("COVO_SHARED_DEVICE") == "1"
            if not shared_device and self.world > 1:
                # ranks of this group that sit on the SAME physical device compete for its CUs: detected here (one
                # object all-gather at construction), not left to the caller.  The identity is the PCI bus id, not the device
                # index: under HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES every isolated rank sees its own GPU as index 0, and
                # comparing indices would put every real multi-GPU run on the slower one-launch-per-phase Sigma chain.
                import socket
                import torch.distributed as dist
                mine = (socket.gethostname(), self.device_bus_id())
                seen = [None] * self.world
                dist.all_gather_object(seen, mine, group=process_group)
                shared_device = seen.count(mine) > 1
        self.shared_device = bool(shared_device)
        # propagate_nan (or COVO_PROPAGATE_NAN=1): jnp.clip's NaN semantics in the action clips (COVO_FLAG_PROPAGATE_NAN) -- quadjax's
        # behaviour, where one NaN sample makes every later mean NaN; the default keeps the kernels' maxNum / minNum clip (NaN -> -1)
        if propagate_nan is None:
            propagate_nan = os.environ.get("COVO_PROPAGATE_NAN") == "1"
        self.propagate_nan = bool(propagate_nan)
        flags = ((_lib.COVO_FLAG_ACTIONS_CLIPPED if trust_clipped else 0) | (_lib.COVO_FLAG_NO_GRAPH if eager else 0) |
                 (_lib.COVO_FLAG_SHARED_DEVICE if self.shared_device else 0) |
                 (_lib.COVO_FLAG_PROPAGATE_NAN if self.propagate_nan else 0))
        cfg = _lib.ConfigC(self.n_local, self.H, 4, self.lam, self.discount, flags)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.covo_create(C.byref(cfg), C.byref(h)), "covo_create")
        self.h = h
        f32 = dict(dtype=torch.float32, device=self.device)
        n = self.n_local
        self._eps = None  # (n, 128) epsilon buffer, only materialised on request (parity tests)
        self._bufs = {}   # fixed-address buffers of the fused step
        self._args_cache = None
        self.a = torch.empty((COVO_H, n, 4), **f32)
        self.cost = torch.empty((n,), **f32)
        self.blockmin = torch.empty(((n + 63) // 64,), **f32)  # per-64-sample cost minima
        # the rank record of a sharded step: {m, s, v[128], pad[2]} + the 192 fp64 position sums, ONE message per step; on a
        # single rank the same buffer simply holds the two parts.  cov_records (MPPI with gamma_sigma != 0, mppi.py:119-125): the
        # record also carries the 320 weighted second moments between the two (COVO_RANK_RECORD_COV_FLOATS = 836 floats)
        self.cov_records = bool(cov_records)
        self.rec_floats = COVO_RANK_RECORD_COV_FLOATS if self.cov_records else COVO_RANK_RECORD_FLOATS
        n_part = COVO_PARTIAL_FLOATS + (COVO_COV_FLOATS if self.cov_records else 0)
        self.record = torch.zeros((self.rec_floats,), **f32)
        self.partial = self.record[:n_part]
        self.stats = self.record[n_part:].view(torch.float64)  # this shard's sums (528- / 1 808-byte offset: 8-aligned)
        self.gathered = torch.zeros((self.world * self.rec_floats,), **f32) if self.world > 1 else None
        self.stats_total = torch.zeros((COVO_POS_STATS_DOUBLES,), dtype=torch.float64, device=self.device) if self.world > 1 else self.stats
        # the step options' attachments (what each option does: _options.py).  Every buffer holds one row per instance of an env-batched
        # step (diag_rows; 1 for a single controller), stays None while its option is off, and is written by the step's own launches
        self._rows = int(diag_rows)
        # self.diag [rows, 8]: {ess, cost_min, cost_weighted, cost_mean, weight_sum, n_samples, 0, 0}
        self.compute_diag = opt.diag
        self.diag = self._attach_rows(_lib.COVO_DIAG_FLOATS, "covo_set_step_diag") if opt.diag else None
        # self.plan [rows, 100]: {cost_plan, 0, 0, 0, pos_plan[H][3]}
        self.compute_plan = opt.plan
        self.plan = self._attach_rows(_lib.COVO_PLAN_FLOATS, "covo_set_step_plan") if opt.plan else None
        # self.fan [rows, K, 100]: rows {cost_s, bits(n_s), 0, 0, pos_s[H][3]} of the samples self.fan_idx [rows, K] (int32) names
        self.compute_fan = fan_K = opt.fan_K
        self.fan = self.fan_idx = None
        if fan_K:
            self.fan = torch.zeros((self._rows, fan_K, _lib.COVO_FAN_FLOATS), **f32)
            stride = (torch.arange(fan_K, dtype=torch.int64) * self.n_local) // fan_K
            self.fan_idx = stride.to(torch.int32).reshape(1, fan_K).repeat(self._rows, 1).to(self.device).contiguous()
            check(self.lib.covo_set_step_fan(self.h, ptr(self.fan), ptr(self.fan_idx), fan_K, self._rows), "covo_set_step_fan")
        # self.arbiter [rows, 8]: {cost_softmax, cost_nominal, cost_best, cost_chosen, bits(choice), bits(n_best), 0, 0}
        self.update_rule = opt.update  # (self.update is the kernel-by-kernel softmax update below)
        self.arb_mask = opt.arb_mask
        self.arbiter = None
        if opt.arb_mask:
            self.arbiter = torch.zeros((self._rows, _lib.COVO_ARB_FLOATS), **f32)
            check(self.lib.covo_set_step_arbiter(self.h, ptr(self.arbiter), opt.arb_mask, self._rows), "covo_set_step_arbiter")
        # self.lam_eff [rows, 4]: {lam_eff, 1 / lam_eff, ESS(lam), evaluations}
        self.ess_min = opt.ess_min
        self.lam_eff = self._attach_rows(_lib.COVO_LAM_FLOATS, "covo_set_step_ess_floor", opt.ess_min) if opt.ess_min != 0.0 else None
        # self.elite_rows [rows, 8]: {bits(threshold cost word), bits(threshold index word), cost_min, cost_kth, K, elites at cost_kth, 0, 0}
        self.elite = opt.elite_K
        self.elite_rows = self._attach_rows(_lib.COVO_ELITE_FLOATS, "covo_set_step_elite", opt.elite_K) if opt.elite_K else None
        # self.iter_cost_min [rows, iters]: the minimum sample cost of every pass
        self.iters = opt.iters
        self.iter_cost_min = self._attach_rows(opt.iters, "covo_set_step_iters", opt.iters) if opt.iters > 1 else None
        self.sigma_period = opt.sigma_period
        if opt.sigma_period > 1:
            check(self.lib.covo_set_step_sigma_period(self.h, opt.sigma_period), "covo_set_step_sigma_period")
        # self.post_cov [rows, 128, 128]: the posterior covariance; self.post_aux [rows, 132]: {shift d[128], W, 0, 0, 0}
        self.compute_post_cov = opt.post_cov
        self.post_cov = self.post_aux = None
        if opt.post_cov:
            self.post_cov = torch.zeros((self._rows, COVO_NA, COVO_NA), **f32)
            self.post_aux = torch.zeros((self._rows, _lib.COVO_POST_AUX_FLOATS), **f32)
            with torch.cuda.device(self.device):
                check(self.lib.covo_set_step_post_cov(self.h, ptr(self.post_cov), ptr(self.post_aux), self._rows), "covo_set_step_post_cov")
        # self.sigma_adapt_rows [rows, 4]: {fallback, c, log det M, 0} of every instance's last step ({0, 1, 0, 0} after a refresh step)
        self.sigma_adapt_gamma = opt.sigma_adapt
        self.sigma_adapt_rows = None
        if opt.sigma_adapt > 0.0:
            self.sigma_adapt_rows = torch.zeros((self._rows, _lib.COVO_SIGMA_ADAPT_FLOATS), **f32)
            self.sigma_adapt_rows[:, 1] = 1.0
            check(self.lib.covo_set_step_sigma_adapt(self.h, opt.sigma_adapt, ptr(self.sigma_adapt_rows), self._rows),
                  "covo_set_step_sigma_adapt")
        # the step switches' attachments (what each switch does: _options.STEP_SWITCH_DEFAULTS), as for the options above
        # self.refine_rows [rows, 8]: {cost_base, cost_chosen, bits(choice), alpha, |g|_2, g.d, 0, bits(flags)}
        self.refine = sw.refine
        self.refine_rows = self._attach_rows(_lib.COVO_REFINE_FLOATS, "covo_set_step_refine") if sw.refine else None
        # self.riccati_rows [rows, 8]: a refine row that ends {.., mu, bits(flags | rung << 8)}
        self.riccati_on = sw.riccati  # (riccati() is the stand-alone sweep)
        self.riccati_rows = self._attach_rows(_lib.COVO_RICCATI_FLOATS, "covo_set_step_riccati") if sw.riccati else None
        # self.riccati_feedback_rows [rows, 8]: {cost_open, cost_closed, bits(index open), bits(index closed), max |K dx|, bits(clipped),
        # bits(invalid mask), 0} (attached behind riccati's rows, which it needs)
        self.riccati_feedback_on = sw.riccati_feedback
        self.riccati_feedback_rows = (self._attach_rows(_lib.COVO_FEEDBACK_FLOATS, "covo_set_step_riccati_feedback")
                                      if sw.riccati_feedback else None)
        # self.plan_hold_rows [rows, 8]: {bits(age), alpha, max |v - v0|, bits(clipped), bits(flags), |dx_pos|, bits(time), 0}
        # (attached behind riccati's rows, which it needs)
        self.plan_hold_period = sw.plan_hold  # (plan_hold() is the stateless hold step)
        self.plan_hold_rows = None
        if sw.plan_hold > 1:
            with torch.cuda.device(self.device):
                self.plan_hold_rows = self._attach_rows(_lib.COVO_HOLD_FLOATS, "covo_set_step_plan_hold", sw.plan_hold)
        # self.riccati_box_masks [rows, 32] int32: the clamp masks of the last sweep (attached behind riccati's rows, which it needs)
        self.riccati_box_on = sw.riccati_box
        self.riccati_box_masks = None
        if sw.riccati_box:
            self.riccati_box_masks = torch.zeros((self._rows, COVO_H), dtype=torch.int32, device=self.device)
            check(self.lib.covo_set_step_riccati_box(self.h, ptr(self.riccati_box_masks), self._rows), "covo_set_step_riccati_box")
        # covo-online in node space (not a step option either: _options.check_sigma_nodes).  self.sigma_nodes_rows [rows, 8]:
        # {lam_min, lam_max, eig_max, eig_min, log det Sigma_M, sweeps, flags, d}; self.sigma_node_cov [rows, d, d] float64 is filled by a
        # copy that sigma_nodes_info enqueues behind the step
        self.sigma_nodes_M = self.sigma_nodes_rows = self.sigma_node_cov = self.sigma_nodes_weights = None
        self.sigma_nodes_interp = node_interp
        if sn is not None:
            self.sigma_nodes_M, self.sigma_nodes_weights = sn.M, np.ascontiguousarray(sn.weights, dtype=np.float64)
            self.sigma_nodes_rows = torch.zeros((self._rows, _lib.COVO_SIGMA_NODES_FLOATS), **f32)
            self.sigma_node_cov = torch.zeros((self._rows, 4 * sn.M, 4 * sn.M), dtype=torch.float64, device=self.device)
            with torch.cuda.device(self.device):
                check(self.lib.covo_set_step_sigma_nodes(self.h, self.sigma_nodes_weights.ctypes.data_as(C.POINTER(C.c_double)), sn.M,
                                                         ptr(self.sigma_nodes_rows), self._rows), "covo_set_step_sigma_nodes")
        # the annealed step (not a step option: the attachment of the controllers of controllers/dial.py; _options.check_dial)
        self.anneal = self.anneal_sigma = self.anneal_rows = self.anneal_node_sigma = None
        self._list_infos()
        if anneal is not None:
            self.attach_anneal(anneal)
        self.exchange = "collective"
        if self.world > 1:
            # "collective" (default): torch.distributed's all-gather = RCCL over xGMI.  "peer": the peer-write exchange
            # (csrc/exchange.hip), raising if it cannot be set up.  "auto": peer when its construction-time self-test passes on EVERY
            # rank, else the collective.  Peer stays opt-in: it is validated on shared-GPU boxes only, never measured over xGMI.
            mode = exchange if exchange is not None else os.environ.get("COVO_EXCHANGE", "collective")
            if mode not in ("collective", "peer", "auto"):
                raise ValueError(f"exchange={mode!r} (auto | collective | peer)")
            if mode == "peer":
                self._connect_peer_exchange()
                self.exchange = "peer"
            elif mode == "auto":
                self.exchange = "peer" if self._try_peer_exchange() else "collective"

    def close(self):
        """covo_destroy now (workspaces, step graphs, side stream, exchange buffers) instead of at garbage collection.
        On sample-sharded ranks every rank closes at the same point: peers hold hipIpc mappings of the exchange buffer."""
        if getattr(self, "h", None):
            self.lib.covo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_bus_id(self) -> str:
        """PCI bus id of this core's GPU (covo_device_bus_id): the physical identity ranks compare, independent of
        HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES renumbering."""
        buf = C.create_string_buffer(32)
        check(self.lib.covo_device_bus_id(int(self._dev_index), buf, 32), "covo_device_bus_id")
        return buf.value.decode()

    def _connect_peer_exchange(self, must: bool = True) -> bool:
        """csrc/exchange.hip setup: every rank exports its exchange buffer (hipIpc), the 64-byte handles are all-gathered once
        over the process group, every rank maps all peers' buffers.  Every rank runs the SAME sequence of collectives whatever
        fails locally (a rank that raised between two of them would leave the others waiting in the next one); a failure
        anywhere makes every rank return False (must = False) or raise (must = True)."""
        import torch.distributed as dist
        hb = (C.c_char * _lib.COVO_EXCHANGE_HANDLE_BYTES)()
        err = None
        with self.torch.cuda.device(self.device):
            try:
                if os.environ.get("COVO_DEBUG_FAIL_EXCHANGE_RANK") == str(self.rank):  # tests: one rank cannot export its buffer
                    raise RuntimeError("covo_exchange_create: injected failure (COVO_DEBUG_FAIL_EXCHANGE_RANK)")
                check(self.lib.covo_exchange_create(self.h, self.world, self.rank, hb), "covo_exchange_create")
            except Exception as e:  # noqa: BLE001 - reported below, after the collective
                err = e
            handles = [None] * self.world
            dist.all_gather_object(handles, None if err else bytes(hb), group=self.pg)
            if all(x is not None for x in handles):
                try:
                    blob = (C.c_char * (self.world * _lib.COVO_EXCHANGE_HANDLE_BYTES)).from_buffer_copy(b"".join(handles))
                    check(self.lib.covo_exchange_connect(self.h, blob), "covo_exchange_connect")
                except Exception as e:  # noqa: BLE001
                    err = e
            elif err is None:
                err = RuntimeError("covo_exchange_create failed on another rank")
        # nobody pushes before everybody has mapped -- and everybody learns whether everybody has
        ok = self._all_agree(err is None)
        if not ok and must:
            raise err if err is not None else RuntimeError("covo_exchange_connect failed on another rank")
        return ok

    def _all_agree(self, ok: bool) -> bool:
        import torch.distributed as dist
        seen = [None] * self.world
        dist.all_gather_object(seen, bool(ok), group=self.pg)
        return all(seen)

    def _try_peer_exchange(self) -> bool:
        """exchange="auto": map the peers' buffers and run two exchanges (both parities) of a known record; the peer path is taken
        only if every rank mapped every buffer and read back every rank's record bit for bit.  A failure costs the wait kernel's
        bounded spin once (2 s for this probe; the product exchanges then wait COVO_EXCHANGE_TIMEOUT_S, default 60 s, like a
        collective that simply waits), leaves the handle clean (status cleared) and the collective in charge."""
        torch = self.torch
        # a rank that could not map must not leave the others spinning on its flag: all agree BEFORE anybody pushes
        if not self._connect_peer_exchange(must=False):
            return False
        ok = True
        keep = self.record.clone()
        try:
            check(self.lib.covo_exchange_set_timeout(self.h, 2.0), "covo_exchange_set_timeout")
            for rnd in range(2):
                probe = torch.arange(self.rec_floats, dtype=torch.float32, device=self.device) + 1000.0 * self.rank + 0.5 * rnd
                self.record.copy_(probe)
                self._peer_exchange()
                torch.cuda.synchronize(self.device)
                got = self.gathered.view(self.world, self.rec_floats).cpu()
                want = torch.stack([torch.arange(self.rec_floats, dtype=torch.float32) + 1000.0 * r + 0.5 * rnd
                                    for r in range(self.world)])
                ok = ok and bool(torch.equal(got, want))
            ok = ok and self.device_status() == 0
        except Exception:
            ok = False
        self.device_status(clear=True)
        self.record.copy_(keep)
        try:
            check(self.lib.covo_exchange_set_timeout(self.h, float(os.environ.get("COVO_EXCHANGE_TIMEOUT_S", "60"))),
                  "covo_exchange_set_timeout")
        except Exception:
            ok = False
        return self._all_agree(ok)

    def _peer_exchange(self):
        fn = self.lib.covo_exchange_records_cov if self.cov_records else self.lib.covo_exchange_records
        check(fn(self.h, ptr(self.record), ptr(self.gathered), self.stream()), "covo_exchange_records")

    def exchange_rank_records(self):
        """THE one exchange of a sharded control step: this rank's record -> self.gathered (world x rec_floats)."""
        if self.exchange == "peer":
            self._peer_exchange()
        else:
            exchange_records(self.record, self.gathered, self.pg)
        return self.gathered

    def merge_rank_records(self, a_mean_shifted, gamma_mean, out):
        # the stride / position-sum offset of the records THIS core exchanges: a core built with cov_records that runs a
        # gamma_sigma == 0 step still exchanges the 836-float kind ({m, s, v} in front, the sums at its end)
        check(self.lib.covo_merge_ranks_wide(self.h, ptr(self.gathered), self.world, int(self.rec_floats), ptr(a_mean_shifted),
                                             float(gamma_mean), ptr(out), ptr(self.stats_total) if self.compute_info else None,
                                             self.stream()), "covo_merge_ranks_wide")
        return out

    def merge_rank_records_cov(self, a_mean_shifted, gamma_mean, a_cov_shifted, gamma_sigma, out_mean, out_cov):
        """MPPI with gamma_sigma != 0 on sharded ranks (mppi.py:109-125): the gathered 836-float records -> new mean and the
        covariances adapted about it, identically on every rank (in place on a_cov_shifted is allowed)."""
        check(self.lib.covo_merge_ranks_cov(self.h, ptr(self.gathered), self.world, ptr(a_mean_shifted), float(gamma_mean),
                                            ptr(a_cov_shifted), float(gamma_sigma), ptr(out_mean), ptr(out_cov),
                                            ptr(self.stats_total) if self.compute_info else None, self.stream()),
              "covo_merge_ranks_cov")
        return out_mean, out_cov

    def _attach_rows(self, width, setter, *ahead):
        """zeros [rows, width], handed to the covo_set_step_* call `setter` (ahead: what it takes in front of the buffer)."""
        rows = self.torch.zeros((self._rows, width), dtype=self.torch.float32, device=self.device)
        check(getattr(self.lib, setter)(self.h, *ahead, ptr(rows), self._rows), setter)
        return rows

    def _list_infos(self):
        """The info functions of what is attached, listed once: step_info sits on the per-step host path."""
        self._infos = [info for on, info in (
            (self.diag is not None, self.diag_info), (self.plan is not None, self.plan_info), (self.fan is not None, self.fan_info),
            (self.lam_eff is not None, self.lam_info), (self.arbiter is not None, self.arbiter_info),
            (self.iter_cost_min is not None, self.iter_info), (self.elite_rows is not None, self.elite_info),
            (self.sigma_period > 1, self.sigma_info), (self.post_cov is not None, self.post_cov_info),
            (self.sigma_adapt_rows is not None, self.sigma_adapt_info), (self.refine_rows is not None, self.refine_info),
            (self.riccati_rows is not None, self.riccati_info),
            (self.riccati_feedback_rows is not None, self.riccati_feedback_info),
            (self.plan_hold_rows is not None, self.plan_hold_info),
            (self.riccati_box_masks is not None, self.riccati_box_info),
            (getattr(self, "sigma_nodes_rows", None) is not None, self.sigma_nodes_info),
            (getattr(self, "anneal_rows", None) is not None, self.anneal_info),
            (getattr(self, "cma_rows", None) is not None, self.cma_info),
            (getattr(self, "estimator", None) is not None, self.estimator_info),
            (getattr(self, "force_observer", None) is not None, self.force_observer_info)) if on]

    def step_info(self) -> dict:
        """Everything attached to the last step, merged: diag_info (compute_diag), plan_info (compute_plan), fan_info (compute_fan),
        lam_info (ess_min), arbiter_info (update), iter_info (iters), elite_info (elite), sigma_info (sigma_period), post_cov_info
        (compute_post_cov), sigma_adapt_info (sigma_adapt) and anneal_info (the annealed controllers' attachment) -- views of the core's
        buffers, no sync, no copy."""
        out = {}
        for info in self._infos:
            out.update(info())
        return out

    def attach_log(self, name, episode, rows_left: int):
        """Bind `episode`'s log `name` (EPISODE_LOGS; allocated on first use) for the segment that starts at episode.n_steps, when this
        core fills it."""
        option, setter, sized, kind, asked = EPISODE_LOGS[name]
        on = getattr(self, option)
        if not on:
            return
        ahead = () if kind is None else (kind,)
        if asked is not None and not getattr(episode, asked, False):  # another episode's log must not stay bound
            check(getattr(self.lib, setter)(self.h, *ahead, None, 0), setter)
            return
        if getattr(episode, name, None) is None:
            episode.alloc_log(name, *((on,) if sized else ()))
        check(getattr(self.lib, setter)(self.h, *ahead, ptr(episode.log_segment(name)), int(rows_left)), setter)

    def attach_episode_logs(self, episode, rows_left: int):
        """Bind every log of `episode` this core fills -- diagnostic log (compute_diag), trace (compute_plan), fan log (compute_fan),
        arbiter log (update), temperature log (ess_min), elite log (elite), iteration log (iters), Sigma log (sigma_period), the
        posterior covariance's side-row log (compute_post_cov) and, for an episode built with log_post_cov, its matrix log -- for the
        segment that starts at episode.n_steps: step k of it writes row n_steps + k of each."""
        for name in EPISODE_LOGS:
            self.attach_log(name, episode, rows_left)
        self.attach_hold_log(episode, rows_left)
        self.attach_estimator_log(episode, rows_left)
        self.attach_force_observer_log(episode, rows_left)

    def attach_hold_log(self, episode, rows_left: int):
        """Bind `episode`'s hold log (episode.holdlog, [.., T + 1, 8]; allocated on first use) under plan_hold > 1: the hold launch,
        and the latch on plan steps, write their rows themselves (covo_set_episode_hold_log) -- not one of EPISODE_LOGS, whose rows a
        copy launch or an attachment's own setter fills."""
        if self.plan_hold_rows is None:
            return
        if getattr(episode, "holdlog", None) is None:
            episode.alloc_hold_log()
        check(self.lib.covo_set_episode_hold_log(self.h, ptr(episode.log_segment("holdlog")), int(rows_left)),
              "covo_set_episode_hold_log")

    @property
    def iters_logged(self) -> int:
        """The width of the iteration log's rows: iters, or 0 when the core runs one pass per step (no rows)."""
        return self.iters if self.iters > 1 else 0

    @property
    def sigma_logged(self) -> bool:
        """A Sigma period is on: the steps have an age to log."""
        return self.sigma_period > 1

    def diag_info(self) -> dict:
        """{"ess", "cost_min", "cost_weighted", "cost_mean"} of the last step as 0-d views of self.diag (no sync, no copy); {} when
        the core was built without compute_diag."""
        if self.diag is None:
            return {}
        return {name: self.diag[0, i] for i, name in enumerate(_lib.DIAG_FIELDS[:4])}

    def plan_info(self) -> dict:
        """{"pos_plan" [H, 3], "cost_plan" 0-d} of the last step as views of self.plan (no sync, no copy); {} when the core was built
        without compute_plan."""
        if self.plan is None:
            return {}
        return {"pos_plan": self.plan[0, 4:].view(COVO_H, 3), "cost_plan": self.plan[0, 0]}

    def post_cov_info(self) -> dict:
        """{"post_cov" [128, 128], "post_shift" [128] (d: posterior mean minus the mean the step sampled around), "post_weight" 0-d (W)}
        of the last step as views of self.post_cov / self.post_aux (no sync, no copy); {} when the core was built without
        compute_post_cov."""
        if self.post_cov is None:
            return {}
        return {"post_cov": self.post_cov[0], "post_shift": self.post_aux[0, :COVO_NA], "post_weight": self.post_aux[0, COVO_NA]}

    def weighted_cov(self, a, cost, mu, lam=None, elite=None):
        """covo_weighted_cov: the weighted sample covariance of the stripes a [H, N, 4] (or [B, H, N, 4]) about mu [128] ([B, 128])
        under the weights of cost [N] ([B, N]) -- softmax at lam (default: the core's), or 1 on the elite set of `elite` samples and 0
        elsewhere; a cost that is not finite weighs 0 -> (C [128, 128], d [128], W 0-d), each with a leading B for batched input:
        C = sum w y y^T / W - d d^T with y = x - mu, d = sum w y / W, W = sum w.  No sync."""
        torch = self.torch
        f32 = dict(dtype=torch.float32, device=self.device)
        a, cost, mu = (torch.as_tensor(t, **f32).contiguous() for t in (a, cost, mu))
        batched = a.dim() == 4
        B = int(a.shape[0]) if batched else 1
        N = int(a.shape[-2])
        if tuple(a.shape[-3:]) != (COVO_H, N, 4) or cost.numel() != B * N or mu.numel() != B * COVO_NA:
            raise ValueError(f"weighted_cov: a {tuple(a.shape)}, cost {tuple(cost.shape)}, mu {tuple(mu.shape)} are not "
                             f"[B,] {COVO_H} x N x 4, [B,] N and [B,] {COVO_NA}")
        K = _lib.check_elite(elite, N)
        cov = torch.empty((B, COVO_NA, COVO_NA), **f32)
        aux = torch.empty((B, _lib.COVO_POST_AUX_FLOATS), **f32)
        with torch.cuda.device(self.device):
            check(self.lib.covo_weighted_cov(self.h, ptr(a), ptr(cost), ptr(mu), N, B, float(self.lam if lam is None else lam), K,
                                             ptr(cov), ptr(aux), self.stream()), "covo_weighted_cov")
        d, W = aux[:, :COVO_NA], aux[:, COVO_NA]
        return (cov, d, W) if batched else (cov[0], d[0], W[0])

    def fan_info(self) -> dict:
        """{"fan_pos" [K, H, 3], "fan_cost" [K], "fan_idx" [K] int32} of the last step as views of self.fan (no sync, no copy); {}
        when the core was built without compute_fan."""
        if self.fan is None:
            return {}
        K = self.compute_fan
        return {"fan_pos": self.fan[0, :, 4:].view(K, COVO_H, 3), "fan_cost": self.fan[0, :, 0],
                "fan_idx": self.fan[0, :, 1].view(self.torch.int32)}

    def rollout_fan(self, dstate, params_c, idx, f_shared=None, f_steps=None, K=None):
        """covo_rollout_fan on self.a: the trajectories of the samples `idx` (int32 device tensor [K], clamped into [0, n_local) by
        the launch; None: K -- default compute_fan or 16 -- samples at the stride) with the inputs of rollout() -> float32 [K, 100] rows
        {cost_s, bits(n_s), 0, 0, pos_s[H][3]}.  The K best samples of a step: idx = torch.topk(-core.cost, K).indices.int()
        together with the step's own f_shared / f_steps."""
        torch = self.torch
        if idx is None:
            K, ip = int(K) if K is not None else min(self.compute_fan or 16, self.n_local), None
        else:
            idx = idx.to(device=self.device, dtype=torch.int32).contiguous()
            K, ip = int(idx.numel()), ptr(idx)
        out = torch.empty((K, _lib.COVO_FAN_FLOATS), dtype=torch.float32, device=self.device)
        fs = (C.c_float * 3)(*[float(x) for x in f_shared]) if f_shared is not None else None
        check(self.lib.covo_rollout_fan(self.h, ptr(dstate.packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj), dstate.T,
                                        C.byref(params_c), fs, ptr(f_steps), ptr(self.a), self.n_local, ip, K, ptr(out),
                                        self.stream()), "covo_rollout_fan")
        return out

    def arbiter_info(self) -> dict:
        """{"arb_cost" [3], "arb_choice", "arb_best" (0-d int32), "arb_cost_chosen"} of the last step as views of self.arbiter (no sync,
        no copy); {} when the core was built with update="softmax"."""
        if self.arbiter is None:
            return {}
        row = self.arbiter[0]
        return {"arb_cost": row[0:3], "arb_cost_chosen": row[3], "arb_choice": row[4:5].view(self.torch.int32)[0],
                "arb_best": row[5:6].view(self.torch.int32)[0]}

    def arbitrate(self, dstate, params_c, a_nominal, a_mean, mask=0b111, f_shared=None, f_steps=None, cost=None, a=None):
        """covo_arbitrate (the stand-alone update arbiter) on self.a / self.cost (or `a` [H, N, 4] / `cost` [N]) with the inputs of
        rollout(): the candidates `a_mean` (softmax mean), `a_nominal` and the best sample are rolled out, the cheapest one `mask`
        enables is written into `a_mean` IN PLACE (float32 device tensor, 128 elements) -> float32 [8] row {cost_softmax,
        cost_nominal, cost_best, cost_chosen, bits(choice), bits(n_best), 0, 0}."""
        torch = self.torch
        a = self.a if a is None else a
        cost = self.cost if cost is None else cost
        N = int(cost.numel())
        for t in (a, cost, a_nominal, a_mean):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        assert a.numel() == COVO_H * N * 4 and a_nominal.numel() == COVO_NA and a_mean.numel() == COVO_NA
        out = torch.empty((_lib.COVO_ARB_FLOATS,), dtype=torch.float32, device=self.device)
        fs = (C.c_float * 3)(*[float(x) for x in f_shared]) if f_shared is not None else None
        check(self.lib.covo_arbitrate(self.h, ptr(dstate.packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj), dstate.T,
                                      C.byref(params_c), fs, ptr(f_steps), ptr(a), ptr(cost), N, ptr(a_nominal), ptr(a_mean),
                                      int(mask), ptr(out), self.stream()), "covo_arbitrate")
        return out

    def refine_info(self) -> dict:
        """{"refine_cost_base", "refine_cost", "refine_choice" (0-d int32), "refine_alpha", "refine_grad_norm", "refine_slope"} of the
        last step as views of self.refine_rows (no sync, no copy); {} when the core was built without refine."""
        if self.refine_rows is None:
            return {}
        row = self.refine_rows[0]
        return {"refine_cost_base": row[0], "refine_cost": row[1], "refine_choice": row[2:3].view(self.torch.int32)[0],
                "refine_alpha": row[3], "refine_grad_norm": row[4], "refine_slope": row[5]}

    def riccati_info(self) -> dict:
        """{"riccati_cost_base", "riccati_cost", "riccati_choice" (0-d int32), "riccati_alpha", "riccati_grad_norm", "riccati_slope",
        "riccati_reg" (mu), "riccati_rung" (0-d int32: flags | rung << 8, shifted down)} of the last step as views of self.riccati_rows
        (no sync, no copy; the rung is one device op on a view); {} when the core was built without riccati."""
        if self.riccati_rows is None:
            return {}
        row = self.riccati_rows[0]
        return {"riccati_cost_base": row[0], "riccati_cost": row[1], "riccati_choice": row[2:3].view(self.torch.int32)[0],
                "riccati_alpha": row[3], "riccati_grad_norm": row[4], "riccati_slope": row[5], "riccati_reg": row[6],
                "riccati_rung": row[7:8].view(self.torch.int32)[0] >> 8}

    def riccati_feedback_info(self) -> dict:
        """{"riccati_closed" (0-d bool: the committed candidate is a closed-loop one, choice > 16), "riccati_cost_open" (the cheapest of
        candidates 0 .. 16), "riccati_cost_closed" (the cheapest valid closed-loop candidate, +inf: none), "riccati_gain_max" (that
        candidate's max |K dx|_inf)} of the last step from self.riccati_rows / self.riccati_feedback_rows (no sync, no copy; the bool is
        one device op on a view); {} when the core was built without riccati_feedback."""
        if self.riccati_feedback_rows is None:
            return {}
        row = self.riccati_feedback_rows[0]
        return {"riccati_closed": self.riccati_rows[0, 2:3].view(self.torch.int32)[0] > _lib.COVO_REFINE_CANDIDATES - 1,
                "riccati_cost_open": row[0], "riccati_cost_closed": row[1], "riccati_gain_max": row[4]}

    def riccati_box_info(self) -> dict:
        """{"riccati_box_mask" [32] int32 (stage k's word: bits 0-3 coordinate i clamped at the lower bound, 4-7 at the upper),
        "riccati_box_count" (0-d: the clamped coordinates)} of the last sweep from self.riccati_box_masks (the mask is a view, the
        count a few device ops on it; no sync); {} when the core was built without riccati_box."""
        if self.riccati_box_masks is None:
            return {}
        m = self.riccati_box_masks[0]
        return {"riccati_box_mask": m, "riccati_box_count": _mask_count(m)}

    def _plan_ages(self):
        nxt, last = C.c_int32(0), C.c_int32(0)
        check(self.lib.covo_step_plan_age(self.h, C.byref(nxt), C.byref(last)), "covo_step_plan_age")
        return int(nxt.value), int(last.value)

    @property
    def plan_age(self) -> int:
        """The age the NEXT control step is scheduled at under plan_hold: 0 = it plans, 1 .. plan_hold - 1 = it holds."""
        return self._plan_ages()[0]

    def plan_hold_info(self) -> dict:
        """{"plan_age": the age the last step ran at, a Python int (0 = it planned); "hold_gain" (max |K dx|_inf as it entered the
        action), "hold_clipped" (0-d int32), "hold_flags" (0-d int32: 1 sweep flagged, 2 not finite, 4 time mismatch), "hold_alpha"}
        of the last step as views of self.plan_hold_rows (no sync, no copy); {} when the core was built with plan_hold=1."""
        if self.plan_hold_rows is None:
            return {}
        row = self.plan_hold_rows[0]
        i32 = self.torch.int32
        return {"plan_age": self._plan_ages()[1], "hold_gain": row[2], "hold_clipped": row[3:4].view(i32)[0],
                "hold_flags": row[4:5].view(i32)[0], "hold_alpha": row[1]}

    def attach_anneal(self, anneal):
        """The annealed step's attachment (covo_set_step_anneal; anneal: the record _options.check_dial returns, its table one row per
        pass of this core's iters): self.anneal_sigma [iters, 32] -- the schedule, a device copy of the table the handle holds -- and
        self.anneal_rows [rows, iters, 4]: instance e's row {lam_eff, 1 / lam_eff, std, bits(|F| | fallback << 31)} of every pass,
        written by the passes' solver launches under temp; without temp no solver runs and the rows stay {lam, 1 / lam, 0, 0}."""
        torch = self.torch
        sigma = np.ascontiguousarray(anneal.sigma, dtype=np.float32)
        if sigma.shape != (self.iters, COVO_H):
            raise ValueError(f"attach_anneal: the schedule is {sigma.shape}, this core runs iters={self.iters} passes of H={COVO_H}")
        self.anneal = anneal
        self.anneal_sigma = torch.from_numpy(sigma).to(self.device)
        self.anneal_rows = torch.zeros((self._rows, self.iters, _lib.COVO_LAM_FLOATS), dtype=torch.float32, device=self.device)
        self.anneal_rows[..., 0] = self.lam
        self.anneal_rows[..., 1] = float(np.float32(1.0) / np.float32(self.lam))
        with torch.cuda.device(self.device):
            check(self.lib.covo_set_step_anneal(self.h, sigma.ctypes.data_as(C.POINTER(C.c_float)), self.iters, float(anneal.temp),
                                                ptr(self.anneal_rows) if anneal.temp > 0.0 else None, self._rows),
                  "covo_set_step_anneal")
            if anneal.nodes is not None:  # nodes=M: the sampler's table next to the schedule, which was fed the marginals above
                basis = np.ascontiguousarray(anneal.basis, dtype=np.float32)
                if basis.shape != (self.iters, COVO_H, anneal.nodes):
                    raise ValueError(f"attach_anneal: the basis table is {basis.shape}, not {(self.iters, COVO_H, anneal.nodes)}")
                check(self.lib.covo_set_step_nodes(self.h, basis.ctypes.data_as(C.POINTER(C.c_float)), self.iters, anneal.nodes),
                      "covo_set_step_nodes")
                self.anneal_node_sigma = torch.from_numpy(np.asarray(anneal.node_sigma, dtype=np.float32)).to(self.device)
        self._list_infos()

    def attach_cma(self, cma):
        """The CMA controller's attachment (covo_set_step_cma; cma: the record _options.check_cma returns): self.cma_rows [rows, 8] --
        instance e's {s, log s, |p|, |z|, mu_eff, c_sigma, d_sigma, flags} of every step, neutral {1, 0, ...} after the first step of an
        episode -- and self.cma_p [rows, 128] float64, the evolution paths, which the handle keeps there between steps.  The core
        must have been built with compute_post_cov and compute_diag: the next step reads what they leave."""
        torch = self.torch
        if self.post_cov is None or self.diag is None:
            raise ValueError("attach_cma: the core needs compute_post_cov=True and compute_diag=True (the next step adapts to the "
                             "covariance, the displacement and the effective sample size this one leaves)")
        self.cma = cma
        self.cma_rows = torch.zeros((self._rows, _lib.COVO_CMA_FLOATS), dtype=torch.float32, device=self.device)
        self.cma_rows[:, 0] = 1.0
        self.cma_p = torch.zeros((self._rows, COVO_NA), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.covo_set_step_cma(self.h, cma.gamma, 1 if cma.step_size else 0, cma.damping, cma.s_min, cma.s_max,
                                             ptr(self.cma_rows), ptr(self.cma_p), self._rows), "covo_set_step_cma")
        self._list_infos()

    def cma_reset(self):
        """covo_cma_reset: the next CMA step is the first of an episode -- it samples from sample_sigma^2 I and writes the reset state."""
        check(self.lib.covo_cma_reset(self.h), "covo_cma_reset")

    def cma_info(self) -> dict:
        """{"cma_scale" (s), "cma_path_norm" (|p|), "cma_mu_eff", "cma_flags" (a float: 1 path kept, 2 clamp hit, 4 shape fell back),
        "cma_rows" [8]} of the last step as views of self.cma_rows (no sync, no copy); {} on a core without the attachment."""
        if getattr(self, "cma_rows", None) is None:
            return {}
        row = self.cma_rows[0]
        return {"cma_scale": row[0], "cma_path_norm": row[2], "cma_mu_eff": row[4], "cma_flags": row[7], "cma_rows": row}

    def cma_path(self, L_prev, d, ess, p, log_s, L_hat, Sigma_hat, *, n_samples=None, W=None, shape_rows=None, step_size=True,
                        damping=1.0, s_min=0.1, s_max=4.0, L_out=None, Sigma_out=None):
        """covo_cma_path (the stand-alone step-size kernel): L_prev, L_hat, Sigma_hat
        float32 device tensors [128, 128] or [E, 128, 128]; d float32 [E, 128] (the previous step's mean displacement), ess float32 [E],
        W float32 [E] (the weight sums; None: 1); p float64 [E, 128] and log_s float64 [E], updated IN PLACE; shape_rows: covo_sigma_adapt's
        rows [E, 4] or None; n_samples: N of mu_eff = clamp(ess, 1, N) (None: this core's).  -> (L', Sigma', rows [E, 8]).  L_out may be
        L_prev and Sigma_out may be Sigma_hat."""
        torch = self.torch
        f32 = dict(dtype=torch.float32, device=self.device)
        L_prev = L_prev.reshape(-1, COVO_NA, COVO_NA).contiguous()
        E = int(L_prev.shape[0])
        L_hat, Sigma_hat = L_hat.reshape(E, COVO_NA, COVO_NA).contiguous(), Sigma_hat.reshape(E, COVO_NA, COVO_NA).contiguous()
        aux = torch.zeros((E, _lib.COVO_POST_AUX_FLOATS), **f32)
        aux[:, :COVO_NA] = d.reshape(E, COVO_NA)
        aux[:, COVO_NA] = 1.0 if W is None else W.reshape(E)
        ess = ess.reshape(E).to(**f32).contiguous()
        assert p.dtype == torch.float64 and log_s.dtype == torch.float64 and p.is_contiguous() and log_s.is_contiguous()
        assert p.numel() == E * COVO_NA and log_s.numel() == E
        L_out = torch.empty_like(L_hat) if L_out is None else L_out
        Sigma_out = torch.empty_like(Sigma_hat) if Sigma_out is None else Sigma_out
        rows = torch.zeros((E, _lib.COVO_CMA_FLOATS), **f32)
        with torch.cuda.device(self.device):
            check(self.lib.covo_cma_path(self.h, ptr(L_prev), ptr(aux), _lib.COVO_POST_AUX_FLOATS, ptr(ess), 1, ptr(L_hat), ptr(Sigma_hat),
                                         ptr(shape_rows), E, int(self.n_local if n_samples is None else n_samples), 1 if step_size else 0,
                                         float(damping), float(s_min), float(s_max), ptr(p), ptr(log_s), ptr(L_out), ptr(Sigma_out),
                                         ptr(rows), self.stream()), "covo_cma_path")
        return L_out, Sigma_out, rows

    # ---- the state estimator (controllers.StateEstimator; csrc/state_estimator.hip)
    estimator = None  # the _options.Estimator record while one is attached

    def attach_estimator(self, est):
        """covo_set_step_estimator (est: the record _options.check_estimator returns): self.est_rows [rows, 8] -- instance e's side row
        of every launch --, self.est_xhat [rows, 16] float64 (the estimate [13], then the force of the row last seen), self.est_P
        [rows, 13, 13] float64 and self.est_meta [rows, 2] int32 {valid, time word}: the filter's state lives there between steps.
        The episode drivers then run the launch behind every env step; the host path goes through estimated()."""
        torch = self.torch
        if self.world > 1:
            raise NotImplementedError("the state estimator on sample-sharded ranks: covo_set_step_estimator refuses sample-sharded steps")
        f64 = dict(dtype=torch.float64, device=self.device)
        self.est_rows = torch.zeros((self._rows, _lib.COVO_EST_FLOATS), dtype=torch.float32, device=self.device)
        self.est_xhat = torch.zeros((self._rows, _lib.COVO_EST_STATE_DOUBLES), **f64)
        self.est_P = torch.zeros((self._rows, 13, 13), **f64)
        self.est_meta = torch.zeros((self._rows, _lib.COVO_EST_META_INTS), dtype=torch.int32, device=self.device)
        obs, proc = (C.c_double * 4)(*est.obs_std), (C.c_double * 4)(*est.proc_std)
        check(self.lib.covo_set_step_estimator(self.h, obs, proc, float(est.force_std), ptr(self.est_xhat), ptr(self.est_P),
                                               ptr(self.est_meta), ptr(self.est_rows), self._rows), "covo_set_step_estimator")
        self.estimator = est
        self._list_infos()

    def detach_estimator(self):
        """covo_set_step_estimator(NULL): the drivers and estimated() are what they were; the buffers stay readable."""
        check(self.lib.covo_set_step_estimator(self.h, None, None, 0.0, None, None, None, None, 0), "covo_set_step_estimator")
        self.estimator = None
        self._list_infos()

    def estimator_reset(self):
        """covo_estimator_reset: the next launch -- a driver's, or estimated()'s -- treats every instance as one without a valid state."""
        check(self.lib.covo_estimator_reset(self.h), "covo_estimator_reset")

    def estimator_info(self) -> dict:
        """{"est_rows" [8], "est_flags" (int32: 1 initialised, 2 re-initialised, 4 measurement not finite, 8 update failed), "est_nis"}
        of the last launch as views of self.est_rows (no sync, no copy); {} with nothing attached."""
        if self.estimator is None:
            return {}
        row = self.est_rows[0]
        return {"est_rows": row, "est_flags": row[0:1].view(self.torch.int32)[0], "est_nis": row[1]}

    def estimate(self, state_rows, u, params_c, xhat, P, meta, *, rows=None, obs_std, proc_std, force_std=0.0, reset=False, u_stride=None):
        """covo_estimate (the stand-alone launch), IN PLACE on state_rows: float32 device tensor [32] or [E, 32], contiguous; u float32
        with instance e's action at u.reshape(-1)[e * u_stride:][:4] (u_stride None: u is [E, 4]); params_c: one EnvParamsC or an
        array of E; xhat float64 [E, 16], P float64 [E, 13, 13], meta int32 [E, 2]: the filter's state, updated in place; obs_std,
        proc_std: four standard deviations each (a negative proc_std[1]: dt force_std / m).  reset: every instance counts as one
        without a valid state (-1: when covo_estimator_reset was called on the handle since its last launch).  -> rows [E, 8]."""
        torch = self.torch
        E = int(state_rows.numel()) // _lib.COVO_STATE_FLOATS
        assert state_rows.dtype == torch.float32 and state_rows.is_contiguous() and u.dtype == torch.float32 and u.is_contiguous()
        assert xhat.dtype == torch.float64 and P.dtype == torch.float64 and meta.dtype == torch.int32
        assert xhat.numel() == E * _lib.COVO_EST_STATE_DOUBLES and P.numel() == E * 169 and meta.numel() == E * _lib.COVO_EST_META_INTS
        assert xhat.is_contiguous() and P.is_contiguous() and meta.is_contiguous()
        stride = 4 if u_stride is None else int(u_stride)
        assert u.numel() >= (E - 1) * stride + 4
        if isinstance(params_c, _lib.EnvParamsC):
            params_c = (_lib.EnvParamsC * E)(*([params_c] * E))
        rows = torch.zeros((E, _lib.COVO_EST_FLOATS), dtype=torch.float32, device=self.device) if rows is None else rows
        with torch.cuda.device(self.device):
            check(self.lib.covo_estimate(self.h, ptr(state_rows), ptr(u), stride, params_c, (C.c_double * 4)(*obs_std),
                                         (C.c_double * 4)(*proc_std), float(force_std), ptr(xhat), ptr(P), ptr(meta), ptr(rows), E,
                                         int(reset), self.stream()), "covo_estimate")
        return rows

    def estimated(self, dstate, a_mean, params_c):
        """The one hook of the controllers' host path: the state the step plans from.  With nothing attached: dstate itself.  Otherwise a
        DeviceState whose packed row is a copy of dstate's with its 13 kinematic floats replaced by the estimate -- the attached filter's
        launch with u = the first four entries of a_mean, the mean that came into the call.  params_c: the step's EnvParamsC, or a
        callable that returns it (called only when attached).  A [E, 32] tensor (the batched controllers' state buffer) is estimated in
        place, with instance e's u at a_mean[e, :4]."""
        est = self.estimator
        if est is None:
            return dstate if self.force_observer is None else self._observed(dstate, a_mean, params_c)
        if callable(params_c):
            params_c = params_c()
        kw = dict(rows=self.est_rows, obs_std=est.obs_std, proc_std=est.proc_std, force_std=est.force_std, reset=-1)
        if self.torch.is_tensor(dstate):
            self.estimate(dstate, a_mean.reshape(-1), params_c, self.est_xhat, self.est_P, self.est_meta, u_stride=COVO_NA, **kw)
            return dstate
        import dataclasses
        row = dstate.packed.clone()
        self.estimate(row, a_mean.reshape(-1)[:4].contiguous(), params_c, self.est_xhat, self.est_P, self.est_meta, **kw)
        return dataclasses.replace(dstate, packed=row)

    def attach_estimator_log(self, episode, rows_left: int):
        """Bind `episode`'s estimator log (episode.estlog, [.., T + 1, 34]; allocated on first use) while an estimator is attached: its
        launch writes the rows itself (covo_set_episode_estimator_log), like the hold log's."""
        if self.estimator is None:
            return
        if getattr(episode, "estlog", None) is None:
            episode.alloc_estimator_log()
        check(self.lib.covo_set_episode_estimator_log(self.h, ptr(episode.log_segment("estlog")), int(rows_left)),
              "covo_set_episode_estimator_log")

    # ---- the force observer (controllers.ForceObserver; csrc/force_observer.hip)
    force_observer = None  # the _options.Observer record while one is attached

    def attach_force_observer(self, obs):
        """covo_set_step_force_observer (obs: the record _options.check_force_observer returns): self.obs_rows [rows, 8] -- instance e's
        side row of every launch --, self.obs_xi [rows, 16] float64 (x [13], then the force estimate [3]), self.obs_P [rows, 16, 16]
        float64 and self.obs_meta [rows, 2] int32 {valid, time word}: the filter's state lives there between steps.  The episode
        drivers then run the launch behind every env step; the host path goes through estimated().  ValueError while a StateEstimator
        is attached."""
        torch = self.torch
        if self.estimator is not None:
            raise ValueError("the force observer on a controller that already has a StateEstimator attached: two filters must not "
                             "write one row -- detach it first")
        if self.world > 1:
            raise NotImplementedError("the force observer on sample-sharded ranks: covo_set_step_force_observer refuses sample-sharded "
                                      "steps")
        f64 = dict(dtype=torch.float64, device=self.device)
        self.obs_rows = torch.zeros((self._rows, _lib.COVO_OBS_FLOATS), dtype=torch.float32, device=self.device)
        self.obs_xi = torch.zeros((self._rows, _lib.COVO_OBS_STATE_DOUBLES), **f64)
        self.obs_P = torch.zeros((self._rows, 16, 16), **f64)
        self.obs_meta = torch.zeros((self._rows, _lib.COVO_OBS_META_INTS), dtype=torch.int32, device=self.device)
        o, p = (C.c_double * 4)(*obs.obs_std), (C.c_double * 4)(*obs.proc_std)
        check(self.lib.covo_set_step_force_observer(self.h, o, p, float(obs.force_walk_std), float(obs.force_init_std), ptr(self.obs_xi),
                                                    ptr(self.obs_P), ptr(self.obs_meta), ptr(self.obs_rows), self._rows),
              "covo_set_step_force_observer")
        self.force_observer = obs
        self._list_infos()

    def detach_force_observer(self):
        """covo_set_step_force_observer(NULL): the drivers and estimated() are what they were; the buffers stay readable."""
        check(self.lib.covo_set_step_force_observer(self.h, None, None, 0.0, 0.0, None, None, None, None, 0), "covo_set_step_force_observer")
        self.force_observer = None
        self._list_infos()

    def force_observer_reset(self):
        """covo_force_observer_reset: the next launch -- a driver's, or estimated()'s -- treats every instance as one without a valid
        state."""
        check(self.lib.covo_force_observer_reset(self.h), "covo_force_observer_reset")

    def force_observer_info(self) -> dict:
        """{"obs_rows" [8], "obs_flags" (int32: 1 initialised, 2 re-initialised, 4 measurement not finite, 8 update failed), "obs_nis",
        "obs_force" [3] (the estimate, float64)} of the last launch as views of self.obs_rows / self.obs_xi (no sync, no copy); {} with
        nothing attached."""
        if self.force_observer is None:
            return {}
        row = self.obs_rows[0]
        return {"obs_rows": row, "obs_flags": row[0:1].view(self.torch.int32)[0], "obs_nis": row[1], "obs_force": self.obs_xi[0, 13:16]}

    def observe_force(self, state_rows, u, params_c, xi, P, meta, *, rows=None, obs_std, proc_std=(0.0, 0.0, 0.0, 0.0), force_walk_std,
                      force_init_std, reset=False, u_stride=None):
        """covo_observe_force (the stand-alone launch), IN PLACE on floats 0 .. 15 of state_rows: float32 device tensor [32] or [E, 32],
        contiguous; u float32 with instance e's action at u.reshape(-1)[e * u_stride:][:4] (u_stride None: u is [E, 4]); params_c: one
        EnvParamsC or an array of E; xi float64 [E, 16], P float64 [E, 16, 16], meta int32 [E, 2]: the filter's state, updated in
        place; obs_std, proc_std: four standard deviations each; force_walk_std, force_init_std in newtons.  reset: every instance
        counts as one without a valid state (-1: when covo_force_observer_reset was called on the handle since its last launch).
        -> rows [E, 8]."""
        torch = self.torch
        E = int(state_rows.numel()) // _lib.COVO_STATE_FLOATS
        assert state_rows.dtype == torch.float32 and state_rows.is_contiguous() and u.dtype == torch.float32 and u.is_contiguous()
        assert xi.dtype == torch.float64 and P.dtype == torch.float64 and meta.dtype == torch.int32
        assert xi.numel() == E * _lib.COVO_OBS_STATE_DOUBLES and P.numel() == E * 256 and meta.numel() == E * _lib.COVO_OBS_META_INTS
        assert xi.is_contiguous() and P.is_contiguous() and meta.is_contiguous()
        stride = 4 if u_stride is None else int(u_stride)
        assert u.numel() >= (E - 1) * stride + 4
        if isinstance(params_c, _lib.EnvParamsC):
            params_c = (_lib.EnvParamsC * E)(*([params_c] * E))
        rows = torch.zeros((E, _lib.COVO_OBS_FLOATS), dtype=torch.float32, device=self.device) if rows is None else rows
        with torch.cuda.device(self.device):
            check(self.lib.covo_observe_force(self.h, ptr(state_rows), ptr(u), stride, params_c, (C.c_double * 4)(*obs_std),
                                              (C.c_double * 4)(*proc_std), float(force_walk_std), float(force_init_std), ptr(xi), ptr(P),
                                              ptr(meta), ptr(rows), E, int(reset), self.stream()), "covo_observe_force")
        return rows

    def _observed(self, dstate, a_mean, params_c):
        """estimated() with a force observer attached: the same contract, on floats 0 .. 15 of the row."""
        obs = self.force_observer
        if callable(params_c):
            params_c = params_c()
        kw = dict(rows=self.obs_rows, obs_std=obs.obs_std, proc_std=obs.proc_std, force_walk_std=obs.force_walk_std,
                  force_init_std=obs.force_init_std, reset=-1)
        if self.torch.is_tensor(dstate):
            self.observe_force(dstate, a_mean.reshape(-1), params_c, self.obs_xi, self.obs_P, self.obs_meta, u_stride=COVO_NA, **kw)
            return dstate
        import dataclasses
        row = dstate.packed.clone()
        self.observe_force(row, a_mean.reshape(-1)[:4].contiguous(), params_c, self.obs_xi, self.obs_P, self.obs_meta, **kw)
        return dataclasses.replace(dstate, packed=row)

    def attach_force_observer_log(self, episode, rows_left: int):
        """Bind `episode`'s observer log (episode.obslog, [.., T + 1, 40]; allocated on first use) while a force observer is attached:
        its launch writes the rows itself (covo_set_episode_force_observer_log), like the estimator log's."""
        if self.force_observer is None:
            return
        if getattr(episode, "obslog", None) is None:
            episode.alloc_force_observer_log()
        check(self.lib.covo_set_episode_force_observer_log(self.h, ptr(episode.log_segment("obslog")), int(rows_left)),
              "covo_set_episode_force_observer_log")

    @property
    def lam_logged(self) -> bool:
        """A temperature row is written per step (the ESS floor's, or the annealed step's last pass's): the episodes keep its log."""
        return self.ess_min != 0.0 or (self.anneal is not None and self.anneal.temp > 0.0)

    def anneal_info(self) -> dict:
        """(under nodes=M also "anneal_nodes" M and "anneal_node_sigma" [k, M]; "anneal_sigma" is then sigma_e)
        {"anneal_sigma" [k, 32], "anneal_rows" [k, 4], "anneal_lam" [k], "anneal_std" [k], "anneal_fallback" [k] bool} of the last
        step's k passes, and under temp "lam_eff", the last pass's -- views of self.anneal_sigma / self.anneal_rows (no sync; the bool
        is one device op on a view); {} on a core without the attachment."""
        if self.anneal_rows is None:
            return {}
        rows = self.anneal_rows[0]
        out = {"anneal_sigma": self.anneal_sigma, "anneal_rows": rows, "anneal_lam": rows[:, 0], "anneal_std": rows[:, 2],
               "anneal_fallback": rows[:, 3].view(self.torch.int32) < 0}
        if self.anneal.temp > 0.0:
            out["lam_eff"] = rows[-1, 0]
        if self.anneal.nodes is not None:  # (anneal_sigma is then the stages' marginal sigma_e)
            out["anneal_nodes"] = self.anneal.nodes
            out["anneal_node_sigma"] = self.anneal_node_sigma
        return out

    def step_nodes(self):
        """covo_step_nodes: (n_pass, n_nodes) of the node table attached to the handle, (0, 0) for none."""
        n_pass, n_nodes = C.c_int32(-1), C.c_int32(-1)
        check(self.lib.covo_step_nodes(self.h, C.byref(n_pass), C.byref(n_nodes)), "covo_step_nodes")
        return n_pass.value, n_nodes.value

    def cost_standardise(self, cost, temp, lam0=None):
        """covo_cost_standardise (the stand-alone standardising solver): cost float32 device tensor [N] or [E, N] -> float32 [E, 4] rows
        {lam_eff, 1 / lam_eff, std, bits(|F| | fallback << 31)}: lam_eff = fp32(temp x the population standard deviation of the finite
        costs), lam0 (default: the core's lam) on fallback (include/covo_hip.h)."""
        torch = self.torch
        assert cost.is_cuda and cost.dtype == torch.float32 and cost.is_contiguous()
        c2 = cost.reshape(1, -1) if cost.dim() == 1 else cost
        E, N = int(c2.shape[0]), int(c2.shape[1])
        out = torch.empty((E, _lib.COVO_LAM_FLOATS), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.covo_cost_standardise(self.h, ptr(cost), N, E, float(self.lam if lam0 is None else lam0), float(temp),
                                                 ptr(out), self.stream()), "covo_cost_standardise")
        return out

    def attach_ilqr(self):
        """The per-iteration logs of an iLQR controller's core (covo_set_step_ilqr; the controllers of controllers/ilqr.py and
        BatchedILQRController call this once, behind a constructor that attached riccati's rows and set iters): self.ilqr_rows /
        self.ilqr_feedback_rows [rows, iters, 8] -- views of [rows, COVO_MAX_STEP_ITERS, 8] buffers: slot j holds iteration j's Riccati
        / feedback row -- and self.ilqr_summary [rows, 8] = {row_0.cost_base, row_{k-1}.cost_chosen, bits(iterations with choice != 0),
        bits(first j with choice 0; k: none), bits(iterations with choice > 16), bits(OR of the flag words), |g|_2 of the last
        iteration, 0}.  The iteration log of iters= (which only carries the count to the C side here) leaves step_info()."""
        torch = self.torch
        assert self.riccati_rows is not None, "attach_ilqr: the core was built without riccati"
        full = (self._rows, _lib.COVO_MAX_STEP_ITERS, _lib.COVO_RICCATI_FLOATS)
        self._ilqr_rows_full = torch.zeros(full, dtype=torch.float32, device=self.device)
        self._ilqr_fb_full = torch.zeros(full, dtype=torch.float32, device=self.device)
        self.ilqr_rows = self._ilqr_rows_full[:, :self.iters]
        self.ilqr_feedback_rows = self._ilqr_fb_full[:, :self.iters]
        self.ilqr_summary = torch.zeros((self._rows, _lib.COVO_ILQR_FLOATS), dtype=torch.float32, device=self.device)
        check(self.lib.covo_set_step_ilqr(self.h, ptr(self._ilqr_rows_full), ptr(self._ilqr_fb_full), ptr(self.ilqr_summary), self._rows),
              "covo_set_step_ilqr")
        self.ilqr_box_count = None
        if self.riccati_box_masks is not None:  # slot j: the clamped coordinates of iteration j's sweep
            self._ilqr_box_full = torch.zeros((self._rows, _lib.COVO_MAX_STEP_ITERS), dtype=torch.int32, device=self.device)
            self.ilqr_box_count = self._ilqr_box_full[:, :self.iters]
            check(self.lib.covo_set_step_ilqr_box(self.h, ptr(self._ilqr_box_full), self._rows), "covo_set_step_ilqr_box")
        self._infos = [f for f in self._infos if f != self.iter_info] + [self.ilqr_info]

    def ilqr_costs(self):
        """Test hook (covo_debug_ilqr_costs): from now on every iteration's line search also stores its candidates' costs -> the float32
        device tensor [rows, COVO_MAX_STEP_ITERS, 33] they land in (slot j: iteration j; 17 entries without riccati_feedback)."""
        if getattr(self, "_ilqr_costs", None) is None:
            self._ilqr_costs = self.torch.zeros((self._rows, _lib.COVO_MAX_STEP_ITERS, _lib.COVO_FEEDBACK_CANDIDATES),
                                                dtype=self.torch.float32, device=self.device)
            check(self.lib.covo_debug_ilqr_costs(self.h, ptr(self._ilqr_costs), self._rows), "covo_debug_ilqr_costs")
        return self._ilqr_costs

    def ilqr_info(self) -> dict:
        """{"ilqr_rows" [iters, 8], "ilqr_feedback_rows" [iters, 8], "ilqr_cost_first" (the cost of the shifted mean), "ilqr_cost" (of
        the committed one), "ilqr_moved" / "ilqr_fixed_at" / "ilqr_closed" (0-d int32: iterations with choice != 0, the first iteration
        with choice 0 or iters, iterations that committed a closed-loop candidate)} of the last plan step as views of the core's
        buffers (no sync, no copy); {} on a core without attach_ilqr()."""
        if getattr(self, "ilqr_summary", None) is None:
            return {}
        row, i32 = self.ilqr_summary[0], self.torch.int32
        box = {} if getattr(self, "ilqr_box_count", None) is None else {"ilqr_box_count": self.ilqr_box_count[0]}
        return {**box, "ilqr_rows": self.ilqr_rows[0], "ilqr_feedback_rows": self.ilqr_feedback_rows[0], "ilqr_cost_first": row[0],
                "ilqr_cost": row[1], "ilqr_moved": row[2:3].view(i32)[0], "ilqr_fixed_at": row[3:4].view(i32)[0],
                "ilqr_closed": row[4:5].view(i32)[0]}

    def plan_latch(self, n_envs=1):
        """What the last plan step latched for its first n_envs instances (covo_debug_plan_latch; copies): {"b" float32 [n, 128] the mean
        its sweep ran at, "t" int32 [n] the time word it planned from, "K" [n, 32, 4, 16], "kff" [n, 32, 4], "x" [n, 32, 16] float64
        the sweep's outputs} -- the inputs of the hold steps that follow, as plan_hold() takes them."""
        torch = self.torch
        n = int(n_envs)
        f64 = dict(dtype=torch.float64, device=self.device)
        out = {"b": torch.empty((n, COVO_NA), dtype=torch.float32, device=self.device),
               "t": torch.empty((n,), dtype=torch.int32, device=self.device), "K": torch.empty((n, COVO_H, 4, 16), **f64),
               "kff": torch.empty((n, COVO_H, 4), **f64), "x": torch.empty((n, COVO_H, 16), **f64)}
        check(self.lib.covo_debug_plan_latch(self.h, n, ptr(out["b"]), ptr(out["t"]), ptr(out["K"]), ptr(out["kff"]), ptr(out["x"]),
                                             self.stream()), "covo_debug_plan_latch")
        return out

    def restart_plan_hold(self):
        """The schedule back to age 0 (a controller's reset()): the next step plans."""
        if self.plan_hold_rows is not None:
            check(self.lib.covo_set_step_plan_hold(self.h, self.plan_hold_period, ptr(self.plan_hold_rows), self._rows),
                  "covo_set_step_plan_hold")

    def plan_hold(self, packed, b, K, kff, x, alpha, stage, t_plan=None, a_mean=None, a_cov=None, rows=None):
        """covo_plan_hold: the stateless hold step (csrc/plan_hold.hip) for n_inst instances.  packed: the measured states float32
        [n_inst, 32]; b float32 [n_inst, 128]: the mean the sweep ran at; K [n_inst, 32, 4, 16], kff [n_inst, 32, 4], x [n_inst, 32, 16]
        (float64): riccati()'s outputs of those names; alpha: a float, or a float32 device tensor with one entry per instance (the
        committed candidate's step size); stage j in [0, 32); t_plan: int32 device tensor [n_inst], the time word the plan was made
        at, or None (no time check); rows: riccati()'s "rows" [n_inst, 4] (float64; entry 3: the sweep's flags), or None (not flagged);
        a_mean float32 [n_inst, 128] / a_cov float32 [n_inst, 32, 4, 4] (MPPI): shifted IN PLACE, u written
        to a_mean[:, 0:4]; None: not touched -> (u float32 [n_inst, 4], rows float32 [n_inst, 8] = {bits(j), alpha, max |v - v0|,
        bits(clipped), bits(flags), |dx_pos|, bits(time), 0}).  No sync."""
        torch = self.torch
        f32 = dict(dtype=torch.float32, device=self.device)
        b = b.reshape(-1, COVO_NA).contiguous()
        n_inst = int(b.shape[0])
        assert b.is_cuda and b.dtype == torch.float32
        packed = packed.reshape(-1, _lib.COVO_STATE_FLOATS)
        assert packed.is_cuda and packed.dtype == torch.float32 and packed.is_contiguous() and int(packed.shape[0]) == n_inst
        if not 0 <= int(stage) < COVO_H:
            raise ValueError(f"plan_hold: stage={stage} outside [0, {COVO_H})")
        gains = []
        for t, shape in ((K, (COVO_H, 4, 16)), (kff, (COVO_H, 4)), (x, (COVO_H, 16))):
            gains.append(t.to(device=self.device, dtype=torch.float64).reshape((n_inst,) + shape).contiguous())
        if torch.is_tensor(alpha):
            al = alpha.to(**f32).reshape(-1).contiguous()
            assert al.numel() == n_inst
        else:
            al = torch.full((n_inst,), float(alpha), **f32)
        if t_plan is not None:
            t_plan = t_plan.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
            assert t_plan.numel() == n_inst
        for t, n in ((a_mean, COVO_NA), (a_cov, COVO_H * 16)):
            assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n_inst * n)
        if rows is not None:
            rows = rows.to(device=self.device, dtype=torch.float64).reshape(n_inst, _lib.COVO_RICCATI_SIDE).contiguous()
        side, rows = rows, torch.empty((n_inst, _lib.COVO_HOLD_FLOATS), **f32)
        u = torch.empty((n_inst, 4), **f32)
        with torch.cuda.device(self.device):
            check(self.lib.covo_plan_hold(self.h, ptr(packed), ptr(b), ptr(gains[0]), ptr(gains[1]), ptr(gains[2]), ptr(side), ptr(al), 1,
                                          int(stage), ptr(t_plan), ptr(a_mean), ptr(a_cov), ptr(u), ptr(rows), n_inst, self.stream()),
                  "covo_plan_hold")
        return u, rows

    def feedback_rollout(self, dstate, params_c, a, K, kff, x, alphas=None, f_shared=None, f_steps=None, packed=None):
        """covo_feedback_rollout: the closed-loop action sequences under the sweep's gains (csrc/feedback_rollout.hip).  a (float32
        [128] or [n_inst, 128]): the plan the sweep ran at; K [n_inst, 32, 4, 16], kff [n_inst, 32, 4], x [n_inst, 32, 16] (float64):
        riccati()'s outputs of those names; alphas: up to 64 step sizes (default: the ladder's 16, 2^(3 - j)); f_shared / f_steps: the
        rollout's shared vector / [n_inst, H, 4] table as for rollout(); packed: the [n_inst, 32] start states (default: dstate's, for
        every instance -- they need not be x[:, 0]) -> (a_out float32 [n_inst, n_alpha, 128], aux float32 [n_inst, n_alpha, 4] =
        {max |K dx|_inf, bits(clipped count), bits(first k with a v that is not finite, -1: none), 0})."""
        torch = self.torch
        a = a.reshape(-1, COVO_NA).contiguous()
        n_inst = int(a.shape[0])
        assert a.is_cuda and a.dtype == torch.float32
        al = [float(v) for v in (_lib.FEEDBACK_LADDER if alphas is None else alphas)]
        if not 1 <= len(al) <= _lib.FEEDBACK_MAX_ALPHAS:
            raise ValueError(f"feedback_rollout: {len(al)} step sizes outside [1, {_lib.FEEDBACK_MAX_ALPHAS}]")
        if params_c.disturb_kind in _lib.STATE_DISTURB_KINDS:
            raise NotImplementedError(f"feedback_rollout: disturb_kind={params_c.disturb_kind} (drag / mixed) is a 16-state plant -- its "
                                      "force is a state of the sweep and a per-sample quantity of the rollout")
        gains = []
        for t, shape in ((K, (COVO_H, 4, 16)), (kff, (COVO_H, 4)), (x, (COVO_H, 16))):
            t = t.to(device=self.device, dtype=torch.float64).reshape((n_inst,) + shape).contiguous()
            gains.append(t)
        if packed is None:
            packed = dstate.packed.reshape(1, -1).expand(n_inst, -1).contiguous()
        assert packed.numel() == n_inst * _lib.COVO_STATE_FLOATS and packed.is_contiguous()
        a_out = torch.empty((n_inst, len(al), COVO_NA), dtype=torch.float32, device=self.device)
        aux = torch.empty((n_inst, len(al), _lib.FEEDBACK_AUX_FLOATS), dtype=torch.float32, device=self.device)
        fs = (C.c_float * 3)(*[float(v) for v in f_shared]) if f_shared is not None else None
        with torch.cuda.device(self.device):
            check(self.lib.covo_feedback_rollout(self.h, ptr(packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj), dstate.T,
                                                 C.byref(params_c), fs, ptr(f_steps), ptr(a), ptr(gains[0]), ptr(gains[1]), ptr(gains[2]),
                                                 (C.c_double * len(al))(*al), len(al), n_inst, ptr(a_out), ptr(aux), self.stream()),
                  "covo_feedback_rollout")
        return a_out, aux

    def riccati(self, dstate, params_c, a, reg0=_lib.COVO_RICCATI_REG0, f_steps=None, packed=None, box=False):
        """covo_riccati: the Riccati sweep (csrc/riccati.hip) over the stage blocks of the Hessian's objective at `a` (float32 device
        tensor [128] or [batch, 128]) -> dict of float64 device tensors: "d" [batch, 128] = -(R + mu I)^-1 g on the lowest rung
        mu = reg0 4^j, j < 8, at which R + mu I is positive definite; "K" [batch, 32, 4, 16] the feedback gains (columns at and above
        the state dimension are 0), "kff" [batch, 32, 4] the feed-forward terms, "x" [batch, 32, 16] the nominal states along the plan;
        "rows" [batch, 4] = {mu, rung, smallest pivot, flags}.  f_steps: the [batch, H, 4] table of
        disturb_table(key_mode=DISTURB_KEYS_HESSIAN) for periodic / sin / drag / mixed; packed: the [batch, 32] states (default:
        dstate's, for every entry).  The workspace is the sweep's own: hessian(), cost_gradient() and the step's Hessian are untouched.
        box=True (covo_riccati_box): every stage solves the box QP on -1 <= clip(a) + du <= 1 (_options.check_riccati_box); the dict
        gains "box" [batch, 32] int32, the clamp masks of the winning rung."""
        torch = self.torch
        if not isinstance(box, bool):
            raise ValueError(f"box={box!r} (True | False)")
        a = a.reshape(-1, COVO_NA).contiguous()
        batch = int(a.shape[0])
        assert a.is_cuda and a.dtype == torch.float32
        if packed is None:
            packed = dstate.packed.reshape(1, -1).expand(batch, -1).contiguous()
        assert packed.numel() == batch * _lib.COVO_STATE_FLOATS and packed.is_contiguous()
        new = lambda *shape: torch.empty((batch,) + shape, dtype=torch.float64, device=self.device)
        out = {"d": new(COVO_NA), "K": new(COVO_H, 4, 16), "kff": new(COVO_H, 4), "x": new(COVO_H, 16), "rows": new(_lib.COVO_RICCATI_SIDE)}
        if box:
            out["box"] = torch.empty((batch, COVO_H), dtype=torch.int32, device=self.device)
            with torch.cuda.device(self.device):
                check(self.lib.covo_riccati_box(self.h, ptr(packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj), dstate.T,
                                                C.byref(params_c), ptr(a), ptr(f_steps), batch, float(reg0), ptr(out["d"]), ptr(out["K"]),
                                                ptr(out["kff"]), ptr(out["x"]), ptr(out["rows"]), ptr(out["box"]), self.stream()),
                      "covo_riccati_box")
            return out
        with torch.cuda.device(self.device):
            check(self.lib.covo_riccati(self.h, ptr(packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj), dstate.T, C.byref(params_c),
                                        ptr(a), ptr(f_steps), batch, float(reg0), ptr(out["d"]), ptr(out["K"]), ptr(out["kff"]),
                                        ptr(out["x"]), ptr(out["rows"]), self.stream()), "covo_riccati")
        return out

    def riccati_refine(self, dstate, params_c, a_mean, reg0=_lib.COVO_RICCATI_REG0, f_shared=None, f_steps=None, f_steps_hessian=None,
                       want_costs=True, feedback=False, box=False):
        """covo_riccati_refine (the stand-alone Riccati line search) on `a_mean` (float32 device tensor, 128 elements, refined IN
        PLACE) with the inputs of rollout(): the sweep's direction d at a_mean (f_steps_hessian: the Hessian's table), the candidates
        clip(a_mean) and clip(a_mean + 2^(3 - j) d), j = 1 .. 16, rolled out, the first cheapest committed -> (float32 [8] row
        {cost_base, cost_chosen, bits(choice), alpha, |g|_2, g.d, mu, bits(flags | rung << 8)}, float32 [17] candidate costs or None).
        feedback=True (covo_riccati_refine_feedback): the 16 closed-loop sequences under the sweep's gains compete as candidates
        17 .. 32 -> (row, float32 [33] costs or None, float32 [8] feedback row {cost_open, cost_closed, bits(index open), bits(index
        closed), max |K dx|_inf, bits(clipped count), bits(invalid mask), 0}).
        box=True (covo_riccati_refine_box): the same over the box sweep; the int32 [32] clamp masks follow the rows in the tuple."""
        torch = self.torch
        if not isinstance(box, bool):
            raise ValueError(f"box={box!r} (True | False)")
        assert a_mean.is_cuda and a_mean.dtype == torch.float32 and a_mean.is_contiguous() and a_mean.numel() == COVO_NA
        if not isinstance(feedback, bool):
            raise ValueError(f"feedback={feedback!r} (True | False)")
        row = torch.empty((_lib.COVO_RICCATI_FLOATS,), dtype=torch.float32, device=self.device)
        ncand = _lib.COVO_FEEDBACK_CANDIDATES if feedback else _lib.COVO_REFINE_CANDIDATES
        costs = torch.empty((ncand,), dtype=torch.float32, device=self.device) if want_costs else None
        fs = (C.c_float * 3)(*[float(x) for x in f_shared]) if f_shared is not None else None
        if feedback:
            if params_c.disturb_kind in _lib.STATE_DISTURB_KINDS:
                raise NotImplementedError(f"riccati_refine(feedback=True): disturb_kind={params_c.disturb_kind} (drag / mixed) is a "
                                          "16-state plant -- its force is a state of the sweep and a per-sample quantity of the rollout")
            fb_row = torch.empty((_lib.COVO_FEEDBACK_FLOATS,), dtype=torch.float32, device=self.device)
        if box:
            masks = torch.empty((COVO_H,), dtype=torch.int32, device=self.device)
            with torch.cuda.device(self.device):
                check(self.lib.covo_riccati_refine_box(self.h, ptr(dstate.packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj), dstate.T,
                                                       C.byref(params_c), fs, ptr(f_steps), ptr(f_steps_hessian), ptr(a_mean),
                                                       float(reg0), 1, ptr(row), ptr(costs), ptr(fb_row) if feedback else None,
                                                       int(feedback), ptr(masks), self.stream()), "covo_riccati_refine_box")
            return (row, costs, fb_row, masks) if feedback else (row, costs, masks)
        if feedback:
            with torch.cuda.device(self.device):
                check(self.lib.covo_riccati_refine_feedback(self.h, ptr(dstate.packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj),
                                                            dstate.T, C.byref(params_c), fs, ptr(f_steps), ptr(f_steps_hessian),
                                                            ptr(a_mean), float(reg0), 1, ptr(row), ptr(costs), ptr(fb_row),
                                                            self.stream()), "covo_riccati_refine_feedback")
            return row, costs, fb_row
        with torch.cuda.device(self.device):
            check(self.lib.covo_riccati_refine(self.h, ptr(dstate.packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj), dstate.T,
                                               C.byref(params_c), fs, ptr(f_steps), ptr(f_steps_hessian), ptr(a_mean), float(reg0), 1,
                                               ptr(row), ptr(costs), self.stream()), "covo_riccati_refine")
        return row, costs

    def cost_gradient(self, dstate, params_c, a, f_steps=None, packed=None):
        """covo_cost_gradient: dC/da of the Hessian's objective (covo.py:134-185) at `a` (float32 device tensor [128] or [batch, 128])
        by the first-order adjoint (cost_gradient.hip) -> float64 [batch, 128]; rows 124 .. 127 are exactly 0.  packed: the [batch, 32]
        states (default: dstate's, for every entry); f_steps: the [batch, H, 4] table of disturb_table(key_mode=DISTURB_KEYS_HESSIAN)
        for periodic / sin / drag / mixed.  It has a workspace of its own: hessian() and the step's Hessian are untouched."""
        torch = self.torch
        a = a.reshape(-1, COVO_NA).contiguous()
        batch = int(a.shape[0])
        assert a.is_cuda and a.dtype == torch.float32
        if packed is None:
            packed = dstate.packed.reshape(1, -1).expand(batch, -1).contiguous()
        assert packed.numel() == batch * _lib.COVO_STATE_FLOATS and packed.is_contiguous()
        g = torch.empty((batch, COVO_NA), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.covo_cost_gradient(self.h, ptr(packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj), dstate.T,
                                              C.byref(params_c), ptr(a), ptr(f_steps), batch, ptr(g), self.stream()), "covo_cost_gradient")
        return g

    def newton_refine(self, dstate, params_c, a_mean, Sigma, inv_c2, f_shared=None, f_steps=None, f_steps_hessian=None, g=None,
                      want_costs=True):
        """covo_newton_refine (the stand-alone Newton line search) on `a_mean` (float32 device tensor, 128 elements, refined IN
        PLACE) with the inputs of rollout(): d = -Sigma (Sigma g) / c^2 from `Sigma` (float32 [128, 128]) and `inv_c2` (1 / c^2: a
        float or a float64 device tensor), g = cost_gradient(a_mean) with f_steps_hessian unless given (float64 [128]); the candidates
        clip(a_mean) and clip(a_mean + 2^(3 - j) d), j = 1 .. 16, are rolled out and the first cheapest is committed -> (float32 [8] row
        {cost_base, cost_chosen, bits(choice), alpha, |g|_2, g.d, 0, bits(flags)}, float32 [17] candidate costs or None)."""
        torch = self.torch
        for t in (a_mean, Sigma):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        assert a_mean.numel() == COVO_NA and Sigma.numel() == COVO_NA * COVO_NA
        ic = torch.as_tensor(inv_c2, dtype=torch.float64, device=self.device).reshape(1)
        if g is not None:
            g = g.to(device=self.device, dtype=torch.float64).contiguous()
            assert g.numel() == COVO_NA
        row = torch.empty((_lib.COVO_REFINE_FLOATS,), dtype=torch.float32, device=self.device)
        costs = torch.empty((_lib.COVO_REFINE_CANDIDATES,), dtype=torch.float32, device=self.device) if want_costs else None
        fs = (C.c_float * 3)(*[float(x) for x in f_shared]) if f_shared is not None else None
        with torch.cuda.device(self.device):
            check(self.lib.covo_newton_refine(self.h, ptr(dstate.packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj), dstate.T,
                                              C.byref(params_c), fs, ptr(f_steps), ptr(f_steps_hessian), ptr(g), ptr(a_mean), ptr(Sigma),
                                              ptr(ic), 1, ptr(row), ptr(costs), self.stream()), "covo_newton_refine")
        return row, costs

    def iter_info(self) -> dict:
        """{"iter_cost_min" [iters]} of the last step -- entry j: the minimum sample cost of pass j -- as a view of self.iter_cost_min
        (no sync, no copy); {} when the core was built with iters=1."""
        if self.iter_cost_min is None:
            return {}
        return {"iter_cost_min": self.iter_cost_min[0]}

    def elite_info(self) -> dict:
        """{"elite_cost_max" (the K-th smallest cost), "elite_cost_min", "elite_count"} of the last step as 0-d views of self.elite_rows
        (no sync, no copy); {} when the core was built without elite."""
        if self.elite_rows is None:
            return {}
        return {"elite_cost_max": self.elite_rows[0, 3], "elite_cost_min": self.elite_rows[0, 2], "elite_count": self.elite_rows[0, 4]}

    def _sigma_ages(self):
        nxt, last = C.c_int32(0), C.c_int32(0)
        check(self.lib.covo_step_sigma_age(self.h, C.byref(nxt), C.byref(last)), "covo_step_sigma_age")
        return int(nxt.value), int(last.value)

    @property
    def sigma_age(self) -> int:
        """The age the NEXT covo-online step is scheduled at: 0 = it refreshes Sigma, 1 .. sigma_period - 1 = it shifts the last factor."""
        return self._sigma_ages()[0]

    def sigma_info(self) -> dict:
        """{"sigma_age": the age the last step ran at, a Python int: 0 = it refreshed Sigma}; {} when the core was built with
        sigma_period=1."""
        if self.sigma_period == 1:
            return {}
        return {"sigma_age": self._sigma_ages()[1]}

    def set_sigma_period(self, sigma_period: int):
        """Another period (1 = off) from the next step on; the age goes back to 0: the next step refreshes.  Calling it with the
        current period is how a controller's reset() restarts the schedule."""
        m = _lib.check_sigma_period(sigma_period)
        if m > 1 and self.world > 1:
            raise sharded_refusal("sigma_period", m)
        check(self.lib.covo_set_step_sigma_period(self.h, m), "covo_set_step_sigma_period")
        self.sigma_period = m
        self._list_infos()

    def sigma_factor(self, n_envs=None):
        """The factor L [128, 128] the last single covo-online step of this core sampled from (n_envs=E: [E, 128, 128], the last
        env-batched step's) -- what the next reuse step of a Sigma period shifts (covo_debug_sigma_factor; a copy)."""
        shape = (COVO_NA, COVO_NA) if n_envs is None else (int(n_envs), COVO_NA, COVO_NA)
        out = self.torch.empty(shape, dtype=self.torch.float32, device=self.device)
        check(self.lib.covo_debug_sigma_factor(self.h, 0 if n_envs is None else 1, ptr(out), out.numel(), self.stream()),
              "covo_debug_sigma_factor")
        return out

    def sigma_shift(self, L, sample_sigma=0.5):
        """covo_sigma_shift (the stand-alone shift of a reuse step): L float32 device tensor [128, 128] or [E, 128, 128], the lower
        Cholesky factor of a covariance Sigma -> (Sigma', L') of the same shape: Sigma' = c S(Sigma) -- the trailing 124 x 124 block of
        Sigma moved up, the last stage's 4 x 4 marginal repeated, no cross terms, c such that log det Sigma' = 2 n log sample_sigma --
        and its lower factor (include/covo_hip.h)."""
        torch = self.torch
        assert L.is_cuda and L.dtype == torch.float32 and L.is_contiguous() and tuple(L.shape[-2:]) == (COVO_NA, COVO_NA)
        E = 1 if L.dim() == 2 else int(L.shape[0])
        Sigma_out, L_out = torch.empty_like(L), torch.empty_like(L)
        check(self.lib.covo_sigma_shift(self.h, ptr(L), E, float(sample_sigma), ptr(Sigma_out), ptr(L_out), self.stream()),
              "covo_sigma_shift")
        return Sigma_out, L_out

    def sigma_adapt_info(self) -> dict:
        """{"sigma_adapt_fallback" (1: the blend was not positive definite and the step took the plain shift), "sigma_adapt_scale" (c)}
        of the last step as 0-d views of self.sigma_adapt_rows (no sync, no copy); 0 and 1 after a refresh step; {} when the core was
        built with sigma_adapt=0."""
        if self.sigma_adapt_rows is None:
            return {}
        return {"sigma_adapt_fallback": self.sigma_adapt_rows[0, 0], "sigma_adapt_scale": self.sigma_adapt_rows[0, 1]}

    def set_sigma_adapt(self, gamma: float):
        """Another gamma (0 = off) from the next step on, on a core built with sigma_adapt > 0 (it owns the rows and the posterior
        covariance target); the age goes back to 0 and the step graphs are captured again."""
        g = _lib.check_sigma_adapt(gamma, self.sigma_period)
        if self.sigma_adapt_rows is None:
            raise ValueError("set_sigma_adapt: the core was built with sigma_adapt=0 (no rows, no posterior covariance target)")
        rows = self.sigma_adapt_rows
        check(self.lib.covo_set_step_sigma_adapt(self.h, g, ptr(rows) if g > 0.0 else None, int(rows.shape[0]) if g > 0.0 else 0),
              "covo_set_step_sigma_adapt")
        self.sigma_adapt_gamma = g

    def sigma_adapt(self, L, C, gamma, sample_sigma=0.5, L_out=None):
        """covo_sigma_adapt (the stand-alone covariance of a reuse step that adapts): L, C float32 device tensors [128, 128] or
        [E, 128, 128] -- the lower Cholesky factor of Sigma and a posterior covariance (the lower triangles are read) -- and
        0 <= gamma < 1 -> (Sigma', L', rows): Sigma' = c ((1 - gamma) S(L L^T) + gamma S(C)) with the Sigma period's shift S and c such
        that log det Sigma' = 2 n log sample_sigma, its lower factor, and rows [E, 4] = {fallback, c, log det M, 0} ([4] for one
        matrix); an instance whose blend is not positive definite gets its gamma = 0 result and fallback = 1 (include/covo_hip.h).
        L_out: where L' goes (may be L itself)."""
        torch = self.torch
        g = _lib.check_sigma_adapt(gamma)
        for t in (L, C):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape[-2:]) == (COVO_NA, COVO_NA)
        assert L.shape == C.shape
        E = 1 if L.dim() == 2 else int(L.shape[0])
        Sigma_out = torch.empty_like(L)
        L_out = torch.empty_like(L) if L_out is None else L_out
        rows = torch.empty((E, _lib.COVO_SIGMA_ADAPT_FLOATS), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.covo_sigma_adapt(self.h, ptr(L), ptr(C), E, g, float(sample_sigma), ptr(Sigma_out), ptr(L_out), ptr(rows),
                                            self.stream()), "covo_sigma_adapt")
        return Sigma_out, L_out, (rows[0] if L.dim() == 2 else rows)

    def elite_select(self, cost, K):
        """covo_elite_select (the stand-alone selector): cost float32 device tensor [N] or [E, N] -> float32 [E, 8] rows
        {bits(threshold cost word), bits(threshold index word), cost_min, cost_kth, K, elites at cost_kth, 0, 0}; the elite set of
        instance e is {n : key(n) <= threshold}, key(n) = (u(cost[e, n]) << 32) | n (include/covo_hip.h)."""
        torch = self.torch
        assert cost.is_cuda and cost.dtype == torch.float32 and cost.is_contiguous()
        c2 = cost.reshape(1, -1) if cost.dim() == 1 else cost
        E, N = int(c2.shape[0]), int(c2.shape[1])
        out = torch.empty((E, _lib.COVO_ELITE_FLOATS), dtype=torch.float32, device=self.device)
        check(self.lib.covo_elite_select(self.h, ptr(cost), N, E, int(K), ptr(out), self.stream()), "covo_elite_select")
        return out

    def lam_info(self) -> dict:
        """{"lam_eff", "ess_lam0"} of the last step as 0-d views of self.lam_eff (no sync, no copy); {} when the core was built
        without ess_min."""
        if self.lam_eff is None:
            return {}
        return {"lam_eff": self.lam_eff[0, 0], "ess_lam0": self.lam_eff[0, 2]}

    def require_fused_for_diag(self):
        """The kernel-by-kernel path honours no attachment: NotImplementedError for the first one that is on."""
        check_kernel_path(self)

    def device_status(self, clear: bool = False) -> int:
        """Sticky COVO_DEVSTAT_* bits raised by kernels of earlier calls (0 = fine); no synchronisation."""
        return int(self.lib.covo_device_status(self.h, 1 if clear else 0))

    # -- individual kernels -------------------------------------------------------------------
    def stream(self):
        # torch's current stream of this device, as the raw hipStream_t (the Stream-object route costs 4.5 us per call,
        # a sixth of the whole host path of a small-N step)
        return C.c_void_p(self._raw_stream(self._dev_index))

    def shift_mean(self, a_mean):
        out = self.torch.empty_like(a_mean)
        check(self.lib.covo_shift_mean(self.h, ptr(a_mean), ptr(out), self.stream()), "covo_shift_mean")
        return out

    @property
    def eps(self):
        if self._eps is None:
            self._eps = self.torch.empty((self.n_local, COVO_NA), dtype=self.torch.float32, device=self.device)
        return self._eps

    def randn(self, key):
        check(self.lib.covo_randn(self.h, int(key[0]), int(key[1]), self.offset, self.n_local, COVO_NA, ptr(self.eps),
                                  self.stream()), "covo_randn")
        return self.eps

    def randn_jax(self, act_key, mppi=False):
        """epsilon of this shard from jax.random's bitstream (random_jax.py / csrc/rng_jax.hip): what quadjax's
        split(act_key, N) + normal draws would be for the same key."""
        check(self.lib.covo_randn_jax(self.h, int(act_key[0]), int(act_key[1]), self.N, self.offset, self.n_local,
                                      1 if mppi else 0, ptr(self.eps), self.stream()), "covo_randn_jax")
        return self.eps

    def noise_gemm(self, L, mu, eps=None):
        eps = self.eps if eps is None else eps
        check(self.lib.covo_noise_gemm(self.h, ptr(L), ptr(mu), ptr(eps), self.n_local, ptr(self.a), self.stream()),
              "covo_noise_gemm")
        return self.a

    def noise_gemm_philox(self, L, mu, key):
        """covo_randn + covo_noise_gemm in one kernel: epsilon is drawn in registers (same values)."""
        check(self.lib.covo_noise_gemm_philox(self.h, ptr(L), ptr(mu), int(key[0]), int(key[1]), self.offset,
                                              self.n_local, ptr(self.a), self.stream()), "covo_noise_gemm_philox")
        return self.a

    def noise_blockdiag_philox(self, Ls, mu, key):
        check(self.lib.covo_noise_blockdiag_philox(self.h, ptr(Ls), ptr(mu), int(key[0]), int(key[1]), self.offset,
                                                   self.n_local, ptr(self.a), self.stream()),
              "covo_noise_blockdiag_philox")
        return self.a

    def noise_nodes(self, basis, mu, key):
        """covo_noise_nodes_philox (the stand-alone spline-node sampler, csrc/noise_nodes.hip): basis float32 device [32, M],
        2 <= M <= 32 -> self.a = clip(mu + basis @ eps[:, :M]) with eps = randn(key), an ascending-m fmaf chain per entry."""
        assert basis.is_cuda and basis.dtype == self.torch.float32 and basis.is_contiguous() and basis.dim() == 2
        assert int(basis.shape[0]) == COVO_H
        check(self.lib.covo_noise_nodes_philox(self.h, ptr(basis), int(basis.shape[1]), ptr(mu), int(key[0]), int(key[1]), self.offset,
                                               self.n_local, ptr(self.a), self.stream()), "covo_noise_nodes_philox")
        return self.a

    def sigma_nodes_info(self) -> dict:
        """{"sigma_nodes": M, "sigma_node_cov": float64 [d, d], "sigma_node_rows": [8]} of the last step (instance 0's of a batched
        one): the rows are a view of self.sigma_nodes_rows; Sigma_M is copied out of the handle's memory by a device-to-device copy
        enqueued on the step's stream (covo_step_sigma_nodes) -- no sync; {} when the core was built with sigma_nodes=None."""
        if self.sigma_nodes_rows is None:
            return {}
        self.read_sigma_node_cov()
        return {"sigma_nodes": self.sigma_nodes_M, "sigma_node_cov": self.sigma_node_cov[0], "sigma_node_rows": self.sigma_nodes_rows[0]}

    def read_sigma_node_cov(self, G_out=None):
        """covo_step_sigma_nodes: every instance's Sigma_M of the last step -> self.sigma_node_cov [rows, d, d] (and, given a float32
        device tensor [rows, 128, d], the factors G), enqueued on the current stream."""
        M = C.c_int32(0)
        check(self.lib.covo_step_sigma_nodes(self.h, C.byref(M), ptr(self.sigma_node_cov), ptr(G_out), self._rows, self.stream()),
              "covo_step_sigma_nodes")
        return self.sigma_node_cov

    def sigma_nodes(self, R, M, node_interp="linear", sample_sigma=0.5):
        """covo_sigma_nodes (the stand-alone node-space Sigma, csrc/sigma_nodes.hip): R float64 device [128, 128] or [B, 128, 128]
        -> (Sigma_M float64 [B, d, d], G float32 [B, 128, d], Sigma_stage float32 [B, 128, 128], rows float32 [B, 8]), d = 4 M, with
        W = node_basis(M, node_interp); one matrix in, one matrix out (no leading axis)."""
        torch = self.torch
        sn = check_sigma_nodes(M, node_interp)
        if sn is None:
            raise ValueError("sigma_nodes: M=None")
        assert R.is_cuda and R.dtype == torch.float64 and R.is_contiguous() and tuple(R.shape[-2:]) == (COVO_NA, COVO_NA)
        B = 1 if R.dim() == 2 else int(R.shape[0])
        d = 4 * sn.M
        W = torch.from_numpy(np.ascontiguousarray(sn.weights, dtype=np.float64)).to(self.device)
        SigM = torch.empty((B, d, d), dtype=torch.float64, device=self.device)
        G = torch.empty((B, COVO_NA, d), dtype=torch.float32, device=self.device)
        Sig = torch.empty((B, COVO_NA, COVO_NA), dtype=torch.float32, device=self.device)
        rows = torch.empty((B, _lib.COVO_SIGMA_NODES_FLOATS), dtype=torch.float32, device=self.device)
        check(self.lib.covo_sigma_nodes(self.h, ptr(R), B, ptr(W), sn.M, float(sample_sigma), ptr(SigM), ptr(G), ptr(Sig), ptr(rows),
                                        self.stream()), "covo_sigma_nodes")
        self._sigma_nodes_keep = W  # alive until the stream has consumed it
        if R.dim() == 2:
            return SigM[0], G[0], Sig[0], rows[0]
        return SigM, G, Sig, rows

    def noise_factor(self, G, mu, key):
        """covo_noise_factor_philox (the stand-alone dense-factor sampler, csrc/sigma_nodes.hip): G float32 device [128, d],
        d = 8, 12, .., 64 -> self.a = clip(mu + G eps[:, :d]) with eps = randn(key), one ascending-c fmaf chain per entry."""
        assert G.is_cuda and G.dtype == self.torch.float32 and G.is_contiguous() and G.dim() == 2 and int(G.shape[0]) == COVO_NA
        check(self.lib.covo_noise_factor_philox(self.h, ptr(G), int(G.shape[1]), ptr(mu), int(key[0]), int(key[1]), self.offset,
                                                self.n_local, ptr(self.a), self.stream()), "covo_noise_factor_philox")
        return self.a

    def noise_blockdiag(self, Ls, mu, eps=None):
        eps = self.eps if eps is None else eps
        check(self.lib.covo_noise_blockdiag(self.h, ptr(Ls), ptr(mu), ptr(eps), self.n_local, ptr(self.a),
                                            self.stream()), "covo_noise_blockdiag")
        return self.a

    def cholesky(self, A, n, batch):
        out = self.torch.empty_like(A)
        check(self.lib.covo_cholesky(self.h, ptr(A), n, batch, ptr(out), self.stream()), "covo_cholesky")
        return out

    def disturb_table(self, params_c, packed, key=None, keys_dev=None, key_mode=_lib.DISTURB_KEYS_SHARED, deterministic=True,
                      batch=1):
        """covo_disturb_table: the per-step disturbance table(s) [batch, H, 4] of rollouts starting at `packed` ([batch, 32]
        device states) for params_c.disturb_kind periodic / sin / drag / mixed (free.py:10-58).  `key` (two uint32) for every
        entry, or `keys_dev` (uint32 [batch, 2] device tensor): the key whose threading `key_mode` describes."""
        out = self.torch.empty((batch, COVO_H, 4), dtype=self.torch.float32, device=self.device)
        k0, k1 = (int(key[0]), int(key[1])) if key is not None else (0, 0)
        check(self.lib.covo_disturb_table(self.h, C.byref(params_c), ptr(packed), int(batch), ptr(keys_dev), k0, k1,
                                          int(key_mode), 1 if deterministic else 0, ptr(out), self.stream()), "covo_disturb_table")
        return out

    def rollout(self, dstate, params_c, f_shared, want_stats, f_steps=None):
        """f_shared: host 3-vector (none / gaussian); f_steps: the device table of disturb_table (periodic / sin / drag / mixed)."""
        fs = (C.c_float * 3)(*[float(x) for x in f_shared])
        check(self.lib.covo_rollout_cost(self.h, ptr(dstate.packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj),
                                         dstate.T, C.byref(params_c), fs, ptr(f_steps), ptr(self.a), self.n_local, ptr(self.cost),
                                         ptr(self.blockmin), ptr(self.stats) if want_stats else None, self.stream()),
              "covo_rollout_cost")
        return self.cost

    def time_rollout(self, dstate, params_c, f_shared=(0.0, 0.0, 0.0), reps=100, with_records=False, f_steps=None):
        """(mean, min-batch) GPU microseconds per covo_rollout_cost launch: three batches of `reps` launches issued back to
        back from C between two events.  with_records: the record-emitting variant the fused step runs."""
        fs = (C.c_float * 3)(*[float(x) for x in f_shared])
        us = (C.c_float * 2)(0.0, 0.0)
        check(self.lib.covo_debug_time_rollout(self.h, ptr(dstate.packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj), dstate.T,
                                               C.byref(params_c), fs, ptr(f_steps), ptr(self.a), self.n_local, ptr(self.cost),
                                               ptr(self.blockmin), 1 if with_records else 0, int(reps), us, self.stream()),
              "covo_debug_time_rollout")
        return float(us[0]), float(us[1])

    def hessian(self, packed, dstate, params_c, a_mean, batch=1, method="adjoint", f_steps=None):
        """d^2 C / da^2 (covo.py:134-185); method "adjoint" (default, hessian_adj.hip) or "pairs" (hessian.hip).  f_steps: the
        [batch, H, 4] table of disturb_table(key_mode=DISTURB_KEYS_HESSIAN) for periodic / sin / drag / mixed."""
        R = self.torch.empty((batch, COVO_NA, COVO_NA), dtype=self.torch.float64, device=self.device)
        fn = self.lib.covo_hessian if method == "adjoint" else self.lib.covo_hessian_pairs
        check(fn(self.h, ptr(packed), ptr(dstate.pos_traj), ptr(dstate.vel_traj), dstate.T,
                 C.byref(params_c), ptr(a_mean), ptr(f_steps), batch, ptr(R), self.stream()), "covo_hessian")
        return R

    def sigma(self, R, sample_sigma, batch=1, method="ns"):
        """(Sigma, chol(Sigma)); method "ns" = eigh-free GEMM pipeline (default), "jacobi" = eigendecomposition."""
        f32 = dict(dtype=self.torch.float32, device=self.device)
        Sigma = self.torch.empty((batch, COVO_NA, COVO_NA), **f32)
        L = self.torch.empty((batch, COVO_NA, COVO_NA), **f32)
        fn = self.lib.covo_sigma if method == "ns" else self.lib.covo_sigma_jacobi
        check(fn(self.h, ptr(R), batch, float(sample_sigma), ptr(Sigma), ptr(L), self.stream()), "covo_sigma")
        return Sigma, L

    # -- the whole step in one C call (hipGraph-replayed from its third invocation) ---------------
    def _persistent(self, name, shape, dtype=None):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self.torch.zeros(shape, dtype=dtype or self.torch.float32, device=self.device)
            self._bufs[name] = t
        return t

    def _prepare_step(self, mode, dstate, a_mean, *, a_cov=None, L_table=None, gamma_mean=1.0, sample_sigma=0.5,
                      want_stats=False, derive_keys=False, rollout_deterministic=True, gamma_sigma=0.0, carry_only=False):
        """Fixed-address buffers + struct covo_step_args of the fused step -> (args, a_mean buffer, shifted-mean
        buffer, a_cov buffer or None)."""
        torch = self.torch
        # the state is read through a pointer that travels with the per-step scalars (step.hip): no copy, and a
        # new address does not invalidate the captured graph.  The tensor must stay alive until the step has run.
        packed = dstate.packed
        self._state_ref = packed
        am = self._persistent("a_mean", (COVO_NA,))
        # control_params.a_mean is an INPUT of the call (covo.py:201): when it is not the handle's own buffer (a returned view of
        # it) the step's first launch reads it where it lies (args.a_mean_in) -- no copy launch on the per-step path
        a_mean_in = None
        if a_mean.data_ptr() != am.data_ptr():
            if (not carry_only and a_mean.is_cuda and a_mean.device == am.device and a_mean.dtype == torch.float32 and
                    a_mean.is_contiguous() and a_mean.numel() == COVO_NA):  # (another GPU's tensor is copied: ADVICE r05)
                a_mean_in = a_mean
                cur = torch.cuda.current_stream(am.device)
                if cur.cuda_stream != 0:  # the tensor may have been allocated on another stream: keep its block until this one is through
                    a_mean.record_stream(cur)
            else:
                am.copy_(a_mean.reshape(-1), non_blocking=True)
        am_shift = self._persistent("a_mean_shift", (COVO_NA,))
        cov_out = None
        if mode in (_lib.MODE_COVO_ONLINE, _lib.MODE_CMA):
            cov_out = self._persistent("a_cov", (COVO_NA, COVO_NA))
        elif mode == _lib.MODE_MPPI:
            cov_out = self._persistent("a_cov_mppi", (COVO_H, 4, 4))
            if a_cov.data_ptr() != cov_out.data_ptr():
                cov_out.copy_(a_cov, non_blocking=True)
        # the argument block only changes when a buffer does (new episode -> new trajectory tensors): it is rebuilt
        # then, otherwise only the state pointer is refreshed (this call sits on the per-step host path)
        sig = (mode, dstate.pos_traj.data_ptr(), dstate.vel_traj.data_ptr(), L_table.data_ptr() if L_table is not None else 0,
               bool(want_stats), float(gamma_mean), float(sample_sigma), bool(derive_keys), bool(rollout_deterministic),
               float(gamma_sigma))
        cached = self._args_cache
        if cached is not None and cached[0] == sig:
            args = cached[1]
        else:
            assert packed.is_contiguous() and packed.dtype == torch.float32 and packed.numel() == _lib.COVO_STATE_FLOATS
            args = _lib.StepArgsC()
            args.mode, args.n_samples, args.T = mode, self.n_local, dstate.T
            args.pos_traj, args.vel_traj = dstate.pos_traj.data_ptr(), dstate.vel_traj.data_ptr()
            args.a_mean, args.a_mean_shift = am.data_ptr(), am_shift.data_ptr()
            if cov_out is not None:
                args.a_cov = cov_out.data_ptr()
            if mode == _lib.MODE_COVO_OFFLINE:
                args.L_table, args.n_table = L_table.data_ptr(), int(L_table.shape[0])
            args.a, args.cost, args.groupmin = self.a.data_ptr(), self.cost.data_ptr(), self.blockmin.data_ptr()
            args.pos_stats = self.stats.data_ptr() if want_stats else None
            args.partial_out = self.partial.data_ptr() if self.world > 1 else None
            args.sample_offset, args.gamma_mean, args.sample_sigma = self.offset, float(gamma_mean), float(sample_sigma)
            args.derive_keys, args.rollout_deterministic = (1 if derive_keys else 0), (1 if rollout_deterministic else 0)
            args.gamma_sigma = float(gamma_sigma)
            self._args_cache = (sig, args, (dstate.pos_traj, dstate.vel_traj, L_table))  # keep the tensors alive
        args.state = packed.data_ptr()
        args.a_mean_in = a_mean_in.data_ptr() if a_mean_in is not None else None
        self._a_mean_in_ref = a_mean_in  # alive until the step has run
        return args, am, am_shift, cov_out

    def step(self, mode, dstate, params_c, a_mean, key, *, f_shared=None, gamma_mean=1.0, **kw):
        """covo_mpc_step: returns (a_mean_new, a_cov_out) as views of persistent buffers (clone to keep).
        derive_keys: `key` is the controller's raw rng_act; the sampling key and MPPI's shared disturbance are derived
        from it on the device (step.hip) -- the host does no RNG work on the per-step path."""
        args, am, am_shift, cov_out = self._prepare_step(mode, dstate, a_mean, gamma_mean=gamma_mean, **kw)
        fs = (C.c_float * 3)(*[float(x) for x in f_shared]) if f_shared is not None else None
        check(self.lib.covo_mpc_step(self.h, C.byref(params_c), C.byref(args), int(key[0]), int(key[1]), fs, self.stream()),
              "covo_mpc_step")
        self._last_step = (params_c, args)
        if self.world > 1:
            self.exchange_rank_records()  # the ONE exchange per step (partial (+ second moments) + position sums in one record)
            gs = float(kw.get("gamma_sigma", 0.0))
            if mode == _lib.MODE_MPPI and gs != 0.0:
                self._need_cov_records()
                self.merge_rank_records_cov(am_shift, gamma_mean, cov_out, gs, am, cov_out)  # a_cov was shifted by the begin launch
            else:
                self.merge_rank_records(am_shift, gamma_mean, am)
        return am, cov_out

    def run_episode(self, mode, episode, params_c, a_mean, rng, n_steps, **kw):
        """covo_run_episode: n_steps x (fused control step on episode.noisy -> env step on the device) enqueued by ONE
        C call, keys threaded like eval_env's run_one_step (quadrotor.py:520-538).  -> (a_mean buffer, a_cov buffer,
        rng after the segment).  Asynchronous; episode.read_log() synchronises."""
        if self.world > 1 and self.exchange != "peer":
            raise NotImplementedError("run_episode on sample-sharded ranks needs the peer-write exchange (exchange='peer' / "
                                      "COVO_EXCHANGE=peer): a torch.distributed collective cannot be enqueued from C")
        if self.world > 1 and mode == _lib.MODE_MPPI and float(kw.get("gamma_sigma", 0.0)) != 0.0:
            self._need_cov_records()
        args, am, _, cov_out = self._prepare_step(mode, episode.noisy_state, a_mean, derive_keys=True, carry_only=True, **kw)
        key = (C.c_uint32 * 2)(int(rng[0]), int(rng[1]))
        env = episode.env
        # step k of the segment also writes row n_steps + k of the episode's [T + 1, 8] diagnostic log, [T + 1, 168] trace (true
        # state, noisy state, u, plan), [T + 1, K, 100] fan log, [T + 1, 8] arbiter log and the logs of the attachments' rows
        self.attach_episode_logs(episode, int(episode.log.shape[0]) - int(episode.n_steps))
        # the env step's auto-reset (base.py:22-40) is a property of the EPISODE, the model constants come from the controller
        params_c = type(params_c).from_buffer_copy(params_c)
        for f in ("reset_traj", "reset_dt", "reset_disturb_scale"):
            setattr(params_c, f, getattr(episode.params_c, f))
        check(self.lib.covo_run_episode(self.h, C.byref(params_c), C.byref(args), ptr(episode.true), ptr(episode.acc_traj),
                                        1 if env.generate_noisy_state else 0, float(env.default_params.obs_noise_scale),
                                        ptr(episode.log[episode.n_steps:]), key, int(n_steps), self.stream()),
              "covo_run_episode")
        episode.n_steps += int(n_steps)
        self._last_step = (params_c, args)
        import numpy as np
        return am, cov_out, np.array([key[0], key[1]], dtype=np.uint32)

    def time_phases(self, step_mask=63, hess_mask=15, sigma_stages=4, reps=20):
        """GPU microseconds of the selected launches of the LAST step() call, replayed `reps` times from one graph."""
        params_c, args = self._last_step
        us = C.c_float(0.0)
        self.torch.cuda.synchronize()
        check(self.lib.covo_debug_time_step(self.h, C.byref(params_c), C.byref(args), step_mask, hess_mask, sigma_stages,
                                            reps, C.byref(us), self.stream()), "covo_debug_time_step")
        return float(us.value)

    def update(self, a_mean_shifted, gamma_mean):
        """softmax weights + weighted mean (+ the one collective when sharded) -> new mean (H,4)."""
        out = self.torch.empty_like(a_mean_shifted)
        if self.world == 1:
            check(self.lib.covo_softmax_update(self.h, ptr(self.cost), ptr(self.a), self.n_local, ptr(self.blockmin),
                                               ptr(a_mean_shifted), float(gamma_mean), ptr(out), self.stream()),
                  "covo_softmax_update")
            return out
        check(self.lib.covo_softmax_reduce(self.h, ptr(self.cost), ptr(self.a), self.n_local, ptr(self.blockmin),
                                           ptr(self.partial), self.stream()), "covo_softmax_reduce")
        self.exchange_rank_records()  # the ONE exchange per step
        return self.merge_rank_records(a_mean_shifted, gamma_mean, out)

    def _need_cov_records(self):
        if not self.cov_records:
            raise NotImplementedError("MPPI covariance adaptation (gamma_sigma != 0) on sample-sharded ranks needs the 836-float rank "
                                      "records: build the controller with control_params.gamma_sigma != 0 "
                                      "(SamplingCore(cov_records=True))")

    def update_cov(self, a_mean_shifted, gamma_mean, a_cov_shifted, gamma_sigma):
        """MPPI's update with covariance adaptation (mppi.py:109-125) -> (new mean (128,), new a_cov (H,4,4)).  Sharded ranks:
        this shard's record with its second moments -> the ONE exchange -> the same merge on every rank."""
        mean = self.torch.empty_like(a_mean_shifted)
        cov = self.torch.empty_like(a_cov_shifted)
        if self.world > 1:
            self._need_cov_records()
            check(self.lib.covo_softmax_reduce_cov(self.h, ptr(self.cost), ptr(self.a), self.n_local, ptr(self.blockmin),
                                                   ptr(a_mean_shifted), ptr(self.partial), self.stream()), "covo_softmax_reduce_cov")
            self.exchange_rank_records()
            return self.merge_rank_records_cov(a_mean_shifted, gamma_mean, a_cov_shifted, gamma_sigma, mean, cov)
        check(self.lib.covo_softmax_update_cov(self.h, ptr(self.cost), ptr(self.a), self.n_local, ptr(self.blockmin),
                                               ptr(a_mean_shifted), float(gamma_mean), ptr(a_cov_shifted), float(gamma_sigma),
                                               ptr(mean), ptr(cov), self.stream()), "covo_softmax_update_cov")
        return mean, cov

    def info(self, dstate):
        """{"pos_mean","pos_std"} (H,3) from the per-step sums (controllers/covo.py:281): covo_pos_info, one launch."""
        torch = self.torch
        stats = self.stats_total  # sharded: the ranks' sums arrived in the rank records and were added by covo_merge_ranks
        out = torch.empty((2, COVO_H, 3), dtype=torch.float32, device=self.device)
        check(self.lib.covo_pos_info(self.h, ptr(stats), ptr(dstate.packed), int(self.N), ptr(out[0]), ptr(out[1]), self.stream()),
              "covo_pos_info")
        return {"pos_mean": out[0], "pos_std": out[1]}
