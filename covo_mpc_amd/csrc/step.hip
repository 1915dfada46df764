// step.hip -- one C entry per MPC control step, replayed as a hipGraph.
//
// covo_mpc_step() enqueues everything quadjax's controller __call__ does between "shift the mean" and
// "new mean" (controllers/covo.py:201-275, mppi.py:43-125) for this rank's shard of samples on ONE
// stream, with no host work in between.  A control step is ~70 tiny launches for covo-online (the
// eigh-free Sigma pipeline alone is ~60); issued one by one from the host they leave ~150 us of gaps.
// The second call with the same buffers captures the sequence into a hipGraph, later calls replay it.
// Quantities that change every step (Philox key, MPPI's shared disturbance draw) live in a 32-byte
// device block refreshed by one async copy before each replay, so the captured kernel arguments stay valid.
#include <cstdlib>
#include <cstring>
#include <vector>
#include "covo_common.hpp"
#include "eps_tiles.hpp"
#include "sym_stats.hpp"
#include "rng_device.hpp"
#include "step_begin.hpp"
#include "step_small.hpp"

// the ONE eager launch of every step, ahead of the replayed graph.  What changes per step travels in its kernel
// arguments (48 bytes; an async H2D copy of the same block runs as a ~5 us copy kernel on this stack): the controller's
// raw rng_act, the caller's shared disturbance, the address of the state.  It shifts the mean (covo.py:201-203), brings
// the state into the fixed-address buffer the captured launches read, and fills the device block the captured
// launches take their per-step scalars from -- with derive_keys, what the host would have computed from rng_act:
//   rng, act_key = split(rng_act); rng, step_key = split(rng)                (covo.py:212,225 / mppi.py:53,69)
//   MPPI: f_shared = scale * normal(split(split(split(step_key)[1])[0])[0], (3,))   (quadrotor.py:262, free.py:136,144)
__global__ void step_begin_kernel(const float *__restrict__ a_mean, float *__restrict__ a_mean_shift,
                                  uint32_t *__restrict__ dyn, float *__restrict__ state_buf, int derive_keys,
                                  float shared_noise_scale, const DynBlock blk, float *__restrict__ mppi_cov,
                                  float *__restrict__ mppi_Ls, unsigned *__restrict__ seq, const int pass)
{
    if (threadIdx.x == 0 && seq != nullptr) seq[0] = seq[0] + 1u;  // the step's sequence number (the streamed finalize launch's flags)
    // MPPI (mppi_cov != null): the covariance shift + the 4x4 block factors ride in this launch (one launch less on a path
    // that is host bound at small N)
    if (mppi_cov != nullptr) mppi_prep(mppi_cov, mppi_Ls, pass == 0);
    const int i = threadIdx.x;  // 128 + 32 + 4 threads
    if (pass > 0) {
        // pass j >= 1 of an iterated step (covo_set_step_iters), enqueued inside the step's graph: the starting mean is what the
        // previous pass's merge (and arbiter) left in a_mean, unshifted; the state stays; the raw key is the previous pass's
        // (dyn[10..11]) advanced -- the four deriving threads are lanes of one wave: all have loaded it before thread 0 stores
        if (i < COVO_NA) {
            a_mean_shift[i] = a_mean[i];
        } else if (i >= COVO_NA + COVO_STATE_FLOATS) {
            const uint32_t p0 = dyn[10], p1 = dyn[11];
            uint32_t raw[2];
            step_begin_derive_next(i - (COVO_NA + COVO_STATE_FLOATS), p0, p1, shared_noise_scale, dyn, raw);
        }
        return;
    }
    if (i < COVO_NA) {
        a_mean_shift[i] = (i < COVO_NA - COVO_DU) ? a_mean[i + COVO_DU] : a_mean[i];
    } else if (i < COVO_NA + COVO_STATE_FLOATS) {
        const float *src;
        __builtin_memcpy(&src, &blk.w[8], sizeof(src));
        state_buf[i - COVO_NA] = src[i - COVO_NA];
    } else {
        step_begin_derive(i - (COVO_NA + COVO_STATE_FLOATS), blk, derive_keys, shared_noise_scale, dyn);
    }
}

// covo_debug_time_step's copies of a step have no begin launch between them: the streamed finalize launch's flags would still
// carry the previous copy's sequence number (its workers would not wait for anything): one bump per copy
__global__ void stream_seq_bump_kernel(unsigned *seq) { seq[0] = seq[0] + 1u; }

// ---- the capture-once / replay cache every step path embeds (StepState, BatchState, BatchSmall).  The owner compares and records
// its key itself (the three keys differ) and tells graph_cache_run whether it is unchanged:
//   unchanged, graph present                    hipGraphLaunch on the caller's stream, nothing else
//   unchanged, no graph, COVO_FLAG_NO_GRAPH clear   capture the step on h->side_stream, instantiate, launch on the caller's stream
//   otherwise                                   a changed key drops the graph before anything is enqueued; eager on the caller's stream
// so the first call with new buffers runs eagerly (all one-time attribute calls / allocations happen there), the second captures,
// later ones replay.
struct GraphCache {
    bool have_key, have_graph;
    hipGraph_t graph;
    hipGraphExec_t exec;
    void drop()
    {
        if (!have_graph) return;
        (void)hipGraphExecDestroy(exec);
        (void)hipGraphDestroy(graph);
        have_graph = false;
    }
    void forget()  // the next call runs eagerly, the one after captures again
    {
        drop();
        have_key = false;
    }
};

// enqueue(stream) enqueues the step.  Capture is on the library's own stream (the caller's may be the legacy default stream, which
// cannot capture); nothing executes during capture, the graph is then launched on the caller's stream.  A failed capture leaves
// the cache without a graph.
template <class Enqueue>
static int graph_cache_run(covo_ctx *h, GraphCache &c, hipStream_t s, bool same, const char *name, Enqueue enqueue)
{
    if (!same) c.drop();
    if (c.have_graph) {
        COVO_CHECK_HIP(hipGraphLaunch(c.exec, s));
        return 0;
    }
    if (!same || (h->cfg.flags & COVO_FLAG_NO_GRAPH) != 0) return enqueue(s);
    hipStream_t cs = h->side_stream;
    COVO_CHECK_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue(cs);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(cs, &g);
    if (rc == 0 && e != hipSuccess) covo_set_error("%s: stream capture failed: %s", name, hipGetErrorString(e));
    if (rc == 0 && e == hipSuccess && (e = hipGraphInstantiate(&c.exec, g, nullptr, nullptr, 0)) != hipSuccess)
        covo_set_error("%s: hipGraphInstantiate failed: %s", name, hipGetErrorString(e));
    if (rc != 0 || e != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        return rc ? rc : (int)e;
    }
    c.graph = g;
    c.have_graph = true;
    COVO_CHECK_HIP(hipGraphLaunch(c.exec, s));
    return 0;
}

// hipFree + null for every pointer given
template <class... T>
static void free_and_null(T *&...p)
{
    ((void)hipFree(p), ...);
    ((p = nullptr), ...);
}

struct StepKey {
    covo_step_args args;
    covo_env_params params;
    hipStream_t stream;
};

struct StepState {
    // device
    uint32_t *dyn;        // {key0, key1, f_shared[3] as float bits, pad[3], state pointer (8 bytes)}
    float *state_buf;     // [COVO_STATE_FLOATS] this step's state at a fixed address
    float *a_mean_shift;  // [128]
    double *R;            // [128][128]
    float *Sigma, *L;     // [128][128]
    float *Ls;            // [H][4][4] MPPI's block factors
    float4 *eps_tiled;    // covo-online: this step's epsilon in tile order, drawn under the Sigma chain (eps_tiles.hpp); or null
    float *f_tab_rollout, *f_tab_hess;  // [H][4] per-step disturbance tables of the sampling rollouts / the Hessian (disturb.hip)
    unsigned *ticket;     // arrival counter of the fused small step (step_small.hip); 0 between launches
    unsigned *sync;       // [16] the streamed finalize launch's sequence number and panel flags (StreamGemmArgs::sync)
    // [0] the step, [1] the reuse step of a Sigma period (covo_set_step_sigma_period: another launch set, its own graph), each with
    // its key: normalised arguments + parameters + stream; recorded by eager calls only
    GraphCache cache[2];
    StepKey key[2];
    void forget_graphs() { cache[0].forget(), cache[1].forget(); }
};
constexpr int DYN_BYTES = 48;
// up to this many samples per GPU the step's epsilon is drawn by passenger workgroups of the Sigma chain's last launch
// (~6 us of work per 65 536 samples inside a ~30 us single-workgroup kernel); beyond, the GEMM draws it itself
constexpr int EPS_TILED_MAX_N = 262144;

static int step_state_init(covo_ctx *h)
{
    StepState *st = new StepState();
    std::memset(st, 0, sizeof(*st));
    COVO_CHECK_HIP(hipMalloc(&st->dyn, DYN_BYTES));
    COVO_CHECK_HIP(hipMalloc(&st->state_buf, COVO_STATE_FLOATS * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&st->a_mean_shift, COVO_NA * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&st->R, (size_t)COVO_NA * COVO_NA * sizeof(double)));
    COVO_CHECK_HIP(hipMalloc(&st->Sigma, (size_t)COVO_NA * COVO_NA * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&st->L, (size_t)COVO_NA * COVO_NA * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&st->Ls, COVO_H * 16 * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&st->f_tab_rollout, COVO_H * 4 * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&st->f_tab_hess, COVO_H * 4 * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&st->ticket, sizeof(unsigned)));
    COVO_CHECK_HIP(hipMemset(st->ticket, 0, sizeof(unsigned)));
    COVO_CHECK_HIP(hipMalloc(&st->sync, 16 * sizeof(unsigned)));
    COVO_CHECK_HIP(hipMemset(st->sync, 0, 16 * sizeof(unsigned)));
    if (h->cfg.n_local <= EPS_TILED_MAX_N)
        COVO_CHECK_HIP(hipMalloc(&st->eps_tiled, (size_t)((h->cfg.n_local + 31) / 32) * 16 * 64 * sizeof(float4)));
    h->step = st;
    return 0;
}

void step_state_destroy(covo_ctx *h)
{
    StepState *st = reinterpret_cast<StepState *>(h->step);
    if (!st) return;
    st->forget_graphs();
    free_and_null(st->dyn, st->state_buf, st->a_mean_shift, st->R, st->Sigma, st->L, st->Ls, st->eps_tiled, st->f_tab_rollout,
                  st->f_tab_hess, st->ticket, st->sync);
    delete st;
    h->step = nullptr;
}

// The experiment switches a new handle starts with (CovoOpts, covo_common.hpp), from the environment:
//   COVO_FUSE_SMALL=0     covo-offline and MPPI steps of <= 256 sample groups run their staged launches (begin | noise | rollout +
//                         records | merge) instead of the one fused launch of step_small.hip
//   COVO_STREAM_GEMM=0    covo-online's noise GEMM as a launch of its own behind the Sigma chain's finalize launch (rounds 1-4)
//                         instead of streamed under the factorisation inside it (sigma_ns.hip: ns_finalize_stream_kernel)
//   COVO_FOLD_BEGIN=0     eager covo-online steps keep the begin launch (default: its work rides in the Hessian's first launch)
//   COVO_NS_MERGED=0      the Sigma chain's two persistent launches (squarings | iterations) as two launches (rounds 4-5) instead of one
//   COVO_NS_DEFLATE=0     the undeflated Newton-Schulz iteration
// covo_debug_set_*(handle, ...) change them per handle afterwards (A/B measurements, parity tests).
CovoOpts covo_default_opts()
{
    auto env_int = [](const char *name, int dflt) {
        const char *v = std::getenv(name);
        return v ? std::atoi(v) : dflt;
    };
    CovoOpts o;
    o.fuse_small = env_int("COVO_FUSE_SMALL", 1);
    o.stream_gemm = env_int("COVO_STREAM_GEMM", 1);
    o.fold_begin = env_int("COVO_FOLD_BEGIN", 1);
    o.ns_deflate = env_int("COVO_NS_DEFLATE", 1) ? 1 : 0;
    o.ns_force_agent = 0;
    o.ns_merged = env_int("COVO_NS_MERGED", 1) ? 1 : 0;
    o.epoch = 0;
    return o;
}

// the launch sequence of one step (everything reads per-step scalars from st->dyn)
// begin != null (eager covo-online steps): no begin launch ran -- the Hessian's first launch does its work (HessBegin) and every
// launch reads the caller's state where it lies (state_direct) instead of the fixed-address copy.  dbg.step bit 1 is unused here (the
// begin launch is not part of the graph).
static int enqueue_step(covo_ctx *h, StepState *st, const covo_env_params &p, const covo_step_args &a, hipStream_t s,
                        const DebugMasks &dbg = DebugMasks(),
                        const HessBegin *begin = nullptr, const float *state_direct = nullptr, const int pass = 0, const bool reuse = false)
{
    const int M = dbg.step;
    float *iter_out = covo_iter_slot(h, pass);  // an iterated step: this pass's merge logs its cost minimum there
    const int N = a.n_samples;
    const float *fdev = reinterpret_cast<const float *>(st->dyn + 2);
    float *am_shift = a.a_mean_shift ? a.a_mean_shift : st->a_mean_shift;
    int rc;
    const float *state = state_direct ? state_direct : st->state_buf;
    // covo-offline / MPPI at small N: noise -> rollout -> records -> merge as ONE launch (the begin launch has left the step's
    // scalars in st->dyn and the state in st->state_buf; MPPI: it has NOT touched a_cov, the fused launch shifts and factors)
    float *lam_rows = covo_lam_target(h);  // the ESS floor: the update's temperature is solved from this step's costs
    float *elite_rows = covo_elite_target(h);  // the elite-set update: the weights are selected from this step's costs
    const bool staged = covo_update_staged(h);
    if (M == 63 && h->opt.fuse_small && step_small_eligible(h, p, a) && !staged)
        return launch_step_small(h, p, a, state, am_shift, nullptr, st->dyn, 0.0f, st->ticket, s, pass, nullptr, iter_out);
    // periodic / sin / drag / mixed (free.py:10-58): the wave-uniform part of every rollout step's force, for the sampling
    // rollouts (shared step key) and for the Hessian's deterministic rollout (per-step keys), resolved once per control step
    const bool tables = covo_needs_tables(p);
    if (tables && (rc = launch_disturb_tables_step(p, state, st->dyn, a.rollout_deterministic, st->f_tab_rollout,
                                                   (a.mode == COVO_MODE_COVO_ONLINE && !reuse) ? st->f_tab_hess : nullptr, s))) return rc;
    // a = clip(am_shift + L eps): what the three modes' noise launches share (epsilon drawn in-kernel from the step's key in st->dyn)
    NoiseDesc nd;
    nd.mu = am_shift;
    nd.dyn = st->dyn;
    nd.sample_offset = a.sample_offset;
    nd.N = N;
    nd.a = a.a;
    nd.propagate_nan = covo_propagate_nan(h);
    if (a.mode == COVO_MODE_COVO_ONLINE && reuse) {
        // a reuse step of a Sigma period: no Hessian, no Sigma chain -- the previous step's factor is shifted in place (sigma_shift.hip),
        // a_cov is its Sigma', and the samples are drawn from it as covo-offline draws from a table row (in-kernel Philox); the later
        // passes of an iterated step sample from the same L'
        if (pass == 0 && (rc = launch_sigma_shift(st->L, 1, a.sample_sigma, a.a_cov ? a.a_cov : st->Sigma, st->L, s))) return rc;
        nd.L = st->L;
        if ((rc = launch_noise_gemm(nd, s))) return rc;
    } else if (a.mode == COVO_MODE_COVO_ONLINE) {
        // the Hessian's last launch leaves the Sigma chain's input statistics in the chain's workspace: no prep launch
        const bool stats = (M & 2) && (M & 4) && (dbg.hess & 15) == 15;
        const SymStatsOut so = sigma_ns_stats_out(h->ws_sigma);
        HessianDesc hd;
        hd.state = state;
        hd.pos_traj = a.pos_traj;
        hd.vel_traj = a.vel_traj;
        hd.T = a.T;
        hd.params = &p;
        hd.a_mean = am_shift;
        hd.R = st->R;
        hd.stats = stats ? &so : nullptr;
        hd.f_tab = tables ? st->f_tab_hess : nullptr;
        hd.status_dev = h->status_dev;
        hd.begin = begin;
        if ((M & 2) && (rc = launch_hessian(hd, h->ws_hess, s, dbg))) return rc;  // :134-185
        float *Sig = a.a_cov ? a.a_cov : st->Sigma;
        // epsilon needs only the act key: it is drawn under the chain's single-workgroup finalize launch, the GEMM loads it
        const bool ahead = st->eps_tiled != nullptr && (M & 4) && dbg.sigma_stages >= 4;
        EpsGenArgs gen;
        gen.eps_tiled = ahead ? st->eps_tiled : nullptr;
        gen.dyn = st->dyn;
        gen.sample_offset = a.sample_offset;
        gen.N = N;
        gen.n_inst = 1;
        gen.dyn_stride = 0;
        gen.eps_stride = 0;
        // a_cov is written by the GEMM's first workgroups, not by the chain's one-workgroup finalize launch (CovDeferred)
        CovDeferred cov;
        std::memset(&cov, 0, sizeof(cov));
        const bool defer = (M & 8) && dbg.sigma_stages >= 4;
        // the GEMM streamed under the factorisation, inside the chain's last launch (one matrix, persistent launches allowed)
        StreamGemmArgs sg;
        sg.mu = am_shift;
        sg.dyn = st->dyn;
        sg.sample_offset = a.sample_offset;
        sg.N = N;
        sg.a_out = a.a;
        sg.L_stream = st->L;
        sg.sync = st->sync;
        sg.a_cov_out = Sig;
        sg.nanp = covo_propagate_nan(h) ? 1 : 0;
        const bool want_stream = h->opt.stream_gemm && (M & 4) && (M & 8) && dbg.sigma_stages >= 4;
        bool streamed = false;
        SigmaNsDesc sd;
        sd.R = st->R;
        sd.sample_sigma = a.sample_sigma;
        sd.Sigma = Sig;
        sd.L = st->L;
        sd.gen = &gen;
        sd.status = h->status_dev;
        sd.persistent_ok = (h->cfg.flags & COVO_FLAG_SHARED_DEVICE) == 0;
        sd.cov = defer ? &cov : nullptr;
        sd.r_has_stats = stats;
        sd.stream = want_stream ? &sg : nullptr;
        sd.streamed = &streamed;
        if ((M & 4) && (rc = launch_sigma_ns(h->opt, sd, h->ws_sigma, s, dbg))) return rc;
        nd.L = st->L;
        nd.eps = ahead ? reinterpret_cast<const float *>(st->eps_tiled) : nullptr;  // (else the GEMM draws from st->dyn)
        nd.eps_tiled = ahead;
        nd.cov = &cov;
        if (!streamed && (M & 8) && (rc = launch_noise_gemm(nd, s))) return rc;
    } else if (a.mode == COVO_MODE_COVO_OFFLINE) {
        nd.L = a.L_table;
        nd.state_for_time = state;
        nd.n_table = a.n_table;
        if ((M & 8) && (rc = launch_noise_gemm(nd, s))) return rc;
    } else {  // MPPI: shift a_cov, factor the 4x4 blocks, per-step draws (mppi.py:43-66)
        nd.L = st->Ls;  // (a_cov was shifted and factored there by the begin launch)
        if ((rc = launch_noise_blockdiag(nd, s))) return rc;
    }
    // the rollout's workgroups leave the softmax update's stage-1 records themselves when they fit the merge (rollout.hip:
    // rollout_record); otherwise the stand-alone stage-1 kernel runs over the costs
    const int G = rollout_workgroups(N, a.pos_stats != nullptr);
    // MPPI's covariance adaptation needs second moments the in-rollout records do not carry: its own stage 1 (reduce.hip)
    const bool cov_adapt = a.mode == COVO_MODE_MPPI && a.gamma_sigma != 0.0f;
    // the ESS floor, the elite set: the rollout's in-launch records are formed with weights fixed before the costs exist -- staged, like
    // cov_adapt
    const bool records = G <= h->max_red_blocks && !cov_adapt && !staged;
    // the step's sampling diagnostics (covo_set_step_diag): the diagnostic variants of the same launches; a sharded step has none
    float *dg = a.partial_out == nullptr ? covo_diag_target(h) : nullptr;
    RolloutDesc ro;
    ro.state = state;
    ro.pos_traj = a.pos_traj;
    ro.vel_traj = a.vel_traj;
    ro.T = a.T;
    ro.params = &p;
    ro.f_shared_dev = fdev;
    ro.f_tab = tables ? st->f_tab_rollout : nullptr;
    ro.a = a.a;
    ro.N = N;
    ro.discount = h->cfg.discount;
    ro.cost = a.cost;
    ro.groupmin = records ? nullptr : a.groupmin;
    ro.pos_stats = a.pos_stats;
    ro.stats_ws = h->ws_stats;
    ro.records = records ? h->ws_partials : nullptr;
    ro.lam = h->cfg.lam;
    ro.diag_rec = (records && dg) ? h->ws_diag_rec : nullptr;
    ro.xcd_groups = a.mode == COVO_MODE_MPPI ? 4 : 0;  // MPPI's block-diagonal kernel: 256 samples per workgroup
    ro.clip = ROLLOUT_CLIP_TRUSTED;                    // a comes straight from the noise kernels above
    if ((M & 16) && (rc = launch_rollout(ro, s))) return rc;
    if (!(M & 32)) return 0;
    // rollout (costs + per-wave minima) -> solver -> stage 1 and merge reading 1 / lam_eff from lam_rows
    if (lam_rows != nullptr && (rc = launch_ess_lambda(a.cost, N, 1, a.groupmin, h->cfg.lam, h->ess_min, lam_rows, s))) return rc;
    // the elite set, in the floor's place: rollout (costs) -> selector -> stage 1 with 0/1 weights off elite_rows -> the same merges
    if (elite_rows != nullptr && (rc = launch_elite_select(a.cost, N, 1, h->elite_K, elite_rows, s))) return rc;
    // weights + update: finish locally (blend with am_shift, diagnostics), or -- a sample-sharded rank -- leave this shard's
    // record for the all-gather (covo.py:266-275)
    UpdateDesc up;
    up.cost = a.cost;
    up.a = a.a;
    up.N = N;
    up.blockmin = a.groupmin;
    up.n_blockmin = (N + 63) / 64;
    up.partials = h->ws_partials;  // (the rollout's records, if it left them)
    up.G = G;
    const bool sharded = a.partial_out != nullptr;
    up.a_mean_old = am_shift;
    up.gamma_mean = a.gamma_mean;
    up.a_mean_out = sharded ? nullptr : a.a_mean;
    up.partial_out = a.partial_out;
    up.diag_rec = h->ws_diag_rec;
    up.diag_out = dg;
    up.lam_rows = lam_rows;
    up.elite_rows = elite_rows;
    up.iter_out = sharded ? nullptr : iter_out;
    if (cov_adapt) {  // mppi.py:109-125: new mean, then a_cov (already shifted by the begin launch) adapted in place; a sharded
                      // rank: its record with the second moments (836-float kind)
        up.a_cov_old = a.a_cov;
        up.gamma_sigma = a.gamma_sigma;
        up.a_cov_out = sharded ? nullptr : a.a_cov;
        return elite_rows != nullptr ? launch_elite_update_cov(h, up, s) : launch_softmax_update_cov(h, up, s);
    }
    if (elite_rows != nullptr) return launch_elite_reduce(h, up, s);
    return records ? launch_merge(up, h->cfg.lam, s) : launch_softmax_reduce(h, up, s);
}

// a debug setter since the last step changed what a captured graph baked in (launch set, deflation switch, diagnostics target)
static void step_sync_epoch(covo_ctx *h)
{
    if (h->dbg_epoch == h->opt.epoch) return;
    step_graphs_drop(h);
    h->dbg_epoch = h->opt.epoch;
}

// reuse: a reuse step of a Sigma period (covo_set_step_sigma_period): enqueue_step's reuse branch, with a graph of its own
static int step_enqueue_all(covo_ctx *h, StepState *st, const covo_env_params *params, const covo_step_args *args, uint32_t key0,
                            uint32_t key1, const float *f_shared, hipStream_t s, const bool reuse)
{
    // per-step scalars: kernel arguments of the begin launch
    DynBlock blk;
    std::memset(&blk, 0, sizeof(blk));
    blk.w[0] = key0;
    blk.w[1] = key1;
    for (int i = 0; i < 3; ++i) {
        const float f = f_shared ? f_shared[i] : 0.0f;
        std::memcpy(&blk.w[2 + i], &f, 4);
    }
    std::memcpy(&blk.w[8], &args->state, sizeof(const float *));
    const float shared_noise_scale = covo_shared_noise_scale(*params, args->rollout_deterministic);
    // control_params.a_mean of this call: the handle's own buffer (a carried mean) or the caller's input (args->a_mean_in)
    const bool small = h->opt.fuse_small && step_small_eligible(h, *params, *args) && !covo_update_staged(h);
    // covo_set_step_iters: K passes on this state.  Pass j >= 1 starts from the mean pass j - 1 committed (args->a_mean, never the
    // caller's a_mean_in) and walks the raw key on the device; with the update arbiter attached its launch sits between the passes
    // (and the passes are enqueued eagerly: the arbiter's launch is not part of any captured graph)
    const int K = covo_step_iters(h);
    covo_step_args later = *args;
    later.a_mean_in = nullptr;
    auto between = [&](int j) -> int {
        return (j + 1 < K && covo_arb_on(h)) ? covo_plan_after_step(h, params, args, key0, key1, f_shared, nullptr, -1, s, true) : 0;
    };
    if (small && (h->cfg.flags & COVO_FLAG_NO_GRAPH) != 0) {
        // an eager handle: the WHOLE step is one launch, the begin launch's work included (per workgroup, step_small.hip)
        st->cache[0].have_key = false;  // (st->dyn / st->state_buf are not refreshed: a later graph capture starts from an eager call)
        for (int j = 0; j < K; ++j) {
            // (an iterated step: the last workgroup of every pass parks the pass's raw key at st->dyn[10..11] for the next one)
            int rc = launch_step_small(h, *params, j ? later : *args, args->state, args->a_mean_shift ? args->a_mean_shift : st->a_mean_shift,
                                       &blk, nullptr, shared_noise_scale, st->ticket, s, j, K > 1 ? st->dyn + 10 : nullptr,
                                       covo_iter_slot(h, j));
            if (rc || (rc = between(j))) return rc;
        }
        return 0;
    }
    // eager covo-online steps (no per-step force tables, whose launch precedes the Hessian and reads the scalars): the begin work
    // rides in the Hessian's first launch -- one launch boundary less (COVO_FOLD_BEGIN=0 keeps the begin launch)
    // (a reuse step has no Hessian launch to fold into: it keeps the begin launch)
    if (h->opt.fold_begin && args->mode == COVO_MODE_COVO_ONLINE && (h->cfg.flags & COVO_FLAG_NO_GRAPH) != 0 &&
        !covo_needs_tables(*params) && !reuse) {
        st->cache[0].have_key = false;
        for (int j = 0; j < K; ++j) {
            HessBegin hb;
            hb.pass = j;
            hb.a_mean_raw = j ? args->a_mean : (args->a_mean_in ? args->a_mean_in : args->a_mean);
            hb.dyn_out = st->dyn;
            hb.seq = st->sync;
            hb.blk = &blk;
            hb.derive_keys = args->derive_keys;
            hb.shared_noise_scale = shared_noise_scale;
            int rc = enqueue_step(h, st, *params, *args, s, DebugMasks(), &hb, args->state, j);
            if (rc || (rc = between(j))) return rc;
        }
        return 0;
    }
    float *mppi_cov = (args->mode == COVO_MODE_MPPI && !small) ? args->a_cov : (float *)nullptr;
    float *am_shift = args->a_mean_shift ? args->a_mean_shift : st->a_mean_shift;
    hipLaunchKernelGGL(step_begin_kernel, dim3(1), dim3(COVO_NA + COVO_STATE_FLOATS + 4), 0, s,
                       args->a_mean_in ? args->a_mean_in : args->a_mean, am_shift, st->dyn, st->state_buf, args->derive_keys,
                       shared_noise_scale, blk, mppi_cov, st->Ls, st->sync, 0);
    // the passes behind the begin launch: pass j >= 1 starts with a begin launch of its own, inside the graph
    auto passes = [&](hipStream_t on, bool with_arbiter) -> int {
        for (int j = 0; j < K; ++j) {
            if (j > 0)
                hipLaunchKernelGGL(step_begin_kernel, dim3(1), dim3(COVO_NA + COVO_STATE_FLOATS + 4), 0, on, (const float *)args->a_mean,
                                   am_shift, st->dyn, st->state_buf, 1, shared_noise_scale, DynBlock(), mppi_cov, st->Ls, st->sync, j);
            int rc = enqueue_step(h, st, *params, *args, on, DebugMasks(), nullptr, nullptr, j, reuse);
            if (rc || (with_arbiter && (rc = between(j)))) return rc;
        }
        return 0;
    };
    if (K > 1 && covo_arb_on(h)) {
        st->forget_graphs();
        return passes(s, true);
    }

    StepKey k;
    std::memset(&k, 0, sizeof(k));
    k.args = *args;
    k.args.state = nullptr;  // read through the dyn block: a new state address does not invalidate the graph
    k.args.a_mean_in = nullptr;  // read by the (eager) begin launch only
    k.params = *params;
    k.params.reset_traj = 0;  // the env step's auto-reset switches: no launch of the control step reads them
    k.params.reset_dt = k.params.reset_disturb_scale = 0.0;
    k.stream = s;
    GraphCache &cache = st->cache[reuse ? 1 : 0];
    StepKey &key = st->key[reuse ? 1 : 0];
    const bool same = cache.have_key && std::memcmp(&k, &key, sizeof(k)) == 0;
    if (!same) {
        key = k;
        cache.have_key = true;
    }
    return graph_cache_run(h, cache, s, same, "covo_mpc_step", [&](hipStream_t on) { return passes(on, false); });
}

int covo_step_impl(covo_ctx *h, const covo_env_params *params, const covo_step_args *args, uint32_t key0, uint32_t key1,
                   const float *f_shared, hipStream_t s)
{
    if (!h->step) {
        int rc = step_state_init(h);
        if (rc) return rc;
    }
    step_sync_epoch(h);
    StepState *st = reinterpret_cast<StepState *>(h->step);
    // covo_set_step_sigma_period: the age this step runs at -- 0: today's step, which leaves its factor in st->L; else a reuse step
    const bool online = args->mode == COVO_MODE_COVO_ONLINE;
    const int age = online ? covo_sigma_step_age(h, st->L, args->sample_sigma, 1) : 0;
    const int rc = step_enqueue_all(h, st, params, args, key0, key1, f_shared, s, age != 0);
    if (rc == 0 && online) covo_sigma_step_done(h, age, st->L, args->sample_sigma, 1);
    return rc;
}

// ---- the flight recorder behind a step (plan_trace.hip): one eager launch that rolls the new mean out with the inputs the step's
// sample rollouts had.  The shared vector is re-derived from the raw key by the launch itself (every step path forms it from the
// same device function); the per-step tables are the ones the step has just built in its own scratch.
int covo_plan_after_step(covo_ctx *h, const covo_env_params *params, const covo_step_args *args, uint32_t key0, uint32_t key1,
                         const float *f_shared, const float *state_true, int trace_index, hipStream_t s, bool arbiter_only)
{
    if (!covo_plan_on(h) && !covo_fan_on(h) && !covo_arb_on(h)) return 0;
    StepState *st = reinterpret_cast<StepState *>(h->step);
    // an iterated step (covo_set_step_iters): the launches describe the pass that has just been enqueued, whose raw key lies in
    // device memory (st->dyn[10..11]) -- they take it from there, through the argument blocks of the batched form
    const bool iterated = covo_step_iters(h) > 1 && st != nullptr;
    PlanInstDesc d;
    std::memset(&d, 0, sizeof(d));
    d.state = args->state;
    d.pos_traj = args->pos_traj;
    d.vel_traj = args->vel_traj;
    d.T = args->T;
    d.params = params;
    d.a_mean = args->a_mean;
    d.a = args->a;
    d.N = args->n_samples;
    d.cost = args->cost;
    d.a_nominal = args->a_mean_shift ? args->a_mean_shift : (st ? st->a_mean_shift : nullptr);
    d.a_mean_out = args->a_mean;
    d.f_tab = (covo_needs_tables(*params) && st) ? st->f_tab_rollout : nullptr;
    d.key[0] = key0;
    d.key[1] = key1;
    d.key_mem = iterated ? st->dyn + 10 : nullptr;
    for (int i = 0; i < 3; ++i) d.f_shared[i] = f_shared ? f_shared[i] : 0.0f;
    d.derive_keys = args->derive_keys;
    d.shared_noise_scale = covo_shared_noise_scale(*params, args->rollout_deterministic);
    int rc = launch_update_arbiter(h, &d, 1, iterated, trace_index, s);  // first: the plan, the trace's u and the env step see its mean
    if (rc || arbiter_only) return rc;
    if ((rc = launch_plan_trace(h, &d, 1, iterated, state_true, trace_index, s))) return rc;
    return launch_sample_fan(h, &d, 1, iterated, trace_index, s);  // (the episode's row index: the fan log counts like the trace)
}


// ---- profiling aids: `reps` copies of the selected part of one step captured into ONE graph and replayed; the average time per
// copy (GPU time between two events around the replay, the best of the last three of four replays).  Inside a graph the launches
// cost what they cost in the product (no host launch overhead, no profiler inflation).  enqueue_copy(stream) enqueues one copy.
template <class Enqueue>
static int time_graph_replays(covo_ctx *h, hipStream_t run, int reps, float *us_out, Enqueue enqueue_copy)
{
    hipStream_t cs = h->side_stream;
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto timed = [&]() -> int {
        int rc = 0;
        hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
        if (e == hipSuccess) {
            for (int r = 0; r < reps && !rc; ++r) rc = enqueue_copy(cs);
            e = hipStreamEndCapture(cs, &g);
        }
        if (rc) return rc;
        COVO_CHECK_HIP(e);
        COVO_CHECK_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        COVO_CHECK_HIP(hipEventCreate(&e0));
        COVO_CHECK_HIP(hipEventCreate(&e1));
        float best = 1e30f;
        for (int it = 0; it < 4; ++it) {
            COVO_CHECK_HIP(hipEventRecord(e0, run));
            COVO_CHECK_HIP(hipGraphLaunch(ge, run));
            COVO_CHECK_HIP(hipEventRecord(e1, run));
            COVO_CHECK_HIP(hipStreamSynchronize(run));
            float ms = 0.f;
            COVO_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
            if (it > 0 && ms < best) best = ms;
        }
        *us_out = best * 1e3f / (float)reps;
        return 0;
    };
    const int rc = timed();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (ge) (void)hipGraphExecDestroy(ge);
    if (g) (void)hipGraphDestroy(g);
    return rc;
}

// step_mask: enqueue_step's phases; hess_mask / sigma_stages: see covo_common.hpp.  The step must have been called once before (scratch).
int covo_debug_time_step_impl(covo_ctx *h, const covo_env_params *params, const covo_step_args *args, int step_mask,
                              int hess_mask, int sigma_stages, int reps, float *us_out, hipStream_t run)
{
    if (!h->step) {
        int rc = step_state_init(h);
        if (rc) return rc;
    }
    StepState *st = reinterpret_cast<StepState *>(h->step);
    const bool folded_online = h->opt.fold_begin && args->mode == COVO_MODE_COVO_ONLINE && !covo_needs_tables(*params);
    if (((h->opt.fuse_small && step_small_eligible(h, *params, *args) && !covo_update_staged(h)) || folded_online) && (h->cfg.flags & COVO_FLAG_NO_GRAPH) != 0 &&
        args->state != nullptr) {
        // the last step ran without a begin launch (the one-launch small step; covo-online with the begin work folded into the
        // Hessian) and never filled the scratch the replayed launches read (state copy, shifted mean, keys; MPPI: shifted
        // covariance + block factors): one begin launch does, with the key the step would derive from (0, 0)
        DynBlock blk;
        std::memset(&blk, 0, sizeof(blk));
        std::memcpy(&blk.w[8], &args->state, sizeof(const float *));
        hipLaunchKernelGGL(step_begin_kernel, dim3(1), dim3(COVO_NA + COVO_STATE_FLOATS + 4), 0, run,
                           args->a_mean_in ? args->a_mean_in : args->a_mean,
                           args->a_mean_shift ? args->a_mean_shift : st->a_mean_shift, st->dyn, st->state_buf, args->derive_keys, 0.0f,
                           blk, args->mode == COVO_MODE_MPPI ? args->a_cov : (float *)nullptr, st->Ls, st->sync, 0);
        COVO_CHECK_HIP(hipStreamSynchronize(run));
    }
    DebugMasks dbg;
    dbg.step = step_mask;
    dbg.hess = hess_mask;
    dbg.sigma_stages = sigma_stages;
    return time_graph_replays(h, run, reps, us_out, [&](hipStream_t cs) {
        if (args->mode == COVO_MODE_COVO_ONLINE && h->opt.stream_gemm && (step_mask & 12) == 12)
            hipLaunchKernelGGL(stream_seq_bump_kernel, dim3(1), dim3(1), 0, cs, st->sync);
        return enqueue_step(h, st, *params, *args, cs, dbg);
    });
}


// =====================================================================================================================
// Env-batched covo-online step (BASELINE configs[4]: E independent env instances, each with its own state, reference
// trajectory, domain-randomised parameters, mean and noise key): ONE graph for all instances.  The latency-bound part
// -- Hessian and the eigh-free Sigma chain -- runs once for all E matrices (every kernel of both takes `batch`), so its
// ~50 launches are amortised over the instances; noise GEMM, rollout and softmax update are enqueued per instance.
// "Replicas only" (SURVEY.md 8e): no exchange between instances, env instances shard over GPUs without a collective.
struct BatchDyn {
    uint32_t w[COVO_MAX_ENVS][4];  // {rng_act[2] -> act_key[2]} per instance
};
__global__ void batch_set_dyn_kernel(uint32_t *__restrict__ dyn, const BatchDyn b, int n)
{
    const int i = threadIdx.x;
    if (i < 4 * n) dyn[12 * (i >> 2) + (i & 3)] = b.w[i >> 2][i & 3];
}
// the eager launch in front of every batched step (its kernel arguments ARE the keys): instance e's raw rng_act to dyn[12 e + 0..1]
static void batch_upload_keys(uint32_t *dyn, const uint32_t *keys, int E, hipStream_t s)
{
    BatchDyn blk;
    std::memset(&blk, 0, sizeof(blk));
    for (int e = 0; e < E; ++e) {
        blk.w[e][0] = keys[2 * e];
        blk.w[e][1] = keys[2 * e + 1];
    }
    hipLaunchKernelGGL(batch_set_dyn_kernel, dim3(1), dim3(256), 0, s, dyn, blk, E);
}
// per instance: shift the mean (covo.py:201-203); act_key = split(rng_act)[1] (covo.py:212); f_shared = 0 (deterministic)
// pass >= 1 of an iterated step (covo_set_step_iters): no shift, and the raw key is the previous pass's (d[10..11]) advanced
__global__ void batch_begin_kernel(const float *__restrict__ a_mean, float *__restrict__ a_mean_shift, uint32_t *__restrict__ dyn,
                                   const int pass)
{
    const int e = blockIdx.x, i = threadIdx.x;
    uint32_t *d = dyn + 12 * e;
    uint32_t raw[2] = {d[pass ? 10 : 0], d[pass ? 11 : 1]};
    __syncthreads();
    if (i < COVO_NA) {
        a_mean_shift[e * COVO_NA + i] = (pass == 0 && i < COVO_NA - COVO_DU) ? a_mean[e * COVO_NA + i + COVO_DU] : a_mean[e * COVO_NA + i];
    } else if (i == COVO_NA) {
        if (pass) step_begin_advance(raw);
        uint32_t k[2];
        host_split(raw, 1u, k);
        d[0] = k[0];
        d[1] = k[1];
        d[2] = d[3] = d[4] = 0u;
        d[10] = raw[0];  // the raw controller key, for the step's disturbance tables (disturb.hip)
        d[11] = raw[1];
    }
}

// the env-batched MPPI / covo-offline step (covo_mpc_step_batched_mode): ONE fused launch for all instances (step_small.hip,
// grid = groups x instances) behind the key upload; scratch and graph cache of its own, next to the covo-online batch's
struct BatchSmall {
    int n_envs = 0, groups = 0;
    uint32_t *dyn = nullptr;     // [E][12]: the instances' raw rng_act of the current step (batch_set_dyn_kernel)
    void *args = nullptr;        // SmallStepArgs[E]
    unsigned *tickets = nullptr; // [E] arrival counters; each wraps to 0 with its instance's last workgroup (atomicInc)
    float *records = nullptr;    // [E][groups][COVO_PARTIAL_FLOATS]
    float *diag_rec = nullptr;   // [E][groups][4] the diagnostic records next to them (covo_set_step_diag)
    std::vector<char> args_host;
    std::vector<covo_env_params> params;
    covo_batch_mode_args key;  // with `stream` and `params`: what the cached argument blocks and graph were built for
    hipStream_t stream = nullptr;
    GraphCache cache{};
};

static void batch_small_free(BatchSmall *m)
{
    m->cache.forget();
    free_and_null(m->dyn, m->args, m->tickets, m->records, m->diag_rec);
    m->n_envs = m->groups = 0;
}

struct BatchState {
    BatchSmall small;
    int n_envs = 0;
    uint32_t *dyn = nullptr;        // [E][12]
    float *a_mean_shift = nullptr;  // [E][128]
    double *R = nullptr;            // [E][128][128]
    float *Sigma = nullptr, *L = nullptr;  // [E][128][128]
    void *consts = nullptr;         // qm::Consts<double>[E]   (Hessian)
    void *ro_args = nullptr;        // RolloutArgs[E]          (rollout)
    float *partials = nullptr;      // [E][max_red_blocks][COVO_PARTIAL_FLOATS]: the instances' softmax stage-1 records
    float *diag_rec = nullptr;      // [E][max_red_blocks][4]: their diagnostic records (covo_set_step_diag)
    void *models = nullptr;         // dm::Model[E]            (disturbance tables, drag / mixed Hessian)
    float *tab_rollout = nullptr, *tab_hess = nullptr;  // [E][H][4] the step's disturbance tables (periodic / sin / drag / mixed)
    bool tables = false;            // the instances' disturbance model needs them
    void *env_inst = nullptr;       // EnvInst[env_inst_n] (env_step.hip): the per-instance constants of covo_env_step_batched
    int env_inst_n = 0;
    std::vector<covo_env_params> env_inst_params;
    std::vector<char> ro_args_host;
    std::vector<covo_env_params> params;
    covo_batch_args key;  // with `stream` and `params`: what the cached scratch and graph were built for
    hipStream_t stream = nullptr;
    GraphCache cache{};
    GraphCache cache_reuse{};  // the reuse step of a Sigma period (covo_set_step_sigma_period): another launch set, its own graph
    float4 *eps_tiled = nullptr;  // [E][ceil(N/32)][16][64]: the step's epsilon of every instance, drawn under the Sigma chain's
    size_t eps_cap = 0;           // finalize launch (eps_tiles.hpp), as in the single step
};

// (not env_inst and eps_tiled: the batched step re-allocates its scratch when the instance count changes, possibly between
// batch_env_inst and the env step launch that reads env_inst; eps_tiled only ever grows)
static void batch_state_free(BatchState *b)
{
    b->cache.drop();
    b->cache_reuse.forget();
    free_and_null(b->dyn, b->a_mean_shift, b->R, b->Sigma, b->L, b->consts, b->ro_args, b->partials, b->diag_rec, b->models,
                  b->tab_rollout, b->tab_hess);
}
// The captured graphs (fused step, env-batched steps) hold the addresses of h->ws_sigma / h->ws_hess in their kernel nodes and bake
// the handle's launch set in: whoever re-allocates a workspace (covo_grow_workspace) or meets a moved debug epoch calls this
// first, so that a later step re-captures instead of replaying launches that point into freed memory.
void step_graphs_drop(covo_ctx *h)
{
    StepState *st = reinterpret_cast<StepState *>(h->step);
    BatchState *b = reinterpret_cast<BatchState *>(h->batch);
    if (st) st->forget_graphs();
    if (b) b->cache.forget();
    if (b) b->cache_reuse.forget();
    if (b) b->small.cache.forget();
}

int covo_grow_workspace(covo_ctx *h, void **ws, size_t *bytes, size_t need, hipStream_t s)
{
    if (need <= *bytes) return 0;
    COVO_CHECK_HIP(hipStreamSynchronize(s));
    step_graphs_drop(h);
    free_and_null(*ws);
    *bytes = 0;
    COVO_CHECK_HIP(hipMalloc(ws, need));
    *bytes = need;
    return 0;
}

static BatchState *batch_state(covo_ctx *h)
{
    if (!h->batch) h->batch = new BatchState();
    return reinterpret_cast<BatchState *>(h->batch);
}

// instance e of a batched step's argument block
struct BatchInst {
    const float *state, *pos_traj, *vel_traj;
    float *a_mean, *a, *cost, *groupmin;
};
static BatchInst batch_inst(const covo_batch_args &a, int e)
{
    const int N = a.n_samples;
    BatchInst i;
    i.state = a.states + (size_t)e * COVO_STATE_FLOATS;
    i.pos_traj = a.pos_traj + (size_t)e * a.T * 3;
    i.vel_traj = a.vel_traj + (size_t)e * a.T * 3;
    i.a_mean = a.a_mean + (size_t)e * COVO_NA;
    i.a = a.a + (size_t)e * COVO_H * N * 4;
    i.cost = a.cost + (size_t)e * N;
    i.groupmin = a.groupmin ? a.groupmin + (size_t)e * ((N + 63) / 64) : nullptr;
    return i;
}

// the device array of per-instance env constants for covo_env_step_batched, rebuilt only when the parameters change
int batch_env_inst(covo_ctx *h, const covo_env_params *params, int E, hipStream_t s, const void **inst_dev)
{
    BatchState *b = batch_state(h);
    const bool same = b->env_inst != nullptr && b->env_inst_n == E && (int)b->env_inst_params.size() == E &&
                      std::memcmp(b->env_inst_params.data(), params, (size_t)E * sizeof(covo_env_params)) == 0;
    if (!same) {
        COVO_CHECK_HIP(hipStreamSynchronize(s));  // launches that read the old array are done
        if (b->env_inst_n != E) {
            free_and_null(b->env_inst);
            b->env_inst_n = 0;
            COVO_CHECK_HIP(hipMalloc(&b->env_inst, env_step_inst_bytes(E)));
            b->env_inst_n = E;
        }
        std::vector<char> tmp(env_step_inst_bytes(E));
        env_step_fill_inst(params, E, tmp.data());
        COVO_CHECK_HIP(hipMemcpy(b->env_inst, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
        b->env_inst_params.assign(params, params + E);
    }
    *inst_dev = b->env_inst;
    return 0;
}

void batch_state_destroy(covo_ctx *h)
{
    BatchState *b = reinterpret_cast<BatchState *>(h->batch);
    if (!b) return;
    batch_state_free(b);
    batch_small_free(&b->small);
    free_and_null(b->eps_tiled, b->env_inst);
    delete b;
    h->batch = nullptr;
}

// Seven batched launch sets for all E instances: begin, Hessian (4 kernels), Sigma chain (~47), noise GEMM, rollout,
// softmax partials, merge -- every kernel takes the instance as a grid dimension.  (Measured alternative, E = 32,
// N = 4096: per-instance GEMM/rollout/softmax launches 1 452 us per call; the same spread over 2 / 4 / 8 forked
// branches of the graph 1 103 / 1 140 / 1 153 us, while hipGraphLaunch's host cost grew from 47 to >300 us.  Round 4: the Sigma
// chain of the two halves of the instances on two forked branches, every phase its own launch: 72 700 control-steps/s against
// 71 200 unforked with the same launches and 76 300 with the persistent tails -- which must not run side by side: two persistent
// launches can starve each other of workgroup slots, the barriers then time out.)
static int batch_enqueue(covo_ctx *h, BatchState *b, const covo_batch_args &a, hipStream_t s, const DebugMasks &dbg = DebugMasks(),
                         const int pass = 0, const bool reuse = false)
{
    const int E = a.n_envs, N = a.n_samples;
    const int M = dbg.step;  // 63 outside covo_debug_time_batched (which replays selected launch groups)
    int rc;
    if (M & 1) hipLaunchKernelGGL(batch_begin_kernel, dim3(E), dim3(COVO_NA + 64), 0, s, a.a_mean, b->a_mean_shift, b->dyn, pass);
    // covo.py:231: CoVO's sampling rollouts run step_env(deterministic=True); get_hessian likewise (covo.py:152)
    if ((M & 1) && b->tables && (rc = launch_disturb_tables_batched(b->models, a.states, b->dyn, E, 1, b->tab_rollout, b->tab_hess, s)))
        return rc;
    NoiseDesc nd;
    nd.L = b->L;
    nd.mu = b->a_mean_shift;
    nd.dyn = b->dyn;
    nd.N = N;
    nd.a = a.a;
    nd.batch = E;
    nd.propagate_nan = covo_propagate_nan(h);
    if (reuse) {
        // a reuse step of a Sigma period: every instance's factor is shifted in place (sigma_shift.hip; pass 0 only), a_cov is its
        // Sigma', the GEMM draws its epsilon itself
        if (pass == 0 && (rc = launch_sigma_shift(b->L, E, a.sample_sigma, a.a_cov ? a.a_cov : b->Sigma, b->L, s))) return rc;
        if ((rc = launch_noise_gemm(nd, s))) return rc;
    } else {
    // as in the single step: the Hessian's last launch leaves every instance's Sigma-chain input statistics, no prep launch
    const bool stats = (M & 2) && (M & 4) && (dbg.hess & 15) == 15;
    const SymStatsOut so = sigma_ns_stats_out(h->ws_sigma, E);
    HessianDesc hd;
    hd.state = a.states;
    hd.pos_traj = a.pos_traj;
    hd.vel_traj = a.vel_traj;
    hd.T = a.T;
    hd.params = &b->params[0];
    hd.a_mean = b->a_mean_shift;
    hd.batch = E;
    hd.R = b->R;
    hd.consts_dev = b->consts;
    hd.traj_stride = (size_t)a.T * 3;
    hd.stats = stats ? &so : nullptr;
    hd.f_tab = b->tables ? b->tab_hess : nullptr;
    hd.models_dev = b->models;
    hd.status_dev = h->status_dev;
    if ((M & 2) && (rc = launch_hessian(hd, h->ws_hess, s, dbg))) return rc;
    float *Sig = a.a_cov ? a.a_cov : b->Sigma;
    // epsilon needs only the act keys: every instance's is drawn under the chain's finalize launch (32 of 256 CUs factor), the GEMM
    // loads it -- the in-kernel Philox costs the batched GEMM ~9 us, its matrix pipe hides no vector work
    const bool ahead = b->eps_tiled != nullptr && (M & 4) && (M & 8) && dbg.sigma_stages >= 4;
    EpsGenArgs gen;
    gen.eps_tiled = ahead ? b->eps_tiled : nullptr;
    gen.dyn = b->dyn;
    gen.sample_offset = 0;
    gen.N = N;
    gen.n_inst = E;
    gen.dyn_stride = 12;
    gen.eps_stride = (size_t)((N + 31) / 32) * 16 * 64;
    SigmaNsDesc sd;
    sd.R = b->R;
    sd.batch = E;
    sd.sample_sigma = a.sample_sigma;
    sd.Sigma = Sig;
    sd.L = b->L;
    sd.gen = &gen;
    sd.status = h->status_dev;
    sd.persistent_ok = (h->cfg.flags & COVO_FLAG_SHARED_DEVICE) == 0;
    sd.r_has_stats = stats;
    if ((M & 4) && (rc = launch_sigma_ns(h->opt, sd, h->ws_sigma, s, dbg))) return rc;
    nd.eps = ahead ? reinterpret_cast<const float *>(b->eps_tiled) : nullptr;  // (else the GEMM draws from b->dyn)
    nd.eps_tiled = ahead;
    if ((M & 8) && (rc = launch_noise_gemm(nd, s))) return rc;
    }
    if ((M & 16) && (rc = launch_rollout_batched(b->ro_args_host.data(), b->ro_args, E, s))) return rc;
    if (!(M & 32)) return 0;
    const int G = rollout_workgroups(N, false, E);
    UpdateDesc up;
    up.cost = a.cost;
    up.a = a.a;
    up.N = N;
    up.blockmin = a.groupmin;
    up.n_blockmin = (N + 63) / 64;
    up.partials_ws = b->partials;
    up.partials = b->partials;
    up.G = G;
    up.a_mean_old = b->a_mean_shift;
    up.gamma_mean = a.gamma_mean;
    up.a_mean_out = a.a_mean;
    up.batch = E;
    up.diag_rec = b->diag_rec;
    up.diag_out = covo_diag_target(h);  // row e of the caller's diagnostic buffer is instance e's
    // the ESS floor: the rollouts left costs and per-wave minima, no records (covo_step_batched_impl); row e of the solver's output
    // is instance e's temperature
    up.lam_rows = covo_lam_target(h);
    up.iter_out = covo_iter_slot(h, pass);  // an iterated step: instance e's cost minimum of this pass to iter_log[e][pass]
    up.iter_stride = covo_step_iters(h);
    if (up.lam_rows != nullptr) {
        if ((rc = launch_ess_lambda(a.cost, N, E, a.groupmin, h->cfg.lam, h->ess_min, covo_lam_target(h), s))) return rc;
        return launch_softmax_reduce(h, up, s);
    }
    // the elite set, likewise: row e of the selector's output is instance e's threshold
    if (float *elite_rows = covo_elite_target(h)) {
        up.elite_rows = elite_rows;
        if ((rc = launch_elite_select(a.cost, N, E, h->elite_K, elite_rows, s))) return rc;
        return launch_elite_reduce(h, up, s);
    }
    // the rollout's workgroups have left the records when they fit the merge (rollout_record): instance e's are [e][G]
    return G <= h->max_red_blocks ? launch_merge(up, h->cfg.lam, s) : launch_softmax_reduce(h, up, s);
}

// profiling aid (bench.py --config envs): `reps` copies of the selected launch groups of the LAST covo_mpc_step_batched call in
// one graph; GPU microseconds per copy.  step_mask as in covo_debug_time_step (1 begin, 2 Hessian, 4 Sigma, 8 GEMM, 16 rollout,
// 32 update).  The copies re-read the same means and states (the begin launch is normally left out: it would re-split the keys).
int covo_debug_time_batched_impl(covo_ctx *h, int step_mask, int reps, float *us_out, hipStream_t run)
{
    BatchState *b = reinterpret_cast<BatchState *>(h->batch);
    if (!b || !b->cache.have_key) {
        covo_set_error("covo_debug_time_batched: call covo_mpc_step_batched first");
        return COVO_E_BADARG;
    }
    COVO_CHECK_HIP(hipStreamSynchronize(run));
    DebugMasks dbg;
    dbg.step = step_mask;
    return time_graph_replays(h, run, reps, us_out, [&](hipStream_t cs) { return batch_enqueue(h, b, b->key, cs, dbg); });
}

int covo_step_batched_impl(covo_ctx *h, const covo_batch_args *args, const covo_env_params *params, const uint32_t *keys,
                           hipStream_t s)
{
    const int E = args->n_envs;
    step_sync_epoch(h);
    BatchState *b = batch_state(h);
    const bool same = b->cache.have_key && b->n_envs == E && std::memcmp(&b->key, args, sizeof(*args)) == 0 && b->stream == s &&
                      std::memcmp(b->params.data(), params, (size_t)E * sizeof(covo_env_params)) == 0;
    if (!same) {
        // new buffers / parameters / instance count: (re)allocate scratch and drop the stale graph (outside the steady state)
        COVO_CHECK_HIP(hipStreamSynchronize(s));
        b->cache.drop();
        b->cache_reuse.forget();
        if (b->n_envs != E) {
            batch_state_free(b);
            h->sigma_L = nullptr;  // (the factor buffer goes: the next step of a Sigma period refreshes)
            const size_t M = (size_t)COVO_NA * COVO_NA;
            COVO_CHECK_HIP(hipMalloc(&b->dyn, (size_t)E * 12 * sizeof(uint32_t)));
            COVO_CHECK_HIP(hipMalloc(&b->a_mean_shift, (size_t)E * COVO_NA * sizeof(float)));
            COVO_CHECK_HIP(hipMalloc(&b->R, (size_t)E * M * sizeof(double)));
            COVO_CHECK_HIP(hipMalloc(&b->Sigma, (size_t)E * M * sizeof(float)));
            COVO_CHECK_HIP(hipMalloc(&b->L, (size_t)E * M * sizeof(float)));
            COVO_CHECK_HIP(hipMalloc(&b->consts, hessian_consts_bytes(E)));
            COVO_CHECK_HIP(hipMalloc(&b->ro_args, rollout_args_bytes(E)));
            COVO_CHECK_HIP(hipMalloc(&b->partials, (size_t)E * h->max_red_blocks * COVO_PARTIAL_FLOATS * sizeof(float)));
            COVO_CHECK_HIP(hipMalloc(&b->diag_rec, (size_t)E * h->max_red_blocks * 4 * sizeof(float)));
            COVO_CHECK_HIP(hipMalloc(&b->models, disturb_models_bytes(E)));
            COVO_CHECK_HIP(hipMalloc(&b->tab_rollout, (size_t)E * COVO_H * 4 * sizeof(float)));
            COVO_CHECK_HIP(hipMalloc(&b->tab_hess, (size_t)E * COVO_H * 4 * sizeof(float)));
            b->n_envs = E;
        }
        b->params.assign(params, params + E);
        std::vector<char> tmp(hessian_consts_bytes(E));
        hessian_fill_consts(params, E, tmp.data());
        COVO_CHECK_HIP(hipMemcpy(b->consts, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
        tmp.assign(disturb_models_bytes(E), 0);
        disturb_fill_models(params, E, tmp.data());
        COVO_CHECK_HIP(hipMemcpy(b->models, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
        b->tables = covo_needs_tables(params[0]);
        b->ro_args_host.assign(rollout_args_bytes(E), 0);
        const int N = args->n_samples;
        const int bG = rollout_workgroups(N, false, E);
        const bool brec = bG <= h->max_red_blocks && !covo_update_staged(h);  // (a floor, an elite set: staged update, see batch_enqueue)
        for (int e = 0; e < E; ++e) {
            const BatchInst i = batch_inst(*args, e);
            RolloutDesc ro;
            ro.state = i.state;
            ro.pos_traj = i.pos_traj;
            ro.vel_traj = i.vel_traj;
            ro.T = args->T;
            ro.params = &params[e];
            ro.f_shared_dev = reinterpret_cast<const float *>(b->dyn + 12 * e + 2);
            ro.f_tab = b->tables ? b->tab_rollout + (size_t)e * COVO_H * 4 : nullptr;
            ro.a = i.a;
            ro.N = N;
            ro.discount = h->cfg.discount;
            ro.cost = i.cost;
            ro.groupmin = brec ? nullptr : i.groupmin;
            ro.records = brec ? b->partials + (size_t)e * bG * COVO_PARTIAL_FLOATS : nullptr;
            ro.lam = h->cfg.lam;
            ro.diag_rec = (brec && covo_diag_target(h)) ? b->diag_rec + (size_t)e * bG * 4 : nullptr;
            ro.clip = ROLLOUT_CLIP_TRUSTED;  // a comes straight from the noise GEMM
            rollout_fill_args(b->ro_args_host.data(), e, ro);
        }
        COVO_CHECK_HIP(hipMemcpy(b->ro_args, b->ro_args_host.data(), b->ro_args_host.size(), hipMemcpyHostToDevice));
        {
            const size_t need_e = (size_t)E * ((N + 31) / 32) * 16 * 64;
            if (need_e > b->eps_cap) {
                free_and_null(b->eps_tiled);
                b->eps_cap = 0;
                COVO_CHECK_HIP(hipMalloc(&b->eps_tiled, need_e * sizeof(float4)));
                b->eps_cap = need_e;
            }
        }
        int rc;  // (a grown workspace forgets every graph and key of the handle: this block records the key after it)
        if ((rc = covo_grow_workspace(h, &h->ws_sigma, &h->ws_sigma_bytes, sigma_ns_workspace_bytes(E), s))) return rc;
        if ((rc = covo_grow_workspace(h, &h->ws_hess, &h->ws_hess_bytes, hessian_workspace_bytes(E), s))) return rc;
        b->key = *args;
        b->stream = s;
        b->cache.have_key = true;
    }
    batch_upload_keys(b->dyn, keys, E, s);
    // covo_set_step_iters: K passes in one graph; with the update arbiter attached its (eager) launch sits between them and the
    // passes are enqueued eagerly
    const int K = covo_step_iters(h);
    // covo_set_step_sigma_period: the batch shares one age -- 0: today's step, which leaves the factors in b->L; else a reuse step
    const int age = covo_sigma_step_age(h, b->L, args->sample_sigma, E);
    const bool reuse = age != 0;
    auto passes = [&](hipStream_t on, bool with_arbiter) -> int {
        for (int j = 0; j < K; ++j) {
            int rc = batch_enqueue(h, b, *args, on, DebugMasks(), j, reuse);
            if (rc == 0 && with_arbiter && j + 1 < K)
                rc = covo_plan_after_batched(h, args, COVO_MODE_COVO_ONLINE, params, nullptr, -1, on, true);
            if (rc) return rc;
        }
        return 0;
    };
    int rc;
    if (K > 1 && covo_arb_on(h)) {
        b->cache.drop();
        b->cache_reuse.forget();
        rc = passes(s, true);
    } else if (reuse) {  // the reuse graph's key is the step's: its first call with these buffers runs eagerly, the second captures
        const bool same_reuse = same && b->cache_reuse.have_key;
        b->cache_reuse.have_key = true;
        rc = graph_cache_run(h, b->cache_reuse, s, same_reuse, "covo_mpc_step_batched", [&](hipStream_t on) { return passes(on, false); });
    } else {
        rc = graph_cache_run(h, b->cache, s, same, "covo_mpc_step_batched", [&](hipStream_t on) { return passes(on, false); });
    }
    if (rc == 0) covo_sigma_step_done(h, age, b->L, args->sample_sigma, E);
    return rc;
}

// MPPI / covo-offline for E instances: key upload + ONE fused launch (no begin launch: every workgroup shifts its instance's mean
// and derives its instance's keys itself, as an eager single step does).  The second identical call captures the fused launch
// into a graph; the key upload stays eager in front of it (its kernel arguments ARE the keys).  The caller (capi.hip) has
// checked eligibility: nothing here is refused after a launch.
static covo_step_args batch_small_instance(const covo_batch_mode_args &m, int e)
{
    const covo_batch_args &a = m.base;
    const BatchInst i = batch_inst(a, e);
    covo_step_args sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.mode = m.mode;
    sa.n_samples = a.n_samples;
    sa.T = a.T;
    sa.n_table = m.n_table;
    sa.state = i.state;
    sa.pos_traj = i.pos_traj;
    sa.vel_traj = i.vel_traj;
    sa.a_mean = i.a_mean;
    sa.a_cov = (m.mode == COVO_MODE_MPPI) ? a.a_cov + (size_t)e * COVO_H * 16 : nullptr;
    sa.L_table = (m.mode == COVO_MODE_COVO_OFFLINE) ? m.L_table + (size_t)e * m.L_table_stride : nullptr;
    sa.a = i.a;
    sa.cost = i.cost;
    sa.gamma_mean = a.gamma_mean;
    sa.sample_sigma = a.sample_sigma;
    sa.derive_keys = 1;
    sa.rollout_deterministic = (m.mode == COVO_MODE_MPPI) ? 0 : 1;  // covo.py:231 / mppi.py:74
    sa.gamma_sigma = m.gamma_sigma;
    return sa;
}

const char *batch_small_refusal(const covo_ctx *h, const covo_batch_mode_args *m, const covo_env_params *params, int *which)
{
    for (int e = 0; e < m->base.n_envs; ++e) {
        const covo_step_args sa = batch_small_instance(*m, e);
        const char *why = step_small_refusal(h, params[e], sa);
        if (why) {
            *which = e;
            return why;
        }
    }
    return nullptr;
}

int covo_step_batched_small_impl(covo_ctx *h, const covo_batch_mode_args *m, const covo_env_params *params, const uint32_t *keys,
                                 hipStream_t s)
{
    const int E = m->base.n_envs, N = m->base.n_samples, ng = (N + COVO_WAVE - 1) / COVO_WAVE;
    if (covo_arb_on(h)) {  // the update arbiter's nominal: the fused launch keeps its shifted mean in LDS only
        const int rc = launch_arbiter_nominal(h, m->base.a_mean, E, s, nullptr);
        if (rc) return rc;
    }
    step_sync_epoch(h);
    BatchSmall *q = &batch_state(h)->small;
    const bool same = q->cache.have_key && q->n_envs == E && std::memcmp(&q->key, m, sizeof(*m)) == 0 && q->stream == s &&
                      std::memcmp(q->params.data(), params, (size_t)E * sizeof(covo_env_params)) == 0;
    if (!same) {
        COVO_CHECK_HIP(hipStreamSynchronize(s));  // launches that read the old argument blocks are done
        q->cache.drop();
        if (q->n_envs != E || q->groups != ng) {
            batch_small_free(q);
            COVO_CHECK_HIP(hipMalloc(&q->dyn, (size_t)E * 12 * sizeof(uint32_t)));
            COVO_CHECK_HIP(hipMalloc(&q->args, step_small_args_bytes(E)));
            COVO_CHECK_HIP(hipMalloc(&q->tickets, (size_t)E * sizeof(unsigned)));
            COVO_CHECK_HIP(hipMalloc(&q->records, (size_t)E * ng * COVO_PARTIAL_FLOATS * sizeof(float)));
            COVO_CHECK_HIP(hipMalloc(&q->diag_rec, (size_t)E * ng * 4 * sizeof(float)));
            q->n_envs = E;
            q->groups = ng;
        }
        COVO_CHECK_HIP(hipMemset(q->tickets, 0, (size_t)E * sizeof(unsigned)));
        q->params.assign(params, params + E);
        q->args_host.assign(step_small_args_bytes(E), 0);
        float *dg = covo_diag_target(h);
        for (int e = 0; e < E; ++e) {
            const covo_step_args sa = batch_small_instance(*m, e);
            // (the shared gaussian vector of MPPI's sampling rollouts, per instance; off for CoVO: deterministic)
            step_small_fill_args(h, q->args_host.data(), e, params[e], sa, q->dyn + 12 * e,
                                 covo_shared_noise_scale(params[e], sa.rollout_deterministic), q->tickets + e,
                                 q->records + (size_t)e * ng * COVO_PARTIAL_FLOATS, q->diag_rec + (size_t)e * ng * 4,
                                 dg ? dg + (size_t)e * COVO_DIAG_FLOATS : nullptr,
                                 covo_step_iters(h) > 1 ? h->iter_log + (size_t)e * covo_step_iters(h) : nullptr);
        }
        COVO_CHECK_HIP(hipMemcpy(q->args, q->args_host.data(), q->args_host.size(), hipMemcpyHostToDevice));
        std::memset(&q->key, 0, sizeof(q->key));
        q->key = *m;
        q->stream = s;
        q->cache.have_key = true;
    }
    batch_upload_keys(q->dyn, keys, E, s);
    const bool mppi = m->mode == COVO_MODE_MPPI;
    // covo_set_step_iters: K launches of the same kernel in one graph (the last workgroup of instance e's pass leaves the pass's raw
    // key at q->dyn[12 e + 0..1] for the next pass and for the recorder's launches)
    const int K = covo_step_iters(h);
    return graph_cache_run(h, q->cache, s, same, "covo_mpc_step_batched_mode", [&](hipStream_t on) {
        for (int j = 0; j < K; ++j) {
            const int rc = launch_step_small_batched(h, q->args_host.data(), q->args, E, mppi, on, j);
            if (rc) return rc;
        }
        return 0;
    });
}

// mode: COVO_MODE_COVO_ONLINE (covo_step_batched_impl has run) or MPPI / COVO_OFFLINE (covo_step_batched_small_impl)
int covo_plan_after_batched(covo_ctx *h, const covo_batch_args *args, int mode, const covo_env_params *params,
                            const float *states_true, int trace_index, hipStream_t s, bool arbiter_only)
{
    if (!covo_plan_on(h) && !covo_fan_on(h) && !covo_arb_on(h)) return 0;
    BatchState *b = reinterpret_cast<BatchState *>(h->batch);
    const int E = args->n_envs;
    const bool online = mode == COVO_MODE_COVO_ONLINE;
    PlanInstDesc d[COVO_MAX_ENVS];
    std::memset(d, 0, sizeof(d));
    const float *nominal = nullptr;  // the update arbiter's: covo-online's begin launch leaves it, the fused launch's was formed ahead of it
    if (covo_arb_on(h)) {
        if (online) nominal = b->a_mean_shift;
        else if (int rc = launch_arbiter_nominal(h, nullptr, E, s, &nominal)) return rc;
    }
    for (int e = 0; e < E; ++e) {
        const BatchInst i = batch_inst(*args, e);
        d[e].state = i.state;
        d[e].pos_traj = i.pos_traj;
        d[e].vel_traj = i.vel_traj;
        d[e].T = args->T;
        d[e].params = &params[e];
        d[e].a_mean = i.a_mean;
        d[e].a = i.a;
        d[e].N = args->n_samples;
        d[e].cost = i.cost;
        d[e].a_nominal = nominal ? nominal + (size_t)e * COVO_NA : nullptr;
        d[e].a_mean_out = i.a_mean;
        d[e].f_tab = (online && b->tables) ? b->tab_rollout + (size_t)e * COVO_H * 4 : nullptr;
        // the instance's raw rng_act: covo-online's begin launch parks it at [10..11] of its block, the fused launch leaves [0..1] alone
        d[e].key_mem = online ? b->dyn + 12 * e + 10 : b->small.dyn + 12 * e;
        d[e].derive_keys = 1;
        d[e].shared_noise_scale = covo_shared_noise_scale(params[e], mode != COVO_MODE_MPPI);  // (CoVO's rollouts are deterministic)
    }
    int rc = launch_update_arbiter(h, d, E, true, trace_index, s);  // first: the plan, the trace's u and the env step see its mean
    if (rc || arbiter_only) return rc;
    if ((rc = launch_plan_trace(h, d, E, true, states_true, trace_index, s))) return rc;
    return launch_sample_fan(h, d, E, true, trace_index, s);
}

// test hook: the factor(s) the LAST single (batched = 0) / env-batched step sampled from -- what the next reuse step of a Sigma period
// shifts -- device -> device
int covo_debug_sigma_factor_impl(covo_ctx *h, int batched, float *out, int64_t count, hipStream_t s)
{
    StepState *st = reinterpret_cast<StepState *>(h->step);
    BatchState *b = reinterpret_cast<BatchState *>(h->batch);
    const float *src = batched ? (b ? b->L : nullptr) : (st ? st->L : nullptr);
    const int64_t have = (int64_t)COVO_NA * COVO_NA * (batched ? (b ? b->n_envs : 0) : 1);
    if (src == nullptr || count > have) {
        covo_set_error("covo_debug_sigma_factor: no %s step has run on this handle, or count=%lld exceeds its %lld floats",
                       batched ? "batched" : "single", (long long)count, (long long)have);
        return COVO_E_BADARG;
    }
    COVO_CHECK_HIP(hipMemcpyAsync(out, src, (size_t)count * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}

// test hook: the Hessians of the LAST batched step (E x 128 x 128 doubles), device -> host
int covo_debug_batched_hessians_impl(covo_ctx *h, double *out, int64_t offset_doubles, int64_t count, hipStream_t s)
{
    BatchState *b = reinterpret_cast<BatchState *>(h->batch);
    if (b == nullptr || b->R == nullptr) {
        covo_set_error("covo_debug_batched_hessians: no batched step has run on this handle");
        return COVO_E_BADARG;
    }
    COVO_CHECK_HIP(hipMemcpyAsync(out, b->R + offset_doubles, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, s));
    return 0;
}
