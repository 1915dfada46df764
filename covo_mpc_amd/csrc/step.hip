// step.hip -- one C entry per MPC control step, replayed as a hipGraph.
//
// covo_mpc_step() enqueues everything quadjax's controller __call__ does between "shift the mean" and
// "new mean" (controllers/covo.py:201-275, mppi.py:43-125) for this rank's shard of samples on ONE
// stream, with no host work in between.  A control step is ~70 tiny launches for covo-online (the
// eigh-free Sigma pipeline alone is ~60); issued one by one from the host they leave ~150 us of gaps.
// The second call with the same buffers captures the sequence into a hipGraph, later calls replay it.
// Quantities that change every step (Philox key, MPPI's shared disturbance draw) live in a 32-byte
// device block refreshed by one async copy before each replay, so the captured kernel arguments stay valid.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "covo_common.hpp"
#include "eps_tiles.hpp"
#include "sym_stats.hpp"
#include "rng_device.hpp"
#include "step_begin.hpp"
#include "step_small.hpp"
#include "step_graph.hpp"

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

// ---- the covo-online chain of a step, single or env-batched: Hessian -> Sigma chain (epsilon drawn ahead, under its finalize launch)
// -> noise GEMM; a reuse step of a Sigma period: factor shift -> GEMM.  The single step is the batched one at E = 1 plus what only
// one matrix may have (sync, defer_cov, hess.begin).  A host-only view in the style of covo_common.hpp's descriptors: filled field by
// field at the two call sites (enqueue_step, batch_enqueue); a null / zero switches the feature off.
struct OnlineChainView {
    int E = 1;                    // instances
    uint32_t *dyn = nullptr;      // the per-step scalars; instance e's at dyn + e * dyn_stride ...
    int dyn_stride = 0;           // ... 0 (single) / 12
    int64_t sample_offset = 0;    // global id of local sample 0 (a sample-sharded single step)
    int N = 0;
    const float *mu = nullptr;    // [E][128] the shifted mean
    double *R = nullptr;          // [E][128][128] the Hessian
    float sample_sigma = 0.0f;
    float *Sigma = nullptr, *L = nullptr;  // [E][128][128] a_cov out and its factor
    float4 *eps_tiled = nullptr;  // the step's epsilon in tile order (eps_tiles.hpp), instance e's eps_stride float4 on; null: the
    size_t eps_stride = 0;        // GEMM draws in-kernel
    float *a = nullptr;           // [E][H][N][4] action stripes out
    // the caller's part of the Hessian's descriptor: state, trajectories, T, params, f_tab (the step's Hessian table, or null) and
    // begin (single) / consts_dev, models_dev, traj_stride (batch); enqueue_online_chain fills the rest
    HessianDesc hess;
    // epsilon is drawn ahead when ALL of these launch groups (DebugMasks::step) are selected -- 4 (single) / 4 | 8 (batch).  The masks
    // only differ inside the two phase timers, whose "Sigma alone" (mask 4) is not the same thing: covo_debug_time_step keeps the draw
    // under the finalize launch (bench.py's GEMM-as-its-own-launch figure is T(4 | 8) - T(4): the draw must be on both sides),
    // covo_debug_time_batched times the chain without passengers (bench.py --config envs lists sigma_us next to a mask-8 GEMM that
    // draws in-kernel).  Mask 4 is reachable from Python on both, so the two stay apart.
    int ahead_groups = 4;
    // one matrix only
    unsigned *sync = nullptr;     // the streamed finalize launch's flags: the GEMM may run inside the chain's last launch
    bool defer_cov = false;       // a_cov may be left to the GEMM's first workgroups (CovDeferred)
    // COVO_MODE_CMA: no Hessian and no Sigma chain ever -- Sigma and L come from the samples (enqueue_cma_sigma); `reuse` then says
    // "not the first step after a reset"
    bool cma = false;
};

// the Sigma of a CMA step (covo_set_step_cma), E instances: the first step after a reset writes the reset state --
// L = sigma0 I, a_cov = sigma0^2 I, p = 0, log s = 0, the neutral row; every later one runs the shape (sigma_adapt.hip as it is: the
// handle's L and the posterior covariance the previous step left, into the handle's second buffer and a_cov) and behind it the step
// size (cma_path.hip: path and log s from the previous step's displacement and ess; L' = s L_hat' back into L, a_cov scaled in place)
static int enqueue_cma_sigma(covo_ctx *h, const OnlineChainView &v, hipStream_t s, bool first)
{
    if (first) return launch_cma_reset(v.sample_sigma, v.E, v.L, v.Sigma, h->cma_p, covo_cma_log_s(h), h->cma_rows, s);
    int rc = launch_sigma_adapt(v.L, h->post_cov_out, v.E, h->cma_gamma, v.sample_sigma, v.Sigma, covo_cma_L_hat(h), covo_cma_shape_rows(h), s);
    if (rc) return rc;
    CmaPathDesc d;
    d.L_prev = v.L;
    d.aux = h->post_aux_out;
    d.ess = covo_diag_target(h);
    d.L_hat = covo_cma_L_hat(h);
    d.Sigma_hat = v.Sigma;
    d.shape_rows = covo_cma_shape_rows(h);
    d.batch = v.E;
    d.n_samples = v.N;
    d.step_size = h->cma_step_size;
    d.damping = (double)h->cma_damping;
    d.log_s_min = std::log((double)h->cma_s_min);
    d.log_s_max = std::log((double)h->cma_s_max);
    d.p = h->cma_p;
    d.log_s = covo_cma_log_s(h);
    d.L_out = v.L;
    d.Sigma_out = v.Sigma;
    d.rows_out = h->cma_rows;
    return launch_cma_path(d, s);
}

static int enqueue_online_chain(covo_ctx *h, const OnlineChainView &v, hipStream_t s, const DebugMasks &dbg, int pass, bool reuse)
{
    const int M = dbg.step;
    int rc;
    NoiseDesc nd;
    nd.L = v.L;
    nd.mu = v.mu;
    nd.dyn = v.dyn;
    nd.sample_offset = v.sample_offset;
    nd.N = v.N;
    nd.a = v.a;
    nd.batch = v.E;
    nd.propagate_nan = covo_propagate_nan(h);
    if (v.cma) {  // the samples are drawn as a reuse step draws them (in-kernel Philox); the later passes sample from the same L'
        if (pass == 0 && (rc = enqueue_cma_sigma(h, v, s, !reuse))) return rc;
        return launch_noise_gemm(nd, s);
    }
    if (reuse) {
        // a reuse step of a Sigma period: no Hessian, no Sigma chain -- every instance's factor of the previous step is shifted in
        // place (sigma_shift.hip), a_cov is its Sigma', and the samples are drawn from it as covo-offline draws from a table row
        // (in-kernel Philox); the later passes of an iterated step sample from the same L'.  Under covo_set_step_sigma_adapt the shift
        // also blends in the posterior covariance the previous step's after-step launches left in the attached target (sigma_adapt.hip)
        if (pass == 0) {
            rc = covo_sigma_adapt_on(h) ? launch_sigma_adapt(v.L, h->post_cov_out, v.E, h->adapt_gamma, v.sample_sigma, v.Sigma, v.L,
                                                             h->adapt_rows, s)
                                        : launch_sigma_shift(v.L, v.E, v.sample_sigma, v.Sigma, v.L, s);
            if (rc) return rc;
        }
        return launch_noise_gemm(nd, s);
    }
    // the Hessian's last launch leaves the Sigma chain's input statistics in the chain's workspace: no prep launch
    const bool stats = (M & 2) && (M & 4) && (dbg.hess & 15) == 15;
    const SymStatsOut so = sigma_ns_stats_out(h->ws_sigma, v.E);
    HessianDesc hd = v.hess;
    hd.a_mean = v.mu;
    hd.batch = v.E;
    hd.R = v.R;
    hd.stats = stats ? &so : nullptr;
    hd.status_dev = h->status_dev;
    if ((M & 2) && (rc = launch_hessian(hd, h->ws_hess, s, dbg))) return rc;  // :134-185
    if (covo_sigma_nodes_on(h)) {
        // covo_set_step_sigma_nodes: Sigma is the optimal covariance of the node-parameterised problem -- ONE launch of one workgroup
        // per instance (projection, eigendecomposition, factor, stage-space factor G, a_cov = P Sigma_M P^T; sigma_nodes.hip) in the
        // place of the Sigma chain, and the dense-factor sampler in the place of the GEMM: no finalize launch, no epsilon drawn
        // ahead, nothing deferred or streamed
        if ((M & 4) && (rc = launch_sigma_nodes(v.R, v.E, h->sn_W, h->sn_M, v.sample_sigma, h->sn_SigmaM, h->sn_G, v.Sigma, h->sn_rows, s)))
            return rc;
        return (M & 8) ? launch_noise_factor(nd, h->sn_G, h->sn_M, s) : 0;
    }
    const bool finalize = dbg.sigma_stages >= 4;
    // epsilon needs only the act keys: it is drawn under the chain's finalize launch (one workgroup per matrix factors), the GEMM loads
    // it -- the in-kernel Philox costs the batched GEMM ~9 us, its matrix pipe hides no vector work
    const bool ahead = v.eps_tiled != nullptr && (M & v.ahead_groups) == v.ahead_groups && finalize;
    EpsGenArgs gen;
    gen.eps_tiled = ahead ? v.eps_tiled : nullptr;
    gen.dyn = v.dyn;
    gen.sample_offset = v.sample_offset;
    gen.N = v.N;
    gen.n_inst = v.E;
    gen.dyn_stride = v.dyn_stride;
    gen.eps_stride = v.eps_stride;
    // a_cov is written by the GEMM's first workgroups, not by the chain's one-workgroup finalize launch (CovDeferred)
    CovDeferred cov;
    std::memset(&cov, 0, sizeof(cov));
    const bool defer = v.defer_cov && (M & 8) && finalize;
    // the GEMM streamed under the factorisation, inside the chain's last launch (one matrix, persistent launches allowed)
    StreamGemmArgs sg;
    sg.mu = v.mu;
    sg.dyn = v.dyn;
    sg.sample_offset = v.sample_offset;
    sg.N = v.N;
    sg.a_out = v.a;
    sg.L_stream = v.L;
    sg.sync = v.sync;
    sg.a_cov_out = v.Sigma;
    sg.nanp = covo_propagate_nan(h) ? 1 : 0;
    const bool want_stream = v.sync != nullptr && h->opt.stream_gemm && (M & 4) && (M & 8) && finalize;
    bool streamed = false;
    SigmaNsDesc sd;
    sd.R = v.R;
    sd.batch = v.E;
    sd.sample_sigma = v.sample_sigma;
    sd.Sigma = v.Sigma;
    sd.L = v.L;
    sd.gen = &gen;
    sd.status = h->status_dev;
    sd.persistent_ok = (h->cfg.flags & COVO_FLAG_SHARED_DEVICE) == 0;
    sd.cov = defer ? &cov : nullptr;
    sd.r_has_stats = stats;
    sd.stream = want_stream ? &sg : nullptr;
    sd.streamed = &streamed;
    if ((M & 4) && (rc = launch_sigma_ns(h->opt, sd, h->ws_sigma, s, dbg))) return rc;
    nd.eps = ahead ? reinterpret_cast<const float *>(v.eps_tiled) : nullptr;  // (else the GEMM draws from v.dyn)
    nd.eps_tiled = ahead;
    nd.cov = v.defer_cov ? &cov : nullptr;
    return (!streamed && (M & 8)) ? launch_noise_gemm(nd, s) : 0;
}

// ---- one description of a step's rollout and update, single or env-batched.  BatchInst: the buffers of one instance (the single
// step's own; instance e of a batched step's argument block)
struct BatchInst {
    const float *state, *pos_traj, *vel_traj;
    float *a_mean, *a, *cost, *groupmin;
};
// Do the rollout's G workgroups leave the softmax update's stage-1 records themselves (rollout.hip: rollout_record)?  When they fit the
// merge; never with MPPI's covariance adaptation (second moments: its own stage 1, reduce.hip) or a staged update (ESS floor, elite
// set: weights that exist only after the costs).  Asked by the two builders below and nobody else: they must agree, or the merge reads
// records nobody wrote.
static bool rollout_leaves_records(const covo_ctx *h, int G, bool cov_adapt)
{
    return G <= h->max_red_blocks && !cov_adapt && !covo_update_staged(h);
}
// one instance's rollout on G workgroups; records / diag_rec (null: no diagnostics): where they would leave their records.  The
// caller adds xcd_groups (the single step: its position statistics)
static RolloutDesc rollout_desc(const covo_ctx *h, const BatchInst &i, int T, int N, const covo_env_params *params,
                                const float *f_shared_dev, const float *f_tab, int G, bool cov_adapt, float *records, float *diag_rec)
{
    const bool rec = rollout_leaves_records(h, G, cov_adapt);
    RolloutDesc ro;
    ro.state = i.state;
    ro.pos_traj = i.pos_traj;
    ro.vel_traj = i.vel_traj;
    ro.T = T;
    ro.params = params;
    ro.f_shared_dev = f_shared_dev;
    ro.f_tab = f_tab;
    ro.a = i.a;
    ro.N = N;
    ro.discount = h->cfg.discount;
    ro.cost = i.cost;
    ro.groupmin = rec ? nullptr : i.groupmin;
    ro.records = rec ? records : nullptr;
    ro.lam = h->cfg.lam;
    ro.diag_rec = rec ? diag_rec : nullptr;
    ro.clip = ROLLOUT_CLIP_TRUSTED;  // a comes straight from the noise kernels
    return ro;
}
// the update behind that rollout (records: it left u.up.partials).  i: the single step's buffers / instance 0's of a batch (dense
// slices); the caller adds its layout (batch_update_desc) and, under cov_adapt, gamma_sigma != 0 with a_cov_old / a_cov_out
struct StepUpdate {
    UpdateDesc up;
    bool records;
    int pass;  // of an iterated step: the annealed step's solver files its row under it
};
static StepUpdate update_desc(const covo_ctx *h, const BatchInst &i, int N, int G, bool cov_adapt, const float *partials,
                              const float *a_mean_old, float gamma_mean, float *diag_rec, float *diag_out, float *iter_out, int pass)
{
    StepUpdate u;
    u.records = rollout_leaves_records(h, G, cov_adapt);
    u.pass = pass;
    u.up.cost = i.cost;
    u.up.a = i.a;
    u.up.N = N;
    u.up.blockmin = i.groupmin;
    u.up.partials = partials;  // (the rollout's records, if it left them)
    u.up.G = G;
    u.up.a_mean_old = a_mean_old;
    u.up.gamma_mean = gamma_mean;
    u.up.a_mean_out = i.a_mean;
    u.up.diag_rec = diag_rec;
    u.up.diag_out = diag_out;
    u.up.iter_out = iter_out;
    return u;
}

// adds the targets of the staged updates and runs: the ESS floor's solver (rollout costs + per-wave minima -> 1 / lam_eff in lam_rows),
// in its place the annealed step's standardising solver (costs -> the same row, and again under the pass in the per-pass rows), or the
// elite selector (costs -> 0/1 weights off elite_rows) when attached -- never two of them (refused at the C boundary) --, then the ONE
// update launch set
static int enqueue_update(covo_ctx *h, StepUpdate &u, hipStream_t s)
{
    UpdateDesc &up = u.up;
    int rc;
    float *lam_rows = covo_lam_target(h), *elite_rows = covo_elite_target(h);
    up.n_blockmin = (up.N + 63) / 64;
    up.lam_rows = lam_rows;
    up.elite_rows = elite_rows;
    if (lam_rows != nullptr && covo_ess_on(h) &&
        (rc = launch_ess_lambda(up.cost, up.N, up.batch, up.blockmin, h->cfg.lam, h->ess_min, lam_rows, s))) return rc;
    if (lam_rows != nullptr && !covo_ess_on(h) &&
        (rc = launch_cost_standardise(up.cost, up.N, up.batch, h->cfg.lam, h->anneal_temp, lam_rows,
                                      h->anneal_rows ? h->anneal_rows + (size_t)u.pass * COVO_LAM_FLOATS : nullptr,
                                      h->anneal_passes * COVO_LAM_FLOATS, s))) return rc;
    if (elite_rows != nullptr && (rc = launch_elite_select(up.cost, up.N, up.batch, h->elite_K, elite_rows, s))) return rc;
    if (up.gamma_sigma != 0.0f) return elite_rows != nullptr ? launch_elite_update_cov(h, up, s) : launch_softmax_update_cov(h, up, s);
    if (elite_rows != nullptr) return launch_elite_reduce(h, up, s);
    return u.records ? launch_merge(up, h->cfg.lam, s) : launch_softmax_reduce(h, up, s);
}

// the launch sequence of one pass of a single step (everything reads per-step scalars from st->dyn)
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
    if (M == 63 && step_takes_small(h, p, a))
        return launch_step_small(h, p, a, state, am_shift, nullptr, st->dyn, 0.0f, st->ticket, s, pass, nullptr, iter_out);
    // periodic / sin / drag / mixed (free.py:10-58): the wave-uniform part of every rollout step's force, for the sampling
    // rollouts (shared step key) and for the Hessian's deterministic rollout (per-step keys), resolved once per control step
    const bool tables = covo_needs_tables(p);
    if (tables && (rc = launch_disturb_tables_step(p, state, st->dyn, a.rollout_deterministic, st->f_tab_rollout,
                                                   (a.mode == COVO_MODE_COVO_ONLINE && !reuse) ? st->f_tab_hess : nullptr, s))) return rc;
    if (a.mode == COVO_MODE_COVO_ONLINE || a.mode == COVO_MODE_CMA) {
        OnlineChainView v;
        v.cma = a.mode == COVO_MODE_CMA;
        v.dyn = st->dyn;
        v.sample_offset = a.sample_offset;
        v.N = N;
        v.mu = am_shift;
        v.R = st->R;
        v.sample_sigma = a.sample_sigma;
        v.Sigma = a.a_cov ? a.a_cov : st->Sigma;
        v.L = st->L;
        v.eps_tiled = st->eps_tiled;
        v.a = a.a;
        v.hess.state = state;
        v.hess.pos_traj = a.pos_traj;
        v.hess.vel_traj = a.vel_traj;
        v.hess.T = a.T;
        v.hess.params = &p;
        v.hess.f_tab = tables ? st->f_tab_hess : nullptr;
        v.hess.begin = begin;
        v.sync = st->sync;
        v.defer_cov = true;
        if ((rc = enqueue_online_chain(h, v, s, dbg, pass, reuse))) return rc;
    } else {
        // a = clip(am_shift + L eps), epsilon drawn in-kernel from the step's key in st->dyn
        NoiseDesc nd;
        nd.mu = am_shift;
        nd.dyn = st->dyn;
        nd.sample_offset = a.sample_offset;
        nd.N = N;
        nd.a = a.a;
        nd.propagate_nan = covo_propagate_nan(h);
        if (a.mode == COVO_MODE_COVO_OFFLINE) {
            nd.L = a.L_table;
            nd.state_for_time = state;
            nd.n_table = a.n_table;
            if ((M & 8) && (rc = launch_noise_gemm(nd, s))) return rc;
        } else {  // MPPI: shift a_cov, factor the 4x4 blocks, per-step draws (mppi.py:43-66)
            nd.L = st->Ls;  // (a_cov was shifted and factored there by the begin launch)
            // covo_set_step_anneal: this pass's row of the schedule replaces both -- a_cov on input is ignored
            if (covo_anneal_sched_on(h) && (rc = launch_anneal_schedule(h->anneal_table, pass, st->Ls, a.a_cov, 1, s))) return rc;
            // covo_set_step_nodes: the pass's perturbations are splines over its nodes (the schedule above was fed their marginals)
            if (covo_nodes_on(h)) { if ((rc = launch_noise_nodes(nd, h->nodes_table, pass, h->nodes_M, s))) return rc; }
            else if ((rc = launch_noise_blockdiag(nd, s))) return rc;
        }
    }
    // the rollout's workgroups leave the softmax update's stage-1 records themselves when they may (rollout_leaves_records); otherwise
    // the stand-alone stage-1 kernel runs over the costs
    const int G = rollout_workgroups(N, a.pos_stats != nullptr);
    const bool cov_adapt = a.mode == COVO_MODE_MPPI && a.gamma_sigma != 0.0f;
    // the step's sampling diagnostics (covo_set_step_diag): the diagnostic variants of the same launches; a sharded step has none
    float *dg = a.partial_out == nullptr ? covo_diag_target(h) : nullptr;
    const BatchInst inst = {state, a.pos_traj, a.vel_traj, a.a_mean, a.a, a.cost, a.groupmin};
    RolloutDesc ro = rollout_desc(h, inst, a.T, N, &p, fdev, tables ? st->f_tab_rollout : nullptr, G, cov_adapt, h->ws_partials,
                                  dg ? h->ws_diag_rec : nullptr);
    ro.pos_stats = a.pos_stats;
    ro.stats_ws = h->ws_stats;
    ro.xcd_groups = a.mode == COVO_MODE_MPPI ? 4 : 0;  // MPPI's block-diagonal kernel: 256 samples per workgroup
    if ((M & 16) && (rc = launch_rollout(ro, s))) return rc;
    if (!(M & 32)) return 0;
    // weights + update: finish locally (blend with am_shift, diagnostics), or -- a sample-sharded rank -- leave this shard's
    // record for the all-gather (covo.py:266-275)
    StepUpdate u = update_desc(h, inst, N, G, cov_adapt, h->ws_partials, am_shift, a.gamma_mean, h->ws_diag_rec, dg, iter_out, pass);
    const bool sharded = a.partial_out != nullptr;
    if (sharded) {
        u.up.partial_out = a.partial_out;
        u.up.a_mean_out = nullptr;
        u.up.iter_out = nullptr;
    }
    if (cov_adapt) {  // mppi.py:109-125: new mean, then a_cov (already shifted by the begin launch) adapted in place; a sharded
                      // rank: its record with the second moments (836-float kind)
        u.up.a_cov_old = a.a_cov;
        u.up.gamma_sigma = a.gamma_sigma;
        u.up.a_cov_out = sharded ? nullptr : a.a_cov;
    }
    return enqueue_update(h, u, s);
}

// a debug setter since the last step changed what a captured graph baked in (launch set, deflation switch, diagnostics target)
static void step_sync_epoch(covo_ctx *h)
{
    if (h->dbg_epoch == h->opt.epoch) return;
    step_graphs_drop(h);
    h->dbg_epoch = h->opt.epoch;
}

// the launches of step_begin_kernel: a step's first pass (eager, ahead of the graph; a_mean_in: the caller's input mean of this call, else
// the handle's own carried one), pass >= 1 of an iterated step (inside the graph: the mean the previous pass committed, the raw key
// walked on the device -- blk is not read), the phase timer's scratch fill.  mppi_cov: MPPI's a_cov, shifted and factored here
static void launch_step_begin(StepState *st, const covo_step_args &a, const DynBlock &blk, float shared_noise_scale, float *mppi_cov,
                              int pass, hipStream_t s)
{
    hipLaunchKernelGGL(step_begin_kernel, dim3(1), dim3(COVO_NA + COVO_STATE_FLOATS + 4), 0, s,
                       (pass == 0 && a.a_mean_in) ? a.a_mean_in : (const float *)a.a_mean,
                       a.a_mean_shift ? a.a_mean_shift : st->a_mean_shift, st->dyn, st->state_buf, pass ? 1 : a.derive_keys,
                       shared_noise_scale, blk, mppi_cov, st->Ls, st->sync, pass);
}

// reuse: a reuse step of a Sigma period (covo_set_step_sigma_period): the chain's reuse form, with a graph of its own
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
    const bool small = step_takes_small(h, *params, *args);
    // covo_set_step_iters: pass j >= 1 starts from the mean pass j - 1 committed (args->a_mean, never the caller's a_mean_in) and
    // walks the raw key on the device; the update arbiter's launch between two passes (step_run_passes)
    const int K = covo_step_iters(h);
    auto between = [&](hipStream_t on, int) { return covo_plan_after_step(h, AFTER_BETWEEN, params, args, key0, key1, f_shared, nullptr, -1, on); };
    const char *name = "covo_mpc_step";
    switch (step_form(h, small, *params, *args, reuse)) {
    case STEP_ONE_LAUNCH: {
        // the WHOLE step is one launch, the begin launch's work included (per workgroup, step_small.hip).  An iterated step: the
        // last workgroup of every pass parks the pass's raw key at st->dyn[10..11] for the next one
        covo_step_args later = *args;
        later.a_mean_in = nullptr;
        float *am_shift = args->a_mean_shift ? args->a_mean_shift : st->a_mean_shift;
        return step_run_passes(h, st->cache, false, false, s, name, [&](hipStream_t on, int j) {
            return launch_step_small(h, *params, j ? later : *args, args->state, am_shift, &blk, nullptr, shared_noise_scale, st->ticket,
                                     on, j, K > 1 ? st->dyn + 10 : nullptr, covo_iter_slot(h, j));
        }, between);
    }
    case STEP_FOLDED_ONLINE:
        // the begin work rides in the Hessian's first launch -- one launch boundary less
        return step_run_passes(h, st->cache, false, false, s, name, [&](hipStream_t on, int j) {
            HessBegin hb;
            hb.pass = j;
            hb.a_mean_raw = j ? args->a_mean : (args->a_mean_in ? args->a_mean_in : args->a_mean);
            hb.dyn_out = st->dyn;
            hb.seq = st->sync;
            hb.blk = &blk;
            hb.derive_keys = args->derive_keys;
            hb.shared_noise_scale = shared_noise_scale;
            return enqueue_step(h, st, *params, *args, on, DebugMasks(), &hb, args->state, j);
        }, between);
    case STEP_BEGIN_PASSES:
        break;
    }
    float *mppi_cov = (args->mode == COVO_MODE_MPPI && !small) ? args->a_cov : (float *)nullptr;
    launch_step_begin(st, *args, blk, shared_noise_scale, mppi_cov, 0, s);
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
    const bool same = graph_cache_seen(cache, std::memcmp(&k, &key, sizeof(k)) == 0);
    if (!same) key = k;
    // the passes behind the begin launch: pass j >= 1 starts with a begin launch of its own, inside the graph
    return step_run_passes(h, st->cache, reuse, same, s, name, [&](hipStream_t on, int j) {
        if (j > 0) launch_step_begin(st, *args, DynBlock(), shared_noise_scale, mppi_cov, j, on);
        return enqueue_step(h, st, *params, *args, on, DebugMasks(), nullptr, nullptr, j, reuse);
    }, between);
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
    const bool online = args->mode == COVO_MODE_COVO_ONLINE, cma = args->mode == COVO_MODE_CMA;
    // (a CMA step keeps its factor in st->L too: a covo-online step between two of them makes the next one a first step)
    const int age = online ? covo_sigma_step_age(h, st->L, args->sample_sigma, 1) : cma ? covo_cma_step_age(h, st->L, args->sample_sigma, 1) : 0;
    int rc = step_enqueue_all(h, st, params, args, key0, key1, f_shared, s, age != 0);
    if (rc == 0 && online) covo_sigma_step_done(h, age, st->L, args->sample_sigma, 1), h->cma_age = 0;
    if (rc == 0 && cma) covo_cma_step_done(h, st->L, args->sample_sigma, 1);
    if (rc == 0 && online && age == 0 && covo_sigma_adapt_on(h)) rc = launch_sigma_adapt_idle(h->adapt_rows, 1, s);  // (eager, behind the step)
    return rc;
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
    if (step_form(h, step_takes_small(h, *params, *args), *params, *args, false) != STEP_BEGIN_PASSES && args->state != nullptr) {
        // the last step ran without a begin launch (the one-launch small step; covo-online with the begin work folded into the
        // Hessian) and never filled the scratch the replayed launches read (state copy, shifted mean, keys; MPPI: shifted
        // covariance + block factors): one begin launch does, with the key the step would derive from (0, 0)
        DynBlock blk;
        std::memset(&blk, 0, sizeof(blk));
        std::memcpy(&blk.w[8], &args->state, sizeof(const float *));
        launch_step_begin(st, *args, blk, 0.0f, args->mode == COVO_MODE_MPPI ? args->a_cov : (float *)nullptr, 0, run);
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
__global__ void hold_park_keys_kernel(uint32_t *__restrict__ dyn, const BatchDyn b, int n)
{
    const int i = threadIdx.x;
    if (i < 2 * n) dyn[12 * (i >> 1) + 10 + (i & 1)] = b.w[i >> 1][2 + (i & 1)];
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

// the begin launch of the env-batched steps with launches of their own (covo-online; MPPI / covo-offline under
// covo_set_step_batched_staged): per instance what step_begin_kernel does for one -- shift the mean (pass 0; covo.py:201-203), the
// step's scalars through step_begin_derive / _next from the instance's raw key (dyn[12 e + 0..1] as uploaded; pass >= 1: the previous
// pass's at [10..11]) with its own shared_noise_scale: act_key to [0..1] (covo.py:212), MPPI's shared gaussian vector to [2..4] (scale
// 0, CoVO's deterministic rollouts: zero bits), the raw key to [10..11]; MPPI (mppi_cov != null): shift (pass 0) + factor a_cov[e] into Ls[e]
struct BatchScales {
    float v[COVO_MAX_ENVS];  // instance e's covo_shared_noise_scale
};
__global__ void batch_mode_begin_kernel(const float *__restrict__ a_mean, float *__restrict__ a_mean_shift, uint32_t *__restrict__ dyn,
                                        const BatchScales scales, float *__restrict__ mppi_cov, float *__restrict__ mppi_Ls, const int pass)
{
    const int e = blockIdx.x, i = threadIdx.x;  // 128 + 64 threads
    uint32_t *d = dyn + 12 * e;
    if (mppi_cov != nullptr) mppi_prep(mppi_cov + (size_t)e * COVO_H * 16, mppi_Ls + (size_t)e * COVO_H * 16, pass == 0);
    const uint32_t p0 = d[pass ? 10 : 0], p1 = d[pass ? 11 : 1];  // every deriving thread holds the key before any of them stores
    __syncthreads();
    if (i < COVO_NA) {
        a_mean_shift[e * COVO_NA + i] = (pass == 0 && i < COVO_NA - COVO_DU) ? a_mean[e * COVO_NA + i + COVO_DU] : a_mean[e * COVO_NA + i];
    } else if (i < COVO_NA + 4) {
        const int q = i - COVO_NA;
        if (pass) {
            uint32_t raw[2];
            step_begin_derive_next(q, p0, p1, scales.v[e], d, raw);
        } else {
            DynBlock blk;
#pragma unroll
            for (int w = 0; w < 12; ++w) blk.w[w] = 0u;
            blk.w[0] = p0;
            blk.w[1] = p1;
            step_begin_derive(q, blk, 1, scales.v[e], d);
        }
    }
}

// the env-batched MPPI / covo-offline step (covo_mpc_step_batched_mode): ONE fused launch for all instances (step_small.hip,
// grid = groups x instances) behind the key upload; scratch and graph cache of its own, next to the staged batches'
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

// What an env-batched step with launches of its own keeps (begin | tables | sampling | rollout | update for all instances per pass, one
// linear stream): their scratch and the graphs over them.  BatchState holds TWO -- covo-online's (covo_mpc_step_batched) and the staged
// MPPI / covo-offline step's (covo_set_step_batched_staged) --: a handle stepped alternately through both keeps either's scratch and graphs
struct BatchCommon {
    int n_envs = 0;                 // the instance count the device arrays were allocated for
    uint32_t *dyn = nullptr;        // [E][12] the instances' per-step scalars (batch_set_dyn_kernel, batch_mode_begin_kernel)
    float *a_mean_shift = nullptr;  // [E][128]
    void *ro_args = nullptr;        // RolloutArgs[E]          (rollout)
    float *partials = nullptr;      // [E][max_red_blocks][COVO_PARTIAL_FLOATS]: the instances' softmax stage-1 records
    float *diag_rec = nullptr;      // [E][max_red_blocks][4]: their diagnostic records (covo_set_step_diag)
    void *models = nullptr;         // dm::Model[E]            (disturbance tables, drag / mixed Hessian)
    float *tab_rollout = nullptr;   // [E][H][4] the step's disturbance tables of the sampling rollouts (periodic / sin / drag / mixed)
    bool tables = false;            // the instances' disturbance model needs them
    std::vector<char> ro_args_host;
    std::vector<covo_env_params> params;
    // with `stream` and `params`: what scratch, argument blocks and graphs were built for, while have_key (covo-online: `base` and
    // mode = COVO_MODE_COVO_ONLINE in a zeroed struct)
    covo_batch_mode_args key;
    hipStream_t stream = nullptr;
    bool have_key = false;
    GraphCache cache[2] = {};  // [0] the step, [1] the reuse step of a Sigma period (covo-online only), as in StepState; both keyed by `key`
    // (the key with the graphs: the rollout's argument blocks, which the cold block rebuilds, bake the launch set in as they do)
    void forget() { cache[0].forget(), cache[1].forget(), have_key = false; }
    void record(const covo_batch_mode_args &m, hipStream_t s) { key = m, stream = s, have_key = true; }
};
static void batch_common_free(BatchCommon *c)
{
    c->forget();
    free_and_null(c->dyn, c->a_mean_shift, c->ro_args, c->partials, c->diag_rec, c->models, c->tab_rollout);
    c->n_envs = 0;
}

// what the staged MPPI / covo-offline batch keeps next to its BatchCommon
struct BatchStagedExtras {
    float *Ls = nullptr;            // [E][H][4][4] MPPI's block factors
    float *diag_merge = nullptr;    // [E][COVO_PARTIAL_FLOATS]: the merged records the covariance update's diagnostics merge leaves
    float *partials_cov = nullptr;  // [E][stage-1 grid][452]: MPPI's covariance adaptation; only ever grows
    size_t partials_cov_cap = 0;
    BatchScales scales;             // the instances' shared_noise_scale (the begin launch's kernel argument)
};

struct BatchState {
    BatchSmall small;
    BatchCommon online, staged;
    BatchStagedExtras sx;
    // covo-online's own
    double *R = nullptr;            // [E][128][128]
    float *Sigma = nullptr, *L = nullptr;  // [E][128][128]
    void *consts = nullptr;         // qm::Consts<double>[E]   (Hessian)
    float *tab_hess = nullptr;      // [E][H][4] the Hessian's disturbance tables
    float4 *eps_tiled = nullptr;    // [E][ceil(N/32)][16][64]: the step's epsilon of every instance, drawn under the Sigma chain's
    size_t eps_cap = 0;             // finalize launch (eps_tiles.hpp), as in the single step; only ever grows
    void *env_inst = nullptr;       // EnvInst[env_inst_n] (env_step.hip): the per-instance constants of covo_env_step_batched
    int env_inst_n = 0;
    std::vector<covo_env_params> env_inst_params;
};

// The captured graphs (fused step, env-batched steps) hold the addresses of h->ws_sigma / h->ws_hess in their kernel nodes and bake
// the handle's launch set in: whoever re-allocates a workspace (covo_grow_workspace) or meets a moved debug epoch calls this
// first, so that a later step re-captures instead of replaying launches that point into freed memory.
void step_graphs_drop(covo_ctx *h)
{
    StepState *st = reinterpret_cast<StepState *>(h->step);
    BatchState *b = reinterpret_cast<BatchState *>(h->batch);
    if (st) st->forget_graphs();
    if (!b) return;
    b->online.forget();
    b->staged.forget();
    b->small.cache.forget();
}

// a device array that only ever grows: at least `need` elements
template <class T>
static int grow_device(T *&p, size_t &cap, size_t need)
{
    if (need <= cap) return 0;
    free_and_null(p);
    cap = 0;
    COVO_CHECK_HIP(hipMalloc(&p, need * sizeof(T)));
    cap = need;
    return 0;
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

// (eps_tiled and env_inst outlive a change of the instance count: see covo_step_batched_impl)
void batch_state_destroy(covo_ctx *h)
{
    BatchState *b = reinterpret_cast<BatchState *>(h->batch);
    if (!b) return;
    batch_common_free(&b->online);
    batch_common_free(&b->staged);
    batch_small_free(&b->small);
    free_and_null(b->R, b->Sigma, b->L, b->consts, b->tab_hess, b->eps_tiled, b->env_inst, b->sx.Ls, b->sx.diag_merge, b->sx.partials_cov);
    delete b;
    h->batch = nullptr;
}

// a batch's update: instance e's records are [e][G] of c.partials; row e of the diagnostic buffer, of the solver's / the selector's
// output and of iter_log ([e][pass]) is instance e's
static StepUpdate batch_update_desc(const covo_ctx *h, const BatchCommon &c, const covo_batch_args &a, int pass, bool cov_adapt)
{
    StepUpdate u = update_desc(h, batch_inst(a, 0), a.n_samples, rollout_workgroups(a.n_samples, false, a.n_envs), cov_adapt, c.partials,
                               c.a_mean_shift, a.gamma_mean, c.diag_rec, covo_diag_target(h), covo_iter_slot(h, pass), pass);
    u.up.partials_ws = c.partials;
    u.up.batch = a.n_envs;
    u.up.iter_stride = covo_step_iters(h);
    return u;
}

// does the key an env-batched scratch was built for (valid: it has one) describe this call?
static bool batch_key_same(bool valid, const covo_batch_mode_args &key, hipStream_t stream, const std::vector<covo_env_params> &have,
                           const covo_batch_mode_args &m, const covo_env_params *params, hipStream_t s)
{
    const size_t E = (size_t)m.base.n_envs;
    return valid && std::memcmp(&key, &m, sizeof(m)) == 0 && stream == s && have.size() == E &&
           std::memcmp(have.data(), params, E * sizeof(covo_env_params)) == 0;
}

// ---- the cold block of both batches: new buffers / parameters / instance count (outside the steady state).  What differs:
struct BatchColdDiff {
    int xcd_groups;       // RolloutDesc::xcd_groups: 4 behind MPPI's block-diagonal kernel (as the single step tells its rollout), else 0
    bool cov_adapt;       // MPPI's covariance adaptation rules the in-rollout records out
    bool deterministic;   // the sampling rollouts' (covo.py:231 / mppi.py:74): with params[e] instance e's shared_noise_scale ...
    BatchScales *scales;  // ... which goes here (null: not wanted)
};
// *same: nothing changed.  Else stale graphs are dropped, the scratch is (re)allocated on a new E and filled, and the key stays unset:
// the caller adds its own allocations and ends with c->record()
static int batch_cold(covo_ctx *h, BatchCommon *c, const covo_batch_mode_args &m, const covo_env_params *params, hipStream_t s,
                      const BatchColdDiff &d, bool *same)
{
    const covo_batch_args &a = m.base;
    const int E = a.n_envs, N = a.n_samples;
    if ((*same = batch_key_same(c->have_key, c->key, c->stream, c->params, m, params, s))) return 0;
    COVO_CHECK_HIP(hipStreamSynchronize(s));  // launches that read the old argument blocks are done
    c->forget();
    if (c->n_envs != E) {
        batch_common_free(c);
        COVO_CHECK_HIP(hipMalloc(&c->dyn, (size_t)E * 12 * sizeof(uint32_t)));
        COVO_CHECK_HIP(hipMalloc(&c->a_mean_shift, (size_t)E * COVO_NA * sizeof(float)));
        COVO_CHECK_HIP(hipMalloc(&c->ro_args, rollout_args_bytes(E)));
        COVO_CHECK_HIP(hipMalloc(&c->partials, (size_t)E * h->max_red_blocks * COVO_PARTIAL_FLOATS * sizeof(float)));
        COVO_CHECK_HIP(hipMalloc(&c->diag_rec, (size_t)E * h->max_red_blocks * 4 * sizeof(float)));
        COVO_CHECK_HIP(hipMalloc(&c->models, disturb_models_bytes(E)));
        COVO_CHECK_HIP(hipMalloc(&c->tab_rollout, (size_t)E * COVO_H * 4 * sizeof(float)));
        c->n_envs = E;
    }
    c->params.assign(params, params + E);
    std::vector<char> tmp(disturb_models_bytes(E), 0);
    disturb_fill_models(params, E, tmp.data());
    COVO_CHECK_HIP(hipMemcpy(c->models, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
    c->tables = covo_needs_tables(params[0]);
    c->ro_args_host.assign(rollout_args_bytes(E), 0);
    const int G = rollout_workgroups(N, false, E);
    if (d.scales) std::memset(d.scales, 0, sizeof(*d.scales));
    for (int e = 0; e < E; ++e) {
        if (d.scales) d.scales->v[e] = covo_shared_noise_scale(params[e], d.deterministic);
        // (f_shared_dev: MPPI's own shared vector of the instance, as the begin launch leaves it)
        RolloutDesc ro = rollout_desc(h, batch_inst(a, e), a.T, N, &params[e], reinterpret_cast<const float *>(c->dyn + 12 * e + 2),
                                      c->tables ? c->tab_rollout + (size_t)e * COVO_H * 4 : nullptr, G, d.cov_adapt,
                                      c->partials + (size_t)e * G * COVO_PARTIAL_FLOATS,
                                      covo_diag_target(h) ? c->diag_rec + (size_t)e * G * 4 : nullptr);
        ro.xcd_groups = d.xcd_groups;
        rollout_fill_args(c->ro_args_host.data(), e, ro);
    }
    COVO_CHECK_HIP(hipMemcpy(c->ro_args, c->ro_args_host.data(), c->ro_args_host.size(), hipMemcpyHostToDevice));
    return 0;
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
    const BatchCommon &c = b->online;
    const int E = a.n_envs, N = a.n_samples;
    const int M = dbg.step;  // 63 outside covo_debug_time_batched (which replays selected launch groups)
    int rc;
    // covo.py:231: CoVO's sampling rollouts run step_env(deterministic=True): no shared vector (every scale 0), no covariance blocks
    if (M & 1)
        hipLaunchKernelGGL(batch_mode_begin_kernel, dim3(E), dim3(COVO_NA + 64), 0, s, a.a_mean, c.a_mean_shift, c.dyn, BatchScales(),
                           (float *)nullptr, (float *)nullptr, pass);
    // get_hessian is deterministic likewise (covo.py:152)
    if ((M & 1) && c.tables && (rc = launch_disturb_tables_batched(c.models, a.states, c.dyn, E, 1, c.tab_rollout, b->tab_hess, s)))
        return rc;
    OnlineChainView v;
    v.E = E;
    v.dyn = c.dyn;
    v.dyn_stride = 12;
    v.N = N;
    v.mu = c.a_mean_shift;
    v.R = b->R;
    v.sample_sigma = a.sample_sigma;
    v.Sigma = a.a_cov ? a.a_cov : b->Sigma;
    v.L = b->L;
    v.eps_tiled = b->eps_tiled;
    v.eps_stride = (size_t)((N + 31) / 32) * 16 * 64;
    v.a = a.a;
    v.hess.state = a.states;
    v.hess.pos_traj = a.pos_traj;
    v.hess.vel_traj = a.vel_traj;
    v.hess.T = a.T;
    v.hess.params = &c.params[0];
    v.hess.consts_dev = b->consts;
    v.hess.traj_stride = (size_t)a.T * 3;
    v.hess.f_tab = c.tables ? b->tab_hess : nullptr;
    v.hess.models_dev = c.models;
    v.ahead_groups = 4 | 8;
    v.cma = c.key.mode == COVO_MODE_CMA;  // (the cold block keys the scratch by the mode)
    if ((rc = enqueue_online_chain(h, v, s, dbg, pass, reuse))) return rc;
    if ((M & 16) && (rc = launch_rollout_batched(c.ro_args_host.data(), c.ro_args, E, s))) return rc;
    if (!(M & 32)) return 0;
    StepUpdate u = batch_update_desc(h, c, a, pass, false);
    return enqueue_update(h, u, s);
}

// profiling aid (bench.py --config envs): `reps` copies of the selected launch groups of the LAST covo_mpc_step_batched call in
// one graph; GPU microseconds per copy.  step_mask as in covo_debug_time_step (1 begin, 2 Hessian, 4 Sigma, 8 GEMM, 16 rollout,
// 32 update).  The copies re-read the same means and states (the begin launch is normally left out: it would re-split the keys).
int covo_debug_time_batched_impl(covo_ctx *h, int step_mask, int reps, float *us_out, hipStream_t run)
{
    BatchState *b = reinterpret_cast<BatchState *>(h->batch);
    if (!b || !b->online.have_key) {
        covo_set_error("covo_debug_time_batched: call covo_mpc_step_batched first");
        return COVO_E_BADARG;
    }
    if (b->online.key.mode == COVO_MODE_CMA) {  // (the scratch's last step: every replayed copy would rewrite the factors, paths and rows)
        covo_set_error("covo_debug_time_batched: the phase timers replay a step without its state; a CMA step (COVO_MODE_CMA) would "
                       "adapt its covariance once per copy");
        return COVO_E_BADARG;
    }
    COVO_CHECK_HIP(hipStreamSynchronize(run));
    DebugMasks dbg;
    dbg.step = step_mask;
    return time_graph_replays(h, run, reps, us_out, [&](hipStream_t cs) { return batch_enqueue(h, b, b->online.key.base, cs, dbg); });
}

// the cold block of the batches that carry per-instance Hessian constants -- covo-online's and the iLQR step's, which share b->online
// (keyed by `mode`: a handle stepped alternately through both rebuilds, as one stepped through two argument blocks does)
static int batch_online_cold(covo_ctx *h, BatchState *b, const covo_batch_args *args, int mode, const covo_env_params *params,
                             hipStream_t s, bool *same_out)
{
    const int E = args->n_envs;
    BatchCommon *c = &b->online;
    covo_batch_mode_args m;  // the scratch's key: this entry's part of it
    std::memset(&m, 0, sizeof(m));
    m.base = *args;
    m.mode = mode;
    const bool new_E = c->n_envs != E;
    bool same;
    int rc;
    if ((rc = batch_cold(h, c, m, params, s, BatchColdDiff{0, false, true, nullptr}, &same))) return rc;
    if (!same) {
        // (not eps_tiled and env_inst: the instance count may change between batch_env_inst and the env step launch that reads
        // env_inst; eps_tiled only ever grows)
        if (new_E || b->tab_hess == nullptr) {  // (null: an earlier attempt failed half way)
            if (h->cma_L == b->L) h->cma_L = nullptr;  // (the factor buffer goes: the next batched CMA step is a first step ...
            free_and_null(b->R, b->Sigma, b->L, b->consts, b->tab_hess);
            h->sigma_L = nullptr;  // ... and the next step of a Sigma period refreshes)
            const size_t M = (size_t)COVO_NA * COVO_NA;
            COVO_CHECK_HIP(hipMalloc(&b->R, (size_t)E * M * sizeof(double)));
            COVO_CHECK_HIP(hipMalloc(&b->Sigma, (size_t)E * M * sizeof(float)));
            COVO_CHECK_HIP(hipMalloc(&b->L, (size_t)E * M * sizeof(float)));
            COVO_CHECK_HIP(hipMalloc(&b->consts, hessian_consts_bytes(E)));
            COVO_CHECK_HIP(hipMalloc(&b->tab_hess, (size_t)E * COVO_H * 4 * sizeof(float)));
        }
        std::vector<char> tmp(hessian_consts_bytes(E));
        hessian_fill_consts(params, E, tmp.data());
        COVO_CHECK_HIP(hipMemcpy(b->consts, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
        if ((rc = grow_device(b->eps_tiled, b->eps_cap, (size_t)E * ((args->n_samples + 31) / 32) * 16 * 64))) return rc;
        // (a grown workspace forgets every graph and key of the handle: the key is recorded after it)
        if ((rc = covo_grow_workspace(h, &h->ws_sigma, &h->ws_sigma_bytes, sigma_ns_workspace_bytes(E), s))) return rc;
        if ((rc = covo_grow_workspace(h, &h->ws_hess, &h->ws_hess_bytes, hessian_workspace_bytes(E), s))) return rc;
        c->record(m, s);
    }
    *same_out = same;
    return 0;
}

// mode: COVO_MODE_COVO_ONLINE, or COVO_MODE_CMA on the same scratch and the same enqueue body (its "reuse" graph: every step but the
// first after a reset)
int covo_step_batched_impl(covo_ctx *h, const covo_batch_args *args, const covo_env_params *params, const uint32_t *keys,
                           hipStream_t s, int mode)
{
    const int E = args->n_envs;
    const bool cma = mode == COVO_MODE_CMA;
    step_sync_epoch(h);
    BatchState *b = batch_state(h);
    BatchCommon *c = &b->online;
    bool same;
    int rc;
    if ((rc = batch_online_cold(h, b, args, mode, params, s, &same))) return rc;
    batch_upload_keys(c->dyn, keys, E, s);
    // covo_set_step_sigma_period: the batch shares one age -- 0: today's step, which leaves the factors in b->L; else a reuse step
    const int age = cma ? covo_cma_step_age(h, b->L, args->sample_sigma, E) : covo_sigma_step_age(h, b->L, args->sample_sigma, E);
    const bool reuse = age != 0;
    // both graphs are keyed by the step's key; each one's first call with these buffers runs eagerly, the second captures
    rc = step_run_passes(
        h, c->cache, reuse, graph_cache_seen(c->cache[reuse ? 1 : 0], same), s, "covo_mpc_step_batched",
        [&](hipStream_t on, int j) { return batch_enqueue(h, b, *args, on, DebugMasks(), j, reuse); },
        [&](hipStream_t on, int) { return covo_plan_after_batched(h, AFTER_BETWEEN, args, mode, params, nullptr, nullptr, -1, on); });
    if (rc == 0 && cma) {
        covo_cma_step_done(h, b->L, args->sample_sigma, E);
        return 0;
    }
    if (rc == 0) covo_sigma_step_done(h, age, b->L, args->sample_sigma, E), h->cma_age = 0;
    if (rc == 0 && !reuse && covo_sigma_adapt_on(h)) return launch_sigma_adapt_idle(h->adapt_rows, E, s);  // (eager, behind the step)
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
    const bool same = batch_key_same(q->cache.have_key, q->key, q->stream, q->params, *m, params, s);
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

// ---- the STAGED env-batched MPPI / covo-offline step (covo_set_step_batched_staged): what the fused launch refuses -- per-step
// disturbance tables, the realworld reward, MPPI's covariance adaptation, more than 16 384 samples, the staged updates (ESS floor, elite
// set), the posterior covariance, arbitrated passes -- runs as the launch sequence of a single staged step with the instance as a grid
// dimension.  Instance e computes what enqueue_step computes for it alone: the same device functions on the same data in the same
// order.  One pass:
static int batch_staged_enqueue(covo_ctx *h, BatchState *b, const covo_batch_mode_args &m, hipStream_t s, const int pass)
{
    const BatchCommon &c = b->staged;
    const BatchStagedExtras &x = b->sx;
    const covo_batch_args &a = m.base;
    const int E = a.n_envs, N = a.n_samples;
    const bool mppi = m.mode == COVO_MODE_MPPI;
    int rc;
    hipLaunchKernelGGL(batch_mode_begin_kernel, dim3(E), dim3(COVO_NA + 64), 0, s, a.a_mean, c.a_mean_shift, c.dyn, x.scales,
                       mppi ? a.a_cov : (float *)nullptr, x.Ls, pass);
    // mppi.py:74: MPPI's sampling rollouts are non-deterministic, CoVO's deterministic (covo.py:231); no Hessian, no Hessian table
    if (c.tables && (rc = launch_disturb_tables_batched(c.models, a.states, c.dyn, E, mppi ? 0 : 1, c.tab_rollout, nullptr, s))) return rc;
    NoiseDesc nd;
    nd.mu = c.a_mean_shift;
    nd.dyn = c.dyn;
    nd.N = N;
    nd.a = a.a;
    nd.batch = E;
    nd.propagate_nan = covo_propagate_nan(h);
    if (mppi) {
        nd.L = x.Ls;
        // covo_set_step_anneal: this pass's row of the schedule into every instance's factors and a_cov, as in the single step
        if (covo_anneal_sched_on(h) && (rc = launch_anneal_schedule(h->anneal_table, pass, x.Ls, a.a_cov, E, s))) return rc;
        if (covo_nodes_on(h)) { if ((rc = launch_noise_nodes(nd, h->nodes_table, pass, h->nodes_M, s))) return rc; }  // (as the single step)
        else if ((rc = launch_noise_blockdiag(nd, s))) return rc;
    } else {
        nd.L = m.L_table;
        nd.state_for_time = a.states;
        nd.n_table = m.n_table;
        nd.batch_table = true;
        nd.table_stride = m.L_table_stride;
        if ((rc = launch_noise_gemm(nd, s))) return rc;
    }
    if ((rc = launch_rollout_batched(c.ro_args_host.data(), c.ro_args, E, s))) return rc;
    const bool cov_adapt = mppi && m.gamma_sigma != 0.0f;
    StepUpdate u = batch_update_desc(h, c, a, pass, cov_adapt);
    if (cov_adapt) {  // mppi.py:109-125 per instance: a_cov[e] (shifted by the begin launch) adapted in place
        u.up.a_cov_old = a.a_cov;
        u.up.gamma_sigma = m.gamma_sigma;
        u.up.a_cov_out = a.a_cov;
        u.up.partials_cov_ws = x.partials_cov;
        u.up.diag_merge_ws = x.diag_merge;
    }
    return enqueue_update(h, u, s);
}

int covo_step_batched_staged_impl(covo_ctx *h, const covo_batch_mode_args *m, const covo_env_params *params, const uint32_t *keys,
                                  hipStream_t s)
{
    const covo_batch_args *args = &m->base;
    const int E = args->n_envs, N = args->n_samples;
    const bool mppi = m->mode == COVO_MODE_MPPI, cov_adapt = mppi && m->gamma_sigma != 0.0f;
    step_sync_epoch(h);
    BatchState *b = batch_state(h);
    BatchCommon *c = &b->staged;
    BatchStagedExtras *x = &b->sx;
    const bool new_E = c->n_envs != E;
    bool same;
    int rc;
    if ((rc = batch_cold(h, c, *m, params, s, BatchColdDiff{mppi ? 4 : 0, cov_adapt, !mppi, &x->scales}, &same))) return rc;
    if (!same) {
        if (new_E || x->diag_merge == nullptr) {  // (null: an earlier attempt failed half way)
            free_and_null(x->Ls, x->diag_merge);
            COVO_CHECK_HIP(hipMalloc(&x->Ls, (size_t)E * COVO_H * 16 * sizeof(float)));
            COVO_CHECK_HIP(hipMalloc(&x->diag_merge, (size_t)E * COVO_PARTIAL_FLOATS * sizeof(float)));
        }
        // the records with second moments
        if (cov_adapt && (rc = grow_device(x->partials_cov, x->partials_cov_cap,
                                           (size_t)E * softmax_cov_workspace_floats(softmax_stage1_blocks(h, N))))) return rc;
        c->record(*m, s);
    }
    batch_upload_keys(c->dyn, keys, E, s);
    // covo_set_step_iters: the K passes in the one graph, the arbiter's launch between two of them eager (step_run_passes)
    return step_run_passes(
        h, c->cache, false, graph_cache_seen(c->cache[0], same), s, "covo_mpc_step_batched_mode",
        [&](hipStream_t on, int j) { return batch_staged_enqueue(h, b, *m, on, j); },
        [&](hipStream_t on, int) { return covo_plan_after_batched(h, AFTER_BETWEEN, args, m->mode, params, nullptr, nullptr, -1, on); });
}

// ---- the hold step of the plan hold (covo_set_step_plan_hold; plan_hold.hip): ONE launch in place of the step's own -- stage `age`
// of the law the last plan step's sweep left, on the state the step would have read, then the begin work's shift with the action in
// front.  alpha comes from the handle's Riccati row (entry 3: the step size of the committed candidate), the sweep's flags from its side row
static HoldDesc hold_desc(const covo_ctx *h, int e, const float *state, const float *a_mean_src, float *a_mean, float *a_cov)
{
    const FeedbackDesc f = covo_feedback_desc(h, e, h->hold_b + (size_t)e * COVO_NA);
    HoldDesc d;
    std::memset(&d, 0, sizeof(d));
    d.state = state;
    d.b = f.b;
    d.K = f.K;
    d.kff = f.kff;
    d.x = f.x;
    d.alpha = h->riccati_out + (size_t)e * COVO_RICCATI_FLOATS + 3;
    d.t_plan = h->hold_t + e;
    d.side = h->riccati_d + (size_t)COVO_MAX_ENVS * COVO_NA + (size_t)e * COVO_RICCATI_SIDE;
    d.a_mean_src = a_mean_src;
    d.a_mean = a_mean;
    d.a_cov = a_cov;
    d.row_out = h->hold_rows + (size_t)e * COVO_HOLD_FLOATS;
    d.log = covo_eplog_inst(h, COVO_EPLOG_HOLD, e, COVO_HOLD_FLOATS);
    return d;
}
int covo_hold_step(covo_ctx *h, const covo_step_args *args, int age, int log_index, hipStream_t s)
{
    const HoldDesc d = hold_desc(h, 0, args->state, args->a_mean_in ? args->a_mean_in : args->a_mean, args->a_mean,
                                 args->mode == COVO_MODE_MPPI ? args->a_cov : nullptr);
    return launch_plan_hold(h, &d, 1, false, false, age, log_index, s);
}
int covo_hold_step_batched(covo_ctx *h, const covo_batch_args *args, int age, int log_index, hipStream_t s)
{
    HoldDesc d[COVO_MAX_ENVS];
    for (int e = 0; e < args->n_envs; ++e) {
        float *am = args->a_mean + (size_t)e * COVO_NA;
        d[e] = hold_desc(h, e, args->states + (size_t)e * COVO_STATE_FLOATS, am, am, nullptr);
    }
    return launch_plan_hold(h, d, args->n_envs, true, false, age, log_index, s);
}
// a hold step's raw keys where a begin launch parks a step's (dyn[12 e + 10..11]): what its plan trace and tables derive from
static void hold_park_keys(uint32_t *dyn, const uint32_t *keys, int E, hipStream_t s)
{
    BatchDyn blk;
    std::memset(&blk, 0, sizeof(blk));
    for (int e = 0; e < E; ++e) {
        blk.w[e][2] = keys[2 * e];
        blk.w[e][3] = keys[2 * e + 1];
    }
    hipLaunchKernelGGL(hold_park_keys_kernel, dim3(1), dim3(256), 0, s, dyn, blk, E);
}

// ---- the iLQR step (COVO_MODE_ILQR; ilqr.hip): its begin work -- the mean shifted in place, the step's scalars from the raw key, the
// rollouts' disturbance table.  Nothing here touches a sample buffer, and nothing is captured: the iterations follow eagerly in the
// after-step frame (ilqr_iterations below), as riccati_after's launches always have
int covo_ilqr_step_impl(covo_ctx *h, const covo_env_params *params, const covo_step_args *args, uint32_t key0, uint32_t key1, hipStream_t s)
{
    if (!h->step) {
        int rc = step_state_init(h);
        if (rc) return rc;
    }
    StepState *st = reinterpret_cast<StepState *>(h->step);
    const uint32_t raw[2] = {key0, key1};
    if (int rc = launch_ilqr_begin(args->a_mean_in ? args->a_mean_in : args->a_mean, args->a_mean, st->dyn, raw, 1, args->derive_keys,
                                   covo_shared_noise_scale(*params, args->rollout_deterministic), s)) return rc;
    if (!covo_needs_tables(*params)) return 0;
    return launch_disturb_tables_step(*params, args->state, st->dyn, args->rollout_deterministic, st->f_tab_rollout, nullptr, s);
}
// ... of E instances: covo-online's scratch (Hessian constants, disturbance models, tables), under a key of its own
int covo_ilqr_step_batched_impl(covo_ctx *h, const covo_batch_args *args, const covo_env_params *params, const uint32_t *keys, hipStream_t s)
{
    const int E = args->n_envs;
    BatchState *b = batch_state(h);
    BatchCommon *c = &b->online;
    bool same;
    if (int rc = batch_online_cold(h, b, args, COVO_MODE_ILQR, params, s, &same)) return rc;
    if (int rc = launch_ilqr_begin(args->a_mean, args->a_mean, c->dyn, keys, E, 1, 0.0f, s)) return rc;  // (deterministic rollouts, as covo-online's)
    if (!c->tables) return 0;
    return launch_disturb_tables_batched(c->models, args->states, c->dyn, E, 1, c->tab_rollout, b->tab_hess, s);
}

// ---- the after-step frame: the launches behind a step (after_step.hpp: the update arbiter, the flight recorder's plan and trace, the
// sample fan; the refinements; the posterior covariance), eager.
// What they need to know about ONE instance of the step that has just been enqueued: the inputs its sample rollouts had.  The shared
// vector is re-derived from the raw key by the launches themselves (every step path forms it from the same device function); the
// per-step tables are the ones the step has just built in its own scratch.  key_mem: the instance's raw rng_act in device memory;
// null (a single step that is not iterated): the caller sets key / f_shared as covo_mpc_step got them
static PlanInstDesc plan_inst(const BatchInst &i, int T, int N, const covo_env_params *params, int derive_keys, bool deterministic,
                              const float *nominal, const float *f_tab, const uint32_t *key_mem)
{
    PlanInstDesc d;
    std::memset(&d, 0, sizeof(d));
    d.state = i.state;
    d.pos_traj = i.pos_traj;
    d.vel_traj = i.vel_traj;
    d.T = T;
    d.params = params;
    d.a_mean = i.a_mean;
    d.a = i.a;
    d.N = N;
    d.cost = i.cost;
    d.a_nominal = nominal;
    d.a_mean_out = i.a_mean;
    d.f_tab = f_tab;
    d.key_mem = key_mem;
    d.derive_keys = derive_keys;
    d.shared_noise_scale = covo_shared_noise_scale(*params, deterministic);
    return d;
}
// ... and about the step of n instances as a whole, built once per call for the form it runs in (AfterForm, covo_common.hpp; an iLQR
// step by its mode) by after_frame_single / after_frame_batched
struct AfterFrame {
    PlanInstDesc d[COVO_MAX_ENVS];
    int n;
    bool batched;          // the launches take their batched form: argument blocks in device memory, the keys from key_mem
    HessianDesc hess;      // the Hessian's inputs at the committed means, dense over the instances; f_tab: left to the entry point,
                           // which sets it next to the launch that forms the table
    bool refine, riccati;  // the step runs the Newton / the Riccati refinement (never both: check_step_attachments)
    const float *Sigma;    // [n][128][128] the Sigma the step sampled from (the Newton refinement's), with ...
    float sample_sigma;    // ... its sample_sigma
    const float *a, *cost, *mu;  // the posterior covariance's inputs, dense over the instances: samples, costs, the means sampled around
    int N;
};
// something behind a step is attached
static bool after_any(const covo_ctx *h)
{
    return covo_plan_on(h) || covo_fan_on(h) || covo_arb_on(h) || covo_post_cov_on(h) || covo_refine_on(h) || covo_riccati_on(h);
}
// a single step (st: its scratch, null before the first one).  Neither a hold step nor an iLQR step has sampled: no nominal, and
// never the batched form.  An iterated step (covo_set_step_iters): the launches describe the pass that has just been enqueued, whose
// raw key lies in device memory (st->dyn[10..11]) -- they take it from there, through the argument blocks of the batched form
static void after_frame_single(const covo_ctx *h, const StepState *st, AfterFrame &f, AfterForm form, const covo_env_params *params,
                               const covo_step_args *args, uint32_t key0, uint32_t key1, const float *f_shared)
{
    const bool sampled = form != AFTER_HOLD && args->mode != COVO_MODE_ILQR;
    f.n = 1;
    f.batched = sampled && covo_step_iters(h) > 1 && st != nullptr;
    const BatchInst i = {args->state, args->pos_traj, args->vel_traj, args->a_mean, args->a, args->cost, args->groupmin};
    PlanInstDesc &d = f.d[0];
    d = plan_inst(i, args->T, args->n_samples, params, args->derive_keys, args->rollout_deterministic,
                  !sampled ? nullptr : (args->a_mean_shift ? args->a_mean_shift : (st ? st->a_mean_shift : nullptr)),
                  (covo_needs_tables(*params) && st) ? st->f_tab_rollout : nullptr, f.batched ? st->dyn + 10 : nullptr);
    d.key[0] = key0;
    d.key[1] = key1;
    for (int c = 0; c < 3; ++c) d.f_shared[c] = f_shared ? f_shared[c] : 0.0f;
    f.hess = covo_hessian_inputs(args->state, args->pos_traj, args->vel_traj, args->T, params, args->a_mean, nullptr, 1);
    f.refine = sampled && covo_refine_on(h) && args->mode == COVO_MODE_COVO_ONLINE && st != nullptr;
    f.riccati = form != AFTER_HOLD && covo_riccati_on(h);  // every mode, every step of a Sigma period
    f.Sigma = !f.refine ? nullptr : (args->a_cov ? args->a_cov : st->Sigma);
    f.sample_sigma = args->sample_sigma;
    // (d.a_nominal is the mean the last pass sampled around)
    f.a = d.a, f.cost = d.cost, f.mu = d.a_nominal, f.N = d.N;
}
// an env-batched step in `mode`.  c: the batch whose begin launch has left the shifted means and parked the raw keys at [10..11] of
// the instances' blocks, or null behind the fused launch, which leaves [0..1] alone; a hold step's keys were parked in the handle.
// nominal: the update arbiter's, or null.  CoVO's rollouts are deterministic
static void after_frame_batched(const covo_ctx *h, const BatchState *b, const BatchCommon *c, AfterFrame &f, AfterForm form,
                                const covo_batch_args *args, int mode, const covo_env_params *params, const float *nominal)
{
    const int E = args->n_envs;
    f.n = E;
    f.batched = true;
    for (int e = 0; e < E; ++e)
        f.d[e] = plan_inst(batch_inst(*args, e), args->T, args->n_samples, &params[e], 1, mode != COVO_MODE_MPPI,
                           nominal ? nominal + (size_t)e * COVO_NA : nullptr,
                           (c && c->tables) ? c->tab_rollout + (size_t)e * COVO_H * 4 : nullptr,
                           form == AFTER_HOLD ? h->hold_keys + 12 * e + 10 : (c ? c->dyn + 12 * e + 10 : b->small.dyn + 12 * e));
    // the refinements: the batches with per-instance Hessian constants only (check_batch_step refuses the other modes)
    const bool online = mode == COVO_MODE_COVO_ONLINE || mode == COVO_MODE_ILQR;
    f.refine = form != AFTER_HOLD && covo_refine_on(h) && online;
    f.riccati = form != AFTER_HOLD && covo_riccati_on(h) && online;
    if (f.refine || f.riccati) {
        f.hess = covo_hessian_inputs(args->states, args->pos_traj, args->vel_traj, args->T, &c->params[0], args->a_mean, nullptr, E);
        f.hess.consts_dev = b->consts;
        f.hess.traj_stride = (size_t)args->T * 3;
        f.hess.models_dev = c->models;
    }
    f.Sigma = !f.refine ? nullptr : (args->a_cov ? args->a_cov : b->Sigma);
    f.sample_sigma = args->sample_sigma;
    // (never behind the fused launch: check_batch_step) dense slices, the begin launch's shifted means
    f.a = args->a, f.cost = args->cost, f.mu = c ? c->a_mean_shift : nullptr, f.N = args->n_samples;
}

// covo_set_step_refine: the gradient's two launches at the committed means, then the line search with c^2 from the Sigma chain's slots
// of this step
static int refine_after(covo_ctx *h, const AfterFrame &f, hipStream_t s)
{
    if (int rc = launch_cost_gradient(f.hess, h->refine_g, h->ws_grad, s)) return rc;
    size_t stride;
    const double *sumlogB = sigma_ns_sumlogB(h->ws_sigma, f.n, &stride);
    RefineDesc r[COVO_MAX_ENVS];
    for (int e = 0; e < f.n; ++e) {
        r[e].g = h->refine_g + (size_t)e * COVO_NA;
        r[e].Sigma = f.Sigma + (size_t)e * COVO_NA * COVO_NA;
        r[e].sumlogB = sumlogB + (size_t)e * stride;
        r[e].sample_sigma = f.sample_sigma;
        r[e].row_out = h->refine_out + (size_t)e * COVO_REFINE_FLOATS;
    }
    return launch_newton_refine(h, f.d, r, f.n, f.batched, s);
}
// covo_set_step_riccati: the Hessian's first two launches at the committed means into the refinement's own workspace, the sweep
// (riccati.hip), [the closed-loop generator (feedback_rollout.hip),] then the line search with the direction supplied
// covo_set_step_plan_hold: the sweep leaves its gains whether or not the closed-loop candidates are on, and the latch (plan_hold.hip)
// sits between the sweep and the line search, which overwrites the mean the sweep ran at; row: the episode's row index, < 0: none
// costs: where instance 0's candidate costs of this call go (test hook: an iteration's slot of h->ilqr_costs), or null
static int riccati_after(covo_ctx *h, const AfterFrame &f, int row, float *costs, hipStream_t s)
{
    HessianDesc hd = f.hess;
    hd.status_dev = h->status_dev;
    // covo_set_step_riccati_feedback: the sweep also leaves its gains, the generator (feedback_rollout.hip) runs the closed-loop
    // sequences under them, and the line search judges them next to its own
    const bool feedback = covo_feedback_on(h);
    const bool hold = covo_plan_hold(h) > 1;
    RiccatiOut o = covo_riccati_out(h, feedback || hold);
    o.box = covo_box_on(h);  // covo_set_step_riccati_box: the masks of the last sweep stay on the handle
    o.masks = h->box_masks;
    if (int rc = launch_riccati(hd, COVO_RICCATI_REG0, o, h->ws_riccati, s)) return rc;
    if (hold) {
        LatchDesc l[COVO_MAX_ENVS];
        for (int e = 0; e < f.n; ++e) {
            l[e].a_mean = f.d[e].a_mean_out;
            l[e].state = f.d[e].state;
            l[e].b_out = h->hold_b + (size_t)e * COVO_NA;
            l[e].t_out = h->hold_t + e;
            l[e].row_out = h->hold_rows + (size_t)e * COVO_HOLD_FLOATS;
            l[e].log = covo_eplog_inst(h, COVO_EPLOG_HOLD, e, COVO_HOLD_FLOATS);
        }
        if (int rc = launch_plan_latch(h, l, f.n, f.batched, row, s)) return rc;
    }
    RefineDesc r[COVO_MAX_ENVS];
    FeedbackDesc fb[COVO_MAX_ENVS];
    for (int e = 0; e < f.n; ++e) {
        if (feedback) fb[e] = covo_feedback_desc(h, e, f.d[e].a_mean_out);
        r[e] = covo_riccati_refine_desc(o, e, h->riccati_out + (size_t)e * COVO_RICCATI_FLOATS,
                                        costs ? costs + (size_t)e * COVO_MAX_STEP_ITERS * COVO_FEEDBACK_CANDIDATES : nullptr,
                                        feedback ? &fb[e] : nullptr,
                                        feedback ? h->feedback_out + (size_t)e * COVO_FEEDBACK_FLOATS : nullptr);
    }
    if (feedback)
        if (int rc = launch_feedback_rollout(h, f.d, fb, f.n, f.batched, s)) return rc;
    return launch_newton_refine(h, f.d, r, f.n, f.batched, s);
}
// the arbiter first: the plan, the trace's u and the env step see its mean; trace_index: the episode's row index (the fan log counts
// like the trace).  The refinement directly behind the arbiter, every pass of an iterated step included; the posterior covariance
// last, behind the (last pass's) update and the launches above
static int plan_after(covo_ctx *h, const AfterFrame &f, AfterForm form, const float *states_true, int trace_index, hipStream_t s)
{
    int rc = launch_update_arbiter(h, f.d, f.n, f.batched, trace_index, s);
    if (rc == 0 && f.refine) rc = refine_after(h, f, s);
    if (rc == 0 && f.riccati) rc = riccati_after(h, f, trace_index, nullptr, s);
    if (rc || form == AFTER_BETWEEN) return rc;
    if ((rc = launch_plan_trace(h, f.d, f.n, f.batched, states_true, trace_index, s))) return rc;
    if ((rc = launch_sample_fan(h, f.d, f.n, f.batched, trace_index, s))) return rc;
    return launch_post_cov_after(h, f.a, f.cost, f.mu, f.N, f.n, s);
}

// the k iterations of an iLQR step behind its begin work: riccati_after as a sampling step enqueues it, k times on the same inputs (the
// key is not walked: one objective per step), each followed by the tally (ilqr.hip); then the plan trace of the committed mean
static int ilqr_iterations(covo_ctx *h, const AfterFrame &f, const float *states_true, int trace_index, hipStream_t s)
{
    const int K = covo_step_iters(h);
    for (int j = 0; j < K; ++j) {
        float *costs = h->ilqr_costs ? h->ilqr_costs + (size_t)j * COVO_FEEDBACK_CANDIDATES : nullptr;
        int rc = riccati_after(h, f, trace_index, costs, s);
        if (rc || (rc = launch_ilqr_tally(h, f.n, f.batched, j, K, s))) return rc;
    }
    return launch_plan_trace(h, f.d, f.n, f.batched, states_true, trace_index, s);
}

int covo_plan_after_step(covo_ctx *h, AfterForm form, const covo_env_params *params, const covo_step_args *args, uint32_t key0,
                         uint32_t key1, const float *f_shared, const float *state_true, int trace_index, hipStream_t s)
{
    if (form == AFTER_HOLD ? !covo_plan_on(h) : !after_any(h)) return 0;
    StepState *st = reinterpret_cast<StepState *>(h->step);
    AfterFrame f;
    after_frame_single(h, st, f, form, params, args, key0, key1, f_shared);
    const bool tables = covo_needs_tables(*params);
    if (form == AFTER_HOLD) {
        // the plan trace alone.  The rollouts' disturbance table is formed here from the raw key, into the step's own scratch (the
        // hold step has enqueued none of the step's launches)
        if (tables && st != nullptr) {
            const uint32_t raw[2] = {key0, key1};
            hold_park_keys(h->hold_keys, raw, 1, s);
            if (int rc = launch_disturb_tables_step(*params, args->state, h->hold_keys, args->rollout_deterministic, st->f_tab_rollout,
                                                    nullptr, s)) return rc;
        }
        return launch_plan_trace(h, f.d, 1, false, state_true, trace_index, s);
    }
    if (f.refine && tables) f.hess.f_tab = st->f_tab_hess;  // the step's own Hessian has left it
    if (f.riccati && tables) {
        // the sweep's is formed here from the raw key, as the call got it or as the pass left it (MPPI, covo-offline and reuse steps
        // build none; a refresh step's own holds the same rows)
        if (int rc = launch_disturb_table(*params, args->state, 1, f.d[0].key_mem, key0, key1, COVO_DISTURB_KEYS_HESSIAN, 1, h->riccati_tab, s))
            return rc;
        f.hess.f_tab = h->riccati_tab;
    }
    // the iterations of an iLQR step: the raw key as the call got it (not walked)
    if (args->mode == COVO_MODE_ILQR) return ilqr_iterations(h, f, state_true, trace_index, s);
    return plan_after(h, f, form, state_true, trace_index, s);
}

// mode: COVO_MODE_COVO_ONLINE (covo_step_batched_impl has run), COVO_MODE_ILQR (covo_ilqr_step_batched_impl, on covo-online's scratch)
// or MPPI / COVO_OFFLINE (covo_step_batched_small_impl / _staged_impl)
int covo_plan_after_batched(covo_ctx *h, AfterForm form, const covo_batch_args *args, int mode, const covo_env_params *params,
                            const uint32_t *keys, const float *states_true, int trace_index, hipStream_t s)
{
    if (form == AFTER_HOLD ? !covo_plan_on(h) : !after_any(h)) return 0;
    BatchState *b = reinterpret_cast<BatchState *>(h->batch);
    const int E = args->n_envs;
    // the batch with a begin launch: covo-online's (a hold step's too: the others refuse the Riccati refinement), the staged MPPI /
    // covo-offline step's (covo_set_step_batched_staged), or none behind the fused launch
    const bool online = mode == COVO_MODE_COVO_ONLINE || mode == COVO_MODE_ILQR || mode == COVO_MODE_CMA || form == AFTER_HOLD;
    const BatchCommon *c = online ? &b->online : (covo_batched_staged(h) ? &b->staged : nullptr);
    const float *nominal = nullptr;  // the update arbiter's: a begin launch leaves it, the fused launch's was formed ahead of it
    if (form != AFTER_HOLD && covo_arb_on(h)) {
        if (c != nullptr) nominal = c->a_mean_shift;
        else if (int rc = launch_arbiter_nominal(h, nullptr, E, s, &nominal)) return rc;
    }
    AfterFrame f;
    after_frame_batched(h, b, c, f, form, args, mode, params, nominal);
    if (form == AFTER_HOLD) {
        // the plan trace alone, the instances' raw keys parked where a begin launch would have left them, the rollouts' tables formed
        // from them into the batch's scratch
        hold_park_keys(h->hold_keys, keys, E, s);
        if (c->tables)
            if (int rc = launch_disturb_tables_batched(c->models, args->states, h->hold_keys, E, 1, c->tab_rollout, nullptr, s)) return rc;
        return launch_plan_trace(h, f.d, E, true, states_true, trace_index, s);
    }
    if ((f.refine || f.riccati) && c->tables) f.hess.f_tab = b->tab_hess;
    if (mode == COVO_MODE_ILQR) return ilqr_iterations(h, f, states_true, trace_index, s);  // (riccati: the step's own checks)
    return plan_after(h, f, form, states_true, trace_index, s);
}

// test hook: the factor(s) the LAST single (batched = 0) / env-batched step sampled from -- what the next reuse step of a Sigma period
// shifts -- device -> device
int covo_debug_sigma_factor_impl(covo_ctx *h, int batched, float *out, int64_t count, hipStream_t s)
{
    StepState *st = reinterpret_cast<StepState *>(h->step);
    BatchState *b = reinterpret_cast<BatchState *>(h->batch);
    const float *src = batched ? (b ? b->L : nullptr) : (st ? st->L : nullptr);
    const int64_t have = (int64_t)COVO_NA * COVO_NA * (batched ? (b ? b->online.n_envs : 0) : 1);
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
