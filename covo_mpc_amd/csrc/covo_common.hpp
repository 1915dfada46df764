// covo_common.hpp -- internal declarations shared by the gfx950 kernels and the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/covo_hip.h"
#include "quad_model.hpp"

#define COVO_WAVE 64

// state buffer offsets (include/covo_hip.h "Data layouts")
enum { ST_POS = 0, ST_VEL = 3, ST_QUAT = 6, ST_OMEGA = 10, ST_FDIST = 13, ST_POSTAR = 16, ST_VELTAR = 19, ST_ACCTAR = 22, ST_TIME = 25 };

// Experiment switches of ONE handle (round 6: rounds 1-5 kept them in process-global variables that flipped every handle of the
// process and were not thread-safe).  covo_create fills them from the environment (covo_default_opts: COVO_STREAM_GEMM,
// COVO_FUSE_SMALL, COVO_FOLD_BEGIN, COVO_NS_DEFLATE, COVO_NS_MERGED, read once per handle); covo_debug_set_*(handle, ...) change
// them for that handle only and bump `epoch`, which makes the handle re-capture its step graphs (they bake the launch set in).
struct CovoOpts {
    int stream_gemm;   // covo-online's noise GEMM streamed inside the Sigma chain's finalize launch (sigma_ns.hip: ns_finalize_stream_kernel)
    int fuse_small;    // the fused small step (step_small.hip) is taken where eligible
    int fold_begin;    // eager covo-online steps: the begin work rides in the Hessian's first launch
    int ns_deflate;      // the Newton-Schulz iteration deflates the bottom eigenpair
    int ns_force_agent;  // take the agent-scope coherence fallback although the placement check passed
    int ns_merged;       // one matrix: squaring chain + evaluations + Newton-Schulz iterations as ONE launch (ns_chain_kernel)
    int epoch;
};
CovoOpts covo_default_opts();  // step.hip

// the episode logs by internal kind: the six COVO_EPLOG_* kinds of covo_set_episode_rows (include/covo_hip.h), then the five with setters of
// their own
enum { COVO_EPLOG_DIAG = COVO_EPLOG_KINDS, COVO_EPLOG_TRACE, COVO_EPLOG_FAN, COVO_EPLOG_ARB, COVO_EPLOG_HOLD, COVO_EPLOG_ALL };

struct covo_ctx {
    covo_config cfg;
    CovoOpts opt;
    int device;
    // workspace (device)
    float *ws_partials;   // [max_blocks][COVO_PARTIAL_FLOATS] stage-1 records of the softmax reduce
    float *ws_partials_cov;  // [max_blocks][452] stage-1 records with second moments (MPPI covariance adaptation, reduce.hip)
    float *ws_blockmin;   // [ceil(n_local/64)] per-wave cost minima when the caller passes none
    double *ws_stats;     // [ceil(n_local/256)][H*6] per-block position statistics
    void *ws_sigma;       // scratch of the eigh-free Sigma pipeline (grown on demand, outside graph capture)
    size_t ws_sigma_bytes;
    void *ws_hess;        // scratch of the second-order-adjoint Hessian (grown on demand, outside graph capture)
    size_t ws_hess_bytes;
    void *step;               // StepState (step.hip): fused-step scratch + graph cache
    void *batch;              // BatchState (step.hip): env-batched step scratch + graph cache
    hipStream_t side_stream;  // forked work inside one call (joined before the call's last kernel)
    hipEvent_t ev_fork, ev_join;
    int max_red_blocks;
    int *status_host;         // host-mapped sticky status word (COVO_DEVSTAT_* bits written by kernels), see covo_device_status
    int *status_dev;          // its device address
    void *exchange;           // Exchange (exchange.hip): peer-write exchange of the rank records, or null
    int dbg_epoch;            // opt.epoch when this handle's step graphs were captured (a debug setter since then: re-capture)
    int batched_staged;       // covo_set_step_batched_staged: the env-batched MPPI / covo-offline step runs its staged launch sequence
    // per-step sampling diagnostics (covo_set_step_diag / covo_set_episode_diag_log); all null / 0: off
    float *diag_out;          // caller's [diag_n][COVO_DIAG_FLOATS]: instance e's row of every step
    int diag_n;
    float *diag_scratch;      // [COVO_MAX_ENVS][COVO_DIAG_FLOATS]: where the steps write when only the log is attached
    float *ws_diag_rec;       // [max_blocks][4] stage-1 diagnostic records next to ws_partials (softmax_merge.hpp)
    // the flight recorder (covo_set_step_plan / covo_set_episode_trace; plan_trace.hip); all null / 0: off
    float *plan_out;          // caller's [plan_n][COVO_PLAN_FLOATS]: instance e's plan row of every step
    int plan_n;
    // the sample fan (covo_set_step_fan / covo_set_episode_fan; sample_fan.hip); all null / 0: off
    float *fan_out;           // caller's [fan_n][fan_K][COVO_FAN_FLOATS]: instance e's fan of every step
    const int32_t *fan_idx;   // caller's [fan_n][fan_K] sample indices, or null: the stride
    int fan_K, fan_n;
    // the ESS floor (covo_set_step_ess_floor; ess_lambda.hip); ess_min == 0: off
    float ess_min;
    float *lam_out;           // caller's [lam_n][COVO_LAM_FLOATS]: instance e's solver row of every step; null: lam_own
    int lam_n;
    float *lam_own;           // [COVO_MAX_ENVS][COVO_LAM_FLOATS]
    // the annealed step (covo_set_step_anneal; cost_standardise.hip); anneal_passes == 0: off
    float *anneal_table;      // [COVO_MAX_STEP_ITERS][H] the handle's own: sigma[i][h] of pass i, stage h (uploaded by the setter)
    int anneal_passes;        // the passes the attachment was set for: the step's iters must equal it
    int anneal_sched;         // a table was given: every pass's schedule launch writes its row into the block factors and a_cov
    float anneal_temp;        // > 0: every pass's temperature is temp x the standard deviation of its finite costs; 0: the configured lam
    float *anneal_rows;       // caller's [anneal_n][anneal_passes][COVO_LAM_FLOATS]: instance e's solver row of every pass, or null
    int anneal_n;
    // the annealed step's spline nodes (covo_set_step_nodes; noise_nodes.hip); nodes_M == 0: off
    float *nodes_table;       // [nodes_passes][H][nodes_M] the handle's own: B[i][h][m] of pass i (uploaded by the setter)
    int nodes_passes;         // the passes the table was set for: the schedule's must equal it
    int nodes_M;              // nodes per pass, 2 .. H
    // covo-online in spline-node space (covo_set_step_sigma_nodes; sigma_nodes.hip); sn_M == 0: off
    double *sn_W;             // [H][sn_M] the handle's own: the interpolation weights (uploaded by the setter)
    int sn_M;                 // nodes, 2 .. COVO_SIGMA_NODES_MAX: d = 4 sn_M
    float *sn_rows;           // caller's [sn_n][COVO_SIGMA_NODES_FLOATS]: instance e's side row of every step
    int sn_n;
    double *sn_SigmaM;        // [COVO_MAX_ENVS][64][64] the handle's own: instance e's Sigma_M [d][d] of the last step, dense at e d d
    float *sn_G;              // [COVO_MAX_ENVS][128][64] the handle's own: instance e's factor G [128][d], dense at e 128 d
    // the elite-set update (covo_set_step_elite; elite_select.hip, reduce_elite.hip); elite_K == 0: off
    int elite_K;              // elites per instance and pass
    float *elite_out;         // caller's [elite_n][COVO_ELITE_FLOATS]: instance e's selector row of every step; null: elite_own
    int elite_n;
    float *elite_own;         // [COVO_MAX_ENVS][COVO_ELITE_FLOATS]
    // the update arbiter (covo_set_step_arbiter / covo_set_episode_arbiter_log; update_arbiter.hip); arb_out null: off
    float *arb_out;           // caller's [arb_n][COVO_ARB_FLOATS]: instance e's arbiter row of every step
    int arb_mask, arb_n;      // enabled candidates (bits 0..2), rows of arb_out
    // what the three launches that follow a step keep on the device (plan_trace.hip, sample_fan.hip, update_arbiter.hip)
    void *after;              // AfterState (after_step.hpp): a batched step's argument blocks per launch, the arbiter's nominals
    // iterations per control step (covo_set_step_iters); iters <= 1 or iter_log null: off
    int iters;                // sample-rollout-update passes per control step
    float *iter_log;          // caller's [iter_n][iters]: entry (e, j) = the minimum sample cost of instance e's pass j
    int iter_n;
    // the Sigma period (covo_set_step_sigma_period; sigma_shift.hip); sigma_period <= 1: off
    int sigma_period;         // every sigma_period-th covo-online step refreshes Sigma; the steps between shift the last factor
    int sigma_age;            // the age the NEXT step runs at: 0 = refresh, 1 .. sigma_period - 1 = reuse
    int sigma_last_age;       // the age the last enqueued step ran at
    const float *sigma_L;     // the factor buffer (the single step's or the batch's) that holds the last step's L; null: none yet
    float sigma_L_sigma;      // the sample_sigma it was built for ...
    int sigma_L_n;            // ... and for how many instances
    // the posterior covariance (covo_set_step_post_cov; post_cov.hip); post_cov_out null: off
    float *post_cov_out;      // caller's [post_n][128][128]: instance e's weighted sample covariance of every step
    float *post_aux_out;      // caller's [post_n][COVO_POST_AUX_FLOATS]: {shift d[128], W, 0, 0, 0}
    int post_n;
    void *post_cov;           // PostCovState (post_cov.hip): the stage-1 partials, the stand-alone entry's selector rows
    // Sigma adapt (covo_set_step_sigma_adapt; sigma_adapt.hip); adapt_rows null: off
    float adapt_gamma;        // the weight of the previous step's posterior covariance in a reuse step's Sigma', in (0, 1)
    float *adapt_rows;        // caller's [adapt_n][COVO_SIGMA_ADAPT_FLOATS]: instance e's {fallback, c, log det M, 0} of every reuse step
    int adapt_n;
    // the CMA controller (covo_set_step_cma; cma_path.hip); cma_rows null: not attached
    float cma_gamma;          // the weight of the previous step's posterior covariance in the shape, in [0, 1)
    int cma_step_size;        // 0: s = 1 for ever
    float cma_damping, cma_s_min, cma_s_max;
    float *cma_rows;          // caller's [cma_n][COVO_CMA_FLOATS]: instance e's row of every step
    double *cma_p;            // caller's [cma_n][128]: the evolution paths, kept there between steps
    int cma_n;                // the rows and paths of the current attachment (0: detached): a step of more instances is refused
    void *cma_ws;             // the handle's own, one allocation: log s [COVO_MAX_ENVS] (fp64), the shape's rows [COVO_MAX_ENVS][4], L_hat [cma_ws_n][128][128]
    int cma_ws_n;             // the instances cma_ws was allocated for (>= cma_n; only ever grows)
    int cma_age;              // 0: the next CMA step is the first after a reset; else 1
    const float *cma_L;       // the factor buffer (the single step's or the batch's) that holds the last CMA step's L ...
    float cma_L_sigma;        // ... the sample_sigma it was built for ...
    int cma_L_n;              // ... and for how many instances
    // the Newton refinement of the committed mean (covo_set_step_refine; cost_gradient.hip, newton_refine.hip); refine_out null: off
    float *refine_out;        // caller's [refine_n][COVO_REFINE_FLOATS]: instance e's refine row of every step
    int refine_n;
    void *ws_grad;            // scratch of the first-order adjoint (its own: the Sigma chain and the debug readers own ws_hess)
    size_t ws_grad_bytes;
    double *refine_g;         // [COVO_MAX_ENVS][128] the gradients of a step's instances at their committed means
    // the Riccati refinement of the committed mean (covo_set_step_riccati; riccati.hip, newton_refine.hip); riccati_out null: off
    float *riccati_out;       // caller's [riccati_n][COVO_RICCATI_FLOATS]: instance e's row of every step
    int riccati_n;
    void *ws_riccati;         // the refinement's own Hessian workspace and sweep slices (riccati_workspace_bytes)
    size_t ws_riccati_bytes;
    double *riccati_d;        // [COVO_MAX_ENVS][128 + COVO_RICCATI_SIDE]: the directions, then the side rows, of a step's instances
    float *riccati_tab;       // [H][4] the Hessian's disturbance table of a single step (MPPI, covo-offline and reuse steps build none)
    // the closed-loop candidates of the Riccati refinement (covo_set_step_riccati_feedback; feedback_rollout.hip); feedback_out null: off
    float *feedback_out;      // caller's [feedback_n][COVO_FEEDBACK_FLOATS]: instance e's feedback row of every step
    int feedback_n;
    double *feedback_gains;   // [COVO_MAX_ENVS][COVO_FEEDBACK_GAIN_DOUBLES]: the sweep's K, kff and x of a step's instances
    float *feedback_a;        // [COVO_MAX_ENVS][16][128 + 4]: the generator's sequences, then their aux rows
    int feedback_poke_armed;  // test hook (covo_debug_feedback_gain): the next covo_riccati_refine_feedback overwrites one gain entry
    int feedback_poke_at;     // ... instance * H * 64 + index into K [H][4][16]
    double feedback_poke;     // ... with this value, between the sweep and the generator
    // the plan hold (covo_set_step_plan_hold; plan_hold.hip); plan_hold <= 1: off
    int plan_hold;            // every plan_hold-th control step plans; the steps between apply the sweep's law to the measured state
    int plan_age;             // the age the NEXT step runs at: 0 = plan, 1 .. plan_hold - 1 = hold
    int plan_last_age;        // the age the last enqueued step ran at
    int hold_latch_n;         // for how many instances the last plan step left its latch (0: none yet)
    float *hold_rows;         // caller's [hold_n][COVO_HOLD_FLOATS]: instance e's hold row of every step
    int hold_n;
    float *hold_b;            // [COVO_MAX_ENVS][128] the latch: the mean the last plan step's sweep ran at ...
    int *hold_t;              // [COVO_MAX_ENVS] ... and the time word of the state it planned from
    uint32_t *hold_keys;      // [COVO_MAX_ENVS][12]: a hold step's raw keys for its plan trace, laid out like a step's scalars
    // the per-iteration logs of the iLQR steps (covo_set_step_ilqr; ilqr.hip); all null: off
    float *ilqr_rows;         // caller's [ilqr_n][COVO_MAX_STEP_ITERS][COVO_RICCATI_FLOATS]: slot j = iteration j's Riccati row
    float *ilqr_fb_rows;      // caller's [ilqr_n][COVO_MAX_STEP_ITERS][COVO_FEEDBACK_FLOATS]: ... and its feedback row
    float *ilqr_summary;      // caller's [ilqr_n][COVO_ILQR_FLOATS]
    int ilqr_n;
    float *ilqr_costs;        // test hook (covo_debug_ilqr_costs): caller's [ilqr_costs_n][COVO_MAX_STEP_ITERS][COVO_FEEDBACK_CANDIDATES], or null
    int ilqr_costs_n;
    // the box form of the Riccati refinement's sweep (covo_set_step_riccati_box; riccati.hip); box_masks null: off
    int *box_masks;           // caller's [box_n][H]: instance e's clamp masks of the last sweep
    int box_n;
    int *ilqr_box;            // caller's [ilqr_box_n][COVO_MAX_STEP_ITERS] (covo_set_step_ilqr_box): slot j = iteration j's clamped coordinates, or null
    int ilqr_box_n;
    // the state estimator (covo_set_step_estimator; state_estimator.hip); est_rows null: not attached
    float *est_rows;          // caller's [est_n][COVO_EST_FLOATS]: instance e's side row of every launch
    double *est_xhat, *est_P; // caller's [est_n][COVO_EST_STATE_DOUBLES], [est_n][13][13]: the filter's state lives there between steps
    int *est_meta;            // caller's [est_n][COVO_EST_META_INTS]
    int est_n;
    double est_obs_std[4], est_proc_std[4], est_force_std;
    int est_fresh;            // 1: the next launch of a driver treats every instance as one without a valid state
    float *est_log;           // caller's [n_inst][est_log_stride][COVO_EST_LOG_FLOATS] (covo_set_episode_estimator_log): the launch writes
    int est_log_stride;       // its rows itself; not one of eplog's kinds -- an episode driver checks its extent next to theirs
    // the force observer (covo_set_step_force_observer; force_observer.hip); obs_rows null: not attached.  Never attached together
    // with the state estimator: two filters must not write one row
    float *obs_rows;          // caller's [obs_n][COVO_OBS_FLOATS]: instance e's side row of every launch
    double *obs_xi, *obs_P;   // caller's [obs_n][COVO_OBS_STATE_DOUBLES], [obs_n][16][16]: the filter's state lives there between steps
    int *obs_meta;            // caller's [obs_n][COVO_OBS_META_INTS]
    int obs_n;
    double obs_obs_std[4], obs_proc_std[4], obs_walk_std, obs_init_std;
    int obs_fresh;            // 1: the next launch of a driver treats every instance as one without a valid state
    float *obs_log;           // caller's [n_inst][obs_log_stride][COVO_OBS_LOG_FLOATS] (covo_set_episode_force_observer_log): like est_log,
    int obs_log_stride;       // written by the launch itself and checked next to it
    // the episode logs, by kind (covo_eplog_kinds below says what each holds and who fills it); log null: off
    struct {
        float *log;  // caller's [n_inst][stride][one row of the kind]: every step of an episode driver leaves row `index` of every instance
        int stride;
    } eplog[COVO_EPLOG_ALL];
};
static inline void covo_eprow_drop(covo_ctx *h, int kind) { h->eplog[kind] = {nullptr, 0}; }
// a log of covo_set_episode_rows (the six public kinds) is attached
static inline bool covo_eprow_any(const covo_ctx *h)
{
    for (int k = 0; k < COVO_EPLOG_KINDS; ++k)
        if (h->eplog[k].log != nullptr) return true;
    return false;
}
// instance e's rows of the log of `kind` (row_floats per row), or null
static inline float *covo_eplog_inst(const covo_ctx *h, int kind, int e, int row_floats)
{
    return h->eplog[kind].log ? h->eplog[kind].log + (size_t)e * h->eplog[kind].stride * row_floats : nullptr;
}
static inline bool covo_post_cov_on(const covo_ctx *h) { return h->post_cov_out != nullptr; }
static inline bool covo_sigma_adapt_on(const covo_ctx *h) { return h->adapt_rows != nullptr && h->adapt_gamma > 0.0f; }
static inline bool covo_cma_on(const covo_ctx *h) { return h->cma_rows != nullptr; }
// the three parts of cma_ws
static inline double *covo_cma_log_s(const covo_ctx *h) { return reinterpret_cast<double *>(h->cma_ws); }
static inline float *covo_cma_shape_rows(const covo_ctx *h) { return reinterpret_cast<float *>(covo_cma_log_s(h) + COVO_MAX_ENVS); }
static inline float *covo_cma_L_hat(const covo_ctx *h) { return covo_cma_shape_rows(h) + (size_t)COVO_MAX_ENVS * COVO_SIGMA_ADAPT_FLOATS; }
static inline size_t covo_cma_ws_bytes(int n_inst)
{
    return (size_t)COVO_MAX_ENVS * (sizeof(double) + COVO_SIGMA_ADAPT_FLOATS * sizeof(float)) + (size_t)n_inst * COVO_NA * COVO_NA * sizeof(float);
}
// the age this CMA step of n_inst instances runs at, given where its factor lives: 0 (the first step after a reset) unless L holds the
// previous CMA step's factor for the same sample_sigma and instance count
static inline int covo_cma_step_age(const covo_ctx *h, const float *L, float sample_sigma, int n_inst)
{
    if (h->cma_age == 0) return 0;
    return (h->cma_L == L && L != nullptr && h->cma_L_sigma == sample_sigma && h->cma_L_n == n_inst) ? 1 : 0;
}
static inline void covo_cma_step_done(covo_ctx *h, const float *L, float sample_sigma, int n_inst)
{
    h->cma_age = 1;
    h->cma_L = L;
    h->cma_L_sigma = sample_sigma;
    h->cma_L_n = n_inst;
}
// passes per control step of this handle (1: today's step) and where pass j of instance 0 logs its cost minimum (instance e: + e * iters)
static inline int covo_sigma_period(const covo_ctx *h) { return h->sigma_period > 1 ? h->sigma_period : 1; }
// the age this covo-online step of n_inst instances runs at, given where its factor lives: 0 (refresh) unless the period is on, the
// schedule says reuse and L holds the previous step's factor for the same sample_sigma and instance count
static inline int covo_sigma_step_age(const covo_ctx *h, const float *L, float sample_sigma, int n_inst)
{
    if (covo_sigma_period(h) == 1 || h->sigma_age == 0) return 0;
    return (h->sigma_L == L && L != nullptr && h->sigma_L_sigma == sample_sigma && h->sigma_L_n == n_inst) ? h->sigma_age : 0;
}
// the step that ran at `age` has been enqueued and left its factor in L: advance the schedule
static inline void covo_sigma_step_done(covo_ctx *h, int age, const float *L, float sample_sigma, int n_inst)
{
    h->sigma_last_age = age;
    if (covo_sigma_period(h) == 1) return;
    h->sigma_L = L;
    h->sigma_L_sigma = sample_sigma;
    h->sigma_L_n = n_inst;
    h->sigma_age = (age + 1) % covo_sigma_period(h);
}
// the plan hold, scheduled the way the Sigma period is: the age this step of n_inst instances runs at -- 0 (a plan step) unless the
// hold is on, the schedule says hold and the last plan step left its latch for as many instances
static inline int covo_plan_hold(const covo_ctx *h) { return (h->plan_hold > 1 && h->hold_rows != nullptr) ? h->plan_hold : 1; }
static inline int covo_plan_step_age(const covo_ctx *h, int n_inst)
{
    if (covo_plan_hold(h) == 1 || h->plan_age == 0) return 0;
    return h->hold_latch_n == n_inst ? h->plan_age : 0;
}
// the step that ran at `age` has been enqueued (a plan step: with its latch): advance the schedule
static inline void covo_plan_step_done(covo_ctx *h, int age, int n_inst)
{
    h->plan_last_age = age;
    if (covo_plan_hold(h) == 1) return;
    if (age == 0) h->hold_latch_n = n_inst;
    h->plan_age = (age + 1) % covo_plan_hold(h);
}
static inline int covo_step_iters(const covo_ctx *h) { return (h->iter_log != nullptr && h->iters > 1) ? h->iters : 1; }
static inline float *covo_iter_slot(const covo_ctx *h, int pass) { return covo_step_iters(h) > 1 ? h->iter_log + pass : nullptr; }
// where the solver of this handle's steps writes the instances' temperatures (null: no floor) and for how many instances
// (the ESS floor, or the annealed step's standardised temperature, whose last pass's row is the handle's own temperature row)
static inline bool covo_ess_on(const covo_ctx *h) { return h->ess_min > 0.0f; }
static inline bool covo_anneal_on(const covo_ctx *h) { return h->anneal_passes > 0; }
static inline bool covo_anneal_sched_on(const covo_ctx *h) { return h->anneal_passes > 0 && h->anneal_sched != 0; }
static inline bool covo_nodes_on(const covo_ctx *h) { return h->nodes_M > 0; }
static inline bool covo_sigma_nodes_on(const covo_ctx *h) { return h->sn_M > 0; }
static inline bool covo_anneal_temp_on(const covo_ctx *h) { return h->anneal_passes > 0 && h->anneal_temp > 0.0f; }
static inline float *covo_lam_target(const covo_ctx *h)
{
    if (covo_ess_on(h)) return h->lam_out ? h->lam_out : h->lam_own;
    return covo_anneal_temp_on(h) ? h->lam_own : nullptr;
}
static inline int covo_lam_capacity(const covo_ctx *h) { return (covo_ess_on(h) && h->lam_out) ? h->lam_n : COVO_MAX_ENVS; }
// where the selector of this handle's steps writes the instances' rows (null: no elite-set update) and for how many instances
static inline float *covo_elite_target(const covo_ctx *h) { return h->elite_K > 0 ? (h->elite_out ? h->elite_out : h->elite_own) : nullptr; }
static inline int covo_elite_capacity(const covo_ctx *h) { return h->elite_out ? h->elite_n : COVO_MAX_ENVS; }
// a step whose update waits for all costs (ESS floor, standardised temperature, elite set): rollout without in-launch records, no
// one-launch small step
static inline bool covo_update_staged(const covo_ctx *h) { return covo_lam_target(h) != nullptr || covo_elite_target(h) != nullptr; }
static inline bool covo_plan_on(const covo_ctx *h) { return h->plan_out != nullptr || h->eplog[COVO_EPLOG_TRACE].log != nullptr; }
static inline bool covo_fan_on(const covo_ctx *h) { return h->fan_out != nullptr || h->eplog[COVO_EPLOG_FAN].log != nullptr; }
static inline bool covo_arb_on(const covo_ctx *h) { return h->arb_out != nullptr; }
static inline bool covo_refine_on(const covo_ctx *h) { return h->refine_out != nullptr; }
static inline bool covo_riccati_on(const covo_ctx *h) { return h->riccati_out != nullptr; }
static inline bool covo_feedback_on(const covo_ctx *h) { return h->feedback_out != nullptr; }
static inline bool covo_box_on(const covo_ctx *h) { return h->box_masks != nullptr; }
// where the steps of this handle write their diagnostics (null: off) and for how many instances
static inline float *covo_diag_target(const covo_ctx *h) { return h->diag_out ? h->diag_out : (h->eplog[COVO_EPLOG_DIAG].log ? h->diag_scratch : nullptr); }
static inline int covo_diag_capacity(const covo_ctx *h) { return h->diag_out ? h->diag_n : (h->eplog[COVO_EPLOG_DIAG].log ? COVO_MAX_ENVS : 0); }

// ---- the episode logs, one entry per kind: what the setters (step_attach.hip: set_episode_log), check_episode_logs and launch_episode_rows
// know about a log.  A new log adds its kind and its entry here, its place in check_episode_logs' order (step_attach.hip), and its
// cases in tests/host/step_attach_check.cpp with their lines of tests/golden/step_refusals.txt.
struct covo_eprows {
    const float *src;  // [n_inst][width]: the rows the step that has just been enqueued left (the Sigma log: Sigma adapt's rows, or null)
    int width;
};
struct covo_eplog_kind {
    const char *name, *setter;        // as check_episode_logs prints them
    bool (*on)(const covo_ctx *);     // the attachment the log follows is on (null: the log needs none) ...
    const char *off;                  // ... and what its setter says when it is not
    covo_eprows (*rows)(const covo_ctx *);  // what launch_episode_rows copies; null: the attachment's own launch writes the log's rows
};
static const covo_eplog_kind covo_eplog_kinds[COVO_EPLOG_ALL] = {
    {"episode temperature log", "covo_set_episode_rows, COVO_EPLOG_LAM", [](const covo_ctx *h) { return covo_lam_target(h) != nullptr; },
     "no ESS floor attached: call covo_set_step_ess_floor (ess_min > 0) first",
     [](const covo_ctx *h) { return covo_eprows{covo_lam_target(h), COVO_LAM_FLOATS}; }},
    {"episode elite log", "covo_set_episode_rows, COVO_EPLOG_ELITE", [](const covo_ctx *h) { return covo_elite_target(h) != nullptr; },
     "no elite-set update attached: call covo_set_step_elite (K > 0) first",
     [](const covo_ctx *h) { return covo_eprows{covo_elite_target(h), COVO_ELITE_FLOATS}; }},
    {"episode iteration log", "covo_set_episode_rows, COVO_EPLOG_ITERS", [](const covo_ctx *h) { return covo_step_iters(h) > 1; },
     "no iteration log attached: call covo_set_step_iters (iters > 1, iter_log) first",
     [](const covo_ctx *h) { return covo_eprows{covo_step_iters(h) > 1 ? h->iter_log : nullptr, covo_step_iters(h)}; }},
    {"episode Sigma log", "covo_set_episode_rows, COVO_EPLOG_SIGMA", [](const covo_ctx *h) { return covo_sigma_period(h) > 1; },
     "no Sigma period: call covo_set_step_sigma_period (period > 1) first",
     [](const covo_ctx *h) { return covo_eprows{covo_sigma_adapt_on(h) ? h->adapt_rows : nullptr, COVO_SIGMA_LOG_FLOATS}; }},
    {"episode posterior side-row log", "covo_set_episode_rows, COVO_EPLOG_POST_AUX", covo_post_cov_on,
     "no posterior covariance attached: call covo_set_step_post_cov first",
     [](const covo_ctx *h) { return covo_eprows{h->post_aux_out, COVO_POST_AUX_FLOATS}; }},
    {"episode posterior covariance log", "covo_set_episode_rows, COVO_EPLOG_POST_COV", covo_post_cov_on,
     "no posterior covariance attached: call covo_set_step_post_cov first",
     [](const covo_ctx *h) { return covo_eprows{h->post_cov_out, COVO_NA * COVO_NA}; }},
    {"diagnostic log", "covo_set_episode_diag_log", nullptr, nullptr,
     [](const covo_ctx *h) { return covo_eprows{covo_diag_target(h), COVO_DIAG_FLOATS}; }},
    {"episode trace", "covo_set_episode_trace", nullptr, nullptr, nullptr},
    {"episode fan log", "covo_set_episode_fan", [](const covo_ctx *h) { return h->fan_K > 0; },
     "covo_set_episode_fan: no fan size: call covo_set_step_fan (K, idx, n_inst) first", nullptr},
    {"episode arbiter log", "covo_set_episode_arbiter_log", covo_arb_on,
     "covo_set_episode_arbiter_log: no arbiter attached: call covo_set_step_arbiter first", nullptr},
    {"episode hold log", "covo_set_episode_hold_log", [](const covo_ctx *h) { return covo_plan_hold(h) > 1; },
     "covo_set_episode_hold_log: no plan hold: call covo_set_step_plan_hold (period > 1) first", nullptr},
};

// periodic / sin / drag / mixed (free.py:10-58): the disturbance model needs per-step force tables (disturb.hip)
static inline bool covo_needs_tables(const covo_env_params &p)
{
    return p.disturb_kind >= COVO_DISTURB_PERIODIC && p.disturb_kind <= COVO_DISTURB_MIXED;
}
// scale of the one shared gaussian vector of the sampling rollouts (free.py:66-70 from the shared step key): off under
// step_env(deterministic=True) (quadrotor.py:234-235)
static inline float covo_shared_noise_scale(const covo_env_params &p, bool rollout_deterministic)
{
    return (p.disturb_kind == COVO_DISTURB_GAUSSIAN && !rollout_deterministic) ? p.dyn_noise_scale : 0.0f;
}

void covo_set_error(const char *fmt, ...);
#define REQUIRE(cond, ...)            \
    do {                              \
        if (!(cond)) {                \
            covo_set_error(__VA_ARGS__); \
            return COVO_E_BADARG;     \
        }                             \
    } while (0)
#define CHECK_MODEL(p, what)               \
    do {                                   \
        const int rc_ = check_model(p, what); \
        if (rc_) return rc_;               \
    } while (0)

// step_attach.hip: everything a step checks before it launches, and the setters that touch no device.  Host code only, no HIP call:
// tests/host/step_attach_check.cpp walks every refusal, their order and every setter's bookkeeping on the CPU against
// tests/golden/step_refusals.txt.  A new attachment adds three things: its setter (there, or in capi.hip if it makes a HIP call),
// its lines in check_step_attachments, and its cases in step_attach_check.cpp with their lines of the golden file
int check_model(const covo_env_params *p, const char *what);
int check_step_attachments(const covo_ctx *h, int n_samples, int n_inst, bool sharded, int derive_keys, int mode, const float *a_cov,
                           const covo_env_params *params, const char *what, float gamma_sigma = 0.0f, bool fused_batch = false);
int check_ilqr_step(const covo_ctx *h, int n_inst, bool sharded, int derive_keys, const char *what);
int check_cma_step(const covo_ctx *h, int n_inst, bool sharded, const float *a_cov, const char *what);
int check_episode_logs(const covo_ctx *h, int first_row, int n_steps, const char *what);
int check_single_step(const covo_ctx *h, const covo_env_params *params, const covo_step_args *args, const char *what);
int check_batch_models(const covo_env_params *params, int E, bool env_step, const char *what);
int check_batch_step(covo_ctx *h, const covo_batch_args *args, const covo_batch_mode_args *m, const covo_env_params *params,
                     bool episode, const char *what, covo_batch_mode_args *norm);
// what every setter asks of the rows of a buffer it attaches (attached: there is one): "<setter>: n_inst=%d outside (0, COVO_MAX_ENVS]"
int check_setter_rows(const char *setter, bool attached, int n_inst);

// hipFuncSetAttribute is per DEVICE: a one-time opt-in (dynamic LDS above 64 KB) guarded by a process-wide `static bool` was set on
// the first device only.  Returns true the first time it is called for the current device with this mask.
static inline bool covo_first_on_device(unsigned long long &mask)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (mask & bit) return false;
    mask |= bit;
    return true;
}

// A pointer a kernel LOADS from memory (a field of a per-instance argument block, a table of buffers) is a GENERIC pointer to the
// compiler: every access through it becomes a flat_load / flat_store, which counts on BOTH vmcnt and lgkmcnt -- an
// `s_waitcnt lgkmcnt(0)` in front of an LDS hand-off or a barrier then also drains the loads in flight (round 6: the env-batched
// rollout kept its 12 prefetched stripes for two steps instead of twelve and ran 30 % slower than the same kernel taking its
// pointers as kernel arguments, which clang knows to be global).  rebase_global re-expresses such a pointer as
// (a kernel-argument pointer of the same kind) + (byte distance between the two): the address space then follows from the kernel
// argument.  The distance goes through an empty asm, else InstCombine folds base + (p - base) back into p.  Neither a cast
// through address space 1 and back nor an llvm.assume(!is.shared && !is.private) survives to InferAddressSpaces here (ROCm 7.2).
template <class T>
__device__ __forceinline__ T *rebase_global(T *kernarg_base, T *loaded)
{
    long long off = (long long)(uintptr_t)loaded - (long long)(uintptr_t)kernarg_base;
    int lo = (int)off, hi = (int)(off >> 32);
    asm volatile("" : "+s"(lo), "+s"(hi));
    off = ((long long)hi << 32) | (unsigned)lo;
    return (T *)((const char *)kernarg_base + off);
}

// Which launches a step enqueues: all of them, except in the graphs covo_debug_time_step / covo_debug_time_batched capture of a part
// of a step.  step: enqueue_step's launch groups (1 begin, 2 Hessian, 4 Sigma, 8 noise GEMM, 16 rollout, 32 softmax update); hess:
// bit k = kernel k of hessian_adj.hip; sigma_stages: how far the Sigma chain goes (1 squarings, 2 + the Ritz scan, 3 + Newton-Schulz,
// 4 + finalize: launch_sigma_ns).
struct DebugMasks {
    int step = 63, hess = 15, sigma_stages = 4;
};

#define COVO_CHECK_HIP(expr)                                                         \
    do {                                                                             \
        hipError_t _e = (expr);                                                      \
        if (_e != hipSuccess) {                                                      \
            covo_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return (int)_e;                                                          \
        }                                                                            \
    } while (0)

template <class U>
__host__ __device__ inline qm::Consts<U> make_consts(const covo_env_params &p)
{
    qm::Consts<U> c;
    // the model constants are the fp32 parameter values (JAX default dtype); derived constants are
    // formed in the working precision U from them (U = float reproduces the reference's fp32 products)
    c.thrust_half = U(0.5) * U(p.max_thrust) * U(p.action_scale);
    for (int i = 0; i < 3; ++i) c.komega[i] = U(p.max_omega[i]) * U(p.action_scale);
    c.dt = U(p.dt);
    c.half_dt = U(0.5) * U(p.dt);
    c.neg_g = -U(p.g);
    c.inv_m = U(1) / U(p.m);
    c.alpha = U(p.alpha_bodyrate);
    c.one_m_alpha = U(1) - U(p.alpha_bodyrate);
    c.pos_limit = U(p.pos_limit);
    return c;
}

// ---- wave-level reductions over 64 lanes (DPP-lowered by the compiler from __shfl_xor)
__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// launch entry points implemented in the .hip files (host functions)
int launch_randn(uint32_t k0, uint32_t k1, int64_t off, int n_samples, int n_cols, float *out, hipStream_t s);
int launch_randn_jax(uint32_t k0, uint32_t k1, int64_t n_total, int64_t off, int n_samples, int mppi, float *out, hipStream_t s);
// Host-side launch descriptors: one per kernel family, filled field by field; every field has a default and a null /
// zero field means "off".  Kernel-argument structs (RolloutArgs, AdjArgs, ...) are built from them inside the launch functions.
//
// threads per workgroup the noise GEMM launches with for (N, batch) (noise_gemm.hip: 512 once a launch fills the chip, else 256);
// the rollout's XCD-affine sample mapping follows it (rollout.hip: xcd_remap = 64-sample groups per GEMM workgroup)
int noise_gemm_block_threads(int N, int batch);
int noise_gemm_groups_per_workgroup(int N, int batch);
struct CovDeferred {
    const double *Z[2], *Zt[2];  // the two Newton-Schulz buffers of Z and of its stored transpose
    const double *zbuf;          // != 0: buffer 1 holds the final iterate
    const double *cz;            // Sigma = cz sym(Z) (NaN when a grid barrier of the chain timed out)
    const double *zcoef, *u;     // deflated chain (sigma_ns.hip): Z = Z~ + zcoef u u^T (*zcoef == 0: off)
    float *out;                  // a_cov [128][128]; null: nothing deferred
};
// a = clip(mu + L eps): launch_noise_gemm (dense L [128][128]) and launch_noise_blockdiag (MPPI's Ls [H][4][4]; it has no
// eps_tiled / state_for_time / cov; batch > 1 with the in-kernel draw and dyn only)
struct NoiseDesc {
    const float *L = nullptr;
    const float *mu = nullptr;
    const float *eps = nullptr;        // [N][128] epsilon; null: drawn in-kernel from (key, sample_offset + n) (rng_device.hpp)
    bool eps_tiled = false;            // eps is the tile-ordered image of eps_tiles.hpp
    uint32_t key[2] = {0u, 0u};        // the in-kernel draw's key ...
    const uint32_t *dyn = nullptr;     // ... or, non-null, where {key0, key1} lie in device memory
    int64_t sample_offset = 0;         // global id of local sample 0 (in-kernel draw)
    int N = 0;
    float *a = nullptr;                // [H][N][4] action stripes
    const float *state_for_time = nullptr;  // non-null: L is a table [n_table][128][128], row state.time is used (covo-offline)
    int n_table = 0;
    int batch = 1;                     // batch > 1 (in-kernel Philox or tiled eps only): dense per-instance L, mu, dyn, a
    // batch_table (launch_noise_gemm, in-kernel Philox; the staged env-batched covo-offline step): L is instance 0's table
    // [n_table][128][128], instance y's lies table_stride floats on (0: one shared table) and its row is picked by the time of
    // state_for_time + y * COVO_STATE_FLOATS -- instead of a dense per-instance L and one state
    bool batch_table = false;
    int64_t table_stride = 0;
    // cov != null (fused covo-online step): a_cov = cz sym(Z) is NOT written by the chain's finalize launch -- one workgroup that
    // everything after it waits for -- but by the first workgroups of the noise GEMM that follows (same expression, same bits);
    // launch_sigma_ns fills *cov with where Z, its transpose and the scalars live.
    const CovDeferred *cov = nullptr;
    bool propagate_nan = false;        // COVO_FLAG_PROPAGATE_NAN: jnp.clip's NaN semantics
};
int launch_noise_gemm(const NoiseDesc &d, hipStream_t s);
int launch_noise_blockdiag(const NoiseDesc &d, hipStream_t s);
// noise_nodes.hip: a = clip(mu + B eps_nodes) with B = slice `pass` of table [.][H][n_nodes] and eps_nodes the first n_nodes normal4
// of the block-diagonal kernel's stream (in-kernel draw only; d.L / eps_tiled / state_for_time / cov are not read)
int launch_noise_nodes(const NoiseDesc &d, const float *table, int pass, int n_nodes, hipStream_t s);
// sigma_nodes.hip: per matrix of R [batch][128][128], Sigma_M = optimize_sigma(P^T sym(R) P) double [batch][d][d] (P = W (x) I_4,
// W_dev device [32][M], d = 4 M), G = fp32(P chol(Sigma_M)) [batch][128][d], Sigma = fp32(P Sigma_M P^T) [batch][128][128] (nullable)
// and the side rows [batch][COVO_SIGMA_NODES_FLOATS] (nullable), one workgroup each; launch_noise_factor: a = clip(mu + G eps) with
// eps the first M normal4 of the block-diagonal kernel's stream (in-kernel draw only; batch > 1: G, mu, dyn, a per instance)
int launch_sigma_nodes(const double *R, int batch, const double *W_dev, int M, float sample_sigma, double *SigmaM, float *G, float *Sigma,
                       float *rows, hipStream_t s);
int launch_noise_factor(const NoiseDesc &d, const float *G, int M, hipStream_t s);
static inline bool covo_propagate_nan(const covo_ctx *h) { return (h->cfg.flags & COVO_FLAG_PROPAGATE_NAN) != 0; }
// how the rollout treats the action stripes it reads (RolloutArgs::clip)
enum RolloutClip {
    ROLLOUT_CLIP_TRUSTED = 0,  // the producer guarantees clipped stripes
    ROLLOUT_CLIP_REAPPLY = 1,  // re-apply step_env's clip (quadrotor.py:223,258)
    ROLLOUT_CLIP_REAPPLY_NAN = 2,  // the same, and the re-clip keeps a NaN (COVO_FLAG_PROPAGATE_NAN)
};
// one rollout over N samples: launch_rollout, rollout_fill_args (instance `index` of an env-batched launch) and
// fill_rollout_args (rollout_common.hpp: the RolloutArgs block itself; step_small.hip, plan_trace.hip)
struct RolloutDesc {
    const float *state = nullptr;
    const float *pos_traj = nullptr, *vel_traj = nullptr;
    int T = 0;
    const covo_env_params *params = nullptr;
    const float *f_shared = nullptr;      // host {fx, fy, fz}: the one shared disturbance vector of steps >= 1 (null: zero)
    const float *f_shared_dev = nullptr;  // the same in device memory (graph replays), overrides f_shared
    const float *f_tab = nullptr;         // [H][4] per-step disturbance table (disturb.hip), device
    const float *a = nullptr;             // [H][N][4] action stripes
    int N = 0;
    float discount = 1.0f;
    float *cost = nullptr;                // [N]
    float *groupmin = nullptr;            // [ceil(N/64)] per-wave cost minima
    double *pos_stats = nullptr;          // [H*6] position statistics (launch_rollout only), with their scratch ...
    double *stats_ws = nullptr;           // ... [workgroups][H*6]
    float *records = nullptr;             // one online-softmax record per workgroup (rollout.hip), at temperature ...
    float lam = 0.0f;
    float *diag_rec = nullptr;            // with records: one diagnostic record per workgroup next to them (softmax_merge.hpp)
    int xcd_groups = 0;  // 64-sample groups per workgroup of the kernel that wrote `a` (0: the noise GEMM's for this N)
    RolloutClip clip = ROLLOUT_CLIP_REAPPLY;
};
int launch_rollout(const RolloutDesc &d, hipStream_t s);
int launch_disturb_table(const covo_env_params &p, const float *state, int batch, const uint32_t *keys_dev, uint32_t key0,
                         uint32_t key1, int key_mode, int deterministic, float *out, hipStream_t s);
int launch_disturb_tables_step(const covo_env_params &p, const float *state, const uint32_t *dyn, int rollout_deterministic,
                               float *tab_rollout, float *tab_hess, hipStream_t s);
// env-batched step: per-instance models (dm::Model[n], host-filled, copied to the device by the caller) and both tables of
// every instance in one launch ([n][H][4] each; raw keys at dyn[12 e + 10..11]; tab_hess null: the rollouts' tables only)
size_t disturb_models_bytes(int n);
void disturb_fill_models(const covo_env_params *params, int n, void *out);
int launch_disturb_tables_batched(const void *models_dev, const float *states, const uint32_t *dyn, int n_envs,
                                  int rollout_deterministic, float *tab_rollout, float *tab_hess, hipStream_t s);
int rollout_workgroups(int N, bool stats, int nbatch = 1);
size_t rollout_args_bytes(int n);
void rollout_fill_args(void *out, int index, const RolloutDesc &d);  // (no position statistics: pos_stats is not read)
int launch_rollout_batched(const void *args_host, const void *args_dev, int nbatch, hipStream_t s);
// The softmax update (covo.py:266-275; reduce.hip).  Stage 1 + merge from the costs: launch_softmax_reduce, and with MPPI's
// covariance adaptation (mppi.py:109-125) launch_softmax_update_cov; the merge alone from records: launch_merge, launch_merge_cov.
struct UpdateDesc {
    // input, from the costs ...
    const float *cost = nullptr;      // [batch][N]
    const float *a = nullptr;         // [batch][H][N][4]
    int N = 0;                        // samples (launch_merge: only the diagnostics' normalisation reads it)
    const float *blockmin = nullptr;  // [n_blockmin] per-wave cost minima; null: formed first (h->ws_blockmin)
    int n_blockmin = 0;
    float *partials_ws = nullptr;     // stage-1 records [batch][blocks][COVO_PARTIAL_FLOATS]; null: h->ws_partials
    // ... or from G records per instance, `stride` floats apart (launch_merge / launch_merge_cov)
    const float *partials = nullptr;
    int G = 0;
    int stride = COVO_PARTIAL_FLOATS;
    // the blend: a_mean_out != null finishes on this GPU (normalise + blend with a_mean_old)
    const float *a_mean_old = nullptr;  // (the covariance kinds centre their second moments on it in every case)
    float gamma_mean = 1.0f;
    float *a_mean_out = nullptr;
    // a_mean_out (a_cov_out for the covariance kinds) == null: a sample-sharded rank, the merged record goes here
    float *partial_out = nullptr;
    // MPPI's covariance adaptation
    const float *a_cov_old = nullptr;
    float gamma_sigma = 0.0f;
    float *a_cov_out = nullptr;
    int batch = 1;                    // batch > 1: dense per-instance slices, own partials_ws
    // launch_softmax_update_cov with an instance dimension (the staged env-batched MPPI step): the records with second moments
    // [batch][blocks][452] and where the diagnostics' merge leaves its merged records [batch][COVO_PARTIAL_FLOATS]; with them
    // batch, diag_rec, a_mean_old / a_cov_old / a_cov_out [batch][...] and iter_stride are read.  null: one instance, the handle's
    // own ws_partials_cov / ws_diag_rec / ws_partials
    float *partials_cov_ws = nullptr;
    float *diag_merge_ws = nullptr;
    // the sampling diagnostics, with a final update only
    float *diag_rec = nullptr;        // stage-1 diagnostic records [batch][blocks or G][4] (scratch of launch_softmax_reduce, input of launch_merge)
    float *diag_out = nullptr;        // [batch][COVO_DIAG_FLOATS]
    // the ESS floor (launch_softmax_reduce / launch_softmax_update_cov, final updates only): instance e takes 1 / lambda from
    // lam_rows[e][1] in device memory -- the solver's output, ess_lambda.hip -- instead of the handle's configured temperature
    const float *lam_rows = nullptr;  // [batch][COVO_LAM_FLOATS]
    // the elite-set update (launch_elite_reduce / launch_elite_update_cov, final updates only): instance e's weights are 1 for the
    // samples whose key is at most the threshold in elite_rows[e] -- the selector's output, elite_select.hip -- and 0 otherwise
    const float *elite_rows = nullptr;  // [batch][COVO_ELITE_FLOATS]
    // an iterated step (covo_set_step_iters), final updates only: the merge also stores its cost minimum m, instance e's at
    // iter_out[e * iter_stride] (the caller has added the pass index)
    float *iter_out = nullptr;
    int iter_stride = 0;
};
// the ESS floor's solver (ess_lambda.hip): out [n_inst][COVO_LAM_FLOATS] from cost [n_inst][N]; groupmin [n_inst][ceil(N/64)] as the
// rollout leaves it, or null (the minimum is then formed from the costs)
int launch_ess_lambda(const float *cost, int N, int n_inst, const float *groupmin, float lam0, float ess_min, float *out, hipStream_t s);
// the annealed step's launches (cost_standardise.hip).  The standardising solver: out [n_inst][COVO_LAM_FLOATS] from cost [n_inst][N] --
// {lam_eff, 1 / lam_eff, std, bits(|F| | fallback << 31)} with lam_eff = temp x the population standard deviation of the finite costs
// (lam0 on fallback); pass_out: instance e's row again at pass_out + e * pass_stride, or null.  The schedule launch: row `pass` of
// table [.][H] -> Ls [n_inst][H][4][4] = sigma I and a_cov [n_inst][H][4][4] = sigma^2 I
int launch_cost_standardise(const float *cost, int N, int n_inst, float lam0, float temp, float *out, float *pass_out, int pass_stride,
                            hipStream_t s);
int launch_anneal_schedule(const float *table, int pass, float *Ls, float *a_cov, int n_inst, hipStream_t s);
int launch_softmax_reduce(covo_ctx *h, const UpdateDesc &d, hipStream_t s);
// reduce_lam.hip: what the two launch functions do with d.lam_rows set
int launch_softmax_reduce_lam(covo_ctx *h, const UpdateDesc &d, hipStream_t s);
int launch_softmax_update_cov_lam(covo_ctx *h, const UpdateDesc &d, hipStream_t s);
int launch_merge(const UpdateDesc &d, float lam, hipStream_t s);
// the elite-set update: the selector (elite_select.hip): out [n_inst][COVO_ELITE_FLOATS] from cost [n_inst][N], 1 <= K <= N; and
// what takes the place of launch_softmax_reduce / launch_softmax_update_cov with d.elite_rows set (reduce_elite.hip)
int launch_elite_select(const float *cost, int N, int n_inst, int K, float *out, hipStream_t s);
int launch_elite_reduce(covo_ctx *h, const UpdateDesc &d, hipStream_t s);
int launch_elite_update_cov(covo_ctx *h, const UpdateDesc &d, hipStream_t s);
// exchange.hip: the rank records of a sample-sharded step and their peer-write exchange
int launch_rank_stats_sum(const float *records, int G, int record_floats, double *out, hipStream_t s);  // COVO_RANK_RECORD_[COV_]FLOATS
int exchange_create(covo_ctx *h, int world, int rank, void *handle_out);
int exchange_connect(covo_ctx *h, const void *handles);
int exchange_set_timeout(covo_ctx *h, double seconds);
void exchange_destroy(covo_ctx *h);
bool exchange_ready(const covo_ctx *h);
int exchange_world(const covo_ctx *h);
int exchange_records(covo_ctx *h, const float *record, float *gathered_dst, const float **gathered_out, hipStream_t s,
                     int nfloats = COVO_RANK_RECORD_FLOATS);
size_t softmax_cov_workspace_floats(int max_blocks);
int softmax_stage1_blocks(const covo_ctx *h, int N);  // workgroups (= records) of the stand-alone stage 1 over N samples
// a_cov_out == null: this rank's record {m, s, v[128], pad[2], S2[320]} (unnormalised) goes to partial_out -- the first
// COVO_PARTIAL_FLOATS + 320 floats of a COVO_RANK_RECORD_COV_FLOATS rank record
int launch_softmax_update_cov(covo_ctx *h, const UpdateDesc &d, hipStream_t s);
int launch_merge_cov(const UpdateDesc &d, float lam, hipStream_t s);
// the diagnostics of a covariance update: the G records of ws_partials_cov and ws_diag_rec -> diag_out (reduce.hip; N: the sample count)
void launch_merge_cov_diag(covo_ctx *h, int G, float inv_lam, float *diag_out, int N, hipStream_t s);
// post_cov.hip: the weighted 128 x 128 sample covariance of n_inst dense instances (covo_weighted_cov, covo_set_step_post_cov).  The
// weights: elite_rows (the selector's rows of the step) or, with elite_rows null, elite_K > 0 (the selector runs first); else
// lam_rows (the ESS solver's rows); else softmax at lam
struct PostCovDesc {
    const float *a = nullptr;     // [n_inst][H][N][4]
    const float *cost = nullptr;  // [n_inst][N]
    const float *mu = nullptr;    // [n_inst][128] the mean the samples were drawn around
    int N = 0, n_inst = 1;
    float lam = 0.0f;
    const float *lam_rows = nullptr;
    const float *elite_rows = nullptr;
    int elite_K = 0;
    float *cov_out = nullptr;     // [n_inst][128][128]
    float *aux_out = nullptr;     // [n_inst][COVO_POST_AUX_FLOATS]
};
int launch_weighted_cov(covo_ctx *h, const PostCovDesc &d, hipStream_t s);
int launch_post_cov_after(covo_ctx *h, const float *a, const float *cost, const float *mu, int N, int n_inst, hipStream_t s);
int post_cov_reserve(covo_ctx *h, int n_inst);
void post_cov_state_destroy(covo_ctx *h);
int launch_shift_mean(const float *in, float *out, hipStream_t s);
size_t hessian_workspace_bytes(int batch);
struct SymStatsOut;  // sym_stats.hpp
// the step's begin work folded into the Hessian's first launch (eager covo-online steps; hessian_adj.hip: AdjArgs): the
// caller's unshifted mean, where the per-step scalars and the sequence number live, and the 48-byte block of step_begin.hpp
struct HessBegin {
    int pass;                 // > 0 (covo_set_step_iters): no shift, the raw key is the advanced one of dyn_out[10..11]
    const float *a_mean_raw;
    uint32_t *dyn_out;
    unsigned *seq;
    const void *blk;  // DynBlock
    int derive_keys;
    float shared_noise_scale;
};
// the Hessian of the cost in the mean: launch_hessian (second-order adjoint, hessian_adj.hip) and launch_hessian_pairs (hessian.hip;
// it reads neither stats, status_dev nor begin)
struct HessianDesc {
    const float *state = nullptr;   // [batch][32]
    const float *pos_traj = nullptr, *vel_traj = nullptr;
    int T = 0;
    const covo_env_params *params = nullptr;  // instance 0's (all instances share reward and disturbance kind)
    const float *a_mean = nullptr;  // [batch][128]
    int batch = 1;
    double *R = nullptr;            // [batch][128][128]
    const void *consts_dev = nullptr;   // qm::Consts<double>[batch]: per-instance constants (hessian_fill_consts), with ...
    size_t traj_stride = 0;             // ... per-instance trajectories, this many floats apart
    const SymStatsOut *stats = nullptr;  // KD also leaves the Sigma chain's input statistics (sym_stats.hpp)
    const float *f_tab = nullptr;        // [batch][H][4] per-step disturbance table (disturb.hip), device
    const void *models_dev = nullptr;    // dm::Model[batch] next to consts_dev (drag / mixed with per-instance parameters)
    int *status_dev = nullptr;           // the handle's sticky status word: COVO_DEVSTAT_ADJOINT on a costate time-out
    const HessBegin *begin = nullptr;    // batch 1: KB also does the step's begin work (a_mean = where the shifted mean goes)
};
int launch_hessian(const HessianDesc &d, void *workspace, hipStream_t s, const DebugMasks &dbg);
// cost_gradient.hip: the gradient of the same objective by the first-order adjoint, g_out [batch][128] fp64; d as for launch_hessian
// (R, stats, status_dev and begin are not read), the workspace the gradient's own (cost_gradient_workspace_bytes)
size_t cost_gradient_workspace_bytes(int batch);
int launch_cost_gradient(const HessianDesc &d, double *g_out, void *workspace, hipStream_t s);
// the Hessian's inputs at the means `a` of `batch` instances that share trajectories and constants: what the primitives (capi.hip) and
// the after-step frame (step.hip) hand the gradient and the sweep
static inline HessianDesc covo_hessian_inputs(const float *state, const float *pos_traj, const float *vel_traj, int T,
                                              const covo_env_params *params, const float *a, const float *f_tab, int batch)
{
    HessianDesc d;
    d.state = state;
    d.pos_traj = pos_traj;
    d.vel_traj = vel_traj;
    d.T = T;
    d.params = params;
    d.a_mean = a;
    d.f_tab = f_tab;
    d.batch = batch;
    return d;
}
// where launches 1 | 2 of launch_hessian leave their results in one entry's workspace, in doubles (hessian_adj_body.hpp: WS_*): x_k
// [32][16], df_k/dz [32][nx][nx + 4], lam_k [33][16], Mxx [32][16][16], Mxu [32][16][4], Muu [32][4][4]; entries lie `count` apart
struct HessianWsLayout {
    int nx;
    size_t count, x, jf, lam, mxx, mxu, muu;
};
HessianWsLayout hessian_workspace_layout(bool fs);
// riccati.hip: launches 1 | 2 of launch_hessian into `workspace` (riccati_workspace_bytes: a Hessian workspace, then the sweep's
// slices), then the Riccati sweep over the stage blocks they leave: d = -(R + mu I)^-1 g on the lowest rung mu = reg0 4^j, j < 8,
// at which R + mu I is positive definite, with the gains and the nominal states along the plan.  d as for launch_hessian (R, stats
// and begin are not read)
struct RiccatiOut {
    double *d = nullptr;     // [batch][128]
    double *g = nullptr;     // [batch][128], nullable: the gradient the sweep formed
    double *K = nullptr;     // [batch][H][4][16], nullable
    double *kff = nullptr;   // [batch][H][4], nullable
    double *x = nullptr;     // [batch][H][16], nullable
    double *side = nullptr;  // [batch][COVO_RICCATI_SIDE] {mu, rung, smallest pivot, flags}, nullable
    // the box form: every stage solves its QP on -1 <= clip(b) + du <= 1 (riccati.hip); masks: the winning rung's clamped coordinates
    bool box = false;
    int *masks = nullptr;    // [batch][H] bits 0-3: coordinate i clamped at lo, 4-7: at hi; nullable (read only when box)
};
size_t riccati_workspace_bytes(int batch);
int launch_riccati(const HessianDesc &d, double reg0, const RiccatiOut &o, void *workspace, hipStream_t s);
size_t hessian_consts_bytes(int n);
void hessian_fill_consts(const covo_env_params *params, int n, void *out);
// the per-pair hyper-dual rollout version (hessian.hip): slower, independent derivation, kept as a cross-check
int launch_hessian_pairs(const HessianDesc &d, hipStream_t s);
int launch_sigma(const double *R, int batch, float sample_sigma, float *Sigma, float *L, unsigned long long *prof,
                 hipStream_t s);
size_t sigma_ns_workspace_bytes(int batch);
struct EpsGenArgs;  // eps_tiles.hpp
struct StreamGemmArgs {
    const float *mu;        // the shifted mean [128]
    const uint32_t *dyn;    // {key0, key1}: the step's sampling key in device memory
    int64_t sample_offset;  // global id of local sample 0
    int N;                  // samples of this shard
    float *a_out;           // [H][N][4] action stripes
    float *L_stream;        // [128][128] fp32: chol(Sigma), written panel by panel (write-through) while the workers read it
    unsigned *sync;         // [16]: [0] the step's sequence number (bumped by the begin launch), [1 + p]: panel p (16 columns) of
                            // L_stream is complete for the sequence number it holds
    float *a_cov_out;       // nullable: a_cov [128][128]
    int nanp;               // COVO_FLAG_PROPAGATE_NAN
};
// Sigma = optimize_sigma(R) and its Cholesky factor without an eigendecomposition (sigma_ns.hip)
struct SigmaNsDesc {
    const double *R = nullptr;   // [batch][128][128]
    int batch = 1;
    float sample_sigma = 0.0f;
    float *Sigma = nullptr;      // [batch][128][128] a_cov, nullable
    float *L = nullptr;          // [batch][128][128] chol(Sigma)
    const EpsGenArgs *gen = nullptr;  // fused step: the finalize launch also draws the step's epsilon in tile order (eps_tiles.hpp)
    int *status = nullptr;       // the handle's sticky status word (a timed-out grid barrier raises COVO_DEVSTAT_GRID_BARRIER there,
                                 // next to the NaN outputs)
    bool persistent_ok = true;   // false (COVO_FLAG_SHARED_DEVICE): every phase its own launch
    CovDeferred *cov = nullptr;  // out: a_cov is left to the consumer of L (NoiseDesc::cov)
    // fused steps: R is exactly symmetric and its statistics (sym_stats.hpp) are already in the workspace -- left there by the
    // Hessian's last launch through sigma_ns_stats_out -- so the chain starts without its prep launch
    bool r_has_stats = false;
    // fused covo-online step, one matrix, persistent launches allowed: the noise GEMM of the step is carried out INSIDE the finalize
    // launch, streamed under the factorisation (sigma_ns.hip: ns_finalize_stream_kernel); *streamed (out) says whether it was (else
    // the caller launches the GEMM).  gen / cov / Sigma / L are then unused: a_cov goes to stream->a_cov_out, the factor to
    // stream->L_stream.
    const StreamGemmArgs *stream = nullptr;
    bool *streamed = nullptr;
};
int launch_sigma_ns(const CovoOpts &opt, const SigmaNsDesc &d, void *workspace, hipStream_t s, const DebugMasks &dbg);
SymStatsOut sigma_ns_stats_out(void *workspace, int batch = 1);
// where the chain that last ran on `workspace` for `batch` matrices left sum_i log diag(chol(R + delta I)) of matrix 0; matrix e's lies
// *stride_doubles further on per matrix (newton_refine.hip: c^2 of the step)
const double *sigma_ns_sumlogB(void *workspace, int batch, size_t *stride_doubles);
void step_state_destroy(covo_ctx *h);
void step_graphs_drop(covo_ctx *h);  // every captured step graph of the handle goes; the next step runs eagerly, the one after captures
// h->ws_sigma / h->ws_hess (ws, bytes) to at least `need` bytes: only for batch sizes not seen before, never inside the steady-state
// step.  The captured step graphs hold the old address in their kernel nodes: they are dropped before it is freed.
int covo_grow_workspace(covo_ctx *h, void **ws, size_t *bytes, size_t need, hipStream_t s);
void batch_state_destroy(covo_ctx *h);
int covo_debug_time_batched_impl(covo_ctx *h, int step_mask, int reps, float *us_out, hipStream_t run);
int covo_debug_batched_hessians_impl(covo_ctx *h, double *out, int64_t offset_doubles, int64_t count, hipStream_t s);
int covo_debug_sigma_factor_impl(covo_ctx *h, int batched, float *out, int64_t count, hipStream_t s);
int covo_step_batched_impl(covo_ctx *h, const covo_batch_args *args, const covo_env_params *params, const uint32_t *keys,
                           hipStream_t s, int mode = COVO_MODE_COVO_ONLINE);  // (or COVO_MODE_CMA)
int covo_step_batched_small_impl(covo_ctx *h, const covo_batch_mode_args *m, const covo_env_params *params, const uint32_t *keys,
                                 hipStream_t s);
// the same step as its staged launch sequence (covo_set_step_batched_staged): begin | tables | sampling | rollout | update per pass
int covo_step_batched_staged_impl(covo_ctx *h, const covo_batch_mode_args *m, const covo_env_params *params, const uint32_t *keys,
                                  hipStream_t s);
// which of the two the handle's MPPI / covo-offline batch runs
static inline bool covo_batched_staged(const covo_ctx *h) { return h->batched_staged != 0; }
// null: every instance of the batch can take the fused launch; else why not (instance index in *which)
const char *batch_small_refusal(const covo_ctx *h, const covo_batch_mode_args *m, const covo_env_params *params, int *which);
int covo_step_impl(covo_ctx *h, const covo_env_params *params, const covo_step_args *args, uint32_t key0, uint32_t key1,
                   const float *f_shared, hipStream_t s);
int launch_cholesky(const float *A, int n, int batch, float *L, hipStream_t s);
// sigma_shift.hip: the covariance of a reuse step from the previous step's factor L_in [batch][128][128] (fp32, lower): L_out its
// shifted, volume-normalised factor (may be L_in), Sigma_out = L_out L_out^T; all three 16-byte aligned
int launch_sigma_shift(const float *L_in, int batch, float sample_sigma, float *Sigma_out, float *L_out, hipStream_t s);
// sigma_adapt.hip: the same step with the previous step's posterior covariance C [batch][128][128] blended in at weight gamma in
// [0, 1) (0: C is not read): Sigma' = c ((1 - gamma) S(L L^T) + gamma S(C)) and its factor; rows_out [batch][4] = {fallback, c,
// log det M, 0} or null; L_out may be L_in; all 16-byte aligned
int launch_sigma_adapt(const float *L_in, const float *C, int batch, float gamma, float sample_sigma, float *Sigma_out, float *L_out,
                       float *rows_out, hipStream_t s);
int launch_sigma_adapt_idle(float *rows_out, int n_inst, hipStream_t s);  // a refresh step's rows {0, 1, 0, 0}
// cma_path.hip: the CMA controller's step size behind sigma_adapt.hip's shape (the header of that file has the formulas).  One
// workgroup per instance; writes p, log_s (on a fall-back: their mended entry values), L_out, Sigma_out and rows_out, nothing else
struct CmaPathDesc {
    const float *L_prev = nullptr;      // [batch][128][128] the factor the previous step sampled from (lower; all of it is read)
    const float *aux = nullptr;         // instance e's {d[128], W, ...} of the previous step at aux + e * aux_stride (post_cov.hip's side row)
    int aux_stride = COVO_POST_AUX_FLOATS;
    const float *ess = nullptr;         // instance e's effective sample size of the previous step at ess + e * ess_stride
    int ess_stride = COVO_DIAG_FLOATS;
    const float *L_hat = nullptr;       // [batch][128][128] the shape's factor ...
    const float *Sigma_hat = nullptr;   // ... and covariance (sigma_adapt.hip's outputs); Sigma_out may be Sigma_hat
    const float *shape_rows = nullptr;  // [batch][COVO_SIGMA_ADAPT_FLOATS] the shape kernel's rows (flag 4), or null
    int batch = 1;
    int n_samples = 1;                  // N: mu_eff = clamp(ess, 1, N)
    int step_size = 1;                  // 0: s = 1, copy only, p and log_s are not touched
    double damping = 1.0;
    double log_s_min = 0.0, log_s_max = 0.0;  // log of the fp32 bounds, taken in fp64 on the host
    double *p = nullptr;                // [batch][128] in/out
    double *log_s = nullptr;            // [batch] in/out
    float *L_out = nullptr;             // [batch][128][128] fp32(s L_hat); may be L_prev
    float *Sigma_out = nullptr;         // [batch][128][128] fp32(s^2 Sigma_hat)
    float *rows_out = nullptr;          // [batch][COVO_CMA_FLOATS] {s, log s, |p|, |z|, mu_eff, c_sigma, d_sigma, flags}
};
int launch_cma_path(const CmaPathDesc &d, hipStream_t s);
// L = sigma I, Sigma = sigma^2 I, p = 0, log s = 0 and the neutral row {1, 0, 0, 0, 0, 0, 0, 0} for `batch` instances; null: skipped
int launch_cma_reset(float sample_sigma, int batch, float *L, float *Sigma, double *p, double *log_s, float *rows, hipStream_t s);
size_t env_step_inst_bytes(int n);
void env_step_fill_inst(const covo_env_params *params, int n, void *out);  // host: EnvInst[n] (to be copied to the device)
int launch_env_step_batched(float *states, float *noisy, const float *pos_traj, const float *vel_traj, const float *acc_traj, int T,
                            const covo_env_params &params0, const void *inst_dev, int E, const float *a_mean,
                            const uint32_t *step_keys, int noisy_on, float obs_noise_scale, float *log, int log_stride,
                            int log_index, hipStream_t s);
int batch_env_inst(covo_ctx *h, const covo_env_params *params, int E, hipStream_t s, const void **inst_dev);  // step.hip
// episode_rows.hip: the rows the step that has just been enqueued (the one that ran at Sigma age `age`) left in its attachments ->
// row `index` of every instance's attached covo_set_episode_rows log (no-op with none attached)
int launch_episode_rows(const covo_ctx *h, int n_inst, int index, int age, hipStream_t s);
// after_step.hpp, plan_trace.hip, sample_fan.hip, update_arbiter.hip: what the launches behind a step need to know about ONE instance of
// the step that has just been enqueued -- the inputs its sample rollouts had.  key_mem (batched steps): the instance's raw rng_act in device memory; else key / f_shared as covo_mpc_step got them
struct PlanInstDesc {
    const float *state;       // the noisy state the step planned from [32]
    const float *pos_traj, *vel_traj;
    int T;
    const covo_env_params *params;
    const float *a_mean;      // [128] the mean the step leaves
    const float *a;           // [H][N][4] the step's action stripes (the sample fan, the update arbiter)
    int N;
    const float *cost;        // [N] the step's costs (the update arbiter)
    const float *a_nominal;   // [128] the shifted mean the step sampled around (the update arbiter)
    float *a_mean_out;        // a_mean, writable: the arbiter commits its choice there
    const float *f_tab;       // the step's per-step disturbance table [H][4] (periodic / sin / drag / mixed), else null
    const uint32_t *key_mem;
    uint32_t key[2];
    float f_shared[3];
    int derive_keys;
    float shared_noise_scale;
};
int launch_plan_trace(covo_ctx *h, const PlanInstDesc *inst, int n_inst, bool batched, const float *states_true, int trace_index,
                      hipStream_t s);
// sample_fan.hip: the fan of the step that has just been enqueued (no-op with nothing attached); log_index >= 0: an episode
// driver's step, which also writes its row of the fan log.  launch_sample_fan_one: covo_rollout_fan
int launch_sample_fan(covo_ctx *h, const PlanInstDesc *inst, int n_inst, bool batched, int log_index, hipStream_t s);
int launch_sample_fan_one(covo_ctx *h, const PlanInstDesc &d, RolloutClip clip, const int32_t *idx, int K, float *fan_out, hipStream_t s);
// update_arbiter.hip: the arbiter of the step that has just been enqueued (no-op with nothing attached), ahead of the plan and fan
// launches, which then see the arbitrated mean; log_index as for the fan.  launch_update_arbiter_one: covo_arbitrate.
// launch_arbiter_nominal: shift(a_mean) of n_inst instances into the handle's nominal buffer (a_mean null: only its address) -- the
// env-batched fused step keeps its shifted mean in LDS, so the nominal is formed ahead of it
int launch_update_arbiter(covo_ctx *h, const PlanInstDesc *inst, int n_inst, bool batched, int log_index, hipStream_t s);
int launch_update_arbiter_one(covo_ctx *h, const PlanInstDesc &d, RolloutClip clip, int mask, float *row_out, hipStream_t s);
int launch_arbiter_nominal(covo_ctx *h, const float *a_mean, int n_inst, hipStream_t s, const float **nominal_out);
// newton_refine.hip: the line search on the committed mean, behind the arbiter (a_mean_out: the mean, in and out).  What one instance
// refines with: its gradient, the Sigma it sampled from, and c^2 -- the caller's reciprocal (covo_newton_refine) or the chain's slot
struct RefineDesc {
    const double *g = nullptr;        // [128]
    const float *Sigma = nullptr;     // [128][128], 16-byte aligned
    const double *inv_c2 = nullptr;   // 1 / c^2, or null: from ...
    const double *sumlogB = nullptr;  // ... sigma_ns_sumlogB's slot of this instance and sample_sigma
    float sample_sigma = 0.0f;
    float *row_out = nullptr;         // [COVO_REFINE_FLOATS], nullable
    float *costs_out = nullptr;       // [COVO_REFINE_CANDIDATES], nullable
    // the direction supplied (riccati.hip): d [128] and the sweep's side row [COVO_RICCATI_SIDE]; Sigma, inv_c2 and sumlogB are then
    // not read, and the row ends {.., mu, bits(flags | rung << 8)}
    const double *dir = nullptr;
    const double *dir_side = nullptr;
    // the closed-loop candidates (feedback_rollout.hip): extra [16][128] clipped fp32 sequences that compete as candidates 17 .. 32, their
    // aux rows [16][4], and where the feedback row goes [COVO_FEEDBACK_FLOATS]; costs_out then has COVO_FEEDBACK_CANDIDATES entries
    const float *extra = nullptr;
    const float *extra_aux = nullptr;
    float *fb_row_out = nullptr;
};
// feedback_rollout.hip: the closed-loop sequences of one instance under the sweep's gains, at n_alpha step sizes (<= 64), behind
// launch_riccati and ahead of the line search; drag / mixed (the 16-state plants) are refused
constexpr int COVO_FEEDBACK_MAX_ALPHAS = 64;
constexpr int COVO_FEEDBACK_LADDER = 16;      // the line search's step sizes 2^(3 - j), j = 1 .. 16
constexpr int COVO_FEEDBACK_AUX_FLOATS = 4;
constexpr int COVO_FEEDBACK_GAIN_DOUBLES = COVO_H * (64 + 4 + 16);  // K [H][4][16], kff [H][4], x [H][16] of one instance
struct FeedbackDesc {
    const float *b = nullptr;     // [128] the plan the sweep ran at, 16-byte aligned
    const double *K = nullptr;    // [H][4][16]
    const double *kff = nullptr;  // [H][4]
    const double *x = nullptr;    // [H][16]
    float *a_out = nullptr;       // [n_alpha][128]
    float *aux_out = nullptr;     // [n_alpha][COVO_FEEDBACK_AUX_FLOATS]
    int n_alpha = COVO_FEEDBACK_LADDER;
};
// the handle's buffers of a step's instances (capi.hip: feedback_reserve): where the sweep leaves the gains, dense by instance as it
// writes them, and instance e's generator launch
static inline void covo_feedback_sweep_out(const covo_ctx *h, RiccatiOut &o)
{
    o.K = h->feedback_gains;
    o.kff = o.K + (size_t)COVO_MAX_ENVS * COVO_H * 64;
    o.x = o.kff + (size_t)COVO_MAX_ENVS * COVO_H * 4;
}
static inline FeedbackDesc covo_feedback_desc(const covo_ctx *h, int e, const float *b)
{
    FeedbackDesc f;
    f.b = b;
    f.K = h->feedback_gains + (size_t)e * COVO_H * 64;
    f.kff = h->feedback_gains + (size_t)COVO_MAX_ENVS * COVO_H * 64 + (size_t)e * COVO_H * 4;
    f.x = h->feedback_gains + (size_t)COVO_MAX_ENVS * COVO_H * (64 + 4) + (size_t)e * COVO_H * 16;
    f.a_out = h->feedback_a + (size_t)e * COVO_FEEDBACK_LADDER * COVO_NA;
    f.aux_out = h->feedback_a + (size_t)COVO_MAX_ENVS * COVO_FEEDBACK_LADDER * COVO_NA + (size_t)e * COVO_FEEDBACK_LADDER * COVO_FEEDBACK_AUX_FLOATS;
    return f;
}
// where a sweep over a step's instances leaves its results in the handle (capi.hip: riccati_reserve): the directions, the gradients,
// the side rows behind the directions; gains: K, kff and x as well
static inline RiccatiOut covo_riccati_out(const covo_ctx *h, bool gains)
{
    RiccatiOut o;
    o.d = h->riccati_d;
    o.g = h->refine_g;
    o.side = h->riccati_d + (size_t)COVO_MAX_ENVS * COVO_NA;
    if (gains) covo_feedback_sweep_out(h, o);
    return o;
}
// instance e's line search on the direction of that sweep; f: its generator launch, whose sequences then compete (fb_row_out: their row), or null
static inline RefineDesc covo_riccati_refine_desc(const RiccatiOut &o, int e, float *row_out, float *costs_out, const FeedbackDesc *f,
                                                  float *fb_row_out)
{
    RefineDesc r;
    r.g = o.g + (size_t)e * COVO_NA;
    r.dir = o.d + (size_t)e * COVO_NA;
    r.dir_side = o.side + (size_t)e * COVO_RICCATI_SIDE;
    r.row_out = row_out;
    r.costs_out = costs_out;
    if (f != nullptr) {
        r.extra = f->a_out;
        r.extra_aux = f->aux_out;
        r.fb_row_out = fb_row_out;
    }
    return r;
}
// plan_hold.hip: one instance of a hold step / of a plan step's latch.  Both are the kernels' argument blocks as they stand (all
// pointers: compared bytewise, no padding); what is null is null for every instance of a launch
struct HoldDesc {
    const float *state;       // [32] the measured (noisy) state
    const float *b;           // [128] the mean the sweep ran at
    const double *K, *kff, *x;  // [H][4][16], [H][4], [H][16]
    const float *alpha;       // one float: the step size of the committed candidate
    const int *t_plan;        // one int32: the time word the plan step planned from, or null: no time check
    const double *side;       // the sweep's side row [COVO_RICCATI_SIDE] (entry 3: its flags), or null: not flagged
    const float *a_mean_src;  // [128] the mean to shift (may be a_mean), 16-byte aligned; with a_mean
    float *a_mean;            // [128] where the shifted mean with u in front goes, or null
    float *a_cov;             // [H][4][4] MPPI's covariance blocks, shifted in place, or null
    float *u_out;             // [4] or null
    float *row_out;           // [COVO_HOLD_FLOATS] or null
    float *log;               // this instance's rows of the episode hold log [stride][COVO_HOLD_FLOATS], or null
};
struct LatchDesc {
    const float *a_mean;      // [128] the mean the sweep has just run at
    const float *state;       // [32] the state the step planned from
    float *b_out;             // [128]
    int *t_out;               // one int32
    float *row_out;           // [COVO_HOLD_FLOATS] or null
    float *log;               // as HoldDesc::log
};
int launch_plan_hold(covo_ctx *h, const HoldDesc *d, int n_inst, bool batched, bool primitive, int stage, int log_index, hipStream_t s);
int launch_plan_latch(covo_ctx *h, const LatchDesc *d, int n_inst, bool batched, int log_index, hipStream_t s);
// state_estimator.hip: one instance of the estimator's launch, the kernel's argument block as it stands (zeroed before it is filled:
// compared bytewise); row_out and log are null or not for every instance of a launch alike
struct EstDesc {
    float *state;             // [32] the measured row: its 13 kinematic floats become the estimate, in place
    const float *u;           // [4] the action applied during the step that led to this row
    double *xhat;             // [COVO_EST_STATE_DOUBLES]: the estimate [13], then the force of the row last seen [3]
    double *P;                // [13][13]
    int *meta;                // [COVO_EST_META_INTS] = {valid, the time word of the row last seen}
    float *row_out;           // [COVO_EST_FLOATS] or null
    float *log;               // this instance's rows of the episode estimator log [stride][COVO_EST_LOG_FLOATS], or null
    qm::Consts<double> c;     // the instance's model
    double R[4], Q[4];        // the variances of the four coordinate groups: measurement, process
};
// fresh: every instance counts as one without a valid state (covo_estimator_reset)
int launch_state_estimator(covo_ctx *h, const EstDesc *d, int n_inst, bool batched, bool primitive, int fresh, int log_index, hipStream_t s);
// d's model and variances from the instance's parameters; 0, or COVO_E_BADARG with the error set (what: the entry's name)
int estimator_fill_model(EstDesc &d, const covo_env_params &p, const double *obs_std, const double *proc_std, double force_std, const char *what);
static inline bool covo_estimator_on(const covo_ctx *h) { return h->est_rows != nullptr; }
// the estimator's launch of an episode driver's step, right behind the env step: on the rows the controller is about to read, with
// u = the first action of each instance's mean (no-op with nothing attached)
int covo_estimator_step(covo_ctx *h, float *states, const float *a_mean, const covo_env_params *params, int n_inst, bool batched,
                        int log_index, hipStream_t s);
// force_observer.hip: one instance of the force observer's launch, the kernel's argument block as it stands (zeroed before it is
// filled: compared bytewise); row_out and log are null or not for every instance of a launch alike
struct ObsDesc {
    float *state;             // [32] the measured row: its floats 0 .. 15 become the estimate (x, then the force), in place
    const float *u;           // [4] the action applied during the step that led to this row
    double *xi;               // [COVO_OBS_STATE_DOUBLES]: x [13], then the force estimate [3]
    double *P;                // [16][16]
    int *meta;                // [COVO_OBS_META_INTS] = {valid, the time word of the row last seen}
    float *row_out;           // [COVO_OBS_FLOATS] or null
    float *log;               // this instance's rows of the episode observer log [stride][COVO_OBS_LOG_FLOATS], or null
    qm::Consts<double> c;     // the instance's model
    double R[4], Q[4];        // the variances of the four kinematic coordinate groups: measurement, process
    double qf, pf;            // force_walk_std^2, force_init_std^2
};
int launch_force_observer(covo_ctx *h, const ObsDesc *d, int n_inst, bool batched, bool primitive, int fresh, int log_index, hipStream_t s);
// d's model and variances from the instance's parameters; 0, or COVO_E_BADARG with the error set (what: the entry's name)
int observer_fill_model(ObsDesc &d, const covo_env_params &p, const double *obs_std, const double *proc_std, double force_walk_std,
                        double force_init_std, const char *what);
static inline bool covo_force_observer_on(const covo_ctx *h) { return h->obs_rows != nullptr; }
// the observer's launch of an episode driver's step, right behind the env step, where covo_estimator_step stands (no-op with
// nothing attached)
int covo_force_observer_step(covo_ctx *h, float *states, const float *a_mean, const covo_env_params *params, int n_inst, bool batched,
                             int log_index, hipStream_t s);
// ilqr.hip: what frames the iterations of an iLQR step (COVO_MODE_ILQR).  IlqrTallyDesc: one instance of the tally launch behind an
// iteration's line search, the kernel's argument block as it stands (all pointers; what is null is null for every instance)
struct IlqrTallyDesc {
    const float *row;         // [COVO_RICCATI_FLOATS] the handle's Riccati row of this instance: the iteration that has just run
    const float *fb_row;      // [COVO_FEEDBACK_FLOATS] ... and its feedback row, or null
    float *rows_log;          // [COVO_MAX_STEP_ITERS][COVO_RICCATI_FLOATS] or null
    float *fb_log;            // [COVO_MAX_STEP_ITERS][COVO_FEEDBACK_FLOATS] or null
    float *summary;           // [COVO_ILQR_FLOATS] or null
    const int *masks;         // [H] the clamp masks of the box sweep that has just run, or null (with box_log)
    int *box_log;             // [COVO_MAX_STEP_ITERS] slot j: the clamped coordinates of iteration j's sweep, or null
};
int launch_ilqr_begin(const float *a_mean_src, float *a_mean, uint32_t *dyn, const uint32_t *keys, int n_inst, int derive_keys,
                      float shared_noise_scale, hipStream_t s);
int launch_ilqr_tally(covo_ctx *h, int n_inst, bool batched, int j, int k, hipStream_t s);
// step.hip: the begin work of an iLQR step (its iterations follow in covo_plan_after_step / covo_plan_after_batched)
int covo_ilqr_step_impl(covo_ctx *h, const covo_env_params *params, const covo_step_args *args, uint32_t key0, uint32_t key1, hipStream_t s);
int covo_ilqr_step_batched_impl(covo_ctx *h, const covo_batch_args *args, const covo_env_params *params, const uint32_t *keys, hipStream_t s);
// step.hip: the hold step of a single / an env-batched schedule (age >= 1) in place of the step's own launches, and the plan trace
// behind it (no arbiter, refinement, fan or posterior covariance: AFTER_HOLD below)
int covo_hold_step(covo_ctx *h, const covo_step_args *args, int age, int log_index, hipStream_t s);
int covo_hold_step_batched(covo_ctx *h, const covo_batch_args *args, int age, int log_index, hipStream_t s);
int launch_feedback_rollout(covo_ctx *h, const PlanInstDesc *inst, const FeedbackDesc *f, int n_inst, bool batched, hipStream_t s);
int launch_feedback_rollout_one(covo_ctx *h, const PlanInstDesc &d, const FeedbackDesc &f, const double *alphas, hipStream_t s);
int launch_newton_refine(covo_ctx *h, const PlanInstDesc *inst, const RefineDesc *r, int n_inst, bool batched, hipStream_t s);
int launch_newton_refine_one(covo_ctx *h, const PlanInstDesc &d, RolloutClip clip, const RefineDesc &r, hipStream_t s);
void after_state_destroy(covo_ctx *h);  // (update_arbiter.hip) the three launches' device state: AfterState, after_step.hpp
// step.hip: the after-step frame -- the launches behind a single / an env-batched step of this handle (no-ops with nothing attached);
// states_true + trace_index >= 0: an episode driver's step, which also writes its trace row.  Its three forms (an iLQR step's
// iterations are the fourth, chosen by the step's mode):
enum AfterForm {
    AFTER_BETWEEN,  // between two passes of an iterated step (covo_set_step_iters): the arbiter and the refinement alone
    AFTER_STEP,     // behind a step: all of them
    AFTER_HOLD,     // behind a hold step of the plan hold: the plan trace alone, on the hold step's own inputs
};
// keys: the instances' raw rng_act (host); read behind a hold step only
int covo_plan_after_step(covo_ctx *h, AfterForm form, const covo_env_params *params, const covo_step_args *args, uint32_t key0,
                         uint32_t key1, const float *f_shared, const float *state_true, int trace_index, hipStream_t s);
int covo_plan_after_batched(covo_ctx *h, AfterForm form, const covo_batch_args *args, int mode, const covo_env_params *params,
                            const uint32_t *keys, const float *states_true, int trace_index, hipStream_t s);
int launch_env_step(float *state, float *noisy, const float *pos_traj, const float *vel_traj, const float *acc_traj, int T,
                    const covo_env_params &p, const float *action, const uint32_t *step_key, int noisy_on,
                    float obs_noise_scale, float *log, int log_index, hipStream_t s);
int launch_pid_nominal(const float *state0, const float *pos_traj, const float *vel_traj, const float *acc_traj, int T,
                       const covo_env_params &p, const covo_env_params &pid_params, float Kp, float Kd, float Kp_att,
                       uint32_t key0, uint32_t key1, int n_steps, float *states, float *a_means, uint32_t *keys_out,
                       hipStream_t s);
int covo_debug_time_step_impl(covo_ctx *h, const covo_env_params *params, const covo_step_args *args, int step_mask,
                              int hess_mask, int sigma_stages, int reps, float *us_out, hipStream_t run);
