// capi.hip -- the extern "C" surface declared in include/covo_hip.h.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include "covo_common.hpp"

static thread_local char g_err[512] = "";

void covo_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// a kernel of an earlier call raised a sticky status bit (covo_device_status): refuse to pile more work on poisoned data
#define CHECK_DEVICE(h, what)                                                                                                \
    do {                                                                                                                     \
        const int st_ = *(volatile int *)(h)->status_host;                                                                   \
        if (st_ != 0) {                                                                                                      \
            covo_set_error("%s: device status 0x%x from an earlier call%s%s (covo_device_status)", what, st_,               \
                           (st_ & COVO_DEVSTAT_EXCHANGE) ? ": a peer's rank record did not arrive (covo_exchange_records)"    \
                           : (st_ & COVO_DEVSTAT_ADJOINT) ? ": the adjoint Hessian's costate wait timed out (that call's R / Sigma / L are NaN)" : "", \
                           (st_ & COVO_DEVSTAT_GRID_BARRIER)                                                                 \
                               ? ": a grid barrier of the Sigma chain timed out -- the GPU is shared with other work; that " \
                                 "call's Sigma / L / mean are NaN.  Create the handle with COVO_FLAG_SHARED_DEVICE"        \
                               : "");                                                                                        \
            return COVO_E_DEVICE;                                                                                            \
        }                                                                                                                    \
    } while (0)

// ---- one scheduled control step, for the step entry points alike (covo_mpc_step, covo_mpc_step_batched[_mode], covo_run_episode,
// run_episode_batched): the plan hold's schedule gives it its age -- 0: the step and its after-step frame as ever; else the hold step
// and its plan trace -- and moves on behind it.  row: the episode's row index (< 0: none).  What an episode driver enqueues in between
// is its own: behind_step (the sharded exchange and merge), behind_frame (the copied episode logs); the others pass step_no_extra
static int step_no_extra() { return 0; }
static int single_step_at_age(covo_ctx *h, const covo_env_params *params, const covo_step_args *args, uint32_t key0, uint32_t key1,
                              const float *f_shared, int age, int row, hipStream_t s)
{
    if (age == 0 && args->mode == COVO_MODE_ILQR) return covo_ilqr_step_impl(h, params, args, key0, key1, s);  // (its begin work)
    if (age == 0) return covo_step_impl(h, params, args, key0, key1, f_shared, s);
    return covo_hold_step(h, args, age, row, s);
}
template <class BehindStep, class BehindFrame>
static int single_scheduled_step(covo_ctx *h, const covo_env_params *params, const covo_step_args *args, uint32_t key0, uint32_t key1,
                                 const float *f_shared, const float *state_true, int row, hipStream_t s, BehindStep behind_step,
                                 BehindFrame behind_frame)
{
    const int age = covo_plan_step_age(h, 1);  // (a hold step uses no rng_act)
    int rc = single_step_at_age(h, params, args, key0, key1, f_shared, age, row, s);
    if (rc || (rc = behind_step())) return rc;
    if ((rc = covo_plan_after_step(h, age != 0 ? AFTER_HOLD : AFTER_STEP, params, args, key0, key1, f_shared, state_true, row, s))) return rc;
    if ((rc = behind_frame())) return rc;
    covo_plan_step_done(h, age, 1);
    return 0;
}
// args: the caller's block (covo-online's and the iLQR step's scratch key themselves by it); norm: check_batch_step's, with the mode
static int batched_step_at_age(covo_ctx *h, const covo_batch_args *args, const covo_batch_mode_args *norm, const covo_env_params *params,
                               const uint32_t *keys, int age, int row, hipStream_t s)
{
    if (age != 0) return covo_hold_step_batched(h, args, age, row, s);  // (covo-online and iLQR only: the others refuse the Riccati refinement)
    if (norm->mode == COVO_MODE_ILQR) return covo_ilqr_step_batched_impl(h, args, params, keys, s);  // (its begin work)
    if (norm->mode == COVO_MODE_CMA) return covo_step_batched_impl(h, args, params, keys, s, COVO_MODE_CMA);  // (covo-online's body)
    return norm->mode == COVO_MODE_COVO_ONLINE ? covo_step_batched_impl(h, args, params, keys, s)
           : covo_batched_staged(h)            ? covo_step_batched_staged_impl(h, norm, params, keys, s)
                                               : covo_step_batched_small_impl(h, norm, params, keys, s);
}
template <class BehindFrame>
static int batched_scheduled_step(covo_ctx *h, const covo_batch_args *args, const covo_batch_mode_args *norm, const covo_env_params *params,
                                  const uint32_t *keys, const float *states_true, int row, hipStream_t s, BehindFrame behind_frame)
{
    const int age = covo_plan_step_age(h, args->n_envs);  // (the batch shares one age)
    int rc = batched_step_at_age(h, args, norm, params, keys, age, row, s);
    if (rc || (rc = covo_plan_after_batched(h, age != 0 ? AFTER_HOLD : AFTER_STEP, args, norm->mode, params, keys, states_true, row, s)))
        return rc;
    if ((rc = behind_frame())) return rc;
    covo_plan_step_done(h, age, args->n_envs);
    return 0;
}

__global__ void raise_status_kernel(int *status, int bits)
{
    __hip_atomic_fetch_or(status, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

extern "C" {

const char *covo_last_error(void) { return g_err; }
int covo_abi_version(void) { return COVO_ABI_VERSION; }

int covo_create(const covo_config *cfg, covo_handle_t *out)
{
    REQUIRE(cfg && out, "covo_create: null argument");
    REQUIRE(cfg->H == COVO_H && cfg->du == COVO_DU, "covo_create: H=%d du=%d unsupported (kernels are built for H=%d du=%d)",
            cfg->H, cfg->du, COVO_H, COVO_DU);
    REQUIRE(cfg->n_local > 0, "covo_create: n_local=%d", cfg->n_local);
    REQUIRE(cfg->lam > 0.0f, "covo_create: lam=%g", (double)cfg->lam);
    covo_ctx *h = new covo_ctx();
    h->opt = covo_default_opts();
    h->dbg_epoch = h->opt.epoch;
    h->cfg = *cfg;
    COVO_CHECK_HIP(hipGetDevice(&h->device));
    h->max_red_blocks = 256;
    h->exchange = nullptr;
    const int nb = (cfg->n_local + 255) / 256, ng = (cfg->n_local + 63) / 64;
    COVO_CHECK_HIP(hipMalloc(&h->ws_partials, (size_t)h->max_red_blocks * COVO_PARTIAL_FLOATS * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&h->ws_partials_cov, softmax_cov_workspace_floats(h->max_red_blocks) * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&h->ws_diag_rec, (size_t)h->max_red_blocks * 4 * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&h->diag_scratch, (size_t)COVO_MAX_ENVS * COVO_DIAG_FLOATS * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&h->ws_blockmin, (size_t)ng * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&h->lam_own, (size_t)COVO_MAX_ENVS * COVO_LAM_FLOATS * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&h->elite_own, (size_t)COVO_MAX_ENVS * COVO_ELITE_FLOATS * sizeof(float)));
    COVO_CHECK_HIP(hipMalloc(&h->ws_stats, (size_t)(nb > 256 ? nb : 256) * COVO_H * 6 * sizeof(double)));  // one row per rollout workgroup
    h->ws_sigma_bytes = sigma_ns_workspace_bytes(1);
    COVO_CHECK_HIP(hipMalloc(&h->ws_sigma, h->ws_sigma_bytes));
    h->ws_hess_bytes = hessian_workspace_bytes(1);
    COVO_CHECK_HIP(hipMalloc(&h->ws_hess, h->ws_hess_bytes));
    COVO_CHECK_HIP(hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking));
    COVO_CHECK_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    COVO_CHECK_HIP(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    COVO_CHECK_HIP(hipHostMalloc(reinterpret_cast<void **>(&h->status_host), sizeof(int), hipHostMallocMapped));
    *h->status_host = 0;
    COVO_CHECK_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&h->status_dev), h->status_host, 0));
    *out = h;
    return 0;
}

int covo_destroy(covo_handle_t h)
{
    if (!h) return COVO_E_NOHANDLE;
    step_state_destroy(h);
    batch_state_destroy(h);
    after_state_destroy(h);
    post_cov_state_destroy(h);
    exchange_destroy(h);
    int rc = 0;
#define DESTROY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess && !rc) {                                                                  \
            covo_set_error("covo_destroy: %s failed: %s", #expr, hipGetErrorString(_e));               \
            rc = (int)_e;                                                                               \
        }                                                                                               \
    } while (0)
    DESTROY(hipFree(h->ws_partials));
    DESTROY(hipFree(h->ws_partials_cov));
    DESTROY(hipFree(h->ws_diag_rec));
    DESTROY(hipFree(h->diag_scratch));
    DESTROY(hipFree(h->ws_blockmin));
    DESTROY(hipFree(h->lam_own));
    DESTROY(hipFree(h->anneal_table));
    DESTROY(hipFree(h->nodes_table));
    DESTROY(hipFree(h->sn_W));
    DESTROY(hipFree(h->sn_SigmaM));
    DESTROY(hipFree(h->sn_G));
    DESTROY(hipFree(h->elite_own));
    DESTROY(hipFree(h->ws_stats));
    DESTROY(hipFree(h->ws_sigma));
    DESTROY(hipFree(h->ws_hess));
    DESTROY(hipFree(h->ws_grad));
    DESTROY(hipFree(h->refine_g));
    DESTROY(hipFree(h->ws_riccati));
    DESTROY(hipFree(h->riccati_d));
    DESTROY(hipFree(h->riccati_tab));
    DESTROY(hipFree(h->feedback_gains));
    DESTROY(hipFree(h->feedback_a));
    DESTROY(hipFree(h->hold_b));
    DESTROY(hipFree(h->hold_t));
    DESTROY(hipFree(h->hold_keys));
    DESTROY(hipFree(h->cma_ws));
    DESTROY(hipEventDestroy(h->ev_fork));
    DESTROY(hipEventDestroy(h->ev_join));
    DESTROY(hipStreamDestroy(h->side_stream));
    DESTROY(hipHostFree(h->status_host));
#undef DESTROY
    (void)hipGetLastError();  // never leave a sticky error behind for the caller's runtime (torch checks it)
    delete h;
    return rc;
}

int covo_device_status(covo_handle_t h, int32_t clear)
{
    if (!h) return COVO_E_NOHANDLE;
    const int st = *(volatile int *)h->status_host;
    if (clear) *(volatile int *)h->status_host = 0;
    return st;
}

int covo_debug_raise_device_status(covo_handle_t h, int32_t bits, void *stream)
{
    REQUIRE(h, "covo_debug_raise_device_status: null handle");
    hipLaunchKernelGGL(raise_status_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, h->status_dev, (int)bits);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

int covo_randn(covo_handle_t h, uint32_t key0, uint32_t key1, int64_t sample_offset, int32_t n_samples, int32_t n_cols,
               float *eps_out, void *stream)
{
    REQUIRE(h, "covo_randn: null handle");
    REQUIRE(eps_out && n_samples > 0 && n_cols > 0, "covo_randn: bad argument");
    return launch_randn(key0, key1, sample_offset, n_samples, n_cols, eps_out, (hipStream_t)stream);
}

int covo_randn_jax(covo_handle_t h, uint32_t key0, uint32_t key1, int64_t n_total, int64_t sample_offset, int32_t n_samples,
                   int32_t mppi, float *eps_out, void *stream)
{
    REQUIRE(h, "covo_randn_jax: null handle");
    REQUIRE(eps_out && n_samples > 0 && sample_offset >= 0 && n_total >= sample_offset + n_samples, "covo_randn_jax: bad argument");
    REQUIRE(n_total < (1ll << 31), "covo_randn_jax: n_total=%lld: jax's iota(2 N) counters are 32-bit", (long long)n_total);
    return launch_randn_jax(key0, key1, n_total, sample_offset, n_samples, mppi, eps_out, (hipStream_t)stream);
}

// what the four stand-alone noise entry points share: a_out = clip(mu + L eps); the caller adds eps, or the key of the in-kernel draw
static NoiseDesc noise_desc(const covo_ctx *h, const float *L, const float *mu, int N, float *a_out)
{
    NoiseDesc d;
    d.L = L;
    d.mu = mu;
    d.N = N;
    d.a = a_out;
    d.propagate_nan = covo_propagate_nan(h);
    return d;
}

int covo_noise_gemm(covo_handle_t h, const float *L, const float *mu, const float *eps, int32_t N, float *a_out,
                    void *stream)
{
    REQUIRE(h, "covo_noise_gemm: null handle");
    CHECK_DEVICE(h, "covo_noise_gemm");
    REQUIRE(L && mu && eps && a_out && N > 0, "covo_noise_gemm: bad argument");
    NoiseDesc d = noise_desc(h, L, mu, N, a_out);
    d.eps = eps;
    return launch_noise_gemm(d, (hipStream_t)stream);
}

int covo_noise_gemm_philox(covo_handle_t h, const float *L, const float *mu, uint32_t key0, uint32_t key1,
                           int64_t sample_offset, int32_t N, float *a_out, void *stream)
{
    REQUIRE(h, "covo_noise_gemm_philox: null handle");
    CHECK_DEVICE(h, "covo_noise_gemm_philox");
    REQUIRE(L && mu && a_out && N > 0, "covo_noise_gemm_philox: bad argument");
    NoiseDesc d = noise_desc(h, L, mu, N, a_out);
    d.key[0] = key0;
    d.key[1] = key1;
    d.sample_offset = sample_offset;
    return launch_noise_gemm(d, (hipStream_t)stream);
}

int covo_noise_blockdiag(covo_handle_t h, const float *Ls, const float *mu, const float *eps, int32_t N, float *a_out,
                         void *stream)
{
    REQUIRE(h, "covo_noise_blockdiag: null handle");
    REQUIRE(Ls && mu && eps && a_out && N > 0, "covo_noise_blockdiag: bad argument");
    NoiseDesc d = noise_desc(h, Ls, mu, N, a_out);
    d.eps = eps;
    return launch_noise_blockdiag(d, (hipStream_t)stream);
}

int covo_noise_blockdiag_philox(covo_handle_t h, const float *Ls, const float *mu, uint32_t key0, uint32_t key1,
                                int64_t sample_offset, int32_t N, float *a_out, void *stream)
{
    REQUIRE(h, "covo_noise_blockdiag_philox: null handle");
    REQUIRE(Ls && mu && a_out && N > 0, "covo_noise_blockdiag_philox: bad argument");
    NoiseDesc d = noise_desc(h, Ls, mu, N, a_out);
    d.key[0] = key0;
    d.key[1] = key1;
    d.sample_offset = sample_offset;
    return launch_noise_blockdiag(d, (hipStream_t)stream);
}

// how the stand-alone entry points treat the caller's action stripes: trusted only under COVO_FLAG_ACTIONS_CLIPPED
static RolloutClip rollout_clip(const covo_ctx *h)
{
    if ((h->cfg.flags & COVO_FLAG_ACTIONS_CLIPPED) != 0) return ROLLOUT_CLIP_TRUSTED;
    return covo_propagate_nan(h) ? ROLLOUT_CLIP_REAPPLY_NAN : ROLLOUT_CLIP_REAPPLY;
}

int covo_rollout_cost(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                      const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                      const float *a, int32_t N, float *cost_out, float *groupmin, double *pos_stats, void *stream)
{
    REQUIRE(h, "covo_rollout_cost: null handle");
    CHECK_DEVICE(h, "covo_rollout_cost");
    REQUIRE(state && pos_traj && vel_traj && params && a && cost_out && T > 0, "covo_rollout_cost: bad argument");
    REQUIRE(N > 0 && N <= h->cfg.n_local, "covo_rollout_cost: N=%d outside (0, n_local=%d]", N, h->cfg.n_local);
    CHECK_MODEL(params, "covo_rollout_cost");
    REQUIRE(!covo_needs_tables(*params) || f_disturb_steps, "covo_rollout_cost: disturb_kind=%d needs f_disturb_steps (covo_disturb_table)",
            params->disturb_kind);
    RolloutDesc d;
    d.state = state;
    d.pos_traj = pos_traj;
    d.vel_traj = vel_traj;
    d.T = T;
    d.params = params;
    d.f_shared = f_disturb_shared;
    d.f_tab = f_disturb_steps;
    d.a = a;
    d.N = N;
    d.discount = h->cfg.discount;
    d.cost = cost_out;
    d.groupmin = groupmin;
    d.pos_stats = pos_stats;
    d.stats_ws = h->ws_stats;
    d.clip = rollout_clip(h);
    return launch_rollout(d, (hipStream_t)stream);
}

int covo_disturb_table(covo_handle_t h, const covo_env_params *params, const float *state, int32_t batch,
                       const uint32_t *keys_dev, uint32_t key0, uint32_t key1, int32_t key_mode, int32_t deterministic,
                       float *out, void *stream)
{
    REQUIRE(h, "covo_disturb_table: null handle");
    REQUIRE(params && state && out && batch > 0, "covo_disturb_table: bad argument");
    REQUIRE(key_mode >= COVO_DISTURB_KEYS_SHARED && key_mode <= COVO_DISTURB_KEYS_NOMINAL, "covo_disturb_table: key_mode=%d", key_mode);
    CHECK_MODEL(params, "covo_disturb_table");
    return launch_disturb_table(*params, state, batch, keys_dev, key0, key1, key_mode, deterministic, out, (hipStream_t)stream);
}

__global__ void pos_info_kernel(const double *__restrict__ stats, const float *__restrict__ state, double inv_n,
                                float *__restrict__ mean, float *__restrict__ sd)
{
    const int t = threadIdx.x;  // (step, axis)
    if (t >= COVO_H * 3) return;
    const int k = t / 3, ax = t % 3;
    const double m1 = stats[k * 6 + ax] * inv_n;
    const double var = fmax(stats[k * 6 + 3 + ax] * inv_n - m1 * m1, 0.0);
    mean[t] = (float)((double)state[ST_POS + ax] + m1);
    sd[t] = (float)sqrt(var);
}

int covo_pos_info(covo_handle_t h, const double *pos_stats, const float *state, int64_t n_total, float *pos_mean_out,
                  float *pos_std_out, void *stream)
{
    REQUIRE(h, "covo_pos_info: null handle");
    CHECK_DEVICE(h, "covo_pos_info");
    REQUIRE(pos_stats && state && pos_mean_out && pos_std_out && n_total > 0, "covo_pos_info: bad argument");
    hipLaunchKernelGGL(pos_info_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, pos_stats, state, 1.0 / (double)n_total,
                       pos_mean_out, pos_std_out);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

int covo_debug_time_rollout(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                            const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                            const float *a, int32_t N, float *cost_out, float *groupmin, int32_t with_records, int32_t reps,
                            float *us_out, void *stream)
{
    REQUIRE(h, "covo_debug_time_rollout: null handle");
    REQUIRE(state && pos_traj && vel_traj && params && a && cost_out && us_out && T > 0 && reps > 0, "covo_debug_time_rollout: bad argument");
    REQUIRE(N > 0 && N <= h->cfg.n_local, "covo_debug_time_rollout: N=%d outside (0, n_local=%d]", N, h->cfg.n_local);
    CHECK_MODEL(params, "covo_debug_time_rollout");
    REQUIRE(!covo_needs_tables(*params) || f_disturb_steps, "covo_debug_time_rollout: disturb_kind=%d needs f_disturb_steps", params->disturb_kind);
    hipStream_t s = (hipStream_t)stream;
    // with_records: the variant the fused step runs (every workgroup also leaves its online-softmax record), when the launch
    // shape allows it there (step.hip: enqueue_step)
    const bool rec = with_records && rollout_workgroups(N, false) <= h->max_red_blocks;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t err = hipEventCreate(&e0);
    if (err == hipSuccess) err = hipEventCreate(&e1);
    int rc = 0;
    RolloutDesc d;
    d.state = state;
    d.pos_traj = pos_traj;
    d.vel_traj = vel_traj;
    d.T = T;
    d.params = params;
    d.f_shared = f_disturb_shared;
    d.f_tab = f_disturb_steps;
    d.a = a;
    d.N = N;
    d.discount = h->cfg.discount;
    d.cost = cost_out;
    d.groupmin = rec ? nullptr : groupmin;
    d.stats_ws = h->ws_stats;
    d.records = rec ? h->ws_partials : nullptr;
    d.lam = h->cfg.lam;
    d.clip = rollout_clip(h);
    auto launch = [&]() { return launch_rollout(d, s); };
    for (int i = 0; i < 3 && !rc && err == hipSuccess; ++i) rc = launch();
    constexpr int BATCHES = 3;
    float best = 1e30f, sum = 0.0f;
    for (int it = 0; it < BATCHES && !rc && err == hipSuccess; ++it) {
        err = hipEventRecord(e0, s);
        for (int i = 0; i < reps && !rc; ++i) rc = launch();
        if (err == hipSuccess) err = hipEventRecord(e1, s);
        if (err == hipSuccess) err = hipStreamSynchronize(s);
        float ms = 0.0f;
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
        best = ms < best ? ms : best;
        sum += ms;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (err != hipSuccess) {
        covo_set_error("covo_debug_time_rollout: %s", hipGetErrorString(err));
        return (int)err;
    }
    us_out[0] = sum * 1e3f / (float)(reps * BATCHES);  // mean over all launches
    us_out[1] = best * 1e3f / (float)reps;             // the fastest batch of `reps`
    return 0;
}

// the input half of the four stand-alone softmax updates below; the merges of rank records: G records, `stride` floats apart,
// blended into the new mean
static UpdateDesc update_from_costs(const float *cost, const float *a, int N, const float *groupmin)
{
    UpdateDesc d;
    d.cost = cost;
    d.a = a;
    d.N = N;
    d.blockmin = groupmin;
    d.n_blockmin = (N + 63) / 64;
    return d;
}
static UpdateDesc update_from_records(const float *records, int G, int stride, const float *a_mean_old, float gamma_mean,
                                      float *a_mean_out)
{
    UpdateDesc d;
    d.partials = records;
    d.G = G;
    d.stride = stride;
    d.a_mean_old = a_mean_old;
    d.gamma_mean = gamma_mean;
    d.a_mean_out = a_mean_out;
    return d;
}

int covo_softmax_reduce(covo_handle_t h, const float *cost, const float *a, int32_t N, const float *groupmin,
                        float *partial_out, void *stream)
{
    REQUIRE(h, "covo_softmax_reduce: null handle");
    CHECK_DEVICE(h, "covo_softmax_reduce");
    REQUIRE(cost && a && partial_out, "covo_softmax_reduce: bad argument");
    REQUIRE(N > 0 && N <= h->cfg.n_local, "covo_softmax_reduce: N=%d outside (0, n_local=%d]", N, h->cfg.n_local);
    UpdateDesc d = update_from_costs(cost, a, N, groupmin);
    d.partial_out = partial_out;
    return launch_softmax_reduce(h, d, (hipStream_t)stream);
}

int covo_softmax_update(covo_handle_t h, const float *cost, const float *a, int32_t N, const float *groupmin,
                        const float *a_mean_old, float gamma_mean, float *a_mean_out, void *stream)
{
    REQUIRE(h, "covo_softmax_update: null handle");
    CHECK_DEVICE(h, "covo_softmax_update");
    REQUIRE(cost && a && a_mean_old && a_mean_out, "covo_softmax_update: bad argument");
    REQUIRE(N > 0 && N <= h->cfg.n_local, "covo_softmax_update: N=%d outside (0, n_local=%d]", N, h->cfg.n_local);
    UpdateDesc d = update_from_costs(cost, a, N, groupmin);
    d.a_mean_old = a_mean_old;
    d.gamma_mean = gamma_mean;
    d.a_mean_out = a_mean_out;
    return launch_softmax_reduce(h, d, (hipStream_t)stream);
}

int covo_softmax_update_cov(covo_handle_t h, const float *cost, const float *a, int32_t N, const float *groupmin,
                            const float *a_mean_old, float gamma_mean, const float *a_cov_old, float gamma_sigma,
                            float *a_mean_out, float *a_cov_out, void *stream)
{
    REQUIRE(h, "covo_softmax_update_cov: null handle");
    CHECK_DEVICE(h, "covo_softmax_update_cov");
    REQUIRE(cost && a && a_mean_old && a_cov_old && a_mean_out && a_cov_out, "covo_softmax_update_cov: bad argument");
    REQUIRE(N > 0 && N <= h->cfg.n_local, "covo_softmax_update_cov: N=%d outside (0, n_local=%d]", N, h->cfg.n_local);
    UpdateDesc d = update_from_costs(cost, a, N, groupmin);
    d.a_mean_old = a_mean_old;
    d.gamma_mean = gamma_mean;
    d.a_mean_out = a_mean_out;
    d.a_cov_old = a_cov_old;
    d.gamma_sigma = gamma_sigma;
    d.a_cov_out = a_cov_out;
    return launch_softmax_update_cov(h, d, (hipStream_t)stream);
}

int covo_softmax_reduce_cov(covo_handle_t h, const float *cost, const float *a, int32_t N, const float *groupmin,
                            const float *a_mean_old, float *record_out, void *stream)
{
    REQUIRE(h, "covo_softmax_reduce_cov: null handle");
    CHECK_DEVICE(h, "covo_softmax_reduce_cov");
    REQUIRE(cost && a && a_mean_old && record_out, "covo_softmax_reduce_cov: bad argument");
    REQUIRE(N > 0 && N <= h->cfg.n_local, "covo_softmax_reduce_cov: N=%d outside (0, n_local=%d]", N, h->cfg.n_local);
    UpdateDesc d = update_from_costs(cost, a, N, groupmin);
    d.a_mean_old = a_mean_old;
    d.partial_out = record_out;
    return launch_softmax_update_cov(h, d, (hipStream_t)stream);
}

int covo_merge_ranks_cov(covo_handle_t h, const float *records, int32_t G, const float *a_mean_old, float gamma_mean,
                         const float *a_cov_old, float gamma_sigma, float *a_mean_out, float *a_cov_out, double *pos_stats_out,
                         void *stream)
{
    REQUIRE(h, "covo_merge_ranks_cov: null handle");
    CHECK_DEVICE(h, "covo_merge_ranks_cov");
    REQUIRE(records && a_mean_old && a_cov_old && a_mean_out && a_cov_out && G > 0, "covo_merge_ranks_cov: bad argument");
    UpdateDesc d = update_from_records(records, G, COVO_RANK_RECORD_COV_FLOATS, a_mean_old, gamma_mean, a_mean_out);
    d.a_cov_old = a_cov_old;
    d.gamma_sigma = gamma_sigma;
    d.a_cov_out = a_cov_out;
    int rc = launch_merge_cov(d, h->cfg.lam, (hipStream_t)stream);
    if (rc) return rc;
    if (pos_stats_out != nullptr) rc = launch_rank_stats_sum(records, G, COVO_RANK_RECORD_COV_FLOATS, pos_stats_out, (hipStream_t)stream);
    return rc;
}

// covo_merge, covo_merge_ranks and covo_merge_ranks_wide (`who`, for the messages): the merge over G records `stride` floats apart
// (rank_stride: the caller's own record_floats, one of the two rank-record sizes), then (pos_stats_out != null) the sum of the ranks'
// position sums
static int merge_records(covo_handle_t h, const char *who, const float *records, int G, int stride, bool rank_stride,
                         const float *a_mean_old, float gamma_mean, float *a_mean_out, double *pos_stats_out, void *stream)
{
    REQUIRE(h, "%s: null handle", who);
    CHECK_DEVICE(h, who);
    REQUIRE(records && a_mean_old && a_mean_out && G > 0, "%s: bad argument", who);
    REQUIRE(!rank_stride || stride == COVO_RANK_RECORD_FLOATS || stride == COVO_RANK_RECORD_COV_FLOATS,
            "%s: record_floats=%d is neither COVO_RANK_RECORD_FLOATS nor COVO_RANK_RECORD_COV_FLOATS", who, stride);
    int rc = launch_merge(update_from_records(records, G, stride, a_mean_old, gamma_mean, a_mean_out), h->cfg.lam, (hipStream_t)stream);
    if (rc == 0 && pos_stats_out != nullptr) rc = launch_rank_stats_sum(records, G, stride, pos_stats_out, (hipStream_t)stream);
    return rc;
}

int covo_merge(covo_handle_t h, const float *partials, int32_t G, const float *a_mean_old, float gamma_mean,
               float *a_mean_out, void *stream)
{
    return merge_records(h, "covo_merge", partials, G, COVO_PARTIAL_FLOATS, false, a_mean_old, gamma_mean, a_mean_out, nullptr, stream);
}

int covo_merge_ranks(covo_handle_t h, const float *records, int32_t G, const float *a_mean_old, float gamma_mean,
                     float *a_mean_out, double *pos_stats_out, void *stream)
{
    return merge_records(h, "covo_merge_ranks", records, G, COVO_RANK_RECORD_FLOATS, false, a_mean_old, gamma_mean, a_mean_out,
                         pos_stats_out, stream);
}

int covo_merge_ranks_wide(covo_handle_t h, const float *records, int32_t G, int32_t record_floats, const float *a_mean_old,
                          float gamma_mean, float *a_mean_out, double *pos_stats_out, void *stream)
{
    return merge_records(h, "covo_merge_ranks_wide", records, G, record_floats, true, a_mean_old, gamma_mean, a_mean_out, pos_stats_out,
                         stream);
}

int covo_exchange_create(covo_handle_t h, int32_t world, int32_t rank, void *handle_out)
{
    REQUIRE(h && handle_out, "covo_exchange_create: null argument");
    return exchange_create(h, world, rank, handle_out);
}

int covo_exchange_connect(covo_handle_t h, const void *handles)
{
    REQUIRE(h && handles, "covo_exchange_connect: null argument");
    return exchange_connect(h, handles);
}

int covo_exchange_set_timeout(covo_handle_t h, double seconds)
{
    REQUIRE(h, "covo_exchange_set_timeout: null handle");
    return exchange_set_timeout(h, seconds);
}

int covo_device_bus_id(int32_t device, char *out, int32_t len)
{
    REQUIRE(out && len >= 16, "covo_device_bus_id: out == NULL or len < 16");
    COVO_CHECK_HIP(hipDeviceGetPCIBusId(out, len, device));
    return 0;
}

int covo_exchange_records(covo_handle_t h, const float *record, float *gathered_out, void *stream)
{
    REQUIRE(h && record && gathered_out, "covo_exchange_records: null argument");
    CHECK_DEVICE(h, "covo_exchange_records");
    return exchange_records(h, record, gathered_out, nullptr, (hipStream_t)stream);
}

int covo_exchange_records_cov(covo_handle_t h, const float *record, float *gathered_out, void *stream)
{
    REQUIRE(h && record && gathered_out, "covo_exchange_records_cov: null argument");
    CHECK_DEVICE(h, "covo_exchange_records_cov");
    return exchange_records(h, record, gathered_out, nullptr, (hipStream_t)stream, COVO_RANK_RECORD_COV_FLOATS);
}

int covo_shift_mean(covo_handle_t h, const float *a_mean_in, float *a_mean_out, void *stream)
{
    REQUIRE(h, "covo_shift_mean: null handle");
    REQUIRE(a_mean_in && a_mean_out && a_mean_in != a_mean_out, "covo_shift_mean: bad argument (in must differ from out)");
    return launch_shift_mean(a_mean_in, a_mean_out, (hipStream_t)stream);
}

int covo_hessian(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                 const covo_env_params *params, const float *a_mean, const float *f_disturb_steps, int32_t batch,
                 double *R_out, void *stream)
{
    REQUIRE(h, "covo_hessian: null handle");
    CHECK_DEVICE(h, "covo_hessian");
    REQUIRE(state && pos_traj && vel_traj && params && a_mean && R_out && T > 0 && batch > 0, "covo_hessian: bad argument");
    CHECK_MODEL(params, "covo_hessian");
    REQUIRE(!covo_needs_tables(*params) || f_disturb_steps, "covo_hessian: disturb_kind=%d needs f_disturb_steps (covo_disturb_table)",
            params->disturb_kind);
    const int rc = covo_grow_workspace(h, &h->ws_hess, &h->ws_hess_bytes, hessian_workspace_bytes(batch), (hipStream_t)stream);
    if (rc) return rc;
    HessianDesc d;
    d.state = state;
    d.pos_traj = pos_traj;
    d.vel_traj = vel_traj;
    d.T = T;
    d.params = params;
    d.a_mean = a_mean;
    d.f_tab = f_disturb_steps;
    d.batch = batch;
    d.R = R_out;
    d.status_dev = h->status_dev;
    return launch_hessian(d, h->ws_hess, (hipStream_t)stream, DebugMasks());
}

int covo_hessian_pairs(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                       const covo_env_params *params, const float *a_mean, const float *f_disturb_steps, int32_t batch,
                       double *R_out, void *stream)
{
    REQUIRE(h, "covo_hessian_pairs: null handle");
    REQUIRE(state && pos_traj && vel_traj && params && a_mean && R_out && T > 0 && batch > 0, "covo_hessian_pairs: bad argument");
    CHECK_MODEL(params, "covo_hessian_pairs");
    HessianDesc d;
    d.state = state;
    d.pos_traj = pos_traj;
    d.vel_traj = vel_traj;
    d.T = T;
    d.params = params;
    d.a_mean = a_mean;
    d.f_tab = f_disturb_steps;
    d.batch = batch;
    d.R = R_out;
    return launch_hessian_pairs(d, (hipStream_t)stream);
}

int covo_sigma(covo_handle_t h, const double *R, int32_t batch, float sample_sigma, float *Sigma_out, float *L_out,
               void *stream)
{
    REQUIRE(h, "covo_sigma: null handle");
    CHECK_DEVICE(h, "covo_sigma");
    REQUIRE(R && L_out && batch > 0 && sample_sigma > 0.0f, "covo_sigma: bad argument");
    const int rc = covo_grow_workspace(h, &h->ws_sigma, &h->ws_sigma_bytes, sigma_ns_workspace_bytes(batch), (hipStream_t)stream);
    if (rc) return rc;
    SigmaNsDesc d;
    d.R = R;
    d.batch = batch;
    d.sample_sigma = sample_sigma;
    d.Sigma = Sigma_out;
    d.L = L_out;
    d.status = h->status_dev;
    d.persistent_ok = (h->cfg.flags & COVO_FLAG_SHARED_DEVICE) == 0;
    return launch_sigma_ns(h->opt, d, h->ws_sigma, (hipStream_t)stream, DebugMasks());
}

int covo_ess_lambda(covo_handle_t h, const float *cost, int32_t n_samples, int32_t n_inst, float lam0, float ess_min, float *out,
                    void *stream)
{
    REQUIRE(h, "covo_ess_lambda: null handle");
    CHECK_DEVICE(h, "covo_ess_lambda");
    REQUIRE(cost && out && n_samples > 0 && n_inst > 0 && n_inst <= 65535, "covo_ess_lambda: bad argument");
    REQUIRE(lam0 > 0.0f && lam0 < __builtin_inff(), "covo_ess_lambda: lam0=%g", (double)lam0);
    REQUIRE(ess_min >= 1.0f && ess_min <= 0.5f * (float)n_samples, "covo_ess_lambda: ess_min=%g outside [1, n_samples / 2 = %g]",
            (double)ess_min, 0.5 * n_samples);
    return launch_ess_lambda(cost, n_samples, n_inst, nullptr, lam0, ess_min, out, (hipStream_t)stream);
}

// ---- the annealed step (cost_standardise.hip).  The captured step graphs bake in the schedule launches, the solver's launch, temp and
// where the rows go, and read the table in the handle's own device memory: any change bumps the epoch, and the table is rewritten only
// after every launch that may still read it has finished.  What the step needs next to it is checked at the step (check_step_attachments)
int covo_set_step_anneal(covo_handle_t h, const float *sigma_table, int32_t n_pass, float temp, float *rows_out, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_anneal: null handle");
    REQUIRE(temp >= 0.0f && temp < __builtin_inff(), "covo_set_step_anneal: temp=%g is not a finite number >= 0 (0 = the configured lam)",
            (double)temp);
    const bool off = sigma_table == nullptr && temp == 0.0f;
    REQUIRE(off || (n_pass >= 1 && n_pass <= COVO_MAX_STEP_ITERS), "covo_set_step_anneal: n_pass=%d outside [1, %d]", n_pass,
            COVO_MAX_STEP_ITERS);
    if (int rc = check_setter_rows("covo_set_step_anneal", !off && rows_out != nullptr, n_inst)) return rc;
    if (sigma_table != nullptr)
        for (int i = 0; i < n_pass * COVO_H; ++i)
            REQUIRE(sigma_table[i] > 0.0f && sigma_table[i] < __builtin_inff(), "covo_set_step_anneal: sigma_table[%d][%d]=%g is not a "
                    "finite number > 0", i / COVO_H, i % COVO_H, (double)sigma_table[i]);
    if (off) {
        if (covo_anneal_on(h)) ++h->opt.epoch;
        h->anneal_passes = h->anneal_sched = 0;
        h->anneal_temp = 0.0f;
        h->anneal_rows = nullptr;
        h->anneal_n = 0;
        if (covo_lam_target(h) == nullptr) covo_eprow_drop(h, COVO_EPLOG_LAM);  // no temperature row any more: the log goes
        return 0;
    }
    CHECK_DEVICE(h, "covo_set_step_anneal");
    if (sigma_table != nullptr) {
        COVO_CHECK_HIP(hipDeviceSynchronize());  // (a setter, off the per-step path) no step in flight reads the old table
        if (h->anneal_table == nullptr)
            COVO_CHECK_HIP(hipMalloc(&h->anneal_table, (size_t)COVO_MAX_STEP_ITERS * COVO_H * sizeof(float)));
        COVO_CHECK_HIP(hipMemcpy(h->anneal_table, sigma_table, (size_t)n_pass * COVO_H * sizeof(float), hipMemcpyHostToDevice));
    }
    ++h->opt.epoch;
    h->anneal_passes = n_pass;
    h->anneal_sched = sigma_table != nullptr ? 1 : 0;
    h->anneal_temp = temp;
    h->anneal_rows = rows_out;
    h->anneal_n = rows_out ? n_inst : 0;
    if (covo_lam_target(h) == nullptr) covo_eprow_drop(h, COVO_EPLOG_LAM);
    return 0;
}

int covo_cost_standardise(covo_handle_t h, const float *cost, int32_t n_samples, int32_t n_inst, float lam0, float temp, float *out,
                          void *stream)
{
    REQUIRE(h, "covo_cost_standardise: null handle");
    CHECK_DEVICE(h, "covo_cost_standardise");
    REQUIRE(cost && out && n_samples > 0 && n_inst > 0 && n_inst <= 65535, "covo_cost_standardise: bad argument");
    REQUIRE(lam0 > 0.0f && lam0 < __builtin_inff(), "covo_cost_standardise: lam0=%g", (double)lam0);
    REQUIRE(temp > 0.0f && temp < __builtin_inff(), "covo_cost_standardise: temp=%g is not a finite number > 0", (double)temp);
    return launch_cost_standardise(cost, n_samples, n_inst, lam0, temp, out, nullptr, 0, (hipStream_t)stream);
}

// ---- the annealed step's spline nodes (noise_nodes.hip).  As covo_set_step_anneal: the captured step graphs bake in the sampler's launch
// and read the table in the handle's own device memory, so any change bumps the epoch and the table is rewritten only after every
// launch that may still read it has finished.  What the step needs next to it is checked at the step (check_step_attachments)
int covo_set_step_nodes(covo_handle_t h, const float *basis_table, int32_t n_pass, int32_t n_nodes)
{
    REQUIRE(h, "covo_set_step_nodes: null handle");
    if (basis_table == nullptr) {
        if (covo_nodes_on(h)) ++h->opt.epoch;
        h->nodes_passes = h->nodes_M = 0;
        return 0;
    }
    REQUIRE(n_pass >= 1 && n_pass <= COVO_MAX_STEP_ITERS, "covo_set_step_nodes: n_pass=%d outside [1, %d]", n_pass, COVO_MAX_STEP_ITERS);
    REQUIRE(n_nodes >= 2 && n_nodes <= COVO_H, "covo_set_step_nodes: n_nodes=%d outside [2, %d]", n_nodes, COVO_H);
    for (int i = 0; i < n_pass * COVO_H * n_nodes; ++i)
        REQUIRE(__builtin_fabsf(basis_table[i]) < __builtin_inff(), "covo_set_step_nodes: basis_table[%d][%d][%d]=%g is not a finite number",
                i / (COVO_H * n_nodes), i / n_nodes % COVO_H, i % n_nodes, (double)basis_table[i]);
    CHECK_DEVICE(h, "covo_set_step_nodes");
    COVO_CHECK_HIP(hipDeviceSynchronize());  // (a setter, off the per-step path) no step in flight reads the old table
    if (h->nodes_table == nullptr)
        COVO_CHECK_HIP(hipMalloc(&h->nodes_table, (size_t)COVO_MAX_STEP_ITERS * COVO_H * COVO_H * sizeof(float)));
    COVO_CHECK_HIP(hipMemcpy(h->nodes_table, basis_table, (size_t)n_pass * COVO_H * n_nodes * sizeof(float), hipMemcpyHostToDevice));
    ++h->opt.epoch;
    h->nodes_passes = n_pass;
    h->nodes_M = n_nodes;
    return 0;
}

int covo_noise_nodes_philox(covo_handle_t h, const float *basis, int32_t n_nodes, const float *mu, uint32_t key0, uint32_t key1,
                            int64_t sample_offset, int32_t N, float *a_out, void *stream)
{
    REQUIRE(h, "covo_noise_nodes_philox: null handle");
    CHECK_DEVICE(h, "covo_noise_nodes_philox");
    REQUIRE(basis && mu && a_out && N > 0, "covo_noise_nodes_philox: bad argument");
    REQUIRE(n_nodes >= 2 && n_nodes <= COVO_H, "covo_noise_nodes_philox: n_nodes=%d outside [2, %d]", n_nodes, COVO_H);
    NoiseDesc d = noise_desc(h, nullptr, mu, N, a_out);
    d.key[0] = key0;
    d.key[1] = key1;
    d.sample_offset = sample_offset;
    return launch_noise_nodes(d, basis, 0, n_nodes, (hipStream_t)stream);
}

// ---- covo-online in spline-node space (sigma_nodes.hip).  As covo_set_step_nodes: the captured step graphs bake in the two launches
// and read W, Sigma_M and G in the handle's own device memory, so any change bumps the epoch and W is rewritten only after every launch
// that may still read it has finished.  What the step refuses next to it is checked at the step (check_step_attachments)
int covo_set_step_sigma_nodes(covo_handle_t h, const double *W, int32_t M, float *rows, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_sigma_nodes: null handle");
    if (W == nullptr) {
        if (covo_sigma_nodes_on(h)) ++h->opt.epoch;
        h->sn_M = h->sn_n = 0;
        h->sn_rows = nullptr;
        return 0;
    }
    REQUIRE(M >= 2 && M <= COVO_SIGMA_NODES_MAX, "covo_set_step_sigma_nodes: M=%d outside [2, %d]", M, COVO_SIGMA_NODES_MAX);
    REQUIRE(rows != nullptr && n_inst > 0 && n_inst <= COVO_MAX_ENVS, "covo_set_step_sigma_nodes: null rows or n_inst=%d outside (0, %d]",
            n_inst, COVO_MAX_ENVS);
    for (int i = 0; i < COVO_H * M; ++i)
        REQUIRE(__builtin_fabs(W[i]) < __builtin_inf(), "covo_set_step_sigma_nodes: W[%d][%d]=%g is not a finite number", i / M, i % M, W[i]);
    CHECK_DEVICE(h, "covo_set_step_sigma_nodes");
    COVO_CHECK_HIP(hipDeviceSynchronize());  // (a setter, off the per-step path) no step in flight reads the old weights
    if (h->sn_W == nullptr) {
        COVO_CHECK_HIP(hipMalloc(&h->sn_W, (size_t)COVO_H * COVO_SIGMA_NODES_MAX * sizeof(double)));
        COVO_CHECK_HIP(hipMalloc(&h->sn_SigmaM, (size_t)COVO_MAX_ENVS * 64 * 64 * sizeof(double)));
        COVO_CHECK_HIP(hipMalloc(&h->sn_G, (size_t)COVO_MAX_ENVS * COVO_NA * 64 * sizeof(float)));
    }
    COVO_CHECK_HIP(hipMemcpy(h->sn_W, W, (size_t)COVO_H * M * sizeof(double), hipMemcpyHostToDevice));
    ++h->opt.epoch;
    h->sn_M = M;
    h->sn_rows = rows;
    h->sn_n = n_inst;
    return 0;
}

int covo_step_sigma_nodes(covo_handle_t h, int32_t *M, double *SigmaM_out, float *G_out, int32_t n_inst, void *stream)
{
    REQUIRE(h, "covo_step_sigma_nodes: null handle");
    REQUIRE(M, "covo_step_sigma_nodes: bad argument");
    *M = h->sn_M;
    if (SigmaM_out == nullptr && G_out == nullptr) return 0;
    REQUIRE(covo_sigma_nodes_on(h), "covo_step_sigma_nodes: nothing attached (covo_set_step_sigma_nodes)");
    REQUIRE(n_inst > 0 && n_inst <= h->sn_n, "covo_step_sigma_nodes: n_inst=%d outside (0, %d]", n_inst, h->sn_n);
    const size_t d = 4 * (size_t)h->sn_M;
    if (SigmaM_out)
        COVO_CHECK_HIP(hipMemcpyAsync(SigmaM_out, h->sn_SigmaM, (size_t)n_inst * d * d * sizeof(double), hipMemcpyDeviceToDevice,
                                      (hipStream_t)stream));
    if (G_out)
        COVO_CHECK_HIP(hipMemcpyAsync(G_out, h->sn_G, (size_t)n_inst * COVO_NA * d * sizeof(float), hipMemcpyDeviceToDevice,
                                      (hipStream_t)stream));
    return 0;
}

int covo_sigma_nodes(covo_handle_t h, const double *R, int32_t batch, const double *W_dev, int32_t M, float sample_sigma,
                     double *SigmaM_out, float *G_out, float *Sigma_out, float *rows_out, void *stream)
{
    REQUIRE(h, "covo_sigma_nodes: null handle");
    CHECK_DEVICE(h, "covo_sigma_nodes");
    REQUIRE(M >= 2 && M <= COVO_SIGMA_NODES_MAX, "covo_sigma_nodes: M=%d outside [2, %d]", M, COVO_SIGMA_NODES_MAX);
    REQUIRE(R && W_dev && SigmaM_out && G_out && batch > 0 && batch <= 65535, "covo_sigma_nodes: bad argument");
    REQUIRE(sample_sigma > 0.0f && sample_sigma < __builtin_inff(), "covo_sigma_nodes: sample_sigma=%g", (double)sample_sigma);
    return launch_sigma_nodes(R, batch, W_dev, M, sample_sigma, SigmaM_out, G_out, Sigma_out, rows_out, (hipStream_t)stream);
}

int covo_noise_factor_philox(covo_handle_t h, const float *G, int32_t d, const float *mu, uint32_t key0, uint32_t key1,
                             int64_t sample_offset, int32_t N, float *a_out, void *stream)
{
    REQUIRE(h, "covo_noise_factor_philox: null handle");
    CHECK_DEVICE(h, "covo_noise_factor_philox");
    REQUIRE(G && mu && a_out && N > 0, "covo_noise_factor_philox: bad argument");
    REQUIRE(d >= 8 && d <= 4 * COVO_SIGMA_NODES_MAX && (d & 3) == 0, "covo_noise_factor_philox: d=%d is no multiple of 4 in [8, %d]", d,
            4 * COVO_SIGMA_NODES_MAX);
    NoiseDesc nd = noise_desc(h, nullptr, mu, N, a_out);
    nd.key[0] = key0;
    nd.key[1] = key1;
    nd.sample_offset = sample_offset;
    return launch_noise_factor(nd, G, d / 4, (hipStream_t)stream);
}

int covo_elite_select(covo_handle_t h, const float *cost, int32_t n_samples, int32_t n_inst, int32_t K, float *out, void *stream)
{
    REQUIRE(h, "covo_elite_select: null handle");
    CHECK_DEVICE(h, "covo_elite_select");
    REQUIRE(cost && out && n_samples > 0, "covo_elite_select: bad argument");
    REQUIRE(n_inst > 0 && n_inst <= 65535, "covo_elite_select: n_inst=%d outside (0, 65535]", n_inst);
    REQUIRE(K >= 1 && K <= n_samples, "covo_elite_select: K=%d outside [1, n_samples = %d]", K, n_samples);
    return launch_elite_select(cost, n_samples, n_inst, K, out, (hipStream_t)stream);
}

// covo_rollout_fan, covo_arbitrate: the caller's buffers and shared vector (derive_keys = 0) as the descriptor of a step's instance
static PlanInstDesc standalone_inst(const float *state, const float *pos_traj, const float *vel_traj, int T, const covo_env_params *params,
                                    const float *f_disturb_shared, const float *f_disturb_steps, const float *a, int N)
{
    PlanInstDesc d;
    std::memset(&d, 0, sizeof(d));
    d.state = state;
    d.pos_traj = pos_traj;
    d.vel_traj = vel_traj;
    d.T = T;
    d.params = params;
    d.a = a;
    d.N = N;
    d.f_tab = f_disturb_steps;
    for (int i = 0; i < 3; ++i) d.f_shared[i] = f_disturb_shared ? f_disturb_shared[i] : 0.0f;
    return d;
}

int covo_rollout_fan(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                     const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                     const float *a, int32_t N, const int32_t *idx, int32_t K, float *fan_out, void *stream)
{
    REQUIRE(h, "covo_rollout_fan: null handle");
    CHECK_DEVICE(h, "covo_rollout_fan");
    REQUIRE(state && pos_traj && vel_traj && params && a && fan_out && T > 0, "covo_rollout_fan: bad argument");
    REQUIRE(N > 0 && N <= h->cfg.n_local, "covo_rollout_fan: N=%d outside (0, n_local=%d]", N, h->cfg.n_local);
    REQUIRE(K >= 1 && K <= COVO_FAN_MAX, "covo_rollout_fan: K=%d outside [1, %d]", K, COVO_FAN_MAX);
    REQUIRE(K <= N, "covo_rollout_fan: K=%d > n_samples=%d", K, N);
    CHECK_MODEL(params, "covo_rollout_fan");
    REQUIRE(!covo_needs_tables(*params) || f_disturb_steps, "covo_rollout_fan: disturb_kind=%d needs f_disturb_steps (covo_disturb_table)",
            params->disturb_kind);
    const PlanInstDesc d = standalone_inst(state, pos_traj, vel_traj, T, params, f_disturb_shared, f_disturb_steps, a, N);
    return launch_sample_fan_one(h, d, rollout_clip(h), idx, K, fan_out, (hipStream_t)stream);  // the clip covo_rollout_cost applies
}

// ---- the posterior covariance (post_cov.hip).  Like the plan's and the fan's, its launches are eager and follow the step: no captured
// step graph changes.  The stage-1 partials of n_inst instances are reserved here, so that no step allocates
int covo_set_step_post_cov(covo_handle_t h, float *cov, float *aux, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_post_cov: null handle");
    if (cov == nullptr) {  // off
        h->post_cov_out = h->post_aux_out = nullptr;
        h->post_n = 0;
        covo_eprow_drop(h, COVO_EPLOG_POST_AUX);  // the logs with it
        covo_eprow_drop(h, COVO_EPLOG_POST_COV);
        return 0;
    }
    REQUIRE(aux != nullptr, "covo_set_step_post_cov: aux is null (float[n_inst][%d])", COVO_POST_AUX_FLOATS);
    if (int rc = check_setter_rows("covo_set_step_post_cov", true, n_inst)) return rc;
    CHECK_DEVICE(h, "covo_set_step_post_cov");
    if (int rc = post_cov_reserve(h, n_inst)) return rc;
    h->post_cov_out = cov;
    h->post_aux_out = aux;
    h->post_n = n_inst;
    if (covo_sigma_adapt_on(h)) {  // a reuse step must never read a C that no step of this schedule wrote; its graph holds C's address
        h->sigma_age = 0;
        ++h->opt.epoch;
    }
    return 0;
}

int covo_weighted_cov(covo_handle_t h, const float *a, const float *cost, const float *mu, int32_t n_samples, int32_t n_inst, float lam,
                      int32_t elite_K, float *cov_out, float *aux_out, void *stream)
{
    REQUIRE(h, "covo_weighted_cov: null handle");
    CHECK_DEVICE(h, "covo_weighted_cov");
    REQUIRE(a && cost && mu && cov_out && aux_out, "covo_weighted_cov: null buffer");
    REQUIRE(n_samples > 0, "covo_weighted_cov: n_samples=%d", n_samples);
    REQUIRE(n_inst > 0 && n_inst <= 65535, "covo_weighted_cov: n_inst=%d outside (0, 65535]", n_inst);
    REQUIRE(((uintptr_t)a & 15) == 0, "covo_weighted_cov: a must be 16-byte aligned");
    REQUIRE(elite_K >= 0 && elite_K <= n_samples, "covo_weighted_cov: elite_K=%d outside [0, n_samples = %d]", elite_K, n_samples);
    REQUIRE(elite_K == 0 || n_inst <= COVO_MAX_ENVS, "covo_weighted_cov: n_inst=%d above %d with an elite set", n_inst, COVO_MAX_ENVS);
    REQUIRE(elite_K > 0 || (lam > 0.0f && lam < __builtin_inff()), "covo_weighted_cov: lam=%g", (double)lam);
    PostCovDesc d;
    d.a = a;
    d.cost = cost;
    d.mu = mu;
    d.N = n_samples;
    d.n_inst = n_inst;
    d.lam = lam;
    d.elite_K = elite_K;
    d.cov_out = cov_out;
    d.aux_out = aux_out;
    return launch_weighted_cov(h, d, (hipStream_t)stream);
}

int covo_sigma_shift(covo_handle_t h, const float *L_in, int32_t batch, float sample_sigma, float *Sigma_out, float *L_out, void *stream)
{
    REQUIRE(h, "covo_sigma_shift: null handle");
    CHECK_DEVICE(h, "covo_sigma_shift");
    REQUIRE(L_in && Sigma_out && L_out && batch > 0 && batch <= 65535, "covo_sigma_shift: bad argument");
    REQUIRE(sample_sigma > 0.0f && sample_sigma < __builtin_inff(), "covo_sigma_shift: sample_sigma=%g", (double)sample_sigma);
    REQUIRE((((uintptr_t)L_in | (uintptr_t)Sigma_out | (uintptr_t)L_out) & 15) == 0, "covo_sigma_shift: L_in / Sigma_out / L_out must be "
            "16-byte aligned");
    REQUIRE((const float *)Sigma_out != L_in && Sigma_out != L_out, "covo_sigma_shift: Sigma_out must not be L_in or L_out (L_out may be L_in)");
    return launch_sigma_shift(L_in, batch, sample_sigma, Sigma_out, L_out, (hipStream_t)stream);
}

int covo_sigma_adapt(covo_handle_t h, const float *L_in, const float *C, int32_t batch, float gamma, float sample_sigma, float *Sigma_out,
                     float *L_out, float *rows_out, void *stream)
{
    REQUIRE(h, "covo_sigma_adapt: null handle");
    CHECK_DEVICE(h, "covo_sigma_adapt");
    REQUIRE(L_in && C && Sigma_out && L_out && batch > 0 && batch <= 65535, "covo_sigma_adapt: bad argument");
    REQUIRE(gamma >= 0.0f && gamma < 1.0f, "covo_sigma_adapt: gamma=%g outside [0, 1)", (double)gamma);
    REQUIRE(sample_sigma > 0.0f && sample_sigma < __builtin_inff(), "covo_sigma_adapt: sample_sigma=%g", (double)sample_sigma);
    REQUIRE((((uintptr_t)L_in | (uintptr_t)C | (uintptr_t)Sigma_out | (uintptr_t)L_out | (uintptr_t)rows_out) & 15) == 0,
            "covo_sigma_adapt: L_in / C / Sigma_out / L_out / rows_out must be 16-byte aligned");
    REQUIRE((const float *)Sigma_out != L_in && Sigma_out != L_out && (const float *)Sigma_out != C && (const float *)L_out != C,
            "covo_sigma_adapt: Sigma_out must not be L_in, L_out or C, and L_out must not be C (L_out may be L_in)");
    return launch_sigma_adapt(L_in, C, batch, gamma, sample_sigma, Sigma_out, L_out, rows_out, (hipStream_t)stream);
}

// ---- the CMA controller (cma_path.hip): the attachment a step in COVO_MODE_CMA reads.  The step's captured graphs
// hold every value given here: a change bumps the epoch like a debug switch, and the state starts over.  What the step needs next to
// it (a posterior covariance and a diagnostics target, no Sigma period ...) is checked at the step (check_cma_step)
static bool cma_bounds_ok(float damping, float s_min, float s_max)
{
    return damping > 0.0f && damping < __builtin_inff() && s_min > 0.0f && s_min <= 1.0f && s_max >= 1.0f && s_max < __builtin_inff();
}

int covo_set_step_cma(covo_handle_t h, float gamma, int32_t step_size, float damping, float s_min, float s_max, float *rows_out,
                      double *path_out, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_cma: null handle");
    const bool on = rows_out != nullptr;
    REQUIRE(!on || (gamma >= 0.0f && gamma < 1.0f), "covo_set_step_cma: gamma=%g outside [0, 1)", (double)gamma);
    REQUIRE(!on || cma_bounds_ok(damping, s_min, s_max), "covo_set_step_cma: damping=%g, s_min=%g, s_max=%g: damping > 0 and 0 < s_min "
            "<= 1 <= s_max < inf are required", (double)damping, (double)s_min, (double)s_max);
    REQUIRE(!on || path_out != nullptr, "covo_set_step_cma: path_out is null (the evolution paths live there)");
    REQUIRE(!on || (n_inst > 0 && n_inst <= COVO_MAX_ENVS), "covo_set_step_cma: n_inst=%d outside (0, %d]", n_inst, COVO_MAX_ENVS);
    REQUIRE(!on || (((uintptr_t)rows_out | (uintptr_t)path_out) & 15) == 0, "covo_set_step_cma: rows_out and path_out must be 16-byte aligned");
    if (on && n_inst > h->cma_ws_n) {  // (the second factor buffer only ever grows; the graphs that hold it are dropped below)
        CHECK_DEVICE(h, "covo_set_step_cma");
        COVO_CHECK_HIP(hipDeviceSynchronize());  // (a setter, off the per-step path) no step in flight reads the old buffer
        COVO_CHECK_HIP(hipFree(h->cma_ws));
        h->cma_ws = nullptr;
        h->cma_ws_n = 0;
        h->cma_rows = nullptr;  // (a failed allocation leaves the mode detached, not pointing into freed memory)
        h->cma_p = nullptr;
        h->cma_n = 0;
        COVO_CHECK_HIP(hipMalloc(&h->cma_ws, covo_cma_ws_bytes(n_inst)));
        h->cma_ws_n = n_inst;
    }
    h->cma_n = on ? n_inst : 0;  // the rows of THIS attachment: what a step's instance count is held to
    h->cma_gamma = on ? gamma : 0.0f;
    h->cma_step_size = on ? (step_size != 0) : 0;
    h->cma_damping = damping;
    h->cma_s_min = s_min;
    h->cma_s_max = s_max;
    h->cma_rows = on ? rows_out : nullptr;
    h->cma_p = on ? path_out : nullptr;
    h->cma_age = 0;
    ++h->opt.epoch;
    return 0;
}

int covo_cma_reset(covo_handle_t h)
{
    REQUIRE(h, "covo_cma_reset: null handle");
    h->cma_age = 0;
    return 0;
}

int covo_cma_path(covo_handle_t h, const float *L_prev, const float *aux, int32_t aux_stride, const float *ess, int32_t ess_stride,
                  const float *L_hat, const float *Sigma_hat, const float *shape_rows, int32_t batch, int32_t n_samples, int32_t step_size,
                  float damping, float s_min, float s_max, double *p, double *log_s, float *L_out, float *Sigma_out, float *rows_out,
                  void *stream)
{
    REQUIRE(h, "covo_cma_path: null handle");
    CHECK_DEVICE(h, "covo_cma_path");
    REQUIRE(L_prev && aux && ess && L_hat && Sigma_hat && p && log_s && L_out && Sigma_out && rows_out && batch > 0 && batch <= 65535,
            "covo_cma_path: bad argument");
    REQUIRE(aux_stride > COVO_NA && ess_stride > 0 && n_samples > 0, "covo_cma_path: aux_stride=%d (> 128: d and W), ess_stride=%d, "
            "n_samples=%d", aux_stride, ess_stride, n_samples);
    REQUIRE(cma_bounds_ok(damping, s_min, s_max), "covo_cma_path: damping=%g, s_min=%g, s_max=%g: damping > 0 and 0 < s_min <= 1 <= s_max "
            "< inf are required", (double)damping, (double)s_min, (double)s_max);
    REQUIRE((((uintptr_t)L_prev | (uintptr_t)L_hat | (uintptr_t)Sigma_hat | (uintptr_t)shape_rows | (uintptr_t)L_out | (uintptr_t)Sigma_out |
              (uintptr_t)rows_out) & 15) == 0 && (((uintptr_t)p | (uintptr_t)log_s) & 7) == 0,
            "covo_cma_path: the matrices and rows must be 16-byte aligned, p and log_s 8-byte");
    REQUIRE(L_out != L_hat && L_out != Sigma_hat && Sigma_out != L_hat && (const float *)Sigma_out != L_prev && Sigma_out != L_out,
            "covo_cma_path: L_out may be L_prev and Sigma_out may be Sigma_hat; no other two matrices may coincide");
    CmaPathDesc d;
    d.L_prev = L_prev;
    d.aux = aux;
    d.aux_stride = aux_stride;
    d.ess = ess;
    d.ess_stride = ess_stride;
    d.L_hat = L_hat;
    d.Sigma_hat = Sigma_hat;
    d.shape_rows = shape_rows;
    d.batch = batch;
    d.n_samples = n_samples;
    d.step_size = step_size != 0;
    d.damping = (double)damping;
    d.log_s_min = std::log((double)s_min);
    d.log_s_max = std::log((double)s_max);
    d.p = p;
    d.log_s = log_s;
    d.L_out = L_out;
    d.Sigma_out = Sigma_out;
    d.rows_out = rows_out;
    return launch_cma_path(d, (hipStream_t)stream);
}

// ---- the state estimator (state_estimator.hip).  Its launch is eager and follows the env step of an episode driver:
// no captured step graph knows about it, nothing here bumps the epoch
static int check_estimator_buffers(const char *what, const double *xhat, const double *P, const int32_t *meta, const float *rows, int n_inst)
{
    REQUIRE(xhat && P && meta && rows, "%s: xhat, P, meta and rows must all be given", what);
    REQUIRE(n_inst > 0 && n_inst <= COVO_MAX_ENVS, "%s: n_inst=%d outside (0, %d]", what, n_inst, COVO_MAX_ENVS);
    REQUIRE((((uintptr_t)xhat | (uintptr_t)P) & 7) == 0 && (((uintptr_t)meta | (uintptr_t)rows) & 3) == 0,
            "%s: xhat and P must be 8-byte aligned, meta and rows 4-byte", what);
    return 0;
}

int covo_set_step_estimator(covo_handle_t h, const double *obs_std, const double *proc_std, double force_std, double *xhat, double *P,
                            int32_t *meta, float *rows, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_estimator: null handle");
    if (rows == nullptr) {  // off, the log with it
        h->est_rows = nullptr;
        h->est_xhat = h->est_P = nullptr;
        h->est_meta = nullptr;
        h->est_n = 0;
        h->est_log = nullptr;
        h->est_log_stride = 0;
        return 0;
    }
    REQUIRE(!covo_force_observer_on(h), "covo_set_step_estimator: a force observer is attached to this handle "
            "(covo_set_step_force_observer): two filters must not write one row");
    REQUIRE(obs_std && proc_std, "covo_set_step_estimator: obs_std and proc_std must be given");
    if (int rc = check_estimator_buffers("covo_set_step_estimator", xhat, P, meta, rows, n_inst)) return rc;
    EstDesc probe;  // (the values are checked on a default model: the derive marker needs the instance's own at the launch)
    covo_env_params unit{};
    unit.dt = unit.m = 1.0f;
    if (int rc = estimator_fill_model(probe, unit, obs_std, proc_std, force_std, "covo_set_step_estimator")) return rc;
    for (int g = 0; g < 4; ++g) {
        h->est_obs_std[g] = obs_std[g];
        h->est_proc_std[g] = proc_std[g];
    }
    h->est_force_std = force_std;
    h->est_xhat = xhat;
    h->est_P = P;
    h->est_meta = meta;
    h->est_rows = rows;
    h->est_n = n_inst;
    h->est_fresh = 1;
    return 0;
}

int covo_estimator_reset(covo_handle_t h)
{
    REQUIRE(h, "covo_estimator_reset: null handle");
    h->est_fresh = 1;
    return 0;
}

int covo_set_episode_estimator_log(covo_handle_t h, float *log, int32_t stride)
{
    REQUIRE(h, "covo_set_episode_estimator_log: null handle");
    REQUIRE(log == nullptr || stride > 0, "covo_set_episode_estimator_log: stride=%d", stride);
    REQUIRE(log == nullptr || covo_estimator_on(h), "covo_set_episode_estimator_log: no estimator attached: call covo_set_step_estimator first");
    h->est_log = log;
    h->est_log_stride = log ? stride : 0;
    return 0;
}

int covo_estimate(covo_handle_t h, float *state_rows, const float *u, int32_t u_stride, const covo_env_params *params,
                  const double *obs_std, const double *proc_std, double force_std, double *xhat, double *P, int32_t *meta, float *rows,
                  int32_t n_inst, int32_t reset, void *hip_stream)
{
    REQUIRE(h, "covo_estimate: null handle");
    CHECK_DEVICE(h, "covo_estimate");
    REQUIRE(state_rows && u && params && obs_std && proc_std && u_stride >= COVO_DU, "covo_estimate: bad argument");
    if (int rc = check_estimator_buffers("covo_estimate", xhat, P, meta, rows, n_inst)) return rc;
    static thread_local EstDesc d[COVO_MAX_ENVS];
    std::memset(d, 0, (size_t)n_inst * sizeof(EstDesc));
    for (int e = 0; e < n_inst; ++e) {
        CHECK_MODEL(&params[e], "covo_estimate");
        if (int rc = estimator_fill_model(d[e], params[e], obs_std, proc_std, force_std, "covo_estimate")) return rc;
        d[e].state = state_rows + (size_t)e * COVO_STATE_FLOATS;
        d[e].u = u + (size_t)e * u_stride;
        d[e].xhat = xhat + (size_t)e * COVO_EST_STATE_DOUBLES;
        d[e].P = P + (size_t)e * 13 * 13;
        d[e].meta = meta + (size_t)e * COVO_EST_META_INTS;
        d[e].row_out = rows + (size_t)e * COVO_EST_FLOATS;
    }
    const int fresh = reset < 0 ? h->est_fresh : (reset != 0);  // (reset < 0: what covo_estimator_reset left, taken once)
    if (reset < 0) h->est_fresh = 0;
    return launch_state_estimator(h, d, n_inst, n_inst > 1, true, fresh, -1, (hipStream_t)hip_stream);
}

// what an episode driver asks of the estimator before its first launch
static int check_episode_estimator(const covo_ctx *h, int n_inst, bool sharded, int first_row, int n_steps, const char *what)
{
    if (!covo_estimator_on(h)) return 0;
    REQUIRE(!sharded, "%s: the state estimator (covo_set_step_estimator) does not run on sample-sharded steps", what);
    REQUIRE(n_inst <= h->est_n, "%s: %d instances, the estimator's rows (covo_set_step_estimator) have n_inst=%d", what, n_inst, h->est_n);
    REQUIRE(h->est_log == nullptr || (first_row >= 0 && first_row + n_steps <= h->est_log_stride),
            "%s: episode estimator log rows [%d, %d) outside [0, %d) (covo_set_episode_estimator_log)", what, first_row, first_row + n_steps,
            h->est_log_stride);
    return 0;
}

// ---- the force observer (force_observer.hip).  Like the state estimator's, its launch is eager and follows the env step
// of an episode driver: no captured step graph knows about it, nothing here bumps the epoch
static int check_observer_buffers(const char *what, const double *xi, const double *P, const int32_t *meta, const float *rows, int n_inst)
{
    REQUIRE(xi && P && meta && rows, "%s: xi, P, meta and rows must all be given", what);
    REQUIRE(n_inst > 0 && n_inst <= COVO_MAX_ENVS, "%s: n_inst=%d outside (0, %d]", what, n_inst, COVO_MAX_ENVS);
    REQUIRE((((uintptr_t)xi | (uintptr_t)P) & 7) == 0 && (((uintptr_t)meta | (uintptr_t)rows) & 3) == 0,
            "%s: xi and P must be 8-byte aligned, meta and rows 4-byte", what);
    return 0;
}

int covo_set_step_force_observer(covo_handle_t h, const double *obs_std, const double *proc_std, double force_walk_std,
                                 double force_init_std, double *xi, double *P, int32_t *meta, float *rows, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_force_observer: null handle");
    if (rows == nullptr) {  // off, the log with it
        h->obs_rows = nullptr;
        h->obs_xi = h->obs_P = nullptr;
        h->obs_meta = nullptr;
        h->obs_n = 0;
        h->obs_log = nullptr;
        h->obs_log_stride = 0;
        return 0;
    }
    REQUIRE(!covo_estimator_on(h), "covo_set_step_force_observer: a state estimator is attached to this handle (covo_set_step_estimator): "
            "two filters must not write one row");
    REQUIRE(obs_std && proc_std, "covo_set_step_force_observer: obs_std and proc_std must be given");
    if (int rc = check_observer_buffers("covo_set_step_force_observer", xi, P, meta, rows, n_inst)) return rc;
    ObsDesc probe;
    covo_env_params unit{};
    unit.dt = unit.m = 1.0f;
    if (int rc = observer_fill_model(probe, unit, obs_std, proc_std, force_walk_std, force_init_std, "covo_set_step_force_observer")) return rc;
    for (int g = 0; g < 4; ++g) {
        h->obs_obs_std[g] = obs_std[g];
        h->obs_proc_std[g] = proc_std[g];
    }
    h->obs_walk_std = force_walk_std;
    h->obs_init_std = force_init_std;
    h->obs_xi = xi;
    h->obs_P = P;
    h->obs_meta = meta;
    h->obs_rows = rows;
    h->obs_n = n_inst;
    h->obs_fresh = 1;
    return 0;
}

int covo_force_observer_reset(covo_handle_t h)
{
    REQUIRE(h, "covo_force_observer_reset: null handle");
    h->obs_fresh = 1;
    return 0;
}

int covo_set_episode_force_observer_log(covo_handle_t h, float *log, int32_t stride)
{
    REQUIRE(h, "covo_set_episode_force_observer_log: null handle");
    REQUIRE(log == nullptr || stride > 0, "covo_set_episode_force_observer_log: stride=%d", stride);
    REQUIRE(log == nullptr || covo_force_observer_on(h),
            "covo_set_episode_force_observer_log: no force observer attached: call covo_set_step_force_observer first");
    h->obs_log = log;
    h->obs_log_stride = log ? stride : 0;
    return 0;
}

int covo_observe_force(covo_handle_t h, float *state_rows, const float *u, int32_t u_stride, const covo_env_params *params,
                       const double *obs_std, const double *proc_std, double force_walk_std, double force_init_std, double *xi, double *P,
                       int32_t *meta, float *rows, int32_t n_inst, int32_t reset, void *hip_stream)
{
    REQUIRE(h, "covo_observe_force: null handle");
    CHECK_DEVICE(h, "covo_observe_force");
    REQUIRE(state_rows && u && params && obs_std && proc_std && u_stride >= COVO_DU, "covo_observe_force: bad argument");
    if (int rc = check_observer_buffers("covo_observe_force", xi, P, meta, rows, n_inst)) return rc;
    static thread_local ObsDesc d[COVO_MAX_ENVS];
    std::memset(d, 0, (size_t)n_inst * sizeof(ObsDesc));
    for (int e = 0; e < n_inst; ++e) {
        CHECK_MODEL(&params[e], "covo_observe_force");
        if (int rc = observer_fill_model(d[e], params[e], obs_std, proc_std, force_walk_std, force_init_std, "covo_observe_force")) return rc;
        d[e].state = state_rows + (size_t)e * COVO_STATE_FLOATS;
        d[e].u = u + (size_t)e * u_stride;
        d[e].xi = xi + (size_t)e * COVO_OBS_STATE_DOUBLES;
        d[e].P = P + (size_t)e * 16 * 16;
        d[e].meta = meta + (size_t)e * COVO_OBS_META_INTS;
        d[e].row_out = rows + (size_t)e * COVO_OBS_FLOATS;
    }
    const int fresh = reset < 0 ? h->obs_fresh : (reset != 0);  // (reset < 0: what covo_force_observer_reset left, taken once)
    if (reset < 0) h->obs_fresh = 0;
    return launch_force_observer(h, d, n_inst, n_inst > 1, true, fresh, -1, (hipStream_t)hip_stream);
}

// what an episode driver asks of the force observer before its first launch (next to check_episode_estimator)
static int check_episode_force_observer(const covo_ctx *h, int n_inst, bool sharded, int first_row, int n_steps, const char *what)
{
    if (!covo_force_observer_on(h)) return 0;
    REQUIRE(!covo_estimator_on(h), "%s: a state estimator and a force observer are both attached: two filters must not write one row", what);
    REQUIRE(!sharded, "%s: the force observer (covo_set_step_force_observer) does not run on sample-sharded steps", what);
    REQUIRE(n_inst <= h->obs_n, "%s: %d instances, the force observer's rows (covo_set_step_force_observer) have n_inst=%d", what, n_inst,
            h->obs_n);
    REQUIRE(h->obs_log == nullptr || (first_row >= 0 && first_row + n_steps <= h->obs_log_stride),
            "%s: episode force observer log rows [%d, %d) outside [0, %d) (covo_set_episode_force_observer_log)", what, first_row,
            first_row + n_steps, h->obs_log_stride);
    return 0;
}

int covo_arbitrate(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                   const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps, const float *a,
                   const float *cost, int32_t N, const float *a_nominal, float *a_mean_inout, int32_t mask, float *row_out,
                   void *stream)
{
    REQUIRE(h, "covo_arbitrate: null handle");
    CHECK_DEVICE(h, "covo_arbitrate");
    REQUIRE(state && pos_traj && vel_traj && params && a && cost && a_nominal && a_mean_inout && row_out && T > 0,
            "covo_arbitrate: bad argument");
    REQUIRE(N > 0 && N <= h->cfg.n_local, "covo_arbitrate: N=%d outside (0, n_local=%d]", N, h->cfg.n_local);
    REQUIRE(mask >= 1 && mask <= 7, "covo_arbitrate: mask=%d outside [1, 7] (bit 0: softmax mean, 1: nominal, 2: best sample)", mask);
    CHECK_MODEL(params, "covo_arbitrate");
    REQUIRE(!covo_needs_tables(*params) || f_disturb_steps, "covo_arbitrate: disturb_kind=%d needs f_disturb_steps (covo_disturb_table)",
            params->disturb_kind);
    PlanInstDesc d = standalone_inst(state, pos_traj, vel_traj, T, params, f_disturb_shared, f_disturb_steps, a, N);
    d.cost = cost;
    d.a_nominal = a_nominal;
    d.a_mean = a_mean_inout;
    d.a_mean_out = a_mean_inout;
    return launch_update_arbiter_one(h, d, rollout_clip(h), mask, row_out, (hipStream_t)stream);  // the clip covo_rollout_cost applies
}

// ---- the Newton refinement (cost_gradient.hip, newton_refine.hip).  Its launches are eager and follow the step: no captured step
// graph changes
int covo_cost_gradient(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                       const covo_env_params *params, const float *a, const float *f_disturb_steps, int32_t batch, double *g_out,
                       void *stream)
{
    REQUIRE(h, "covo_cost_gradient: null handle");
    CHECK_DEVICE(h, "covo_cost_gradient");
    REQUIRE(state && pos_traj && vel_traj && params && a && g_out && T > 0 && batch > 0, "covo_cost_gradient: bad argument");
    CHECK_MODEL(params, "covo_cost_gradient");
    REQUIRE(!covo_needs_tables(*params) || f_disturb_steps, "covo_cost_gradient: disturb_kind=%d needs f_disturb_steps (covo_disturb_table)",
            params->disturb_kind);
    const int rc = covo_grow_workspace(h, &h->ws_grad, &h->ws_grad_bytes, cost_gradient_workspace_bytes(batch), (hipStream_t)stream);
    if (rc) return rc;
    return launch_cost_gradient(covo_hessian_inputs(state, pos_traj, vel_traj, T, params, a, f_disturb_steps, batch), g_out, h->ws_grad,
                                (hipStream_t)stream);
}

int covo_newton_refine(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                       const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                       const float *f_tab_hessian, const double *g, float *a_mean, const float *Sigma, const double *inv_c2,
                       int32_t n_inst, float *rows_out, float *costs_out, void *stream)
{
    REQUIRE(h, "covo_newton_refine: null handle");
    CHECK_DEVICE(h, "covo_newton_refine");
    REQUIRE(state && pos_traj && vel_traj && params && a_mean && Sigma && inv_c2 && rows_out && T > 0, "covo_newton_refine: bad argument");
    REQUIRE(n_inst > 0 && n_inst <= COVO_MAX_ENVS, "covo_newton_refine: n_inst=%d outside (0, %d]", n_inst, COVO_MAX_ENVS);
    REQUIRE(((uintptr_t)Sigma & 15) == 0 && ((uintptr_t)a_mean & 15) == 0, "covo_newton_refine: Sigma and a_mean must be 16-byte aligned");
    CHECK_MODEL(params, "covo_newton_refine");
    REQUIRE(!covo_needs_tables(*params) || (f_disturb_steps && (g || f_tab_hessian)),
            "covo_newton_refine: disturb_kind=%d needs f_disturb_steps and f_tab_hessian (covo_disturb_table)", params->disturb_kind);
    hipStream_t s = (hipStream_t)stream;
    if (g == nullptr) {
        int rc = covo_grow_workspace(h, &h->ws_grad, &h->ws_grad_bytes, cost_gradient_workspace_bytes(n_inst), s);
        if (rc) return rc;
        if (h->refine_g == nullptr) COVO_CHECK_HIP(hipMalloc(&h->refine_g, (size_t)COVO_MAX_ENVS * COVO_NA * sizeof(double)));
        if ((rc = launch_cost_gradient(covo_hessian_inputs(state, pos_traj, vel_traj, T, params, a_mean, f_tab_hessian, n_inst), h->refine_g,
                                       h->ws_grad, s)))
            return rc;
        g = h->refine_g;
    }
    for (int e = 0; e < n_inst; ++e) {
        PlanInstDesc d = standalone_inst(state + (size_t)e * COVO_STATE_FLOATS, pos_traj, vel_traj, T, params, f_disturb_shared,
                                         f_disturb_steps ? f_disturb_steps + (size_t)e * COVO_H * 4 : nullptr, nullptr, 1);
        d.a_mean = d.a_mean_out = a_mean + (size_t)e * COVO_NA;
        RefineDesc r;
        r.g = g + (size_t)e * COVO_NA;
        r.Sigma = Sigma + (size_t)e * COVO_NA * COVO_NA;
        r.inv_c2 = inv_c2 + e;
        r.row_out = rows_out + (size_t)e * COVO_REFINE_FLOATS;
        r.costs_out = costs_out ? costs_out + (size_t)e * COVO_REFINE_CANDIDATES : nullptr;
        if (int rc = launch_newton_refine_one(h, d, rollout_clip(h), r, s)) return rc;
    }
    return 0;
}

int covo_set_step_refine(covo_handle_t h, float *rows, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_refine: null handle");
    if (rows == nullptr) {
        h->refine_out = nullptr;
        h->refine_n = 0;
        return 0;
    }
    if (int rc = check_setter_rows("covo_set_step_refine", true, n_inst)) return rc;
    // the step's gradient scratch, here and not in a step: a workspace never grows inside the steady state
    const int rc = covo_grow_workspace(h, &h->ws_grad, &h->ws_grad_bytes, cost_gradient_workspace_bytes(n_inst), nullptr);
    if (rc) return rc;
    if (h->refine_g == nullptr) COVO_CHECK_HIP(hipMalloc(&h->refine_g, (size_t)COVO_MAX_ENVS * COVO_NA * sizeof(double)));
    h->refine_out = rows;
    h->refine_n = n_inst;
    return 0;
}

// ---- the Riccati refinement (riccati.hip, newton_refine.hip with the direction supplied).  Like the Newton refinement's, its launches
// are eager and follow the step: no captured step graph changes
static int riccati_reserve(covo_ctx *h, int batch, hipStream_t s)
{
    if (int rc = covo_grow_workspace(h, &h->ws_riccati, &h->ws_riccati_bytes, riccati_workspace_bytes(batch), s)) return rc;
    if (h->riccati_d == nullptr)
        COVO_CHECK_HIP(hipMalloc(&h->riccati_d, (size_t)COVO_MAX_ENVS * (COVO_NA + COVO_RICCATI_SIDE) * sizeof(double)));
    if (h->refine_g == nullptr) COVO_CHECK_HIP(hipMalloc(&h->refine_g, (size_t)COVO_MAX_ENVS * COVO_NA * sizeof(double)));
    if (h->riccati_tab == nullptr) COVO_CHECK_HIP(hipMalloc(&h->riccati_tab, (size_t)COVO_H * 4 * sizeof(float)));
    return 0;
}

// covo_riccati (box false) and covo_riccati_box
static int riccati_sweep_body(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                              const covo_env_params *params, const float *a, const float *f_tab_hessian, int32_t batch, double reg0,
                              double *d_out, double *K_out, double *kff_out, double *x_out, double *rows_out, bool box, int32_t *masks_out,
                              const char *who, void *stream)
{
    REQUIRE(h, "%s: null handle", who);
    CHECK_DEVICE(h, who);
    REQUIRE(state && pos_traj && vel_traj && params && a && d_out && T > 0 && batch > 0, "%s: bad argument", who);
    CHECK_MODEL(params, who);
    REQUIRE(!covo_needs_tables(*params) || f_tab_hessian, "%s: disturb_kind=%d needs f_tab_hessian (covo_disturb_table)", who,
            params->disturb_kind);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = covo_grow_workspace(h, &h->ws_riccati, &h->ws_riccati_bytes, riccati_workspace_bytes(batch), s)) return rc;
    HessianDesc d = covo_hessian_inputs(state, pos_traj, vel_traj, T, params, a, f_tab_hessian, batch);
    d.status_dev = h->status_dev;
    RiccatiOut o;
    o.d = d_out;
    o.K = K_out;
    o.kff = kff_out;
    o.x = x_out;
    o.side = rows_out;
    o.box = box;
    o.masks = masks_out;
    return launch_riccati(d, reg0, o, h->ws_riccati, s);
}

int covo_riccati(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                 const covo_env_params *params, const float *a, const float *f_tab_hessian, int32_t batch, double reg0, double *d_out,
                 double *K_out, double *kff_out, double *x_out, double *rows_out, void *stream)
{
    return riccati_sweep_body(h, state, pos_traj, vel_traj, T, params, a, f_tab_hessian, batch, reg0, d_out, K_out, kff_out, x_out,
                              rows_out, false, nullptr, "covo_riccati", stream);
}

int covo_riccati_box(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                     const covo_env_params *params, const float *a, const float *f_tab_hessian, int32_t batch, double reg0, double *d_out,
                     double *K_out, double *kff_out, double *x_out, double *rows_out, int32_t *masks_out, void *stream)
{
    return riccati_sweep_body(h, state, pos_traj, vel_traj, T, params, a, f_tab_hessian, batch, reg0, d_out, K_out, kff_out, x_out,
                              rows_out, true, masks_out, "covo_riccati_box", stream);
}

// the sweep's gains and the generator's sequences of a step's instances, here and not in a step (covo_common.hpp: the layouts)
static int feedback_reserve(covo_ctx *h)
{
    if (h->feedback_gains == nullptr)
        COVO_CHECK_HIP(hipMalloc(&h->feedback_gains, (size_t)COVO_MAX_ENVS * COVO_FEEDBACK_GAIN_DOUBLES * sizeof(double)));
    if (h->feedback_a == nullptr)
        COVO_CHECK_HIP(hipMalloc(&h->feedback_a, (size_t)COVO_MAX_ENVS * COVO_FEEDBACK_LADDER * (COVO_NA + COVO_FEEDBACK_AUX_FLOATS) * sizeof(float)));
    return 0;
}
static bool feedback_refuses(const covo_env_params *p) { return p->disturb_kind == COVO_DISTURB_DRAG || p->disturb_kind == COVO_DISTURB_MIXED; }
#define FEEDBACK_PLANT_MSG                                                                                                            \
    "%s: disturb_kind=%d (drag / mixed) is a 16-state plant -- its force is a state of the sweep and a per-sample quantity of the "    \
    "rollout; the closed-loop generator carries the 13-state plants only"

// covo_riccati_refine (fb_rows_out null: 17 candidates), covo_riccati_refine_feedback (33) and, over the box sweep (masks_out
// [n_inst][H] or null), covo_riccati_refine_box
static int riccati_refine_body(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                               const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                               const float *f_tab_hessian, float *a_mean, double reg0, int32_t n_inst, float *rows_out, float *costs_out,
                               float *fb_rows_out, bool feedback, bool box, int32_t *masks_out, const char *who, void *stream)
{
    REQUIRE(h, "%s: null handle", who);
    CHECK_DEVICE(h, who);
    REQUIRE(state && pos_traj && vel_traj && params && a_mean && rows_out && (fb_rows_out || !feedback) && T > 0, "%s: bad argument", who);
    REQUIRE(n_inst > 0 && n_inst <= COVO_MAX_ENVS, "%s: n_inst=%d outside (0, %d]", who, n_inst, COVO_MAX_ENVS);
    REQUIRE(((uintptr_t)a_mean & 15) == 0, "%s: a_mean must be 16-byte aligned", who);
    CHECK_MODEL(params, who);
    REQUIRE(!covo_needs_tables(*params) || (f_disturb_steps && f_tab_hessian),
            "%s: disturb_kind=%d needs f_disturb_steps and f_tab_hessian (covo_disturb_table)", who, params->disturb_kind);
    REQUIRE(!feedback || !feedback_refuses(params), FEEDBACK_PLANT_MSG, who, params->disturb_kind);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = riccati_reserve(h, n_inst, s)) return rc;
    if (feedback)
        if (int rc = feedback_reserve(h)) return rc;
    HessianDesc hd = covo_hessian_inputs(state, pos_traj, vel_traj, T, params, a_mean, f_tab_hessian, n_inst);
    hd.status_dev = h->status_dev;
    RiccatiOut o = covo_riccati_out(h, feedback);
    o.box = box;
    o.masks = masks_out;
    if (int rc = launch_riccati(hd, reg0, o, h->ws_riccati, s)) return rc;
    if (feedback && h->feedback_poke_armed) {  // covo_debug_feedback_gain: once
        h->feedback_poke_armed = 0;
        REQUIRE(h->feedback_poke_at < n_inst * COVO_H * 64, "%s: covo_debug_feedback_gain names an instance beyond n_inst=%d", who, n_inst);
        COVO_CHECK_HIP(hipMemcpyAsync(h->feedback_gains + h->feedback_poke_at, &h->feedback_poke, sizeof(double), hipMemcpyHostToDevice, s));
        COVO_CHECK_HIP(hipStreamSynchronize(s));  // (the source is a member of the handle)
    }
    const int ncost = feedback ? COVO_FEEDBACK_CANDIDATES : COVO_REFINE_CANDIDATES;
    for (int e = 0; e < n_inst; ++e) {
        PlanInstDesc d = standalone_inst(state + (size_t)e * COVO_STATE_FLOATS, pos_traj, vel_traj, T, params, f_disturb_shared,
                                         f_disturb_steps ? f_disturb_steps + (size_t)e * COVO_H * 4 : nullptr, nullptr, 1);
        d.a_mean = d.a_mean_out = a_mean + (size_t)e * COVO_NA;
        FeedbackDesc f;
        if (feedback) {
            f = covo_feedback_desc(h, e, d.a_mean);
            double ladder[COVO_FEEDBACK_LADDER];
            for (int j = 1; j <= COVO_FEEDBACK_LADDER; ++j) ladder[j - 1] = std::ldexp(1.0, 3 - j);
            if (int rc = launch_feedback_rollout_one(h, d, f, ladder, s)) return rc;
        }
        const RefineDesc r = covo_riccati_refine_desc(o, e, rows_out + (size_t)e * COVO_RICCATI_FLOATS,
                                                      costs_out ? costs_out + (size_t)e * ncost : nullptr, feedback ? &f : nullptr,
                                                      feedback ? fb_rows_out + (size_t)e * COVO_FEEDBACK_FLOATS : nullptr);
        if (int rc = launch_newton_refine_one(h, d, rollout_clip(h), r, s)) return rc;
    }
    return 0;
}

int covo_riccati_refine(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                        const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                        const float *f_tab_hessian, float *a_mean, double reg0, int32_t n_inst, float *rows_out, float *costs_out,
                        void *stream)
{
    return riccati_refine_body(h, state, pos_traj, vel_traj, T, params, f_disturb_shared, f_disturb_steps, f_tab_hessian, a_mean, reg0,
                               n_inst, rows_out, costs_out, nullptr, false, false, nullptr, "covo_riccati_refine", stream);
}

int covo_riccati_refine_feedback(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                                 const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                                 const float *f_tab_hessian, float *a_mean, double reg0, int32_t n_inst, float *rows_out,
                                 float *costs_out, float *fb_rows_out, void *stream)
{
    return riccati_refine_body(h, state, pos_traj, vel_traj, T, params, f_disturb_shared, f_disturb_steps, f_tab_hessian, a_mean, reg0,
                               n_inst, rows_out, costs_out, fb_rows_out, true, false, nullptr, "covo_riccati_refine_feedback", stream);
}

int covo_riccati_refine_box(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                            const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                            const float *f_tab_hessian, float *a_mean, double reg0, int32_t n_inst, float *rows_out, float *costs_out,
                            float *fb_rows_out, int32_t feedback, int32_t *masks_out, void *stream)
{
    return riccati_refine_body(h, state, pos_traj, vel_traj, T, params, f_disturb_shared, f_disturb_steps, f_tab_hessian, a_mean, reg0,
                               n_inst, rows_out, costs_out, feedback ? fb_rows_out : nullptr, feedback != 0, true, masks_out,
                               "covo_riccati_refine_box", stream);
}

int covo_feedback_rollout(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                          const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps, const float *a,
                          const double *K, const double *kff, const double *x, const double *alphas, int32_t n_alpha, int32_t n_inst,
                          float *a_out, float *aux_out, void *stream)
{
    REQUIRE(h, "covo_feedback_rollout: null handle");
    CHECK_DEVICE(h, "covo_feedback_rollout");
    REQUIRE(state && pos_traj && vel_traj && params && a && K && kff && x && alphas && a_out && aux_out && T > 0,
            "covo_feedback_rollout: bad argument");
    REQUIRE(n_inst > 0 && n_inst <= COVO_MAX_ENVS, "covo_feedback_rollout: n_inst=%d outside (0, %d]", n_inst, COVO_MAX_ENVS);
    REQUIRE(n_alpha >= 1 && n_alpha <= COVO_FEEDBACK_MAX_ALPHAS, "covo_feedback_rollout: n_alpha=%d outside [1, %d]", n_alpha,
            COVO_FEEDBACK_MAX_ALPHAS);
    REQUIRE((((uintptr_t)a | (uintptr_t)K | (uintptr_t)kff | (uintptr_t)x | (uintptr_t)a_out) & 15) == 0,
            "covo_feedback_rollout: a, K, kff, x and a_out must be 16-byte aligned");
    CHECK_MODEL(params, "covo_feedback_rollout");
    REQUIRE(!feedback_refuses(params), FEEDBACK_PLANT_MSG, "covo_feedback_rollout", params->disturb_kind);
    REQUIRE(!covo_needs_tables(*params) || f_disturb_steps, "covo_feedback_rollout: disturb_kind=%d needs f_disturb_steps (covo_disturb_table)",
            params->disturb_kind);
    for (int e = 0; e < n_inst; ++e) {
        const PlanInstDesc d = standalone_inst(state + (size_t)e * COVO_STATE_FLOATS, pos_traj, vel_traj, T, params, f_disturb_shared,
                                               f_disturb_steps ? f_disturb_steps + (size_t)e * COVO_H * 4 : nullptr, nullptr, 1);
        FeedbackDesc f;
        f.b = a + (size_t)e * COVO_NA;
        f.K = K + (size_t)e * COVO_H * 64;
        f.kff = kff + (size_t)e * COVO_H * 4;
        f.x = x + (size_t)e * COVO_H * 16;
        f.a_out = a_out + (size_t)e * n_alpha * COVO_NA;
        f.aux_out = aux_out + (size_t)e * n_alpha * COVO_FEEDBACK_AUX_FLOATS;
        f.n_alpha = n_alpha;
        if (int rc = launch_feedback_rollout_one(h, d, f, alphas, (hipStream_t)stream)) return rc;
    }
    return 0;
}

int covo_debug_feedback_gain(covo_handle_t h, int32_t inst, int32_t index, double value)
{
    REQUIRE(h, "covo_debug_feedback_gain: null handle");
    REQUIRE(inst >= 0 && inst < COVO_MAX_ENVS && index >= 0 && index < COVO_H * 64,
            "covo_debug_feedback_gain: inst=%d outside [0, %d) or index=%d outside [0, %d)", inst, COVO_MAX_ENVS, index, COVO_H * 64);
    h->feedback_poke_armed = 1;
    h->feedback_poke_at = inst * COVO_H * 64 + index;
    h->feedback_poke = value;
    return 0;
}

int covo_set_step_riccati_feedback(covo_handle_t h, float *fb_rows, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_riccati_feedback: null handle");
    if (fb_rows == nullptr) {
        h->feedback_out = nullptr;
        h->feedback_n = 0;
        return 0;
    }
    if (int rc = check_setter_rows("covo_set_step_riccati_feedback", true, n_inst)) return rc;
    REQUIRE(covo_riccati_on(h) && n_inst <= h->riccati_n,
            "covo_set_step_riccati_feedback: n_inst=%d needs the Riccati refinement attached on the handle with at least as many "
            "instances (covo_set_step_riccati: %d)", n_inst, h->riccati_n);
    // the step's scratch, here and not in a step
    if (int rc = feedback_reserve(h)) return rc;
    h->feedback_out = fb_rows;
    h->feedback_n = n_inst;
    return 0;
}

int covo_set_step_riccati(covo_handle_t h, float *rows, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_riccati: null handle");
    if (rows == nullptr) {
        h->riccati_out = nullptr;
        h->riccati_n = 0;
        return 0;
    }
    if (int rc = check_setter_rows("covo_set_step_riccati", true, n_inst)) return rc;
    // the step's scratch, here and not in a step: a workspace never grows inside the steady state
    if (int rc = riccati_reserve(h, n_inst, nullptr)) return rc;
    h->riccati_out = rows;
    h->riccati_n = n_inst;
    return 0;
}

// ---- the plan hold (plan_hold.hip; the schedule: covo_plan_step_age / _done, covo_common.hpp).  Plan steps keep their launches and
// graphs; a hold step is one eager launch: no epoch bump.  What the step needs next to it is checked at the step (check_step_attachments)
int covo_set_step_plan_hold(covo_handle_t h, int32_t period, float *rows, int32_t n_inst)
{
    REQUIRE(h, "covo_set_step_plan_hold: null handle");
    REQUIRE(period >= 1 && period <= COVO_MAX_PLAN_HOLD, "covo_set_step_plan_hold: period=%d outside [1, %d] (1 = off: every step plans)",
            period, COVO_MAX_PLAN_HOLD);
    h->plan_age = 0;
    h->hold_latch_n = 0;
    if (period == 1) {
        h->plan_hold = 1;
        h->hold_rows = nullptr;
        h->hold_n = 0;
        covo_eprow_drop(h, COVO_EPLOG_HOLD);  // off, the log with it
        return 0;
    }
    REQUIRE(rows != nullptr && n_inst > 0 && n_inst <= COVO_MAX_ENVS, "covo_set_step_plan_hold: period=%d needs rows and n_inst=%d in (0, %d]",
            period, n_inst, COVO_MAX_ENVS);
    // the step's scratch, here and not in a step: the sweep's gains, the latch, a hold step's keys
    if (int rc = feedback_reserve(h)) return rc;
    if (h->hold_b == nullptr) COVO_CHECK_HIP(hipMalloc(&h->hold_b, (size_t)COVO_MAX_ENVS * COVO_NA * sizeof(float)));
    if (h->hold_t == nullptr) COVO_CHECK_HIP(hipMalloc(&h->hold_t, (size_t)COVO_MAX_ENVS * sizeof(int)));
    if (h->hold_keys == nullptr) {
        COVO_CHECK_HIP(hipMalloc(&h->hold_keys, (size_t)COVO_MAX_ENVS * 12 * sizeof(uint32_t)));
        COVO_CHECK_HIP(hipMemset(h->hold_keys, 0, (size_t)COVO_MAX_ENVS * 12 * sizeof(uint32_t)));
    }
    h->plan_hold = period;
    h->hold_rows = rows;
    h->hold_n = n_inst;
    return 0;
}

int covo_plan_hold(covo_handle_t h, const float *state, const float *b, const double *K, const double *kff, const double *x,
                   const double *side, const float *alpha, int32_t alpha_stride, int32_t stage, const int32_t *t_plan, float *a_mean,
                   float *a_cov, float *u_out, float *rows_out, int32_t n_inst, void *stream)
{
    REQUIRE(h, "covo_plan_hold: null handle");
    CHECK_DEVICE(h, "covo_plan_hold");
    REQUIRE(state && b && K && kff && x && alpha && u_out && rows_out, "covo_plan_hold: bad argument");
    REQUIRE(n_inst > 0 && n_inst <= COVO_MAX_ENVS, "covo_plan_hold: n_inst=%d outside (0, %d]", n_inst, COVO_MAX_ENVS);
    REQUIRE(stage >= 0 && stage < COVO_H, "covo_plan_hold: stage=%d outside [0, %d)", stage, COVO_H);
    REQUIRE(alpha_stride >= 0, "covo_plan_hold: alpha_stride=%d", alpha_stride);
    REQUIRE((((uintptr_t)a_mean | (uintptr_t)a_cov) & 15) == 0, "covo_plan_hold: a_mean and a_cov must be 16-byte aligned");
    HoldDesc d[COVO_MAX_ENVS];
    std::memset(d, 0, (size_t)n_inst * sizeof(HoldDesc));
    for (int e = 0; e < n_inst; ++e) {
        d[e].state = state + (size_t)e * COVO_STATE_FLOATS;
        d[e].b = b + (size_t)e * COVO_NA;
        d[e].K = K + (size_t)e * COVO_H * 64;
        d[e].kff = kff + (size_t)e * COVO_H * 4;
        d[e].x = x + (size_t)e * COVO_H * 16;
        d[e].side = side ? side + (size_t)e * COVO_RICCATI_SIDE : nullptr;
        d[e].alpha = alpha + (size_t)e * alpha_stride;
        d[e].t_plan = t_plan ? t_plan + e : nullptr;
        d[e].a_mean_src = d[e].a_mean = a_mean ? a_mean + (size_t)e * COVO_NA : nullptr;
        d[e].a_cov = a_cov ? a_cov + (size_t)e * COVO_H * 16 : nullptr;
        d[e].u_out = u_out + (size_t)e * COVO_DU;
        d[e].row_out = rows_out + (size_t)e * COVO_HOLD_FLOATS;
    }
    return launch_plan_hold(h, d, n_inst, n_inst > 1, true, stage, -1, (hipStream_t)stream);
}

int covo_debug_plan_latch(covo_handle_t h, int32_t n_inst, float *b_out, int32_t *t_out, double *K_out, double *kff_out, double *x_out,
                          void *stream)
{
    REQUIRE(h, "covo_debug_plan_latch: null handle");
    REQUIRE(b_out && t_out && K_out && kff_out && x_out, "covo_debug_plan_latch: bad argument");
    REQUIRE(h->hold_b != nullptr && h->hold_latch_n > 0 && n_inst > 0 && n_inst <= h->hold_latch_n,
            "covo_debug_plan_latch: no plan step has latched on this handle, or n_inst=%d exceeds its %d instances", n_inst, h->hold_latch_n);
    hipStream_t s = (hipStream_t)stream;
    const FeedbackDesc f = covo_feedback_desc(h, 0, nullptr);  // (dense by instance)
    COVO_CHECK_HIP(hipMemcpyAsync(b_out, h->hold_b, (size_t)n_inst * COVO_NA * sizeof(float), hipMemcpyDeviceToDevice, s));
    COVO_CHECK_HIP(hipMemcpyAsync(t_out, h->hold_t, (size_t)n_inst * sizeof(int), hipMemcpyDeviceToDevice, s));
    COVO_CHECK_HIP(hipMemcpyAsync(K_out, f.K, (size_t)n_inst * COVO_H * 64 * sizeof(double), hipMemcpyDeviceToDevice, s));
    COVO_CHECK_HIP(hipMemcpyAsync(kff_out, f.kff, (size_t)n_inst * COVO_H * 4 * sizeof(double), hipMemcpyDeviceToDevice, s));
    COVO_CHECK_HIP(hipMemcpyAsync(x_out, f.x, (size_t)n_inst * COVO_H * 16 * sizeof(double), hipMemcpyDeviceToDevice, s));
    return 0;
}

int covo_debug_sigma_workspace(covo_handle_t h, double *out, int64_t offset_doubles, int64_t count, void *stream)
{
    REQUIRE(h && out, "covo_debug_sigma_workspace: bad argument");
    REQUIRE((size_t)(offset_doubles + count) * sizeof(double) <= h->ws_sigma_bytes, "covo_debug_sigma_workspace: range");
    COVO_CHECK_HIP(hipMemcpyAsync(out, (const double *)h->ws_sigma + offset_doubles, (size_t)count * sizeof(double),
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int covo_env_step(covo_handle_t h, float *state, float *noisy_state, const float *pos_traj, const float *vel_traj,
                  const float *acc_traj, int32_t T, const covo_env_params *params, const float *action,
                  const uint32_t *step_key, int32_t noisy_on, float obs_noise_scale, float *log, int32_t log_index,
                  void *stream)
{
    REQUIRE(h, "covo_env_step: null handle");
    REQUIRE(state && noisy_state && pos_traj && vel_traj && acc_traj && params && action && step_key && T > 0 &&
                log_index >= 0,
            "covo_env_step: bad argument");
    CHECK_MODEL(params, "covo_env_step");
    return launch_env_step(state, noisy_state, pos_traj, vel_traj, acc_traj, T, *params, action, step_key, noisy_on,
                           obs_noise_scale, log, log_index, (hipStream_t)stream);
}

int covo_pid_nominal(covo_handle_t h, const float *state0, const float *pos_traj, const float *vel_traj,
                     const float *acc_traj, int32_t T, const covo_env_params *params, const covo_env_params *pid_params,
                     float Kp, float Kd, float Kp_att, uint32_t key0, uint32_t key1, int32_t n_steps,
                     float *states_out, float *a_means_out, uint32_t *keys_out, void *stream)
{
    REQUIRE(h, "covo_pid_nominal: null handle");
    REQUIRE(state0 && pos_traj && vel_traj && acc_traj && params && pid_params && states_out && a_means_out && T > 0 &&
                n_steps > 0,
            "covo_pid_nominal: bad argument");
    CHECK_MODEL(params, "covo_pid_nominal");
    return launch_pid_nominal(state0, pos_traj, vel_traj, acc_traj, T, *params, *pid_params, Kp, Kd, Kp_att, key0, key1, n_steps,
                              states_out, a_means_out, keys_out, (hipStream_t)stream);
}

// Philox4x32-10 on the host: child i of split(key, num) as covo_mpc_amd/random.py forms it
static void host_philox_split(const uint32_t key[2], uint32_t i, uint32_t child[2])
{
    uint32_t c0 = i, c1 = 0, c2 = 0, c3 = 0x5EEDu, k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    child[0] = c0;
    child[1] = c1;
}

int covo_run_episode(covo_handle_t h, const covo_env_params *params, const covo_step_args *args, float *state_true,
                     const float *acc_traj, int32_t noisy_on, float obs_noise_scale, float *log, uint32_t *rng,
                     int32_t n_steps, void *stream)
{
    REQUIRE(h, "covo_run_episode: null handle");
    CHECK_DEVICE(h, "covo_run_episode");
    REQUIRE(params && args && state_true && acc_traj && rng && n_steps > 0, "covo_run_episode: bad argument");
    REQUIRE(args->derive_keys == 1, "covo_run_episode: args->derive_keys must be 1 (the controller key is the raw rng_act)");
    REQUIRE(args->a_mean_in == nullptr, "covo_run_episode: args->a_mean_in must be NULL (the episode carries the mean in args->a_mean)");
    REQUIRE(args->partial_out == nullptr || (exchange_ready(h) && args->a_mean_shift != nullptr),
            "covo_run_episode: a sample-sharded step (partial_out != NULL) needs the peer-write exchange (covo_exchange_create / "
            "covo_exchange_connect) and a_mean_shift");
    int rc = check_single_step(h, params, args, "covo_run_episode");
    if (rc || (rc = check_episode_logs(h, 0, n_steps, "covo_run_episode"))) return rc;
    if ((rc = check_episode_estimator(h, 1, args->partial_out != nullptr, 0, n_steps, "covo_run_episode"))) return rc;
    if ((rc = check_episode_force_observer(h, 1, args->partial_out != nullptr, 0, n_steps, "covo_run_episode"))) return rc;
    hipStream_t s = (hipStream_t)stream;
    uint32_t key[2] = {rng[0], rng[1]};
    for (int t = 0; t < n_steps; ++t) {
        // run_one_step (quadrotor.py:520-538): rng, rng_act, rng_step, rng_control = split(rng, 4); ...; rng, _ = split(rng)
        uint32_t nrng[2], rng_act[2], rng_step[2];
        host_philox_split(key, 0u, nrng);
        host_philox_split(key, 1u, rng_act);
        host_philox_split(key, 2u, rng_step);
        auto exchange = [&]() -> int {
            if (args->partial_out == nullptr) return 0;
            // sample-sharded: every rank's record to every rank (peer writes, exchange.hip), then the same merge on all of them.
            // partial_out is this rank's RANK record: {m, s, v} there, its position sums (if any) at + COVO_PARTIAL_FLOATS
            const float *gathered = nullptr;
            if (args->mode == COVO_MODE_MPPI && args->gamma_sigma != 0.0f) {
                // mppi.py:119-125 on sharded ranks: the record also carries the 320 second moments (COVO_RANK_RECORD_COV_FLOATS);
                // a_cov was shifted in place by the begin launch and is adapted in place, identically on every rank
                if ((rc = exchange_records(h, args->partial_out, nullptr, &gathered, s, COVO_RANK_RECORD_COV_FLOATS))) return rc;
                UpdateDesc d = update_from_records(gathered, exchange_world(h), COVO_RANK_RECORD_COV_FLOATS, args->a_mean_shift,
                                                   args->gamma_mean, args->a_mean);
                d.a_cov_old = args->a_cov;
                d.gamma_sigma = args->gamma_sigma;
                d.a_cov_out = args->a_cov;
                if ((rc = launch_merge_cov(d, h->cfg.lam, s))) return rc;
            } else {
                if ((rc = exchange_records(h, args->partial_out, nullptr, &gathered, s))) return rc;
                if ((rc = launch_merge(update_from_records(gathered, exchange_world(h), COVO_RANK_RECORD_FLOATS, args->a_mean_shift,
                                                           args->gamma_mean, args->a_mean),
                                       h->cfg.lam, s)))
                    return rc;
            }
            return 0;
        };
        // (rng_step is what it was on a hold step too; the posterior covariance's rows are formed in the frame)
        auto rows = [&] { return launch_episode_rows(h, 1, t, h->sigma_last_age, s); };
        if ((rc = single_scheduled_step(h, params, args, rng_act[0], rng_act[1], nullptr, state_true, t, s, exchange, rows))) return rc;
        rc = launch_env_step(state_true, const_cast<float *>(args->state), args->pos_traj, args->vel_traj, acc_traj, args->T,
                             *params, args->a_mean, rng_step, noisy_on, obs_noise_scale, log, t, s);
        if (rc) return rc;
        if ((rc = covo_estimator_step(h, const_cast<float *>(args->state), args->a_mean, params, 1, false, t, s))) return rc;
        if ((rc = covo_force_observer_step(h, const_cast<float *>(args->state), args->a_mean, params, 1, false, t, s))) return rc;
        host_philox_split(nrng, 0u, key);
    }
    rng[0] = key[0];
    rng[1] = key[1];
    return 0;
}

int covo_env_step_batched(covo_handle_t h, int32_t n_envs, float *states, float *noisy_states, const float *pos_traj,
                          const float *vel_traj, const float *acc_traj, int32_t T, const covo_env_params *params,
                          const float *a_mean, const uint32_t *step_keys, int32_t noisy_on, float obs_noise_scale, float *log,
                          int32_t log_stride, int32_t log_index, void *stream)
{
    REQUIRE(h, "covo_env_step_batched: null handle");
    CHECK_DEVICE(h, "covo_env_step_batched");
    REQUIRE(n_envs > 0 && n_envs <= COVO_MAX_ENVS, "covo_env_step_batched: n_envs=%d outside (0, %d]", n_envs, COVO_MAX_ENVS);
    REQUIRE(states && noisy_states && pos_traj && vel_traj && acc_traj && params && a_mean && step_keys && T > 0,
            "covo_env_step_batched: bad argument");
    REQUIRE(log == nullptr || (log_index >= 0 && log_index < log_stride), "covo_env_step_batched: log_index=%d outside [0, %d)",
            log_index, log_stride);
    int rc = check_batch_models(params, n_envs, true, "covo_env_step_batched");
    if (rc) return rc;
    const void *inst = nullptr;
    if ((rc = batch_env_inst(h, params, n_envs, (hipStream_t)stream, &inst))) return rc;
    return launch_env_step_batched(states, noisy_states, pos_traj, vel_traj, acc_traj, T, params[0], inst, n_envs, a_mean, step_keys,
                                   noisy_on, obs_noise_scale, log, log_stride, log_index, (hipStream_t)stream);
}

static int run_episode_batched(covo_handle_t h, const covo_batch_args *args, const covo_batch_mode_args *m, const covo_env_params *params,
                               float *states_true, const float *acc_traj, int32_t noisy_on, float obs_noise_scale, float *log,
                               int32_t log_stride, int32_t log_index, uint32_t *rngs, int32_t n_steps, void *stream, const char *what)
{
    REQUIRE(h, "%s: null handle", what);
    CHECK_DEVICE(h, what);
    REQUIRE(args && params && states_true && acc_traj && rngs && n_steps > 0, "%s: bad argument", what);
    const int E = args->n_envs;
    covo_batch_mode_args norm;
    int rc = check_batch_step(h, args, m, params, true, what, &norm);
    if (rc) return rc;
    REQUIRE(log == nullptr || (log_index >= 0 && log_index + n_steps <= log_stride),
            "%s: log rows [%d, %d) outside [0, %d)", what, log_index, log_index + n_steps, log_stride);
    if ((rc = check_episode_logs(h, log_index, n_steps, what))) return rc;
    if ((rc = check_episode_estimator(h, E, false, log_index, n_steps, what))) return rc;
    if ((rc = check_episode_force_observer(h, E, false, log_index, n_steps, what))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const void *inst = nullptr;
    if ((rc = batch_env_inst(h, params, E, s, &inst))) return rc;
    uint32_t act_keys[2 * COVO_MAX_ENVS], step_keys[2 * COVO_MAX_ENVS], next[2 * COVO_MAX_ENVS];
    for (int t = 0; t < n_steps; ++t) {
        // per instance, run_one_step (quadrotor.py:520-538): rng, rng_act, rng_step, rng_control = split(rng, 4); ...; rng, _ = split(rng)
        for (int e = 0; e < E; ++e) {
            const uint32_t key[2] = {rngs[2 * e], rngs[2 * e + 1]};
            uint32_t nrng[2];
            host_philox_split(key, 0u, nrng);
            host_philox_split(key, 1u, &act_keys[2 * e]);
            host_philox_split(key, 2u, &step_keys[2 * e]);
            host_philox_split(nrng, 0u, &next[2 * e]);
        }
        // (the posterior covariance's rows are formed in the frame)
        auto rows = [&] { return launch_episode_rows(h, E, log_index + t, h->sigma_last_age, s); };
        if ((rc = batched_scheduled_step(h, args, &norm, params, act_keys, states_true, log_index + t, s, rows))) return rc;
        if ((rc = launch_env_step_batched(states_true, const_cast<float *>(args->states), args->pos_traj, args->vel_traj, acc_traj,
                                          args->T, params[0], inst, E, args->a_mean, step_keys, noisy_on, obs_noise_scale, log,
                                          log_stride, log_index + t, s)))
            return rc;
        if ((rc = covo_estimator_step(h, const_cast<float *>(args->states), args->a_mean, params, E, true, log_index + t, s))) return rc;
        if ((rc = covo_force_observer_step(h, const_cast<float *>(args->states), args->a_mean, params, E, true, log_index + t, s))) return rc;
        std::memcpy(rngs, next, (size_t)2 * E * sizeof(uint32_t));
    }
    return 0;
}

int covo_run_episode_batched(covo_handle_t h, const covo_batch_args *args, const covo_env_params *params, float *states_true,
                             const float *acc_traj, int32_t noisy_on, float obs_noise_scale, float *log, int32_t log_stride,
                             int32_t log_index, uint32_t *rngs, int32_t n_steps, void *stream)
{
    return run_episode_batched(h, args, nullptr, params, states_true, acc_traj, noisy_on, obs_noise_scale, log, log_stride, log_index,
                               rngs, n_steps, stream, "covo_run_episode_batched");
}

int covo_run_episode_batched_mode(covo_handle_t h, const covo_batch_mode_args *args, const covo_env_params *params, float *states_true,
                                  const float *acc_traj, int32_t noisy_on, float obs_noise_scale, float *log, int32_t log_stride,
                                  int32_t log_index, uint32_t *rngs, int32_t n_steps, void *stream)
{
    return run_episode_batched(h, args ? &args->base : nullptr, args, params, states_true, acc_traj, noisy_on, obs_noise_scale, log,
                               log_stride, log_index, rngs, n_steps, stream, "covo_run_episode_batched_mode");
}

int covo_debug_time_batched(covo_handle_t h, int32_t step_mask, int32_t reps, float *us_out, void *stream)
{
    REQUIRE(h && us_out && reps > 0, "covo_debug_time_batched: bad argument");
    CHECK_DEVICE(h, "covo_debug_time_batched");
    REQUIRE(covo_step_iters(h) == 1, "covo_debug_time_batched: the phase timers replay ONE pass; iterations per step are on "
            "(covo_set_step_iters, iters=%d): set iters = 1", covo_step_iters(h));
    return covo_debug_time_batched_impl(h, step_mask, reps, us_out, (hipStream_t)stream);
}

int covo_mpc_step_batched(covo_handle_t h, const covo_batch_args *args, const covo_env_params *params, const uint32_t *keys,
                          void *stream)
{
    REQUIRE(h, "covo_mpc_step_batched: null handle");
    CHECK_DEVICE(h, "covo_mpc_step_batched");
    REQUIRE(args && params && keys, "covo_mpc_step_batched: null argument");
    covo_batch_mode_args norm;
    const int rc = check_batch_step(h, args, nullptr, params, false, "covo_mpc_step_batched", &norm);
    if (rc) return rc;
    return batched_scheduled_step(h, args, &norm, params, keys, nullptr, -1, (hipStream_t)stream, step_no_extra);
}

int covo_mpc_step_batched_mode(covo_handle_t h, const covo_batch_mode_args *args, const covo_env_params *params, const uint32_t *keys,
                               void *stream)
{
    REQUIRE(h, "covo_mpc_step_batched_mode: null handle");
    CHECK_DEVICE(h, "covo_mpc_step_batched_mode");
    REQUIRE(args && params && keys, "covo_mpc_step_batched_mode: null argument");
    covo_batch_mode_args norm;
    const int rc = check_batch_step(h, &args->base, args, params, false, "covo_mpc_step_batched_mode", &norm);
    if (rc) return rc;
    return batched_scheduled_step(h, &args->base, &norm, params, keys, nullptr, -1, (hipStream_t)stream, step_no_extra);
}

int covo_debug_time_step(covo_handle_t h, const covo_env_params *params, const covo_step_args *args, int32_t step_mask,
                         int32_t hess_mask, int32_t sigma_stages, int32_t reps, float *us_out, void *stream)
{
    REQUIRE(h && params && args && us_out && reps > 0, "covo_debug_time_step: bad argument");
    REQUIRE(args->mode != COVO_MODE_ILQR, "covo_debug_time_step: the phase masks name the launches of a sampling step; an iLQR step "
            "(COVO_MODE_ILQR) has none of them");
    REQUIRE(args->mode != COVO_MODE_CMA, "covo_debug_time_step: the phase timers replay a step without its state; a CMA step "
            "(COVO_MODE_CMA) would adapt its covariance once per copy");
    REQUIRE(covo_step_iters(h) == 1, "covo_debug_time_step: the phase timers replay ONE pass; iterations per step are on "
            "(covo_set_step_iters, iters=%d): set iters = 1", covo_step_iters(h));
    return covo_debug_time_step_impl(h, params, args, step_mask, hess_mask, sigma_stages, reps, us_out, (hipStream_t)stream);  // (a refresh step's launches)
}

int covo_debug_hess_workspace(covo_handle_t h, double *out, int64_t offset_doubles, int64_t count, void *stream)
{
    REQUIRE(h && out, "covo_debug_hess_workspace: bad argument");
    REQUIRE((size_t)(offset_doubles + count) * sizeof(double) <= h->ws_hess_bytes, "covo_debug_hess_workspace: range");
    COVO_CHECK_HIP(hipMemcpyAsync(out, (const double *)h->ws_hess + offset_doubles, (size_t)count * sizeof(double),
                                  hipMemcpyDeviceToHost, (hipStream_t)stream));
    return 0;
}

int covo_debug_batched_hessians(covo_handle_t h, double *out, int64_t offset_doubles, int64_t count, void *stream)
{
    REQUIRE(h && out && offset_doubles >= 0 && count > 0, "covo_debug_batched_hessians: bad argument");
    return covo_debug_batched_hessians_impl(h, out, offset_doubles, count, (hipStream_t)stream);
}

int covo_debug_sigma_factor(covo_handle_t h, int32_t batched, float *out, int64_t count, void *stream)
{
    REQUIRE(h && out && count > 0, "covo_debug_sigma_factor: bad argument");
    return covo_debug_sigma_factor_impl(h, batched, out, count, (hipStream_t)stream);
}

int covo_sigma_jacobi(covo_handle_t h, const double *R, int32_t batch, float sample_sigma, float *Sigma_out, float *L_out,
                      void *stream)
{
    REQUIRE(h, "covo_sigma_jacobi: null handle");
    REQUIRE(R && L_out && batch > 0 && sample_sigma > 0.0f, "covo_sigma_jacobi: bad argument");
    return launch_sigma(R, batch, sample_sigma, Sigma_out, L_out, nullptr, (hipStream_t)stream);
}

int covo_sigma_profile(covo_handle_t h, const double *R, float sample_sigma, float *Sigma_out, float *L_out,
                       uint64_t *ticks_out, void *stream)
{
    REQUIRE(h, "covo_sigma_profile: null handle");
    REQUIRE(R && L_out && ticks_out, "covo_sigma_profile: bad argument");
    return launch_sigma(R, 1, sample_sigma, Sigma_out, L_out, (unsigned long long *)ticks_out, (hipStream_t)stream);
}

int covo_mpc_step(covo_handle_t h, const covo_env_params *params, const covo_step_args *args, uint32_t key0, uint32_t key1,
                  const float *f_disturb_shared, void *stream)
{
    REQUIRE(h, "covo_mpc_step: null handle");
    CHECK_DEVICE(h, "covo_mpc_step");
    REQUIRE(params && args, "covo_mpc_step: null argument");
    const int rc = check_single_step(h, params, args, "covo_mpc_step");
    if (rc) return rc;
    return single_scheduled_step(h, params, args, key0, key1, f_disturb_shared, nullptr, -1, (hipStream_t)stream, step_no_extra, step_no_extra);
}

int covo_cholesky(covo_handle_t h, const float *A, int32_t n, int32_t batch, float *L_out, void *stream)
{
    REQUIRE(h, "covo_cholesky: null handle");
    REQUIRE(A && L_out && batch > 0, "covo_cholesky: bad argument");
    return launch_cholesky(A, n, batch, L_out, (hipStream_t)stream);
}

}  // extern "C"
