// reduce.hip -- exp(-cost/lambda)-weighted aggregation as a two-stage wavefront reduction (gfx950).
//
// Replaces quadjax/controllers/covo.py:266-278 (mppi.py:109-129):
//     w = exp(-(cost - min cost)/lam) / sum ;  a_mean' = gamma * sum_n w_n a_n + (1-gamma) a_mean
//
// Stage 1 (softmax_partial_kernel): every workgroup first reduces the per-wave (64-sample) cost minima left
//   by the rollout kernel (4 KiB at N = 65536, L2-resident) to the exact global minimum m, so weights are
//   formed exactly like the reference's `cost - jnp.min(cost)`.  A wave then walks 64-sample
//   groups: one coalesced cost load, w = exp((m-c)/lam); 8-sample sub-groups whose weights are
//   all exactly 0 (the overwhelming majority at lam = 0.01: exp underflows once c-m > 1.04) are
//   skipped -- their contribution is an exact zero.  For a live sub-group the wave reads the
//   stripes a[t][8 samples][4] as full 128-B lines (lane = (t mod 8, sample)), 4 loads cover all
//   32 steps, accumulating float4 partial sums; 3 xor-shuffle steps fold the 8 sample lanes.
//   Cross-wave fold through LDS; one {m, s, v[128]} record per workgroup (no atomics ->
//   bit-reproducible).
// Stage 2 (merge_kernel): one workgroup merges records with the online-softmax rule
//   (m = min m_g, scale_g = exp(-(m_g - m)/lam)); the same kernel merges the all-gathered
//   records of the G ranks of a sample-sharded step and applies the gamma blend.
// HBM roofline: 516 B/sample algorithmic (cost + stripes); far less is actually fetched when
// sub-groups are skipped.
#include <cstdlib>
#include <cstring>
#include "covo_common.hpp"
#include "softmax_merge.hpp"
#include "softmax_stage1.hpp"

__global__ __launch_bounds__(256) void groupmin_kernel(const float *__restrict__ cost, int N, float *__restrict__ gm)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    const float wm = wave_min(n < N ? cost[n] : __builtin_inff());
    if ((threadIdx.x & 63) == 0 && (n >> 6) < (N + 63) / 64) gm[n >> 6] = wm;
}


template <bool COV>
__global__ __launch_bounds__(RD_BLOCK) void softmax_partial_kernel(const float *__restrict__ cost,
                                                                   const float4 *__restrict__ a, int N,
                                                                   const float *__restrict__ blockmin, int nbm,
                                                                   float inv_lam, float *__restrict__ partials,
                                                                   const float4 *__restrict__ mu)
{
    softmax_partial_body<COV, false>(cost, a, N, SoftmaxWeights{blockmin, nbm, inv_lam}, partials, mu, nullptr);
}
template <bool COV>
__global__ __launch_bounds__(RD_BLOCK) void softmax_partial_diag_kernel(const float *__restrict__ cost,
                                                                        const float4 *__restrict__ a, int N,
                                                                        const float *__restrict__ blockmin, int nbm,
                                                                        float inv_lam, float *__restrict__ partials,
                                                                        const float4 *__restrict__ mu, float *__restrict__ dpart)
{
    softmax_partial_body<COV, true>(cost, a, N, SoftmaxWeights{blockmin, nbm, inv_lam}, partials, mu, dpart);
}


template <bool FINAL, bool INST = false>
__global__ __launch_bounds__(MG_THREADS) void merge_cov_kernel(const float *__restrict__ partials, int G, float inv_lam,
                                                               const float *__restrict__ a_mean_old, float gamma_mean,
                                                               const float *__restrict__ a_cov_old, float gamma_sigma,
                                                               float *__restrict__ a_mean_out, float *__restrict__ a_cov_out,
                                                               int stride, float *__restrict__ iter_out, int iter_stride)
{
    // INST (FINAL; the staged env-batched MPPI step): workgroup x = instance x merges its own G records into its own mean and adapts
    // its own covariance blocks in place; its cost minimum to iter_out[x * iter_stride]
    if (INST) {
        const size_t x = blockIdx.x;
        partials += x * G * stride;
        a_mean_old += x * COVO_NA;
        a_cov_old += x * (COVO_H * 16);
        a_mean_out += x * COVO_NA;
        a_cov_out += x * (COVO_H * 16);
        if (iter_out != nullptr) iter_out += x * (size_t)iter_stride;
    }
    merge_cov_body<FINAL>(partials, G, inv_lam, a_mean_old, gamma_mean, a_cov_old, gamma_sigma, a_mean_out, a_cov_out, stride, iter_out);
}

// Merges G records {m, s, v[128]} with 1024 threads = 8 record-slices x 128 columns (softmax_merge.hpp: the body is shared
// with the launches that finish their own update); blockIdx.x (env-batched step): instance x merges its own G records into its own mean.
// FINAL: a_mean_out = gamma * v/s + (1-gamma) * a_mean_old (covo.py:270-275); otherwise writes the
// merged record to out.  Fixed summation order -> bit-reproducible.
// stride: floats between consecutive records (COVO_PARTIAL_FLOATS, or COVO_RANK_RECORD_FLOATS for the all-gathered rank records
// that also carry the position sums)
template <bool FINAL>
__global__ __launch_bounds__(MG_THREADS) void merge_kernel(const float *__restrict__ partials, int G, float inv_lam,
                                                           const float *__restrict__ a_mean_old, float gamma_mean,
                                                           float *__restrict__ out, int stride, float *__restrict__ iter_out,
                                                           int iter_stride)
{
    // -DMERGE_STAMPS (a measuring build; the product kernel stores nothing extra): 10 ns wall-clock ticks from entry to "records
    // in hand" -- this thread's share of the records (the v rows and headers merge_body asks for first) pulled once ahead of the
    // merge, which then finds them in the caches: the first-touch round trip on its own -- and to "done"
#ifdef MERGE_STAMPS
    const long long mt0 = wall_clock64();
    float touch = 0.0f;
    {
        const float *p = partials + (size_t)blockIdx.x * G * stride;
        const int col = threadIdx.x & (COVO_NA - 1), slice = threadIdx.x >> 7;
        for (int g = slice; g < G; g += MG_SLICES) touch += p[(size_t)g * stride + 2 + col];
        if ((int)threadIdx.x < G) touch += p[(size_t)threadIdx.x * stride] + p[(size_t)threadIdx.x * stride + 1];
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(touch)::"memory");
    const long long mt1 = wall_clock64();
#endif
    merge_instance<FINAL, false>(partials, G, inv_lam, a_mean_old, gamma_mean, out, stride, nullptr, nullptr, 0.0f, iter_out, iter_stride);
#ifdef MERGE_STAMPS
    if (threadIdx.x == 0 && blockIdx.x == 0)
        printf("merge G %d: records-in-hand %lld done %lld (10 ns ticks from entry)\n", G, mt1 - mt0, (long long)wall_clock64() - mt0);
#endif
}

// the same, and the diagnostic records dpart [instances][G][MG_DIAG_REC] merged into row x of diag_out [instances][COVO_DIAG_FLOATS]
template <bool FINAL>
__global__ __launch_bounds__(MG_THREADS) void merge_diag_kernel(const float *__restrict__ partials, int G, float inv_lam,
                                                                const float *__restrict__ a_mean_old, float gamma_mean,
                                                                float *__restrict__ out, int stride, const float *__restrict__ dpart,
                                                                float *__restrict__ diag_out, float n_samples, float *__restrict__ iter_out,
                                                                int iter_stride)
{
    merge_instance<FINAL, true>(partials, G, inv_lam, a_mean_old, gamma_mean, out, stride, dpart, diag_out, n_samples, iter_out, iter_stride);
}

__global__ void shift_mean_kernel(const float *__restrict__ in, float *__restrict__ out)
{
    const int i = threadIdx.x;  // 128 threads; covo.py:201-203
    out[i] = (i < COVO_NA - COVO_DU) ? in[i + COVO_DU] : in[i];
}

// stage 1's cost minima, for the two entry points below: d's own per-wave minima, or formed over the costs first (only this file
// forms them itself: reduce_lam.hip refuses a step without them, reduce_elite.hip does not read them)
struct Minima {
    const float *blockmin;
    int n_blockmin;
};
static Minima stage1_minima(covo_ctx *h, const UpdateDesc &d, hipStream_t s)
{
    if (d.blockmin != nullptr) return {d.blockmin, d.n_blockmin};
    hipLaunchKernelGGL(groupmin_kernel, dim3((d.N + 255) / 256), dim3(256), 0, s, d.cost, d.N, h->ws_blockmin);
    return {h->ws_blockmin, (d.N + 63) / 64};
}

int launch_softmax_reduce(covo_ctx *h, const UpdateDesc &d, hipStream_t s)
{
    if (d.lam_rows != nullptr) return launch_softmax_reduce_lam(h, d, s);  // (reduce_lam.hip)
    const float inv_lam = 1.0f / h->cfg.lam;
    float *partials_ws = d.partials_ws ? d.partials_ws : h->ws_partials;
    const Minima mn = stage1_minima(h, d, s);
    const int grid = stage1_grid(h, d.N);
    const float4 *a4 = reinterpret_cast<const float4 *>(d.a);
    if (d.diag_out != nullptr && d.a_mean_out != nullptr) {  // the same two launches in their diagnostic variants
        hipLaunchKernelGGL(softmax_partial_diag_kernel<false>, dim3(grid, d.batch), dim3(RD_BLOCK), 0, s, d.cost, a4, d.N, mn.blockmin,
                           mn.n_blockmin, inv_lam, partials_ws, (const float4 *)nullptr, d.diag_rec);
        hipLaunchKernelGGL(merge_diag_kernel<true>, dim3(d.batch), dim3(MG_THREADS), 0, s, partials_ws, grid, inv_lam, d.a_mean_old,
                           d.gamma_mean, d.a_mean_out, COVO_PARTIAL_FLOATS, (const float *)d.diag_rec, d.diag_out, (float)d.N, d.iter_out, d.iter_stride);
        COVO_CHECK_HIP(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(softmax_partial_kernel<false>, dim3(grid, d.batch), dim3(RD_BLOCK), 0, s, d.cost, a4, d.N, mn.blockmin,
                       mn.n_blockmin, inv_lam, partials_ws, (const float4 *)nullptr);
    if (d.a_mean_out != nullptr)
        hipLaunchKernelGGL(merge_kernel<true>, dim3(d.batch), dim3(MG_THREADS), 0, s, partials_ws, grid, inv_lam, d.a_mean_old,
                           d.gamma_mean, d.a_mean_out, COVO_PARTIAL_FLOATS, d.iter_out, d.iter_stride);
    else
        hipLaunchKernelGGL(merge_kernel<false>, dim3(d.batch), dim3(MG_THREADS), 0, s, partials_ws, grid, inv_lam,
                           (const float *)nullptr, 1.0f, d.partial_out, COVO_PARTIAL_FLOATS, (float *)nullptr, 0);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

// MPPI's update with covariance adaptation (mppi.py:109-125): stage 1 with second moments, then merge_cov_kernel.  Single shard: one
// instance on the handle's own ws_partials_cov / ws_diag_rec (d.batch, d.partials_ws and d.diag_rec are not read); with
// d.partials_cov_ws (the staged env-batched MPPI step, final updates only): d.batch instances, instance y's records [grid][452] behind
// those of instance y - 1, every instance's sums in the single launch's order
size_t softmax_cov_workspace_floats(int max_blocks) { return (size_t)max_blocks * RD_COV_RECORD_FLOATS; }
int softmax_stage1_blocks(const covo_ctx *h, int N) { return stage1_grid(h, N); }
int launch_softmax_update_cov(covo_ctx *h, const UpdateDesc &d, hipStream_t s)
{
    if (d.lam_rows != nullptr) return launch_softmax_update_cov_lam(h, d, s);  // (reduce_lam.hip)
    const float inv_lam = 1.0f / h->cfg.lam;
    const bool diag = d.diag_out != nullptr && d.a_cov_out != nullptr;
    const Minima mn = stage1_minima(h, d, s);
    const int grid = stage1_grid(h, d.N);
    const float4 *a4 = reinterpret_cast<const float4 *>(d.a), *mean4 = reinterpret_cast<const float4 *>(d.a_mean_old);
    const bool inst = d.partials_cov_ws != nullptr;
    const int batch = inst ? d.batch : 1;
    float *recs = inst ? d.partials_cov_ws : h->ws_partials_cov, *drec = inst ? d.diag_rec : h->ws_diag_rec;
    if (diag)
        hipLaunchKernelGGL(softmax_partial_diag_kernel<true>, dim3(grid, batch), dim3(RD_BLOCK), 0, s, d.cost, a4, d.N, mn.blockmin,
                           mn.n_blockmin, inv_lam, recs, mean4, drec);
    else
        hipLaunchKernelGGL(softmax_partial_kernel<true>, dim3(grid, batch), dim3(RD_BLOCK), 0, s, d.cost, a4, d.N, mn.blockmin,
                           mn.n_blockmin, inv_lam, recs, mean4);
    if (diag && inst)  // launch_merge_cov_diag's launch with an instance per workgroup
        hipLaunchKernelGGL(merge_diag_kernel<false>, dim3(batch), dim3(MG_THREADS), 0, s, recs, grid, inv_lam, (const float *)nullptr, 1.0f,
                           d.diag_merge_ws, RD_COV_RECORD_FLOATS, (const float *)drec, d.diag_out, (float)d.N, (float *)nullptr, 0);
    else if (diag)
        launch_merge_cov_diag(h, grid, inv_lam, d.diag_out, d.N, s);
    if (d.a_cov_out != nullptr && inst)
        hipLaunchKernelGGL((merge_cov_kernel<true, true>), dim3(batch), dim3(MG_THREADS), 0, s, recs, grid, inv_lam, d.a_mean_old,
                           d.gamma_mean, d.a_cov_old, d.gamma_sigma, d.a_mean_out, d.a_cov_out, RD_COV_RECORD_FLOATS, d.iter_out,
                           d.iter_stride);
    else if (d.a_cov_out != nullptr)
        hipLaunchKernelGGL(merge_cov_kernel<true>, dim3(1), dim3(MG_THREADS), 0, s, recs, grid, inv_lam, d.a_mean_old,
                           d.gamma_mean, d.a_cov_old, d.gamma_sigma, d.a_mean_out, d.a_cov_out, RD_COV_RECORD_FLOATS, d.iter_out, 0);
    else  // a sample-sharded rank: its record {m, s, v, pad, S2}, unnormalised and unblended
        hipLaunchKernelGGL(merge_cov_kernel<false>, dim3(1), dim3(MG_THREADS), 0, s, h->ws_partials_cov, grid, inv_lam, d.a_mean_old,
                           1.0f, (const float *)nullptr, 0.0f, d.partial_out, (float *)nullptr, RD_COV_RECORD_FLOATS, (float *)nullptr, 0);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

// The covariance merge has its own body: the diagnostics of MPPI's covariance update come from one more merge launch over the headers
// {m_g, s_g} of the G 452-float records in ws_partials_cov and their diagnostic records in ws_diag_rec (its merged record goes to the
// idle ws_partials), off the path of a step without diagnostics.  Also the elite-set update's, at 1 / lambda = 1 (reduce_elite.hip).
void launch_merge_cov_diag(covo_ctx *h, int G, float inv_lam, float *diag_out, int N, hipStream_t s)
{
    hipLaunchKernelGGL(merge_diag_kernel<false>, dim3(1), dim3(MG_THREADS), 0, s, h->ws_partials_cov, G, inv_lam, (const float *)nullptr,
                       1.0f, h->ws_partials, RD_COV_RECORD_FLOATS, (const float *)h->ws_diag_rec, diag_out, (float)N, (float *)nullptr, 0);
}

// the G all-gathered rank records (stride floats apart) -> new mean and adapted covariances, identically on every rank
int launch_merge_cov(const UpdateDesc &d, float lam, hipStream_t s)
{
    if (d.G > MG_MAXG) { covo_set_error("covo_merge_ranks_cov: G=%d > %d", d.G, MG_MAXG); return COVO_E_BADARG; }
    hipLaunchKernelGGL(merge_cov_kernel<true>, dim3(1), dim3(MG_THREADS), 0, s, d.partials, d.G, 1.0f / lam, d.a_mean_old, d.gamma_mean,
                       d.a_cov_old, d.gamma_sigma, d.a_mean_out, d.a_cov_out, d.stride, d.iter_out, 0);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_merge(const UpdateDesc &d, float lam, hipStream_t s)
{
    if (d.G > MG_MAXG) { covo_set_error("covo_merge: G=%d > %d", d.G, MG_MAXG); return COVO_E_BADARG; }
    if (d.a_mean_out != nullptr && d.diag_out != nullptr)
        hipLaunchKernelGGL(merge_diag_kernel<true>, dim3(d.batch), dim3(MG_THREADS), 0, s, d.partials, d.G, 1.0f / lam, d.a_mean_old,
                           d.gamma_mean, d.a_mean_out, d.stride, (const float *)d.diag_rec, d.diag_out, (float)d.N, d.iter_out, d.iter_stride);
    else if (d.a_mean_out != nullptr)
        hipLaunchKernelGGL(merge_kernel<true>, dim3(d.batch), dim3(MG_THREADS), 0, s, d.partials, d.G, 1.0f / lam, d.a_mean_old,
                           d.gamma_mean, d.a_mean_out, d.stride, d.iter_out, d.iter_stride);
    else
        hipLaunchKernelGGL(merge_kernel<false>, dim3(d.batch), dim3(MG_THREADS), 0, s, d.partials, d.G, 1.0f / lam,
                           (const float *)nullptr, 1.0f, d.partial_out, d.stride, (float *)nullptr, 0);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_shift_mean(const float *in, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(shift_mean_kernel, dim3(1), dim3(COVO_NA), 0, s, in, out);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
