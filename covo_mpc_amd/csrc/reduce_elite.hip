// reduce_elite.hip -- the elite-set update (covo_set_step_elite): the softmax update of reduce.hip with weights
// w_n = 1 for the K samples of smallest key and 0 otherwise.  Stage 1 is softmax_partial_body (softmax_stage1.hpp) with the weight
// read off the selector's threshold (elite_select.hip: row blockIdx.y) instead of an exponential; every record carries the
// selector's cost_min as its m, so the unchanged merges of reduce.hip (launch_merge, launch_merge_cov, launch_merge_cov_diag at
// 1 / lambda = 1) rescale every record by expf(0) = 1, divide by s = K and log the pass's minimum cost.  A translation unit of its
// own: the kernels of reduce.hip and reduce_lam.hip are compiled exactly as without it.
#include "covo_common.hpp"
#include "elite_key.hpp"
#include "softmax_stage1.hpp"

// The 0/1 weights (the policy of softmax_partial_body): w_n = key(n) <= threshold, the threshold's two words and m = cost_min from
// the selector's row of instance blockIdx.y; nothing to fold, no LDS.  The record's s is then the workgroup's elites, its diagnostic
// record {sum w^2 = s, sum over the elites of c - m, sum over all samples of c - m, samples}.
struct EliteWeights {
    const float *__restrict__ elite_rows;  // [instances][COVO_ELITE_FLOATS]
    uint32_t thr_u, thr_i;
    static constexpr int RED_FLOATS = 0;
    __device__ __forceinline__ float begin(float *)
    {
        const float *row = elite_rows + (size_t)blockIdx.y * COVO_ELITE_FLOATS;
        thr_u = __float_as_uint(row[ELITE_ROW_COST_WORD]);
        thr_i = __float_as_uint(row[ELITE_ROW_INDEX_WORD]);
        return row[ELITE_ROW_COST_MIN];
    }
    __device__ __forceinline__ float weight(float c, float, int n, int N) const
    {
        const uint32_t u = elite_cost_word(c);
        return (n < N && (u < thr_u || (u == thr_u && (uint32_t)n <= thr_i))) ? 1.0f : 0.0f;
    }
    __device__ __forceinline__ float diag_w2(float w) const { return w; }
    // a select, not a product: an infinite cost outside the set must not make the sum NaN
    __device__ __forceinline__ float diag_wdc(float w, float dc) const { return w > 0.0f ? dc : 0.0f; }
};

template <bool COV, bool DIAG>
__global__ __launch_bounds__(RD_BLOCK) void elite_partial_kernel(const float *__restrict__ cost, const float4 *__restrict__ a, int N,
                                                                 const float *__restrict__ elite_rows, float *__restrict__ partials,
                                                                 const float4 *__restrict__ mu, float *__restrict__ dpart)
{
    softmax_partial_body<COV, DIAG>(cost, a, N, EliteWeights{elite_rows}, partials, mu, dpart);
}

// the elite-set variant of launch_softmax_reduce: d.elite_rows [batch][COVO_ELITE_FLOATS] in device memory, a final update only
int launch_elite_reduce(covo_ctx *h, const UpdateDesc &d, hipStream_t s)
{
    if (d.a_mean_out == nullptr || d.elite_rows == nullptr) {
        covo_set_error("launch_elite_reduce: the elite-set update needs a final update and the selector's rows");
        return COVO_E_BADARG;
    }
    float *partials_ws = d.partials_ws ? d.partials_ws : h->ws_partials;
    const int grid = stage1_grid(h, d.N);
    const float4 *a4 = reinterpret_cast<const float4 *>(d.a);
    if (d.diag_out != nullptr)
        hipLaunchKernelGGL((elite_partial_kernel<false, true>), dim3(grid, d.batch), dim3(RD_BLOCK), 0, s, d.cost, a4, d.N, d.elite_rows,
                           partials_ws, (const float4 *)nullptr, d.diag_rec);
    else
        hipLaunchKernelGGL((elite_partial_kernel<false, false>), dim3(grid, d.batch), dim3(RD_BLOCK), 0, s, d.cost, a4, d.N, d.elite_rows,
                           partials_ws, (const float4 *)nullptr, (float *)nullptr);
    COVO_CHECK_HIP(hipGetLastError());
    UpdateDesc mg = d;  // the unchanged merge over the records just written: every scale is expf((m - m) * 1) = 1
    mg.partials = partials_ws;
    mg.G = grid;
    mg.stride = COVO_PARTIAL_FLOATS;
    return launch_merge(mg, 1.0f, s);
}

// the elite-set variant of launch_softmax_update_cov: row 0 of d.elite_rows, a final update only (CEM's refit, smoothed by gamma_sigma)
int launch_elite_update_cov(covo_ctx *h, const UpdateDesc &d, hipStream_t s)
{
    if (d.a_cov_out == nullptr || d.elite_rows == nullptr) {
        covo_set_error("launch_elite_update_cov: the elite-set update needs a final update and the selector's rows");
        return COVO_E_BADARG;
    }
    const int grid = stage1_grid(h, d.N);
    const float4 *a4 = reinterpret_cast<const float4 *>(d.a), *mean4 = reinterpret_cast<const float4 *>(d.a_mean_old);
    if (d.diag_out != nullptr) {
        hipLaunchKernelGGL((elite_partial_kernel<true, true>), dim3(grid, 1), dim3(RD_BLOCK), 0, s, d.cost, a4, d.N, d.elite_rows,
                           h->ws_partials_cov, mean4, h->ws_diag_rec);
        launch_merge_cov_diag(h, grid, 1.0f, d.diag_out, d.N, s);
    } else {
        hipLaunchKernelGGL((elite_partial_kernel<true, false>), dim3(grid, 1), dim3(RD_BLOCK), 0, s, d.cost, a4, d.N, d.elite_rows,
                           h->ws_partials_cov, mean4, (float *)nullptr);
    }
    COVO_CHECK_HIP(hipGetLastError());
    UpdateDesc mg = d;
    mg.partials = h->ws_partials_cov;
    mg.G = grid;
    mg.stride = RD_COV_RECORD_FLOATS;
    return launch_merge_cov(mg, 1.0f, s);
}
