// reduce_lam.hip -- the softmax update of reduce.hip with the temperature in DEVICE memory (the ESS floor, covo_set_step_ess_floor):
// thin __global__ wrappers that load 1 / lambda from the solver's row of their instance (ess_lambda.hip: float[instances]
// [COVO_LAM_FLOATS], [1] = 1 / lam_eff) and pass it by value to the unchanged bodies (softmax_stage1.hpp, softmax_merge.hpp).  A
// translation unit of its own: the kernels of reduce.hip are compiled exactly as without it.
#include "covo_common.hpp"
#include "softmax_merge.hpp"
#include "softmax_stage1.hpp"

// The ESS floor (covo_set_step_ess_floor): the same stage 1 with 1 / lambda read from row blockIdx.y of the solver's output
// (ess_lambda.hip: float[instances][COVO_LAM_FLOATS], [1] = 1 / lam_eff) instead of a kernel argument
template <bool COV, bool DIAG>
__global__ __launch_bounds__(RD_BLOCK) void softmax_partial_lam_kernel(const float *__restrict__ cost, const float4 *__restrict__ a,
                                                                       int N, const float *__restrict__ blockmin, int nbm,
                                                                       const float *__restrict__ lam_rows, float *__restrict__ partials,
                                                                       const float4 *__restrict__ mu, float *__restrict__ dpart)
{
    const float inv_lam = lam_rows[(size_t)blockIdx.y * COVO_LAM_FLOATS + 1];
    softmax_partial_body<COV, DIAG>(cost, a, N, SoftmaxWeights{blockmin, nbm, inv_lam}, partials, mu, dpart);
}

// The ESS floor: the two merges above with 1 / lambda read from row blockIdx.x of the solver's output
template <bool FINAL>
__global__ __launch_bounds__(MG_THREADS) void merge_lam_kernel(const float *__restrict__ partials, int G,
                                                               const float *__restrict__ lam_rows,
                                                               const float *__restrict__ a_mean_old, float gamma_mean,
                                                               float *__restrict__ out, int stride, float *__restrict__ iter_out,
                                                               int iter_stride)
{
    const float inv_lam = lam_rows[(size_t)blockIdx.x * COVO_LAM_FLOATS + 1];
    merge_instance<FINAL, false>(partials, G, inv_lam, a_mean_old, gamma_mean, out, stride, nullptr, nullptr, 0.0f, iter_out, iter_stride);
}
template <bool FINAL>
__global__ __launch_bounds__(MG_THREADS) void merge_diag_lam_kernel(const float *__restrict__ partials, int G,
                                                                    const float *__restrict__ lam_rows,
                                                                    const float *__restrict__ a_mean_old, float gamma_mean,
                                                                    float *__restrict__ out, int stride,
                                                                    const float *__restrict__ dpart, float *__restrict__ diag_out,
                                                                    float n_samples, float *__restrict__ iter_out, int iter_stride)
{
    const float inv_lam = lam_rows[(size_t)blockIdx.x * COVO_LAM_FLOATS + 1];
    merge_instance<FINAL, true>(partials, G, inv_lam, a_mean_old, gamma_mean, out, stride, dpart, diag_out, n_samples, iter_out, iter_stride);
}

// the ESS floor: 1 / lambda from row 0 of the solver's output (the covariance update is a single-instance launch)
__global__ __launch_bounds__(MG_THREADS) void merge_cov_lam_kernel(const float *__restrict__ partials, int G,
                                                                   const float *__restrict__ lam_rows,
                                                                   const float *__restrict__ a_mean_old, float gamma_mean,
                                                                   const float *__restrict__ a_cov_old, float gamma_sigma,
                                                                   float *__restrict__ a_mean_out, float *__restrict__ a_cov_out,
                                                                   int stride, float *__restrict__ iter_out)
{
    merge_cov_body<true>(partials, G, lam_rows[1], a_mean_old, gamma_mean, a_cov_old, gamma_sigma, a_mean_out, a_cov_out, stride, iter_out);
}


// the ESS floor's variant of launch_softmax_reduce: d.lam_rows [batch][COVO_LAM_FLOATS] in device memory, a final update only
int launch_softmax_reduce_lam(covo_ctx *h, const UpdateDesc &d, hipStream_t s)
{
    if (d.a_mean_out == nullptr || d.blockmin == nullptr) {
        covo_set_error("launch_softmax_reduce: a device temperature needs a final update and the per-wave cost minima");
        return COVO_E_BADARG;
    }
    float *partials_ws = d.partials_ws ? d.partials_ws : h->ws_partials;
    const int grid = stage1_grid(h, d.N);  // (the caller's per-wave minima: a step with a floor always has them)
    const float4 *a4 = reinterpret_cast<const float4 *>(d.a);
    if (d.diag_out != nullptr) {
        hipLaunchKernelGGL((softmax_partial_lam_kernel<false, true>), dim3(grid, d.batch), dim3(RD_BLOCK), 0, s, d.cost, a4, d.N,
                           d.blockmin, d.n_blockmin, d.lam_rows, partials_ws, (const float4 *)nullptr, d.diag_rec);
        hipLaunchKernelGGL(merge_diag_lam_kernel<true>, dim3(d.batch), dim3(MG_THREADS), 0, s, partials_ws, grid, d.lam_rows,
                           d.a_mean_old, d.gamma_mean, d.a_mean_out, COVO_PARTIAL_FLOATS, (const float *)d.diag_rec, d.diag_out,
                           (float)d.N, d.iter_out, d.iter_stride);
    } else {
        hipLaunchKernelGGL((softmax_partial_lam_kernel<false, false>), dim3(grid, d.batch), dim3(RD_BLOCK), 0, s, d.cost, a4, d.N,
                           d.blockmin, d.n_blockmin, d.lam_rows, partials_ws, (const float4 *)nullptr, (float *)nullptr);
        hipLaunchKernelGGL(merge_lam_kernel<true>, dim3(d.batch), dim3(MG_THREADS), 0, s, partials_ws, grid, d.lam_rows,
                           d.a_mean_old, d.gamma_mean, d.a_mean_out, COVO_PARTIAL_FLOATS, d.iter_out, d.iter_stride);
    }
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

// the ESS floor's variant of launch_softmax_update_cov: row 0 of d.lam_rows, a final update only
int launch_softmax_update_cov_lam(covo_ctx *h, const UpdateDesc &d, hipStream_t s)
{
    if (d.a_cov_out == nullptr || d.blockmin == nullptr) {
        covo_set_error("launch_softmax_update_cov: a device temperature needs a final update and the per-wave cost minima");
        return COVO_E_BADARG;
    }
    const int grid = stage1_grid(h, d.N);  // (the caller's per-wave minima: a step with a floor always has them)
    const float4 *a4 = reinterpret_cast<const float4 *>(d.a), *mean4 = reinterpret_cast<const float4 *>(d.a_mean_old);
    if (d.diag_out != nullptr) {  // (the diagnostics' own merge over the same headers, as in launch_softmax_update_cov)
        hipLaunchKernelGGL((softmax_partial_lam_kernel<true, true>), dim3(grid, 1), dim3(RD_BLOCK), 0, s, d.cost, a4, d.N, d.blockmin,
                           d.n_blockmin, d.lam_rows, h->ws_partials_cov, mean4, h->ws_diag_rec);
        hipLaunchKernelGGL(merge_diag_lam_kernel<false>, dim3(1), dim3(MG_THREADS), 0, s, h->ws_partials_cov, grid, d.lam_rows,
                           (const float *)nullptr, 1.0f, h->ws_partials, RD_COV_RECORD_FLOATS, (const float *)h->ws_diag_rec, d.diag_out,
                           (float)d.N, (float *)nullptr, 0);
    } else {
        hipLaunchKernelGGL((softmax_partial_lam_kernel<true, false>), dim3(grid, 1), dim3(RD_BLOCK), 0, s, d.cost, a4, d.N, d.blockmin,
                           d.n_blockmin, d.lam_rows, h->ws_partials_cov, mean4, (float *)nullptr);
    }
    hipLaunchKernelGGL(merge_cov_lam_kernel, dim3(1), dim3(MG_THREADS), 0, s, h->ws_partials_cov, grid, d.lam_rows, d.a_mean_old,
                       d.gamma_mean, d.a_cov_old, d.gamma_sigma, d.a_mean_out, d.a_cov_out, RD_COV_RECORD_FLOATS, d.iter_out);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

