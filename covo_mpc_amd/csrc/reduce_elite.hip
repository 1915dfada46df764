// reduce_elite.hip -- the elite-set update (covo_set_step_elite): the softmax update of reduce.hip with weights
// w_n = 1 for the K samples of smallest key and 0 otherwise.  Stage 1 is softmax_partial_body's loop and record layout
// (softmax_stage1.hpp) with the weight read off the selector's threshold (elite_select.hip: row blockIdx.y) instead of an
// exponential; every record carries the selector's cost_min as its m, so the unchanged merges of reduce.hip (launch_merge,
// launch_merge_cov at 1 / lambda = 1) rescale every record by expf(0) = 1, divide by s = K and log the pass's minimum cost.  A
// translation unit of its own: the kernels of reduce.hip and reduce_lam.hip are compiled exactly as without it.
#include "covo_common.hpp"
#include "elite_key.hpp"
#include "softmax_merge.hpp"
#include "softmax_stage1.hpp"

// rec = {m = cost_min, s = this workgroup's elites, v[128] = their action sums} (+ COV: their 320 second moments about mu; DIAG: the
// record {sum w^2 = s, sum over the elites of c - m, sum over all samples of c - m, samples})
template <bool COV, bool DIAG>
__global__ __launch_bounds__(RD_BLOCK) void elite_partial_kernel(const float *__restrict__ cost, const float4 *__restrict__ a, int N,
                                                                 const float *__restrict__ elite_rows, float *__restrict__ partials,
                                                                 const float4 *__restrict__ mu, float *__restrict__ dpart)
{
    constexpr int REC = COV ? RD_COV_RECORD_FLOATS : COVO_PARTIAL_FLOATS;
    __shared__ float sv[RD_WAVES][COVO_NA];
    __shared__ float sv2[COV ? RD_WAVES : 1][COV ? RD_COV_FLOATS : 1];
    __shared__ float ss[RD_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t thr_u, thr_i;
    float m;
    {   // blockIdx.y (env-batched step): instance y's dense slices and selector row; its records follow those of instance y - 1
        const size_t y = blockIdx.y;
        cost += y * N;
        a += y * ((size_t)COVO_H * N);
        partials += y * gridDim.x * REC;
        if (DIAG) dpart += y * gridDim.x * MG_DIAG_REC;
        const float *row = elite_rows + y * COVO_ELITE_FLOATS;
        thr_u = __float_as_uint(row[ELITE_ROW_COST_WORD]);
        thr_i = __float_as_uint(row[ELITE_ROW_INDEX_WORD]);
        m = row[ELITE_ROW_COST_MIN];
    }

    const int ngroups = (N + 63) / 64;
    const int sub = lane & 7, tq = lane >> 3;
    float4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    float s_lane = 0.0f;
    float d_lane[DIAG ? MG_DIAG_REC : 1];
    if (DIAG) {
#pragma unroll
        for (int j = 0; j < MG_DIAG_REC; ++j) d_lane[j] = 0.0f;
    }
    float acc2[COV ? 4 : 1][10];  // COV: pairs (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3) of steps 8 tb + tq
    float4 mu4[COV ? 4 : 1];
    if (COV) {
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) {
            mu4[tb] = mu[8 * tb + tq];
#pragma unroll
            for (int j = 0; j < 10; ++j) acc2[tb][j] = 0.0f;
        }
    }

    for (int g = blockIdx.x * RD_WAVES + wave; g < ngroups; g += gridDim.x * RD_WAVES) {
        const int n = g * 64 + lane;
        const float c = (n < N) ? cost[n] : __builtin_inff();
        const uint32_t u = elite_cost_word(c);
        const bool elite = n < N && (u < thr_u || (u == thr_u && (uint32_t)n <= thr_i));  // key(n) <= threshold
        const float w = elite ? 1.0f : 0.0f;
        s_lane += w;
        if (DIAG && n < N) {
            const float dc = c - m;
            d_lane[0] += w;
            d_lane[1] += elite ? dc : 0.0f;
            d_lane[2] += dc;
            d_lane[3] += 1.0f;
        }
        const unsigned long long live = __ballot(elite);
        if (live == 0ull) continue;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (((live >> (8 * q)) & 0xffull) == 0ull) continue;  // wave-uniform
            const float wv = __shfl(w, 8 * q + sub, 64);
            int ns = g * 64 + 8 * q + sub;
            ns = ns < N ? ns : N - 1;  // wv == 0 there
#pragma unroll
            for (int tb = 0; tb < 4; ++tb) {
                const float4 av = a[(size_t)(8 * tb + tq) * N + ns];
                acc[tb].x = fmaf(wv, av.x, acc[tb].x);
                acc[tb].y = fmaf(wv, av.y, acc[tb].y);
                acc[tb].z = fmaf(wv, av.z, acc[tb].z);
                acc[tb].w = fmaf(wv, av.w, acc[tb].w);
                if (COV) {
                    const float d0 = av.x - mu4[tb].x, d1 = av.y - mu4[tb].y, d2 = av.z - mu4[tb].z, d3 = av.w - mu4[tb].w;
                    const float w0 = wv * d0, w1 = wv * d1, w2 = wv * d2, w3 = wv * d3;
                    acc2[tb][0] = fmaf(w0, d0, acc2[tb][0]);
                    acc2[tb][1] = fmaf(w0, d1, acc2[tb][1]);
                    acc2[tb][2] = fmaf(w0, d2, acc2[tb][2]);
                    acc2[tb][3] = fmaf(w0, d3, acc2[tb][3]);
                    acc2[tb][4] = fmaf(w1, d1, acc2[tb][4]);
                    acc2[tb][5] = fmaf(w1, d2, acc2[tb][5]);
                    acc2[tb][6] = fmaf(w1, d3, acc2[tb][6]);
                    acc2[tb][7] = fmaf(w2, d2, acc2[tb][7]);
                    acc2[tb][8] = fmaf(w2, d3, acc2[tb][8]);
                    acc2[tb][9] = fmaf(w3, d3, acc2[tb][9]);
                }
            }
        }
    }
    if (COV) {
#pragma unroll
        for (int tb = 0; tb < 4; ++tb)
#pragma unroll
            for (int j = 0; j < 10; ++j) {
#pragma unroll
                for (int o = 1; o < 8; o <<= 1) acc2[tb][j] += __shfl_xor(acc2[tb][j], o, 64);
                if (sub == 0) sv2[wave][10 * (8 * tb + tq) + j] = acc2[tb][j];
            }
    }
    // fold the 8 sample lanes (lane bits 0..2)
#pragma unroll
    for (int tb = 0; tb < 4; ++tb) {
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            acc[tb].x += __shfl_xor(acc[tb].x, o, 64);
            acc[tb].y += __shfl_xor(acc[tb].y, o, 64);
            acc[tb].z += __shfl_xor(acc[tb].z, o, 64);
            acc[tb].w += __shfl_xor(acc[tb].w, o, 64);
        }
    }
    const float s_wave = wave_sum(s_lane);
    if (sub == 0) {
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) *reinterpret_cast<float4 *>(&sv[wave][4 * (8 * tb + tq)]) = acc[tb];
    }
    if (lane == 0) ss[wave] = s_wave;
    __syncthreads();
    float *rec = partials + (size_t)blockIdx.x * REC;
    if (tid < COVO_NA) rec[2 + tid] = (sv[0][tid] + sv[1][tid]) + (sv[2][tid] + sv[3][tid]);
    if (COV) {
        for (int i = tid; i < RD_COV_FLOATS; i += RD_BLOCK)
            rec[COVO_PARTIAL_FLOATS + i] = (sv2[0][i] + sv2[1][i]) + (sv2[2][i] + sv2[3][i]);
    }
    if (tid == 0) {
        rec[0] = m;
        rec[1] = (ss[0] + ss[1]) + (ss[2] + ss[3]);
    }
    if constexpr (DIAG) {
        __shared__ float sd[RD_WAVES][MG_DIAG_REC];
#pragma unroll
        for (int j = 0; j < MG_DIAG_REC; ++j) {
            const float d = wave_sum(d_lane[j]);
            if (lane == 0) sd[wave][j] = d;
        }
        __syncthreads();
        if (tid < MG_DIAG_REC)  // the waves' sums in ascending order
            dpart[(size_t)blockIdx.x * MG_DIAG_REC + tid] = ((sd[0][tid] + sd[1][tid]) + sd[2][tid]) + sd[3][tid];
    }
}

// MPPI's covariance adaptation with diagnostics: the diagnostics' own merge over the headers {m, s} of the 452-float records, as
// launch_softmax_update_cov does it (reduce.hip keeps that instantiation to itself)
__global__ __launch_bounds__(MG_THREADS) void elite_merge_diag_kernel(const float *__restrict__ partials, int G, float *__restrict__ out,
                                                                      int stride, const float *__restrict__ dpart,
                                                                      float *__restrict__ diag_out, float n_samples)
{
    __shared__ MergeLds lds;
    __shared__ float dred[3][MG_VWAVES];
    MergeDiag D;
    D.rec = dpart;
    D.out = diag_out;
    D.n = n_samples;
    D.red = dred;
    merge_body<MG_THREADS, false, false, true>(partials, G, 1.0f, nullptr, 1.0f, out, stride, lds, D);
}

static int elite_stage1_grid(const covo_ctx *h, const UpdateDesc &d)
{
    const int grid = ((d.N + 63) / 64 + RD_WAVES - 1) / RD_WAVES;
    return grid > h->max_red_blocks ? h->max_red_blocks : grid;
}

// the elite-set variant of launch_softmax_reduce: d.elite_rows [batch][COVO_ELITE_FLOATS] in device memory, a final update only
int launch_elite_reduce(covo_ctx *h, const UpdateDesc &d, hipStream_t s)
{
    if (d.a_mean_out == nullptr || d.elite_rows == nullptr) {
        covo_set_error("launch_elite_reduce: the elite-set update needs a final update and the selector's rows");
        return COVO_E_BADARG;
    }
    float *partials_ws = d.partials_ws ? d.partials_ws : h->ws_partials;
    const int grid = elite_stage1_grid(h, d);
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
    const int grid = elite_stage1_grid(h, d);
    const float4 *a4 = reinterpret_cast<const float4 *>(d.a), *mean4 = reinterpret_cast<const float4 *>(d.a_mean_old);
    if (d.diag_out != nullptr) {
        hipLaunchKernelGGL((elite_partial_kernel<true, true>), dim3(grid, 1), dim3(RD_BLOCK), 0, s, d.cost, a4, d.N, d.elite_rows,
                           h->ws_partials_cov, mean4, h->ws_diag_rec);
        hipLaunchKernelGGL(elite_merge_diag_kernel, dim3(1), dim3(MG_THREADS), 0, s, (const float *)h->ws_partials_cov, grid,
                           h->ws_partials, RD_COV_RECORD_FLOATS, (const float *)h->ws_diag_rec, d.diag_out, (float)d.N);
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
