// softmax_stage1.hpp -- the device bodies of the weighted update's stage 1 and of MPPI's covariance merge (see reduce.hip), shared by
// the kernels of reduce.hip (1 / lambda as a kernel argument), of reduce_lam.hip (1 / lambda read from device memory: the ESS floor)
// and of reduce_elite.hip (0/1 weights off the selector's threshold: the elite set).
#pragma once
#include "covo_common.hpp"
#include "softmax_merge.hpp"

constexpr int RD_BLOCK = 256;
constexpr int RD_WAVES = RD_BLOCK / 64;

// stage 1's grid for N samples: one wave per 64-sample group, capped at the handle's max_red_blocks (the waves then stride)
static inline int stage1_grid(const covo_ctx *h, int N)
{
    const int grid = ((N + 63) / 64 + RD_WAVES - 1) / RD_WAVES;
    return grid > h->max_red_blocks ? h->max_red_blocks : grid;
}

// COV (MPPI's covariance adaptation, mppi.py:119-125): the record also carries the weighted second moments of d = a - mu
// about the SHIFTED OLD mean mu (known before sampling; d is the clipped L eps, so no cancellation against mean^2):
// rec[COVO_PARTIAL_FLOATS + 10 t + j] = sum_n w_n d_i d_j for the 10 pairs i <= j of step t (cov_pair below).
constexpr int RD_COV_FLOATS = COVO_H * 10;                                   // 320
constexpr int RD_COV_RECORD_FLOATS = COVO_PARTIAL_FLOATS + RD_COV_FLOATS;    // 452

// The weights of stage 1 are a policy, passed by value: RED_FLOATS (the LDS floats begin() folds through), begin(red) -> the
// record's m for instance blockIdx.y, weight(c, m, n, N) -> w_n, and the diagnostic sums' terms diag_w2(w), diag_wdc(w, c - m).
// SoftmaxWeights (covo.py:266): w = exp((m - c) / lambda), m the exact global minimum of the costs from the per-wave minima the
// rollout left -- weights formed exactly like the reference's `cost - jnp.min(cost)`.  (The elite set's 0/1 weights: reduce_elite.hip.)
struct SoftmaxWeights {
    const float *__restrict__ blockmin;  // [instances][nbm]
    int nbm;
    float inv_lam;
    static constexpr int RED_FLOATS = RD_WAVES;
    __device__ __forceinline__ float begin(float *red) const
    {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const float *mins = blockmin + (size_t)blockIdx.y * nbm;
        float m = __builtin_inff();
        for (int i = tid; i < nbm; i += RD_BLOCK) m = fminf(m, mins[i]);
        m = wave_min(m);
        if (lane == 0) red[wave] = m;
        __syncthreads();
        return fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    }
    __device__ __forceinline__ float weight(float c, float m, int, int) const { return expf((m - c) * inv_lam); }
    // every product rounded on its own: no contraction into the sums
    __device__ __forceinline__ float diag_w2(float w) const { return __fmul_rn(w, w); }
    __device__ __forceinline__ float diag_wdc(float w, float dc) const { return __fmul_rn(w, dc); }
};

// DIAG (covo_set_step_diag): the workgroup also leaves its diagnostic record {sum w^2, sum w (c - m), sum (c - m), samples}
// (softmax_merge.hpp: MergeDiag; m is the policy's m here) in dpart[workgroup].
template <bool COV, bool DIAG, class Weights>
__device__ __forceinline__ void softmax_partial_body(const float *__restrict__ cost, const float4 *__restrict__ a, int N, Weights wt,
                                                     float *__restrict__ partials, const float4 *__restrict__ mu,
                                                     float *__restrict__ dpart)
{
    constexpr int REC = COV ? RD_COV_RECORD_FLOATS : COVO_PARTIAL_FLOATS;
    __shared__ float sv[RD_WAVES][COVO_NA];
    __shared__ float sv2[COV ? RD_WAVES : 1][COV ? RD_COV_FLOATS : 1];
    __shared__ float ss[RD_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {   // blockIdx.y (env-batched step): instance y's dense slices; its records follow those of instance y - 1
        const size_t y = blockIdx.y;
        cost += y * N;
        a += y * ((size_t)COVO_H * N);
        partials += y * gridDim.x * REC;
        if (DIAG) dpart += y * gridDim.x * MG_DIAG_REC;
        if (COV) mu += y * (COVO_NA / 4);  // (the mean instance y's second moments are centred on)
    }
    float m;
    if constexpr (Weights::RED_FLOATS > 0) {
        __shared__ float red[Weights::RED_FLOATS];
        m = wt.begin(red);
    } else {
        m = wt.begin(nullptr);
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
        const float w = wt.weight(c, m, n, N);
        s_lane += w;
        if (DIAG && n < N) {
            const float dc = c - m;
            d_lane[0] += wt.diag_w2(w);
            d_lane[1] += wt.diag_wdc(w, dc);
            d_lane[2] += dc;
            d_lane[3] += 1.0f;
        }
        const unsigned long long live = __ballot(w > 0.0f);
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


// index of the pair (i, j), i <= j, in a record's 10 second moments per step
__device__ __forceinline__ int cov_pair(int i, int j)
{
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    return lo * 4 - lo * (lo - 1) / 2 + (hi - lo);
}

// MPPI with gamma_sigma != 0 (mppi.py:109-125): merge G stage-1 records that carry second moments, new mean as merge_kernel,
// then a_cov'[t] = gamma_sigma sum_n w_n (a_n - mean')(a_n - mean')^T + (1 - gamma_sigma) a_cov[t] with the NEW mean (sic):
// with d = a - mu, e = mean' - mu, m1 = sum w d:  sum w (d - e)(d - e)^T = S2 - m1 e^T - e m1^T + e e^T   (sum w = 1).
// FINAL = false (a sample-sharded rank, round 4): the merged, UNNORMALISED record {m, s, v[128], pad[2], S2[320]} goes to
// a_mean_out instead -- this rank's contribution to the exchange; the G rank records are then merged by the FINAL variant on
// every rank (the second moments are about mu, the shifted OLD mean, which all ranks share).
// stride: floats between consecutive records (RD_COV_RECORD_FLOATS, or COVO_RANK_RECORD_COV_FLOATS for all-gathered rank records).
template <bool FINAL>
__device__ __forceinline__ void merge_cov_body(const float *__restrict__ partials, int G, float inv_lam,
                                               const float *__restrict__ a_mean_old, float gamma_mean,
                                               const float *__restrict__ a_cov_old, float gamma_sigma,
                                               float *__restrict__ a_mean_out, float *__restrict__ a_cov_out, int stride,
                                               float *__restrict__ iter_out = nullptr)  // (an iterated step: m goes there too)
{
    __shared__ float scale[MG_MAXG];
    __shared__ float redm[MG_THREADS / 64];
    __shared__ float reds[MG_THREADS / 64];
    __shared__ float sv[MG_SLICES][COVO_NA];
    __shared__ float sv2[MG_SLICES][RD_COV_FLOATS];
    __shared__ float smean[COVO_NA], sm1[COVO_NA], se[COVO_NA], s2[RD_COV_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int REC = stride;
    float m = __builtin_inff();
    for (int g = tid; g < G; g += MG_THREADS) m = fminf(m, partials[(size_t)g * REC]);
    m = wave_min(m);
    if (lane == 0) redm[wave] = m;
    __syncthreads();
    m = redm[0];
#pragma unroll
    for (int i = 1; i < MG_THREADS / 64; ++i) m = fminf(m, redm[i]);
    if (iter_out != nullptr && tid == 0) *iter_out = m;
    float s = 0.0f;
    for (int g = tid; g < G; g += MG_THREADS) {
        const float *rec = partials + (size_t)g * REC;
        const float sg = rec[1];
        const float sc = (sg > 0.0f) ? expf((m - rec[0]) * inv_lam) : 0.0f;
        scale[g] = sc;
        s = fmaf(sg, sc, s);
    }
    s = wave_sum(s);
    if (lane == 0) reds[wave] = s;
    __syncthreads();
    s = 0.0f;
#pragma unroll
    for (int i = 0; i < MG_THREADS / 64; ++i) s += reds[i];
    const int col = tid & (COVO_NA - 1), slice = tid >> 7;
    // one workgroup reads all G records (G x 1.8 KB): the loads of a thread's G / 8 records are independent, only the fmaf chain
    // is ordered -- unrolled so that eight are in flight (rolled, every trip paid its own memory round trip: 37 us at G = 256)
    float v = 0.0f;
#pragma unroll 8
    for (int g = slice; g < G; g += MG_SLICES) v = fmaf(partials[(size_t)g * REC + 2 + col], scale[g], v);
    sv[slice][col] = v;
    {
        // the 320 second-moment columns: columns col, col + 128 and (col < 64) col + 256 side by side
        const bool third = col + 2 * COVO_NA < RD_COV_FLOATS;
        float va = 0.0f, vb = 0.0f, vc = 0.0f;
#pragma unroll 4
        for (int g = slice; g < G; g += MG_SLICES) {
            const float *rec = partials + (size_t)g * REC + COVO_PARTIAL_FLOATS + col;
            const float sc = scale[g];
            va = fmaf(rec[0], sc, va);
            vb = fmaf(rec[COVO_NA], sc, vb);
            if (third) vc = fmaf(rec[2 * COVO_NA], sc, vc);
        }
        sv2[slice][col] = va;
        sv2[slice][col + COVO_NA] = vb;
        if (third) sv2[slice][col + 2 * COVO_NA] = vc;
    }
    __syncthreads();
    if (!FINAL) {  // the merged record, unnormalised (a_mean_out = record [RD_COV_RECORD_FLOATS])
        float *__restrict__ rec = a_mean_out;
        if (tid < COVO_NA) {
            v = 0.0f;
#pragma unroll
            for (int i = 0; i < MG_SLICES; ++i) v += sv[i][tid];
            rec[2 + tid] = v;
        }
        for (int c2 = tid; c2 < RD_COV_FLOATS; c2 += MG_THREADS) {
            float v2 = 0.0f;
#pragma unroll
            for (int i = 0; i < MG_SLICES; ++i) v2 += sv2[i][c2];
            rec[COVO_PARTIAL_FLOATS + c2] = v2;
        }
        if (tid == 0) {
            rec[0] = m;
            rec[1] = s;
        }
        return;
    }
    const float inv_s = 1.0f / s;
    if (tid < COVO_NA) {
        v = 0.0f;
#pragma unroll
        for (int i = 0; i < MG_SLICES; ++i) v += sv[i][tid];
        const float wmean = v * inv_s, mu = a_mean_old[tid];
        const float mean_new = wmean * gamma_mean + mu * (1.0f - gamma_mean);  // mppi.py:112-117
        smean[tid] = mean_new;
        sm1[tid] = wmean - mu;
        se[tid] = mean_new - mu;
    }
    for (int c2 = tid; c2 < RD_COV_FLOATS; c2 += MG_THREADS) {
        float v2 = 0.0f;
#pragma unroll
        for (int i = 0; i < MG_SLICES; ++i) v2 += sv2[i][c2];
        s2[c2] = v2 * inv_s;
    }
    __syncthreads();
    if (tid < COVO_NA) a_mean_out[tid] = smean[tid];
    if (tid < COVO_H * 16) {
        const int t = tid >> 4, i = (tid >> 2) & 3, j = tid & 3;
        const float c = s2[10 * t + cov_pair(i, j)] - sm1[4 * t + i] * se[4 * t + j] - se[4 * t + i] * sm1[4 * t + j] +
                        se[4 * t + i] * se[4 * t + j];
        a_cov_out[tid] = c * gamma_sigma + a_cov_old[tid] * (1.0f - gamma_sigma);  // mppi.py:119-125 (in place is fine: own element)
    }
}
