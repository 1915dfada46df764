// softmax_merge.hpp -- stage 2 of the exp(-cost/lambda)-weighted aggregation (covo.py:266-275) as a device function: merges G
// online-softmax records {m, s, v[128]} into the new mean (or into one merged record).  ONE body for its callers, so that
// they agree bit for bit whatever their workgroup size:
//   merge_kernel (reduce.hip, reduce_lam.hip; 1 024 threads)   the stand-alone launch: the records of the record-leaving rollout or of
//                                                      the stand-alone stage 1; also merges the all-gathered rank records
//   the last workgroup of the fused small step         (step_small.hip, 256 threads: the launch finishes its own update;
//                                                      rollout_common.hpp: rollout_merge_last)
// (The merge inside the product rollout launch -- its last workgroup, 192 .. 768 threads -- was removed in round 6: DESIGN 4.7.)
// The arithmetic is laid out over VIRTUAL lanes, not over the caller's threads: record g is "thread g" of a 1 024-thread
// workgroup (its 64-record virtual waves are summed with the wave butterfly, the 16 wave sums in ascending order), column c of
// slice q sums the records g = q, q + 8, q + 16, ... in ascending order with one fma each, the 8 slices are added in ascending
// order.  A caller with fewer threads walks the same virtual lanes in several rounds.  Fixed order: bit-reproducible, and
// independent of which workgroup happens to run it.
// COH: the records were written by OTHER workgroups of the SAME launch (agent-scope relaxed atomic stores, write-through): read
// them with agent-scope relaxed atomic loads (sc1: served coherently across the XCDs' L2s, no cache-wide fence).
#pragma once
#include "covo_common.hpp"

constexpr int MG_THREADS = 1024;
constexpr int MG_SLICES = MG_THREADS / COVO_NA;  // 8
constexpr int MG_MAXG = 1024;
constexpr int MG_VWAVES = MG_THREADS / 64;       // 16

struct MergeLds {
    float scale[MG_MAXG];
    float redm[MG_VWAVES];
    float reds[MG_VWAVES];
    float sv[MG_SLICES][COVO_NA];
};

// DIAG (the per-step sampling diagnostics, covo_set_step_diag): next to its record every stage-1 workgroup leaves a diagnostic
// record {sum w^2, sum w (c - m_g), sum (c - m_g), valid samples} over its samples (w = exp(-(c - m_g)/lam), m_g the record's own
// minimum: the cost sums are formed relative to a minimum, at lam = 0.01 the differences that matter are 1e-2 on costs of order
// 1-100).  The merge rescales them like s -- sum w^2 = sum_g s2_g scale_g^2, the two cost sums shifted by m_g - m -- over the same
// virtual lanes in the same order, and writes the COVO_DIAG_FLOATS of include/covo_hip.h.
constexpr int MG_DIAG_REC = 4;  // floats per stage-1 diagnostic record
struct MergeDiag {
    const float *rec = nullptr;  // [G][MG_DIAG_REC]
    float *out = nullptr;        // [COVO_DIAG_FLOATS]
    float n = 0.0f;              // the step's sample count
    float (*red)[MG_VWAVES] = nullptr;  // LDS [3][MG_VWAVES]: the virtual waves' sums
};

// An iterated step (covo_set_step_iters): after merge_body, the cost minimum m it formed -- the minimum over its waves' minima in
// L.redm (phase 1; nothing overwrites them) -- to the pass's slot of the iteration log.  Called by thread 0 behind the body's barriers.
template <int THREADS>
__device__ __forceinline__ void merge_log_min(const MergeLds &L, float *__restrict__ slot)
{
    float m = L.redm[0];
#pragma unroll
    for (int i = 1; i < THREADS / 64; ++i) m = fminf(m, L.redm[i]);
    *slot = m;
}

template <bool COH>
__device__ __forceinline__ float mg_load(const float *p)
{
    if (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}

// FINAL: out[128] = gamma * v / s + (1 - gamma) * a_mean_old (covo.py:270-275); else out[130] = the merged record {m, s, v}.
// stride: floats between consecutive records.  Every thread of the workgroup calls it (it contains barriers); THREADS is a
// multiple of 64.  G <= MG_MAXG.
template <int THREADS, bool FINAL, bool COH, bool DIAG = false>
__device__ __forceinline__ void merge_body(const float *__restrict__ partials, int G, float inv_lam, const float *__restrict__ a_mean_old,
                                           float gamma_mean, float *__restrict__ out, int stride, MergeLds &L,
                                           const MergeDiag &D = MergeDiag())
{
#pragma clang fp contract(off)  // every fused multiply-add below is written out: the same bits in every translation unit
    static_assert(THREADS % 64 == 0 && THREADS <= MG_THREADS, "merge_body: THREADS");
    constexpr int ROUNDS = (MG_THREADS + THREADS - 1) / THREADS;  // virtual threads per thread
    constexpr int NW = THREADS / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // phase 3's operands of this thread's first virtual lane first (they depend on nothing: their round trip overlaps phases 1
    // and 2 -- the records other XCDs have just written are most of this merge's time)
    constexpr int MG_PRE = 32;
    float vals[MG_PRE];
    {
        const int col = tid & (COVO_NA - 1), slice = tid >> 7;  // (tid < 1 024: slice < 8)
#pragma unroll
        for (int i = 0; i < MG_PRE; ++i) {
            const int g = slice + MG_SLICES * i;
            vals[i] = (g < G) ? mg_load<COH>(partials + (size_t)g * stride + 2 + col) : 0.0f;
        }
    }
    // phase 1: m = min_g m_g (exact in any order); a virtual thread's header {m_g, s_g} stays in registers for phase 2
    float my_m[ROUNDS], my_s[ROUNDS];
    float my_d[DIAG ? ROUNDS : 1][MG_DIAG_REC];
    float m = __builtin_inff();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int g = tid + r * THREADS;
        const bool mine = g < G && g < MG_THREADS;
        my_m[r] = mine ? mg_load<COH>(partials + (size_t)g * stride) : __builtin_inff();
        my_s[r] = mine ? mg_load<COH>(partials + (size_t)g * stride + 1) : 0.0f;
        m = fminf(m, my_m[r]);
        if (DIAG) {
#pragma unroll
            for (int j = 0; j < MG_DIAG_REC; ++j) my_d[r][j] = mine ? mg_load<COH>(D.rec + (size_t)g * MG_DIAG_REC + j) : 0.0f;
        }
    }
    m = wave_min(m);
    if (lane == 0) L.redm[wave] = m;
    if (tid < MG_VWAVES) L.reds[tid] = 0.0f;
    __syncthreads();
    m = L.redm[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) m = fminf(m, L.redm[i]);
    // phase 2: per-record scale; s = sum_g s_g scale_g as 16 virtual-wave butterflies, then in ascending wave order
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int g = tid + r * THREADS;  // THREADS % 64 == 0: a wave holds one whole virtual wave, lane = g & 63
        if (g - lane < MG_THREADS) {      // (wave-uniform)
            float sg = 0.0f, d2 = 0.0f, dw = 0.0f, dc = 0.0f;
            if (g < G) {
                const float sc = (my_s[r] > 0.0f) ? expf((m - my_m[r]) * inv_lam) : 0.0f;  // empty shard -> 0
                L.scale[g] = sc;
                sg = my_s[r] * sc;
                if (DIAG && my_d[r][3] > 0.0f) {  // (a record without samples has m_g = inf)
                    const float dm = my_m[r] - m;  // >= 0: c - m = (c - m_g) + dm
                    d2 = my_d[r][0] * (sc * sc);
                    dw = (my_d[r][1] + my_s[r] * dm) * sc;
                    dc = my_d[r][2] + my_d[r][3] * dm;
                }
            }
            sg = wave_sum(sg);
            if (lane == 0) L.reds[g >> 6] = sg;
            if (DIAG) {
                d2 = wave_sum(d2);
                dw = wave_sum(dw);
                dc = wave_sum(dc);
                if (lane == 0) {
                    D.red[0][g >> 6] = d2;
                    D.red[1][g >> 6] = dw;
                    D.red[2][g >> 6] = dc;
                }
            }
        }
    }
    __syncthreads();
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < MG_VWAVES; ++i) s += L.reds[i];
    if (DIAG && tid == 0) {  // the virtual waves' sums in ascending order, like s
        float s2 = 0.0f, sw = 0.0f, sc = 0.0f;
#pragma unroll
        for (int i = 0; i < MG_VWAVES; ++i) {
            s2 += D.red[0][i];
            sw += D.red[1][i];
            sc += D.red[2][i];
        }
        D.out[0] = (s * s) / s2;  // ess
        D.out[1] = m;             // cost_min
        D.out[2] = m + sw / s;    // cost_weighted
        D.out[3] = m + sc / D.n;  // cost_mean
        D.out[4] = s;             // weight_sum
        D.out[5] = D.n;           // n_samples
        D.out[6] = 0.0f;
        D.out[7] = 0.0f;
    }
    // phase 3: v[col] = sum_g v_g[col] scale_g per slice (ascending g within a slice)
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int vt = tid + r * THREADS;
        if (vt < MG_THREADS) {
            const int col = vt & (COVO_NA - 1), slice = vt >> 7;
            float v = 0.0f;
            if (r == 0) {
#pragma unroll
                for (int i = 0; i < MG_PRE; ++i) {
                    const int g = slice + MG_SLICES * i;
                    if (g < G) v = __builtin_fmaf(vals[i], L.scale[g], v);
                }
#pragma unroll 4
                for (int g = slice + MG_SLICES * MG_PRE; g < G; g += MG_SLICES)
                    v = __builtin_fmaf(mg_load<COH>(partials + (size_t)g * stride + 2 + col), L.scale[g], v);
            } else {
#pragma unroll 8
                for (int g = slice; g < G; g += MG_SLICES)
                    v = __builtin_fmaf(mg_load<COH>(partials + (size_t)g * stride + 2 + col), L.scale[g], v);
            }
            L.sv[slice][col] = v;
        }
    }
    __syncthreads();
    if (tid < COVO_NA) {
        float v = 0.0f;
#pragma unroll
        for (int i = 0; i < MG_SLICES; ++i) v += L.sv[i][tid];
        if (FINAL) {
            out[tid] = __builtin_fmaf(gamma_mean, v / s, a_mean_old[tid] * (1.0f - gamma_mean));
        } else {
            out[2 + tid] = v;
            if (tid == 0) {
                out[0] = m;
                out[1] = s;
            }
        }
    }
}

// The stand-alone merge launch (reduce.hip, reduce_lam.hip): workgroup blockIdx.x of MG_THREADS threads merges instance x's G
// records into its own mean (FINAL) or merged record, DIAG: and the diagnostic records dpart [instances][G][MG_DIAG_REC] into row x
// of diag_out [instances][COVO_DIAG_FLOATS]; iter_out != null (an iterated step): the cost minimum to slot x * iter_stride.
template <bool FINAL, bool DIAG>
__device__ __forceinline__ void merge_instance(const float *partials, int G, float inv_lam, const float *a_mean_old, float gamma_mean,
                                               float *out, int stride, const float *dpart, float *diag_out, float n_samples,
                                               float *iter_out, int iter_stride)
{
    __shared__ MergeLds lds;
    const size_t x = blockIdx.x;
    partials += x * G * stride;
    if (FINAL) a_mean_old += x * COVO_NA;
    out += x * (FINAL ? COVO_NA : COVO_PARTIAL_FLOATS);
    MergeDiag D;
    if constexpr (DIAG) {
        __shared__ float dred[3][MG_VWAVES];
        D.rec = dpart + x * G * MG_DIAG_REC;
        D.out = diag_out + x * COVO_DIAG_FLOATS;
        D.n = n_samples;
        D.red = dred;
    }
    merge_body<MG_THREADS, FINAL, false, DIAG>(partials, G, inv_lam, a_mean_old, gamma_mean, out, stride, lds, D);
    if (iter_out != nullptr && threadIdx.x == 0) merge_log_min<MG_THREADS>(lds, iter_out + blockIdx.x * (size_t)iter_stride);
}
