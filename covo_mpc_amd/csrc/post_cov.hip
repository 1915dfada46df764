// post_cov.hip -- the posterior covariance of a control step (gfx950): the weighted 128 x 128 sample covariance of the step's own
// samples under the step's own weights (covo_weighted_cov / covo_set_step_post_cov, include/covo_hip.h).
//
//   x_i[4 t + d] = a[t][i][d]   the clipped samples the update used          y_i = x_i - mu   (mu: the mean the step sampled around)
//   w_i                         the update's weight of sample i (below); 0 for a cost that is not finite
//   W = sum w_i,  dm = sum w_i y_i / W,  C = sum w_i y_i y_i^T / W - dm dm^T
//
// Two launches, (workgroups, instance) grids over dense per-instance slices:
//   stage 1  post_cov_partial_kernel: min(PC_WGS, chunks) persistent workgroups of four waves per instance stride over chunks of
//            PC_CHUNK = 64 samples.  Lane (p, kh) of every wave loads the float4 a[t = p][sample 2 j + kh] of k-step j: the four
//            components of one stage for one sample.  MFMA row / column index p is therefore the STAGE and the four 32-row operand
//            tiles are the four action components: tile (A, B) holds C[4 p + A][4 q + B].  The ten tiles A >= B are computed, split
//            3 / 3 / 2 / 2 over the waves, on v_mfma_f32_32x32x2_f32 with w_i y_i as the A operand and y_i as the B operand.  After
//            every chunk -- PC_NACC = 64 products per accumulator -- the fp32 accumulators are flushed into fp64 totals, so no fp32
//            accumulator ever sums more than PC_NACC products whatever N is.  sum w y and W are summed in fp64 by wave 2.  A
//            workgroup leaves ONE partial of PC_PARTIAL_FLOATS = 128 * 128 + 128 + 1 floats (the totals rounded once): tile (A, B)
//            at [(4 A + B) * 1024 + 64 r + lane] in the MFMA's own C/D layout (the six tiles A < B stay unwritten), sum w y at
//            [16384 + 4 p + d], W at [16512].
//   stage 2  post_cov_merge_kernel: sums the partials in fp64 in ascending workgroup order, forms C, rounds it to fp32 once and
//            stores every element of an off-diagonal tile at (row, col) and (col, row), every element p >= q of a diagonal tile
//            likewise (its elements p < q are not used): C is symmetric bit for bit.  dm dm^T is rounded to fp32 before it is
//            subtracted, as the single product of a one-sample S is: N = 1 gives C = 0 exactly.  W = 0 gives C = 0, dm = 0.
// The weights are the update's, from the update's sources, bit for bit: softmax exp((m - c) / lambda) with m the minimum of the costs
// (fminf over all of them: the value the update folds from the rollout's per-wave minima, which some step paths never store) and
// 1 / lambda either the host's 1.0f / lam (reduce.hip) or the ESS solver's row (ess_lambda.hip); or the elite selector's threshold and
// tie rule (elite_key.hpp, reduce_elite.hip).  Plain vector stores only.
#include <cstring>
#include "covo_common.hpp"
#include "elite_key.hpp"

constexpr int PC_BLOCK = 256;
constexpr int PC_CHUNK = 64;        // samples per workgroup trip: 32 k-steps of two samples
constexpr int PC_NACC = PC_CHUNK;   // products one fp32 accumulator sums before it is flushed into its fp64 total
constexpr int PC_WGS = 64;          // persistent workgroups per instance (all busy from N = PC_WGS * PC_CHUNK = 4 096 on)
constexpr int PC_TILE = 32 * 32;
constexpr int PC_OFF_WY = COVO_NA * COVO_NA, PC_OFF_W = PC_OFF_WY + COVO_NA;
constexpr int PC_PARTIAL_FLOATS = PC_OFF_W + 1;  // 16 513
constexpr int PC_BATCH = 8;         // k-steps whose loads are in flight ahead of their products
constexpr int PC_MERGE_WGS = 10 * PC_TILE / PC_BLOCK;  // 40: one thread per element of the ten tiles
static_assert(COVO_H == 32 && COVO_NA == 128, "post_cov.hip maps the 32 stages onto the MFMA's 32 rows");

typedef float pc_f32x16 __attribute__((ext_vector_type(16)));

enum PcKind { PC_SOFTMAX = 0, PC_SOFTMAX_ROWS = 1, PC_ELITE = 2 };
struct PcArgs {
    const float *cost;        // [n_inst][N]
    const float4 *a;          // [n_inst][H][N] float4
    const float *mu;          // [n_inst][128]
    int N;
    int kind;                 // PcKind
    float inv_lam;            // PC_SOFTMAX
    const float *lam_rows;    // PC_SOFTMAX_ROWS: [n_inst][COVO_LAM_FLOATS], [1] = 1 / lam_eff
    const float *elite_rows;  // PC_ELITE: [n_inst][COVO_ELITE_FLOATS]
    float *partials;          // [n_inst][gridDim.x][PC_PARTIAL_FLOATS]
};

// the update's weight of sample n (softmax_stage1.hpp: SoftmaxWeights::weight, reduce_elite.hip: EliteWeights::weight), 0 for a
// cost that is not finite
struct PcWeights {
    int kind;
    float m, inv_lam;
    uint32_t thr_u, thr_i;
    __device__ __forceinline__ float weight(float c, int n, int N) const
    {
        float w;
        if (kind == PC_ELITE) {
            const uint32_t u = elite_cost_word(c);
            w = (n < N && (u < thr_u || (u == thr_u && (uint32_t)n <= thr_i))) ? 1.0f : 0.0f;
        } else {
            w = expf((m - c) * inv_lam);
        }
        return (n < N && c - c == 0.0f) ? w : 0.0f;
    }
};

// the tiles (A, B), A >= B, of wave WAVE: {(0,0) (1,0) (1,1)} {(2,0) (2,1) (2,2)} {(3,0) (3,1)} {(3,2) (3,3)}
template <int WAVE>
struct PcTiles {
    static constexpr int NT = WAVE < 2 ? 3 : 2;
    static __host__ __device__ constexpr int A(int t) { return WAVE == 0 ? (t == 0 ? 0 : 1) : (WAVE == 1 ? 2 : 3); }
    static __host__ __device__ constexpr int B(int t) { return WAVE == 0 ? (t == 2 ? 1 : 0) : (WAVE == 3 ? 2 + t : t); }
};

// one wave's share of a workgroup's partial.  cost / a / mu: the instance's slices; part: the workgroup's partial
template <int WAVE>
__device__ __forceinline__ void pc_wave(const float *__restrict__ cost, const float4 *__restrict__ a, const float *__restrict__ mu,
                                        const int N, const PcWeights wt, float *__restrict__ part)
{
    using T = PcTiles<WAVE>;
    constexpr int NT = T::NT;
    constexpr bool SUMS = WAVE == 2;  // this wave also sums w y and W
    const int lane = threadIdx.x & 63, p = lane & 31, kh = lane >> 5;
    const float mu4[4] = {mu[4 * p + 0], mu[4 * p + 1], mu[4 * p + 2], mu[4 * p + 3]};
    const float4 *__restrict__ ap = a + (size_t)p * N;  // stage p's stripe
    double tot[NT][16];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[i][r] = 0.0;
    double sy[4] = {0.0, 0.0, 0.0, 0.0}, sw = 0.0;

    const int nchunks = (N + PC_CHUNK - 1) / PC_CHUNK;
    for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int s0 = ch * PC_CHUNK;
        const int n = s0 + lane;
        const float c = n < N ? cost[n] : __builtin_inff();
        const float w = wt.weight(c, n, N);
        if (__ballot(w > 0.0f) == 0ull) continue;  // (wave-uniform, and the same for the four waves)
        pc_f32x16 acc[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
        // k-step j takes samples s0 + 2 j (lanes kh = 0) and s0 + 2 j + 1 (kh = 1); the loads of batch b + 1 are issued ahead of
        // the products of batch b
        float4 cur[PC_BATCH], nxt[PC_BATCH];
        float wc[PC_BATCH], wn[PC_BATCH];
        auto load = [&](int b, float4 *v, float *wv) {
#pragma unroll
            for (int i = 0; i < PC_BATCH; ++i) {
                const int sl = 2 * (PC_BATCH * b + i) + kh;
                v[i] = ap[min(s0 + sl, N - 1)];  // (past the end: its weight is 0)
                wv[i] = __shfl(w, sl, 64);
            }
        };
        load(0, cur, wc);
#pragma unroll
        for (int b = 0; b < PC_NACC / 2 / PC_BATCH; ++b) {
            if (b + 1 < PC_NACC / 2 / PC_BATCH) load(b + 1, nxt, wn);
#pragma unroll
            for (int i = 0; i < PC_BATCH; ++i) {
                const float wv = wc[i];
                const bool live = wv > 0.0f;  // a sample of weight 0 is dropped whatever it holds (a NaN stripe)
                float y[4] = {cur[i].x - mu4[0], cur[i].y - mu4[1], cur[i].z - mu4[2], cur[i].w - mu4[3]};
                float wy[4];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    y[d] = live ? y[d] : 0.0f;
                    wy[d] = __fmul_rn(wv, y[d]);
                }
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wy[T::A(t)], y[T::B(t)], acc[t], 0, 0, 0);
                if (SUMS) {
#pragma unroll
                    for (int d = 0; d < 4; ++d) sy[d] += (double)wy[d];
                    sw += live ? (double)wv : 0.0;
                }
            }
            if (b + 1 < PC_NACC / 2 / PC_BATCH) {
#pragma unroll
                for (int i = 0; i < PC_BATCH; ++i) {
                    cur[i] = nxt[i];
                    wc[i] = wn[i];
                }
            }
        }
        // PC_NACC products per accumulator: into the fp64 totals
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[i][r] += (double)acc[i][r];
    }
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[(4 * T::A(i) + T::B(i)) * PC_TILE + 64 * r + lane] = (float)tot[i][r];
    if (SUMS) {
        // lanes (p, 0) and (p, 1) hold the even and the odd samples' sums of stage p; every lane of a half holds that half's W
#pragma unroll
        for (int d = 0; d < 4; ++d) sy[d] += __shfl_xor(sy[d], 32, 64);
        sw += __shfl_xor(sw, 32, 64);
        if (kh == 0) {
#pragma unroll
            for (int d = 0; d < 4; ++d) part[PC_OFF_WY + 4 * p + d] = (float)sy[d];
        }
        if (lane == 0) part[PC_OFF_W] = (float)sw;
    }
}

__global__ __launch_bounds__(PC_BLOCK) void post_cov_partial_kernel(const PcArgs P)
{
    __shared__ float red[PC_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t inst = blockIdx.y;
    const int N = P.N;
    const float *__restrict__ cost = P.cost + inst * N;
    const float4 *__restrict__ a = P.a + inst * ((size_t)COVO_H * N);
    const float *__restrict__ mu = P.mu + inst * COVO_NA;
    float *__restrict__ part = P.partials + (inst * gridDim.x + blockIdx.x) * PC_PARTIAL_FLOATS;
    PcWeights wt;
    wt.kind = P.kind;
    wt.m = 0.0f;
    wt.inv_lam = 0.0f;
    wt.thr_u = wt.thr_i = 0u;
    if (P.kind == PC_ELITE) {
        const float *row = P.elite_rows + inst * COVO_ELITE_FLOATS;
        wt.thr_u = __float_as_uint(row[ELITE_ROW_COST_WORD]);
        wt.thr_i = __float_as_uint(row[ELITE_ROW_INDEX_WORD]);
    } else {
        wt.inv_lam = P.kind == PC_SOFTMAX_ROWS ? P.lam_rows[inst * COVO_LAM_FLOATS + 1] : P.inv_lam;
        float m = __builtin_inff();
#pragma unroll 1
        for (int i = tid; i < N; i += 4 * PC_BLOCK) {  // four loads in flight; past the end: the last cost again
            const float c0 = cost[i], c1 = cost[min(i + PC_BLOCK, N - 1)], c2 = cost[min(i + 2 * PC_BLOCK, N - 1)],
                        c3 = cost[min(i + 3 * PC_BLOCK, N - 1)];
            m = fminf(fminf(m, c0), fminf(fminf(c1, c2), c3));
        }
        m = wave_min(m);
        if (lane == 0) red[wave] = m;
        __syncthreads();
        wt.m = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    }
    switch (wave) {
    case 0: pc_wave<0>(cost, a, mu, N, wt, part); break;
    case 1: pc_wave<1>(cost, a, mu, N, wt, part); break;
    case 2: pc_wave<2>(cost, a, mu, N, wt, part); break;
    default: pc_wave<3>(cost, a, mu, N, wt, part); break;
    }
}

// grid (PC_MERGE_WGS, n_inst): thread e of an instance owns element e = tile * 1024 + 64 r + lane of the ten computed tiles
__global__ __launch_bounds__(PC_BLOCK) void post_cov_merge_kernel(const float *__restrict__ partials, const int G,
                                                                  float *__restrict__ cov, float *__restrict__ aux)
{
    __shared__ double sd[COVO_NA];
    __shared__ double sW;
    const int tid = threadIdx.x;
    const size_t inst = blockIdx.y;
    const float *__restrict__ part = partials + inst * G * PC_PARTIAL_FLOATS;
    if (tid <= COVO_NA) {  // threads 0..127: sum w y of row tid; thread 128: W
        double s = 0.0;
#pragma unroll 8
        for (int g = 0; g < G; ++g) s += (double)part[(size_t)g * PC_PARTIAL_FLOATS + PC_OFF_WY + tid];
        if (tid < COVO_NA) sd[tid] = s;
        else sW = s;
    }
    __syncthreads();
    const double W = sW;
    const bool any = W > 0.0;
    const int e = blockIdx.x * PC_BLOCK + tid;
    const int tile = e >> 10, r = (e >> 6) & 15, lane = e & 63;
    // tile -> (A, B) in the order (0,0) (1,0) (1,1) (2,0) (2,1) (2,2) (3,0) (3,1) (3,2) (3,3)
    const int A = tile < 1 ? 0 : (tile < 3 ? 1 : (tile < 6 ? 2 : 3));
    const int B = tile - (A * (A + 1)) / 2;
    const int p = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), q = lane & 31;  // the 32x32 C/D layout: row p, column q
    const int row = 4 * p + A, col = 4 * q + B;
    if (A != B || p >= q) {
        double S = 0.0;
        const float *__restrict__ src = part + (4 * A + B) * PC_TILE + 64 * r + lane;
#pragma unroll 8
        for (int g = 0; g < G; ++g) S += (double)src[(size_t)g * PC_PARTIAL_FLOATS];
        float c = 0.0f;
        if (any) {
            const float dd = (float)((sd[row] / W) * (sd[col] / W));  // rounded as a one-sample S is
            c = (float)(S / W - (double)dd);
        }
        float *__restrict__ C = cov + inst * ((size_t)COVO_NA * COVO_NA);
        C[row * COVO_NA + col] = c;
        if (row != col) C[col * COVO_NA + row] = c;
    }
    if (blockIdx.x == 0 && tid < COVO_POST_AUX_FLOATS) {
        float v = 0.0f;
        if (tid < COVO_NA) v = any ? (float)(sd[tid] / W) : 0.0f;
        else if (tid == COVO_NA) v = (float)W;
        aux[inst * COVO_POST_AUX_FLOATS + tid] = v;
    }
}

// ---- host
struct PostCovState {
    float *partials = nullptr;  // [cap][PC_WGS][PC_PARTIAL_FLOATS]
    int cap = 0;                // instances
    float *elite_rows = nullptr;  // [COVO_MAX_ENVS][COVO_ELITE_FLOATS]: the stand-alone entry's selector rows
};
static PostCovState *post_cov_state(covo_ctx *h)
{
    if (h->post_cov == nullptr) h->post_cov = new PostCovState();
    return reinterpret_cast<PostCovState *>(h->post_cov);
}
void post_cov_state_destroy(covo_ctx *h)
{
    PostCovState *st = reinterpret_cast<PostCovState *>(h->post_cov);
    if (st == nullptr) return;
    (void)hipFree(st->partials);
    (void)hipFree(st->elite_rows);
    delete st;
    h->post_cov = nullptr;
}

// the partials of n_inst instances.  Growing synchronises the device first (the launches that read the old buffer are done): at an
// attachment or a first stand-alone call, never inside a steady-state step
int post_cov_reserve(covo_ctx *h, int n_inst)
{
    PostCovState *st = post_cov_state(h);
    if (n_inst <= st->cap) return 0;
    COVO_CHECK_HIP(hipDeviceSynchronize());
    (void)hipFree(st->partials);
    st->partials = nullptr;
    st->cap = 0;
    COVO_CHECK_HIP(hipMalloc(&st->partials, (size_t)n_inst * PC_WGS * PC_PARTIAL_FLOATS * sizeof(float)));
    st->cap = n_inst;
    return 0;
}

// d.elite_K > 0 with d.elite_rows null: the selector runs first, into the handle's own rows (the stand-alone entry)
int launch_weighted_cov(covo_ctx *h, const PostCovDesc &d, hipStream_t s)
{
    PostCovState *st = post_cov_state(h);
    if (int rc = post_cov_reserve(h, d.n_inst)) return rc;
    PcArgs P;
    std::memset(&P, 0, sizeof(P));
    P.cost = d.cost;
    P.a = reinterpret_cast<const float4 *>(d.a);
    P.mu = d.mu;
    P.N = d.N;
    P.partials = st->partials;
    if (d.elite_rows != nullptr || d.elite_K > 0) {
        P.kind = PC_ELITE;
        P.elite_rows = d.elite_rows;
        if (d.elite_rows == nullptr) {
            if (d.n_inst > COVO_MAX_ENVS) {
                covo_set_error("launch_weighted_cov: n_inst=%d above %d with an elite set", d.n_inst, COVO_MAX_ENVS);
                return COVO_E_BADARG;
            }
            if (st->elite_rows == nullptr)
                COVO_CHECK_HIP(hipMalloc(&st->elite_rows, (size_t)COVO_MAX_ENVS * COVO_ELITE_FLOATS * sizeof(float)));
            if (int rc = launch_elite_select(d.cost, d.N, d.n_inst, d.elite_K, st->elite_rows, s)) return rc;
            P.elite_rows = st->elite_rows;
        }
    } else if (d.lam_rows != nullptr) {
        P.kind = PC_SOFTMAX_ROWS;
        P.lam_rows = d.lam_rows;
    } else {
        P.kind = PC_SOFTMAX;
        P.inv_lam = 1.0f / d.lam;  // the float the update multiplies by (reduce.hip: launch_softmax_reduce)
    }
    const int nchunks = (d.N + PC_CHUNK - 1) / PC_CHUNK;
    const int G = nchunks < PC_WGS ? nchunks : PC_WGS;
    hipLaunchKernelGGL(post_cov_partial_kernel, dim3(G, d.n_inst), dim3(PC_BLOCK), 0, s, P);
    hipLaunchKernelGGL(post_cov_merge_kernel, dim3(PC_MERGE_WGS, d.n_inst), dim3(PC_BLOCK), 0, s, (const float *)st->partials, G,
                       d.cov_out, d.aux_out);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

// the attachment's launches behind the step that has just been enqueued (no-op with nothing attached): n_inst dense instances of
// the step's stripes and costs, mu the mean(s) the step sampled around; the weights are the step's own update's
int launch_post_cov_after(covo_ctx *h, const float *a, const float *cost, const float *mu, int N, int n_inst, hipStream_t s)
{
    if (!covo_post_cov_on(h)) return 0;
    if (mu == nullptr) {
        covo_set_error("posterior covariance (covo_set_step_post_cov): this step path leaves no shifted mean in device memory");
        return COVO_E_BADARG;
    }
    PostCovDesc d;
    d.a = a;
    d.cost = cost;
    d.mu = mu;
    d.N = N;
    d.n_inst = n_inst;
    d.lam = h->cfg.lam;
    d.lam_rows = covo_lam_target(h);
    d.elite_rows = covo_elite_target(h);
    d.elite_K = h->elite_K;
    d.cov_out = h->post_cov_out;
    d.aux_out = h->post_aux_out;
    return launch_weighted_cov(h, d, s);
}
