// ess_lambda.hip -- the ESS floor's temperature solver (covo_set_step_ess_floor, covo_ess_lambda).
//
// For the step's costs c_n, m = min c_n, w_n(lam) = expf((m - c_n) * (1 / lam)) -- the fp32 expression of the softmax update's stage 1
// (reduce.hip: softmax_partial_body) -- and ESS(lam) = (sum w)^2 / sum w^2, which is non-decreasing in lam:
//   ESS(lam0) >= ess_min     lam_eff = lam0, the floor is inactive (one pass over the costs, the common case)
//   otherwise                lam_eff solves ESS(lam) = ess_min on (lam0, 3 R], R = max finite c - m.  At lam = k R every w >= e^(-1/k), so
//                            ESS >= N e^(-2/k) >= N / 2 for k >= 2 / ln 2 = 2.89: the bracket holds the solution for ess_min <= N / 2.
// Bisection in ln(lam) (the mid point is the geometric mean of the bracket's ends, which stay fp32 temperatures) until no float
// lies strictly between the ends; the upper end -- ESS >= ess_min -- is the result.  A halving of ln(hi / lo) <= ln(2^254) down
// to one ulp takes at most ~35 evaluations; EL_MAX_EVALS caps them whatever the data is (NaN comparisons included).
// One workgroup of 1 024 threads per instance: thread t keeps the costs t, t + 1024, ... in registers up to N = 65 536 (64 per
// thread), beyond that every evaluation re-reads them (L2-resident).  Sums: wave butterflies, the 16 wave sums through LDS, added
// in ascending order by every thread -- no atomics, no flags: the result is a function of the costs alone, and every thread
// holds the same bracket, so all control flow is workgroup-uniform.
#include "covo_common.hpp"

constexpr int EL_THREADS = 1024;
constexpr int EL_WAVES = EL_THREADS / 64;
constexpr int EL_REG = 64;                     // costs per thread kept in registers
constexpr int EL_REG_MAX_N = EL_THREADS * EL_REG;  // 65 536
constexpr int EL_MAX_EVALS = 64;               // hard cap of ESS evaluations per instance (the first, at lam0, included)

struct EssLds {
    float a[2][EL_WAVES], b[2][EL_WAVES];  // two wave-sum buffers, alternating: one barrier per reduction
};

// (sum x, sum y) over the workgroup, identical in every thread; `flip` alternates between calls
__device__ __forceinline__ void ess_reduce2(float &x, float &y, EssLds &L, int &flip)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    x = wave_sum(x);
    y = wave_sum(y);
    if (lane == 0) {
        L.a[flip][wave] = x;
        L.b[flip][wave] = y;
    }
    __syncthreads();
    x = 0.0f;
    y = 0.0f;
#pragma unroll
    for (int i = 0; i < EL_WAVES; ++i) {
        x += L.a[flip][i];
        y += L.b[flip][i];
    }
    flip ^= 1;
}

// REG: N <= EL_REG_MAX_N, c[] holds this thread's costs (inf beyond N: weight exactly 0)
template <bool REG>
__device__ __forceinline__ float ess_eval(const float (&c)[EL_REG], const float *__restrict__ cost, int N, float m, float inv_lam,
                                          EssLds &L, int &flip)
{
    float s = 0.0f, s2 = 0.0f;
    if (REG) {
#pragma unroll
        for (int i = 0; i < EL_REG; ++i) {
            if (i * EL_THREADS < N) {  // (workgroup-uniform)
                const float w = expf((m - c[i]) * inv_lam);
                s += w;
                s2 += __fmul_rn(w, w);
            }
        }
    } else {
        for (int n = threadIdx.x; n < N; n += EL_THREADS) {
            const float w = expf((m - cost[n]) * inv_lam);
            s += w;
            s2 += __fmul_rn(w, w);
        }
    }
    ess_reduce2(s, s2, L, flip);
    return (s * s) / s2;
}

// grid (1, instances); groupmin: [instances][ngm] per-wave cost minima as the rollout leaves them, or null (formed from the costs)
// out: [instances][COVO_LAM_FLOATS] = {lam_eff, 1 / lam_eff, ESS(lam0), evaluations}
template <bool REG>
__global__ __launch_bounds__(EL_THREADS) void ess_lambda_kernel(const float *__restrict__ cost, int N,
                                                                const float *__restrict__ groupmin, int ngm, float lam0,
                                                                float inv_lam0, float ess_min, float *__restrict__ out)
{
    __shared__ EssLds L;
    const int tid = threadIdx.x;
    int flip = 0;
    {
        const size_t y = blockIdx.y;
        cost += y * N;
        if (groupmin != nullptr) groupmin += y * ngm;
        out += y * COVO_LAM_FLOATS;
    }
    // ---- pass 0: the costs (into registers), their exact minimum and their largest finite value
    float c[EL_REG];
    const bool own_min = groupmin == nullptr;
    float m = __builtin_inff(), cmax = -__builtin_inff();
    if (REG) {
#pragma unroll
        for (int i = 0; i < EL_REG; ++i) {
            const int n = tid + i * EL_THREADS;
            c[i] = (n < N) ? cost[n] : __builtin_inff();
            // compares, not fminf / fmaxf: those quiet a NaN first, and the quieted copy of every cost would live next to c[]
            if (own_min && c[i] < m) m = c[i];
            if (c[i] > cmax && c[i] < __builtin_inff()) cmax = c[i];  // (false for NaN)
        }
    } else {
        for (int n = tid; n < N; n += EL_THREADS) {
            const float cn = cost[n];
            if (own_min && cn < m) m = cn;
            if (cn > cmax && cn < __builtin_inff()) cmax = cn;
        }
    }
    if (!own_min) {  // the rollout's per-wave minima: the same exact minimum from N / 64 values
        for (int i = tid; i < ngm; i += EL_THREADS) m = fminf(m, groupmin[i]);
    }
    {   // min and max are exact in any order
        const int lane = tid & 63, wave = tid >> 6;
        m = wave_min(m);
        cmax = -wave_min(-cmax);
        if (lane == 0) {
            L.a[flip][wave] = m;
            L.b[flip][wave] = cmax;
        }
        __syncthreads();
        m = L.a[flip][0];
        cmax = L.b[flip][0];
#pragma unroll
        for (int i = 1; i < EL_WAVES; ++i) {
            m = fminf(m, L.a[flip][i]);
            cmax = fmaxf(cmax, L.b[flip][i]);
        }
        flip ^= 1;
    }
    const float ess0 = ess_eval<REG>(c, cost, N, m, inv_lam0, L, flip);
    float lo = lam0, hi = 3.0f * (cmax - m);
    float evals = 1.0f;
    // inactive floor; all-inf / NaN costs (m, the range or ESS(lam0) not finite); an empty bracket: lam0 stays
    const bool solve = fabsf(m) < __builtin_inff() && ess0 < ess_min && hi > lo && hi < __builtin_inff();
    if (!solve) {
        if (tid == 0) {
            out[0] = lam0;
            out[1] = inv_lam0;
            out[2] = ess0;
            out[3] = evals;
        }
        return;
    }
    // ---- ESS(lo) < ess_min <= ESS(hi): halve ln(hi / lo) until no float lies strictly between the ends
#pragma unroll 1
    for (int it = 1; it < EL_MAX_EVALS; ++it) {
        const float mid = sqrtf(lo) * sqrtf(hi);
        if (!(mid > lo && mid < hi)) break;
        const float ess = ess_eval<REG>(c, cost, N, m, __fdiv_rn(1.0f, mid), L, flip);
        evals += 1.0f;
        if (ess >= ess_min) hi = mid;
        else lo = mid;  // (a NaN evaluation lands here: the loop still ends, by the bracket or by the cap)
    }
    if (tid == 0) {
        out[0] = hi;
        out[1] = __fdiv_rn(1.0f, hi);
        out[2] = ess0;
        out[3] = evals;
    }
}

int launch_ess_lambda(const float *cost, int N, int n_inst, const float *groupmin, float lam0, float ess_min, float *out,
                      hipStream_t s)
{
    const int ngm = (N + 63) / 64;
    const float inv_lam0 = 1.0f / lam0;  // the float the unfloored update multiplies by (reduce.hip: launch_softmax_reduce)
    if (N <= EL_REG_MAX_N)
        hipLaunchKernelGGL(ess_lambda_kernel<true>, dim3(1, n_inst), dim3(EL_THREADS), 0, s, cost, N, groupmin, ngm, lam0, inv_lam0,
                           ess_min, out);
    else
        hipLaunchKernelGGL(ess_lambda_kernel<false>, dim3(1, n_inst), dim3(EL_THREADS), 0, s, cost, N, groupmin, ngm, lam0, inv_lam0,
                           ess_min, out);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
