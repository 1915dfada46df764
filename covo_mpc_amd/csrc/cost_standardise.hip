// cost_standardise.hip -- the annealed step's two launches (covo_set_step_anneal, covo_cost_standardise).
//
// 1. The standardising solver.  For a pass's costs c_n, F = {n : c_n finite} (neither NaN nor +-inf):
//      mean = sum_F c / |F|,   std = sqrt(sum_F (c - mean)^2 / |F|)        two passes over the costs, fp64, the population form
//      lam_eff = (float)((double)temp * std)                               one rounding to fp32
//    and the row {lam_eff, inv_lam_eff, (float)std, bits(|F| | fallback << 31)}.  inv_lam_eff = __fdiv_rn(1.0f, lam_eff): the fp32
//    expression of the ESS solver's entry 1 (ess_lambda.hip) -- the correctly rounded fp32 quotient 1 / lam_eff, which is also what
//    the host's 1.0f / lam0 of the fallback is.  Fallback (decided here, reported in bit 31 of entry 3, never an error): |F| < 2, or
//    std == 0, or lam_eff not a normal fp32 number (zero, denormal, inf) -> lam_eff = lam0, inv_lam_eff = 1.0f / lam0.  |F| = 0: std = 0.
//    One workgroup of 1 024 threads per instance, as ess_lambda.hip: thread t keeps the costs t, t + 1024, ... in registers up to
//    N = 65 536 (64 per thread), so both passes read HBM once; beyond that the second pass re-reads them (L2-resident).  Sums: fp64
//    per thread in ascending index order, wave butterflies, the 16 wave sums through LDS, added in ascending order by every thread
//    -- no atomics, no flags: the row is a function of the costs alone, every thread holds the same sums, and all control flow is
//    workgroup-uniform.  No per-wave minima are read: the solver needs none.
// 2. The schedule launch.  One wave per instance: pass i's row sigma[i][0..31] of the table in device memory -> the block factors
//    Ls[e][h] = sigma I_4 (the layout step_begin_kernel's mppi_prep leaves: lower triangle, row-major) and a_cov[e][h] =
//    (sigma * sigma in fp32) I_4.  The table is formed on the host (fp64, rounded once): there is no pow on the device.
#include "covo_common.hpp"

constexpr int CS_THREADS = 1024;
constexpr int CS_WAVES = CS_THREADS / 64;
constexpr int CS_REG = 64;                          // costs per thread kept in registers
constexpr int CS_REG_MAX_N = CS_THREADS * CS_REG;   // 65 536

struct StdLds {
    double a[2][CS_WAVES], b[2][CS_WAVES];  // two wave-sum buffers, alternating: one barrier per reduction
};

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// (sum x, sum y) over the workgroup, identical in every thread; `flip` alternates between calls
__device__ __forceinline__ void cs_reduce2(double &x, double &y, StdLds &L, int &flip)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    x = wave_sum_f64(x);
    y = wave_sum_f64(y);
    if (lane == 0) {
        L.a[flip][wave] = x;
        L.b[flip][wave] = y;
    }
    __syncthreads();
    x = 0.0;
    y = 0.0;
#pragma unroll
    for (int i = 0; i < CS_WAVES; ++i) {
        x += L.a[flip][i];
        y += L.b[flip][i];
    }
    flip ^= 1;
}

__device__ __forceinline__ bool cs_finite(float c) { return fabsf(c) < __builtin_inff(); }  // (false for NaN)

// grid (1, instances); out: [instances][COVO_LAM_FLOATS] the temperature rows the update reads; pass_out: the same row again at
// pass_out[instance * pass_stride .. + 4] (the per-pass rows of covo_set_step_anneal), or null
// REG: N <= CS_REG_MAX_N, c[] holds this thread's costs (inf beyond N: not finite, not counted)
template <bool REG>
__global__ __launch_bounds__(CS_THREADS) void cost_standardise_kernel(const float *__restrict__ cost, int N, float lam0, float inv_lam0,
                                                                      float temp, float *__restrict__ out,
                                                                      float *__restrict__ pass_out, int pass_stride)
{
    __shared__ StdLds L;
    const int tid = threadIdx.x;
    int flip = 0;
    {
        const size_t y = blockIdx.y;
        cost += y * N;
        out += y * COVO_LAM_FLOATS;
        if (pass_out != nullptr) pass_out += y * pass_stride;
    }
    // ---- pass 1: the costs (into registers), the sum and the count of the finite ones
    float c[CS_REG];
    double s = 0.0, cnt = 0.0;
    if (REG) {
#pragma unroll
        for (int i = 0; i < CS_REG; ++i) {
            const int n = tid + i * CS_THREADS;
            c[i] = (n < N) ? cost[n] : __builtin_inff();
            if (cs_finite(c[i])) {
                s += (double)c[i];
                cnt += 1.0;
            }
        }
    } else {
        for (int n = tid; n < N; n += CS_THREADS) {
            const float cn = cost[n];
            if (cs_finite(cn)) {
                s += (double)cn;
                cnt += 1.0;
            }
        }
    }
    cs_reduce2(s, cnt, L, flip);
    const double mean = cnt > 0.0 ? s / cnt : 0.0;
    // ---- pass 2: the squared deviations
    double q = 0.0, none = 0.0;
    if (REG) {
        // (an empty statement the compiler cannot see through: without it the 64 widened costs of pass 1 are kept alive next to c[],
        // and the kernel spills)
#pragma unroll
        for (int i = 0; i < CS_REG; ++i) asm volatile("" : "+v"(c[i]));
#pragma unroll
        for (int i = 0; i < CS_REG; ++i) {
            if (i * CS_THREADS < N && cs_finite(c[i])) {  // (the first test is workgroup-uniform)
                const double d = (double)c[i] - mean;
                q += d * d;
            }
        }
    } else {
        for (int n = tid; n < N; n += CS_THREADS) {
            const float cn = cost[n];
            if (cs_finite(cn)) {
                const double d = (double)cn - mean;
                q += d * d;
            }
        }
    }
    cs_reduce2(q, none, L, flip);
    const double sd = cnt > 0.0 ? sqrt(q / cnt) : 0.0;
    const float lam = (float)((double)temp * sd);
    // a normal fp32 number: judged on the widened value, so a flushed denormal cannot pass
    const double lamw = (double)lam;
    const bool normal = lamw >= 1.17549435082228750797e-38 && lamw < (double)__builtin_inff();
    const bool ok = cnt >= 2.0 && sd > 0.0 && normal;
    if (tid == 0) {
        const float r0 = ok ? lam : lam0;
        const float r1 = ok ? __fdiv_rn(1.0f, lam) : inv_lam0;
        const float r2 = (float)sd;
        const float r3 = __int_as_float((int)cnt | (ok ? 0 : (int)0x80000000u));
        out[0] = r0;
        out[1] = r1;
        out[2] = r2;
        out[3] = r3;
        if (pass_out != nullptr) {
            pass_out[0] = r0;
            pass_out[1] = r1;
            pass_out[2] = r2;
            pass_out[3] = r3;
        }
    }
}

int launch_cost_standardise(const float *cost, int N, int n_inst, float lam0, float temp, float *out, float *pass_out, int pass_stride,
                            hipStream_t s)
{
    const float inv_lam0 = 1.0f / lam0;  // the float the update at the configured lam multiplies by (reduce.hip: launch_softmax_reduce)
    if (N <= CS_REG_MAX_N)
        hipLaunchKernelGGL(cost_standardise_kernel<true>, dim3(1, n_inst), dim3(CS_THREADS), 0, s, cost, N, lam0, inv_lam0, temp, out,
                           pass_out, pass_stride);
    else
        hipLaunchKernelGGL(cost_standardise_kernel<false>, dim3(1, n_inst), dim3(CS_THREADS), 0, s, cost, N, lam0, inv_lam0, temp, out,
                           pass_out, pass_stride);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

// grid (instances), one wave each: lane l writes entries l, l + 64, ... of the instance's 512-float Ls and a_cov
__global__ __launch_bounds__(64) void anneal_schedule_kernel(const float *__restrict__ table, int pass, float *__restrict__ Ls,
                                                             float *__restrict__ a_cov)
{
    const float *row = table + (size_t)pass * COVO_H;
    const size_t base = (size_t)blockIdx.x * COVO_H * 16;
#pragma unroll
    for (int j = 0; j < COVO_H * 16 / 64; ++j) {
        const int idx = (int)threadIdx.x + 64 * j;
        const int h = idx >> 4, e = idx & 15;
        const float sg = row[h];
        const bool diag = (e % 5) == 0;
        Ls[base + idx] = diag ? sg : 0.0f;
        a_cov[base + idx] = diag ? __fmul_rn(sg, sg) : 0.0f;
    }
}

int launch_anneal_schedule(const float *table, int pass, float *Ls, float *a_cov, int n_inst, hipStream_t s)
{
    hipLaunchKernelGGL(anneal_schedule_kernel, dim3(n_inst), dim3(64), 0, s, table, pass, Ls, a_cov);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
