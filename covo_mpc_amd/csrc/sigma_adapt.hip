// sigma_adapt.hip -- the covariance of a reuse step that adapts (covo_set_step_sigma_adapt): the shifted blend of the
// covariance the previous step sampled from and the covariance its samples came back with.  With Sigma = L L^T, C the previous step's
// posterior covariance (post_cov.hip), S the shift of sigma_shift.hip (trailing 124 x 124 block up, the last stage's 4 x 4 marginal
// repeated, cross block zero) and 0 <= gamma < 1:
//   M = (1 - gamma) S(Sigma) + gamma S(C),   Sigma' = c M,   c such that log det Sigma' = 2 n log sample_sigma,   L' = chol(Sigma').
// S only re-indexes rows and columns: with rho(i) = i + 4 for i < 124 and rho(i) = i for the last stage,
//   S(X)[i][j] = X[rho(i)][rho(j)]   unless exactly one of i, j lies in the last stage (then 0),
// so S(L L^T) is a product of re-indexed rows of L and needs no Sigma in memory.
//
// One 512-thread workgroup per matrix; M lives in LDS as fp64 at the leading dimension of the finalize launch's factorisation (129).
//   form     the 36 lower 16 x 16 tiles over the 8 waves: tile (ti, tj) = rows rho(16 ti ..) of L times rows rho(16 tj ..) of L on
//            v_mfma_f64_16x16x4_f64, the fp32 operands read from global memory (the strict upper triangle of L_in counts as zero),
//            blended with C[rho(i)][rho(j)] (the lower triangle of S(C) is read), the cross block set to exact zero, each value
//            written to (i, j) and (j, i): M is fully symmetric, as chol128_lds_mfma needs it
//   factor   chol128_lds_mfma<129>
//   guard    all 128 pivots finite and > 0 and their log sum finite; else (C was not positive semidefinite, or not finite) the form
//            and factor phases run again at gamma = 0 without reading C -- the same code, hence the same bits as a gamma = 0 launch
//   scale    log det M from the fp64 diagonal -> sqrt(c), c
//   output   L' = sqrt(c) L_f, exact zeros above the diagonal and left of the last stage's block; Sigma' = c L_f L_f^T by MFMA tiles
//            from the fp64 factor, every off-diagonal tile also stored transposed, of a diagonal tile the lower part mirrored: Sigma'
//            is symmetric bit for bit, its cross block exact zeros; the row {fallback, c, log det M, 0}
// L_out may be L_in: every read of L_in (the guard's second form phase included) precedes a barrier that every store follows.
#include "covo_common.hpp"
#include "chol_lds.hpp"

namespace {

constexpr int SA_N = COVO_NA;            // 128
constexpr int SA_M = COVO_NA - COVO_DU;  // 124: where the last stage starts
constexpr int SA_LD = SA_N + 1;          // the finalize launch's leading dimension
constexpr int SA_THREADS = 512;
constexpr int SA_TILES = 36;             // lower 16 x 16 tiles of the 8 x 8 grid
constexpr size_t SA_LDS_BYTES = (size_t)SA_N * SA_LD * sizeof(double);

__device__ __forceinline__ int sa_rho(int i) { return i < SA_M ? i + COVO_DU : i; }
// exactly one of i, j in the last stage: S(.) is zero there
__device__ __forceinline__ bool sa_cross(int i, int j) { return (i >= SA_M) != (j >= SA_M); }

// lower tile t = 0 .. 35, enumerated by tile column: (ti, tj), tj <= ti
__device__ __forceinline__ void sa_tile(int t, int &ti, int &tj)
{
    tj = 0;
    int first = 0;
    while (first + (8 - tj) <= t) first += 8 - tj, ++tj;
    ti = tj + (t - first);
}

__device__ __forceinline__ double sa_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// M = (1 - gamma) S(L L^T) + gamma S(C) into Md (both triangles); use_c false: M = S(L L^T), C is not read
__device__ __forceinline__ void sa_form(double *__restrict__ Md, const float *__restrict__ Lg, const float *__restrict__ Cg, const bool use_c,
                                        const double gamma, const int wave, const int lo, const int hi)
{
    for (int t = wave; t < SA_TILES; t += SA_THREADS / 64) {
        int ti, tj;
        sa_tile(t, ti, tj);
        // S(C) in the accumulator's layout: register g of lane (lo, hi) is entry (16 ti + 4 g + hi, 16 tj + lo)
        float cv[4] = {0.f, 0.f, 0.f, 0.f};
        if (use_c) {
#pragma unroll
            for (int g = 0; g < 4; ++g) cv[g] = Cg[(size_t)sa_rho(16 * ti + 4 * g + hi) * SA_N + sa_rho(16 * tj + lo)];
        }
        // operands: lane (lo, hi) holds columns 16 q + 4 hi .. + 3 of its row of L (one float4); MFMA kk of block q multiplies
        // column 16 q + 4 hi + kk of both operands: the same column on both sides, every column once
        const int ra = sa_rho(16 * ti + lo), rb = sa_rho(16 * tj + lo);
        const int nq = tj + 2 < 8 ? tj + 2 : 8;  // the rows of the B operand end at column 16 tj + 19
        float4 av[8], bv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            av[q] = bv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < nq) {
                av[q] = *reinterpret_cast<const float4 *>(Lg + (size_t)ra * SA_N + 16 * q + 4 * hi);
                bv[q] = *reinterpret_cast<const float4 *>(Lg + (size_t)rb * SA_N + 16 * q + 4 * hi);
            }
        }
        chol_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (q < nq) {
                const int k = 16 * q + 4 * hi;
                const float a4[4] = {av[q].x, av[q].y, av[q].z, av[q].w}, b4[4] = {bv[q].x, bv[q].y, bv[q].z, bv[q].w};
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const double a = k + kk <= ra ? (double)a4[kk] : 0.0, b = k + kk <= rb ? (double)b4[kk] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = 16 * ti + 4 * g + hi, j = 16 * tj + lo;
            if (i >= j) {  // (a diagonal tile: its lower part, mirrored)
                double v = use_c ? fma(gamma, (double)cv[g], (1.0 - gamma) * acc[g]) : acc[g];
                if (sa_cross(i, j)) v = 0.0;
                Md[j * SA_LD + i] = v;
                Md[i * SA_LD + j] = v;
            }
        }
    }
}

__global__ __launch_bounds__(SA_THREADS) void sigma_adapt_kernel(const float *L_in, const float *__restrict__ C, const float gamma,
                                                                  const float sample_sigma, float *__restrict__ Sigma_out, float *L_out,
                                                                  float *__restrict__ rows_out)
{
    extern __shared__ __align__(16) double sa_lds[];
    __shared__ double sc[4];  // [0..1] the two waves' log sums, [2] sqrt(c), [3] c
    __shared__ int okf[2];    // the two waves' "every pivot finite and positive"
    double *Md = sa_lds;      // [128][129]: M, then its factor (element (r, c), r >= c, at Md[c * 129 + r])
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lo = lane & 15, hi = lane >> 4;
    const size_t mat = (size_t)blockIdx.x * SA_N * SA_N;
    const float *Lg = L_in + mat, *Cg = C + mat;

    int fallback = 0;
    double logsum = 0.0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        sa_form(Md, Lg, Cg, attempt == 0 && gamma > 0.0f, (double)gamma, wave, lo, hi);
        chol128_lds_mfma<SA_LD>(Md, tid);  // (a barrier first and last)
        if (tid < SA_N) {
            const double dg = Md[tid * SA_LD + tid];
            const bool good = dg > 0.0 && dg < __builtin_inf();  // (false for a NaN)
            const double s = sa_wave_sum(good ? log(dg) : 0.0);
            const bool all_good = __ballot(good) == ~0ull;
            if (lane == 0) sc[wave] = s, okf[wave] = all_good ? 1 : 0;
        }
        __syncthreads();
        logsum = sc[0] + sc[1];
        const bool ok = okf[0] && okf[1] && logsum == logsum && fabs(logsum) < __builtin_inf();
        if (ok || attempt == 1) break;  // (uniform: every thread reads the same words)
        fallback = 1;
    }
    // ---- scale: log det Sigma' = 2 sum log L_ii + n log c = 2 n log sigma
    if (tid == 0) {
        const double rc = exp(log((double)sample_sigma) - logsum / (double)SA_N);
        sc[2] = rc;
        sc[3] = rc * rc;
    }
    __syncthreads();
    const double rc = sc[2], cc = sc[3];
    float *Lo = L_out + mat, *So = Sigma_out + mat;
    if (tid == 0 && rows_out) {
        *reinterpret_cast<float4 *>(rows_out + (size_t)blockIdx.x * 4) = make_float4((float)fallback, (float)cc, (float)(2.0 * logsum), 0.f);
    }

    // ---- L': rows of float4
    for (int idx = tid; idx < SA_N * (SA_N / 4); idx += SA_THREADS) {
        const int i = idx / (SA_N / 4), k4 = (idx - i * (SA_N / 4)) * 4;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = k4 + q;
            v[q] = (k <= i && !sa_cross(i, k)) ? (float)(rc * Md[k * SA_LD + i]) : 0.0f;
        }
        *reinterpret_cast<float4 *>(Lo + (size_t)i * SA_N + k4) = make_float4(v[0], v[1], v[2], v[3]);
    }

    // ---- Sigma' = c L_f L_f^T: tile (ti, tj) sums over the columns k < 16 tj + 16 (the entries above the factor's diagonal are
    // don't-cares of the factorisation: masked)
    for (int t = wave; t < SA_TILES; t += SA_THREADS / 64) {
        int ti, tj;
        sa_tile(t, ti, tj);
        const int ra = 16 * ti + lo, rb = 16 * tj + lo;
        chol_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < 16 * tj + 16; k0 += 4) {
            const int k = k0 + hi;
            const double a = k <= ra ? Md[k * SA_LD + ra] : 0.0, b = k <= rb ? Md[k * SA_LD + rb] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = 16 * ti + 4 * g + hi, j = 16 * tj + lo;
            if (i >= j) {
                const float o = sa_cross(i, j) ? 0.0f : (float)(cc * acc[g]);
                So[(size_t)i * SA_N + j] = o;
                So[(size_t)j * SA_N + i] = o;
            }
        }
    }
}

// a refresh step's rows: no fallback, scale 1
__global__ void sigma_adapt_rows_idle_kernel(float *__restrict__ rows, const int n)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) *reinterpret_cast<float4 *>(rows + (size_t)e * 4) = make_float4(0.f, 1.f, 0.f, 0.f);
}

}  // namespace

int launch_sigma_adapt_idle(float *rows_out, int n_inst, hipStream_t s)
{
    hipLaunchKernelGGL(sigma_adapt_rows_idle_kernel, dim3((n_inst + 63) / 64), dim3(64), 0, s, rows_out, n_inst);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_sigma_adapt(const float *L_in, const float *C, int batch, float gamma, float sample_sigma, float *Sigma_out, float *L_out,
                       float *rows_out, hipStream_t s)
{
    static unsigned long long attr_devices = 0;  // (per device: covo_first_on_device)
    if (covo_first_on_device(attr_devices)) {
        COVO_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(sigma_adapt_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)SA_LDS_BYTES));
    }
    hipLaunchKernelGGL(sigma_adapt_kernel, dim3(batch), dim3(SA_THREADS), SA_LDS_BYTES, s, L_in, C, gamma, sample_sigma, Sigma_out, L_out,
                       rows_out);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
