// sigma_shift.hip -- the covariance of a reuse step (covo_set_step_sigma_period): the previous step's factor moved one
// stage down the horizon, as the mean is.  With Sigma = L L^T, n = 128 = 32 stages x 4 actions:
//   Sigma' = c S(Sigma),   S(Sigma)[0:124, 0:124] = Sigma[4:128, 4:128],   S(Sigma)[124:, 124:] = Sigma[124:, 124:],   cross block 0,
//   c such that log det Sigma' = 2 n log sample_sigma.
// The factor needs neither Sigma nor a fresh factorisation: with L partitioned after its first 4 columns,
//   Sigma[4:, 4:] = L22 L22^T + L21 L21^T,
// so the leading 124 x 124 block of L' is the rank-4 Cholesky UPDATE of L22 by the four columns of L21 (no downdate: unconditionally
// stable); the trailing 4 x 4 block is the factor of B = L[124:, :] L[124:, :]^T.
//
// One 512-thread workgroup per matrix, L22 resident in LDS as fp64 (124 rows, leading dimension 125: 121 KiB of the CU's 160), all
// arithmetic fp64, every output rounded to fp32 once.
//   load     all waves: L22 -> LDS (upper triangle zero); wave 0: the four update vectors x^j = L[4:, j] into registers, rows l and
//            l + 64 per lane; wave 1: B, its 4 x 4 factor -> LDS
//   update   wave 0 alone.  The pivots serialise the columns; rows are the parallel axis, and ONE wave holds all 124 rows, so the
//            pivot row's x reaches the other rows by v_readlane and no barrier or LDS round trip sits on the chain.  Within column k
//            the four rotations depend on each other only through L_kk, whose squares accumulate: with a_j = x^j_k,
//              d_0 = L_kk^2, d_{j+1} = d_j + a_j^2, r_j = sqrt(d_j)          (r_0 = L_kk, the new diagonal is r_4)
//            the four reciprocal square roots are independent chains, and the rotations
//              r = sqrt(L_kk^2 + x_k^2), c_k = r / L_kk, s_k = x_k / L_kk, L_ik <- (L_ik + s_k x_i) / c_k, x_i <- c_k x_i - s_k L_ik
//            applied for j = 0 .. 3 collapse to
//              p_0 = L_ik r_0, p_{j+1} = p_j + a_j x^j_i,  x^j_i <- (r_{j+1} / r_j) x^j_i - (a_j / (r_j r_{j+1})) p_{j+1},  L_ik <- p_4 / r_4
//            (the same numbers: l after rotation j is p_{j+1} / r_{j+1}).  The next column's L_kk and L_ik are loaded ahead.
//   scale    log det from the diagonal (fp64, before any rounding) -> sqrt(c), c
//   output   all waves: L' = sqrt(c) (updated L22 | 0 ; 0 | chol B) with an exactly zero strict upper triangle; Sigma' = c L22' L22'^T by
//            4 x 4 register tiles of the lower triangle, k ascending, each tile also stored transposed (Sigma' symmetric bit for bit),
//            the cross block exactly zero, the last block c B.
// L_out may be L_in (the step shifts its factor in place): every read of L_in precedes the first barrier, every store follows it.
#include "covo_common.hpp"

namespace {

constexpr int SS_N = COVO_NA;            // 128
constexpr int SS_M = COVO_NA - COVO_DU;  // 124: the order of L22
constexpr int SS_LD = SS_M + 1;          // fp64 leading dimension 125 = 250 dwords: a column read by 32 lanes hits 32 distinct bank pairs
constexpr int SS_THREADS = 512;
constexpr int SS_TILES_1D = SS_M / 4;    // 31 tiles of 4 rows
constexpr int SS_TILES = SS_TILES_1D * (SS_TILES_1D + 1) / 2;  // 496 lower tiles <= SS_THREADS
constexpr size_t SS_LDS_DOUBLES = (size_t)SS_M * SS_LD + 16 + 16 + 8;
static_assert(SS_TILES <= SS_THREADS, "one Sigma tile per thread");

__device__ __forceinline__ double readlane_f64(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// columns [K0, K1) of the update; HALF: which of the lane's two rows holds the pivot row (k >> 6).  Rows below 64 are finished once
// k >= 64: the second half touches the upper rows only.
template <int HALF>
__device__ __forceinline__ void update_columns(double *__restrict__ Ld, const int lane, const int k0, const int k1, double (&x)[2][4])
{
    const int i0 = lane, i1 = lane + 64;
    const bool row1 = i1 < SS_M;
    // column k's operands, loaded one column ahead (they are untouched by the columns before k)
    double lkk = Ld[k0 * SS_LD + k0];
    double l0 = HALF == 0 ? Ld[i0 * SS_LD + k0] : 0.0;
    double l1 = row1 ? Ld[i1 * SS_LD + k0] : 0.0;
    for (int k = k0; k < k1; ++k) {
        const int kn = k + 1 < k1 ? k + 1 : k;
        const double lkk_n = Ld[kn * SS_LD + kn];
        const double l0_n = HALF == 0 ? Ld[i0 * SS_LD + kn] : 0.0;
        const double l1_n = row1 ? Ld[i1 * SS_LD + kn] : 0.0;
        double a[4], d[5], ir[5], r[5];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = readlane_f64(x[HALF][j], k & 63);
        d[0] = lkk * lkk;
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j + 1] = fma(a[j], a[j], d[j]);
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            ir[j] = rsqrt(d[j]);
            r[j] = d[j] * ir[j];
        }
        r[0] = lkk;
        double al[4], be[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            al[j] = r[j + 1] * ir[j];
            be[j] = a[j] * ir[j] * ir[j + 1];
        }
        if (HALF == 0) {
            double p = l0 * r[0];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                p = fma(a[j], x[0][j], p);
                x[0][j] = al[j] * x[0][j] - be[j] * p;
            }
            if (i0 >= k) Ld[i0 * SS_LD + k] = p * ir[4];  // (row k itself: p = d_4, the new diagonal r_4)
        }
        {
            double p = l1 * r[0];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                p = fma(a[j], x[1][j], p);
                x[1][j] = al[j] * x[1][j] - be[j] * p;
            }
            if (row1 && i1 >= k) Ld[i1 * SS_LD + k] = p * ir[4];
        }
        lkk = lkk_n;
        l0 = l0_n;
        l1 = l1_n;
    }
}

__global__ __launch_bounds__(SS_THREADS) void sigma_shift_kernel(const float *L_in, const float sample_sigma, float *__restrict__ Sigma_out,
                                                                  float *L_out)
{
    extern __shared__ __align__(16) double ss_lds[];
    double *Ld = ss_lds;                    // [124][125] L22, then the updated block
    double *Tb = Ld + SS_M * SS_LD;         // [4][4] chol(B), lower
    double *Bb = Tb + 16;                   // [4][4] B
    double *sc = Bb + 16;                   // [0..1] the two waves' log sums, [2] sqrt(c), [3] c
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t mat = (size_t)blockIdx.x * SS_N * SS_N;
    const float *Lg = L_in + mat;

    // ---- load: L22[i][k] = L[4 + i][4 + k] for k <= i, zero above
    for (int idx = tid; idx < SS_M * SS_M; idx += SS_THREADS) {
        const int i = idx / SS_M, k = idx - i * SS_M;
        Ld[i * SS_LD + k] = k <= i ? (double)Lg[(size_t)(i + COVO_DU) * SS_N + (k + COVO_DU)] : 0.0;
    }
    double x[2][4];
    if (wave == 0) {
#pragma unroll
        for (int hrow = 0; hrow < 2; ++hrow) {
            const int i = lane + 64 * hrow;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < SS_M) v = *reinterpret_cast<const float4 *>(Lg + (size_t)(i + COVO_DU) * SS_N);
            x[hrow][0] = v.x;
            x[hrow][1] = v.y;
            x[hrow][2] = v.z;
            x[hrow][3] = v.w;
        }
    } else if (wave == 1) {
        // B[a][b] = sum_k L[124 + a][k] L[124 + b][k] (lower rows: the entries right of the diagonal are not read), then its factor
        double part[10];
#pragma unroll
        for (int q = 0; q < 10; ++q) part[q] = 0.0;
#pragma unroll
        for (int hk = 0; hk < 2; ++hk) {
            const int k = lane + 64 * hk;
            double row[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) row[a] = k <= SS_M + a ? (double)Lg[(size_t)(SS_M + a) * SS_N + k] : 0.0;
            int q = 0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) part[q] = fma(row[a], row[b], part[q]), ++q;
        }
        double B[4][4], T[4][4];
        {
            int q = 0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) B[a][b] = B[b][a] = wave_sum_f64(part[q]), ++q;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) T[a][b] = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double dsum = B[c][c];
#pragma unroll
            for (int m = 0; m < c; ++m) dsum -= T[c][m] * T[c][m];
            T[c][c] = sqrt(dsum);
            const double inv = 1.0 / T[c][c];
#pragma unroll
            for (int a = c + 1; a < 4; ++a) {
                double v = B[a][c];
#pragma unroll
                for (int m = 0; m < c; ++m) v -= T[a][m] * T[c][m];
                T[a][c] = v * inv;
            }
        }
        if (lane < 16) {
            double tv = 0.0, bv = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (lane == a * 4 + b) tv = T[a][b], bv = B[a][b];
            Tb[lane] = tv;
            Bb[lane] = bv;
        }
    }
    __syncthreads();

    // ---- update: wave 0 alone, the other waves wait at the barrier
    if (wave == 0) {
        update_columns<0>(Ld, lane, 0, 64, x);
        update_columns<1>(Ld, lane, 64, SS_M, x);
    }
    __syncthreads();

    // ---- scale: log det Sigma' = 2 sum log L'_ii + n log c = 2 n log sigma
    if (tid < SS_N) {
        const double dg = tid < SS_M ? Ld[tid * SS_LD + tid] : Tb[(tid - SS_M) * 5];
        const double s = wave_sum_f64(log(dg));
        if (lane == 0) sc[wave] = s;
    }
    __syncthreads();
    if (tid == 0) {
        const double rc = exp(log((double)sample_sigma) - (sc[0] + sc[1]) / (double)SS_N);
        sc[2] = rc;
        sc[3] = rc * rc;
    }
    __syncthreads();
    const double rc = sc[2], cc = sc[3];
    float *Lo = L_out + mat, *So = Sigma_out + mat;

    // ---- L': rows of float4
    for (int idx = tid; idx < SS_N * (SS_N / 4); idx += SS_THREADS) {
        const int i = idx / (SS_N / 4), k4 = (idx - i * (SS_N / 4)) * 4;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = k4 + q;
            double e = 0.0;
            if (k <= i) {
                if (i < SS_M) e = Ld[i * SS_LD + k];
                else if (k >= SS_M) e = Tb[(i - SS_M) * 4 + (k - SS_M)];
            }
            v[q] = k <= i ? (float)(rc * e) : 0.0f;
        }
        *reinterpret_cast<float4 *>(Lo + (size_t)i * SS_N + k4) = make_float4(v[0], v[1], v[2], v[3]);
    }

    // ---- Sigma': the cross block and the last block (rows 124 .. 127 whole, columns 124 .. 127 of the rows above)
    for (int idx = tid; idx < 4 * (SS_N / 4) + SS_M; idx += SS_THREADS) {
        if (idx < 4 * (SS_N / 4)) {
            const int a = idx / (SS_N / 4), k4 = (idx - a * (SS_N / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k4 == SS_M) v = make_float4((float)(cc * Bb[a * 4 + 0]), (float)(cc * Bb[a * 4 + 1]), (float)(cc * Bb[a * 4 + 2]),
                                            (float)(cc * Bb[a * 4 + 3]));
            *reinterpret_cast<float4 *>(So + (size_t)(SS_M + a) * SS_N + k4) = v;
        } else {
            const int i = idx - 4 * (SS_N / 4);
            *reinterpret_cast<float4 *>(So + (size_t)i * SS_N + SS_M) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }

    // ---- Sigma'[0:124, 0:124] = c L22' L22'^T: tile (tr, tc), tc <= tr, enumerated column-major so that the lanes of a wave share
    // their trip count 4 tc + 4 (the terms k > min(s, t) are exact zeros of the upper triangle)
    if (tid < SS_TILES) {
        int tc = 0, first = 0;
        while (first + (SS_TILES_1D - tc) <= tid) first += SS_TILES_1D - tc, ++tc;
        const int tr = tc + (tid - first);
        const double *rs = Ld + (size_t)(4 * tr) * SS_LD, *rt = Ld + (size_t)(4 * tc) * SS_LD;
        double acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
        const int kend = 4 * tc + 4;
        for (int k = 0; k < kend; ++k) {
            double u[4], w[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) u[a] = rs[a * SS_LD + k], w[a] = rt[a * SS_LD + k];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(u[a], w[b], acc[a][b]);
        }
        float o[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) o[a][b] = (float)(cc * acc[a][b]);
        if (tr == tc) {  // a diagonal tile: (a, b) and (b, a) are the same products in the same order; store one of them for both
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = a + 1; b < 4; ++b) o[a][b] = o[b][a];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
            *reinterpret_cast<float4 *>(So + (size_t)(4 * tr + a) * SS_N + 4 * tc) = make_float4(o[a][0], o[a][1], o[a][2], o[a][3]);
        if (tr != tc) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                *reinterpret_cast<float4 *>(So + (size_t)(4 * tc + b) * SS_N + 4 * tr) = make_float4(o[0][b], o[1][b], o[2][b], o[3][b]);
        }
    }
}

}  // namespace

int launch_sigma_shift(const float *L_in, int batch, float sample_sigma, float *Sigma_out, float *L_out, hipStream_t s)
{
    const size_t lds = SS_LDS_DOUBLES * sizeof(double);
    static unsigned long long attr_devices = 0;  // (per device: covo_first_on_device)
    if (covo_first_on_device(attr_devices)) {
        COVO_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(sigma_shift_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    hipLaunchKernelGGL(sigma_shift_kernel, dim3(batch), dim3(SS_THREADS), lds, s, L_in, sample_sigma, Sigma_out, L_out);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
