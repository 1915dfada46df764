// cma_path.hip -- the step size of the CMA controller (COVO_MODE_CMA, covo_set_step_cma): cumulative step-size
// adaptation in Cholesky-whitened coordinates, and the scaling of the shape sigma_adapt.hip has just left.  Per instance, with L the
// factor the previous step sampled from (fp32, lower, step size included), d that step's mean displacement and W its weight sum
// (post_cov.hip's side row), ess its effective sample size (the diagnostics' row), p the evolution path and log s the log step
// size (fp64, in place), N the samples of a step and n = 128:
//   z = L^-1 d                                      forward substitution, fp64
//   mu_eff = clamp(ess, 1, N),  c_s = (mu_eff + 2) / (n + mu_eff + 5),
//   d_s = damping (1 + 2 max(0, sqrt((mu_eff - 1) / (n + 1)) - 1) + c_s)
//   p <- (1 - c_s) p + sqrt(c_s (2 - c_s) mu_eff) z
//   log s <- clamp(log s + (c_s / d_s) (|p| / chi_n - 1), log s_min, log s_max),   chi_n = sqrt(n) (1 - 1/(4n) + 1/(21 n^2))
//   L' = fp32(s L_hat),  Sigma' = fp32(s^2 Sigma_hat)                              each rounded once from fp64
// p is not shifted between steps: in whitened coordinates it is treated as isotropic.
// Fall-backs, per instance, in the row's flag word and never an error:
//   1  p and log s are left as they are: W is not a positive finite number, ess or an entry of d or z is not finite, or a diagonal
//      entry of L is not positive and finite
//   2  the clamp was hit
//   4  the shape kernel fell back (its row's first word)
// The state on entry is mended before use: a log s that is not finite counts as 0 and is then held inside [log s_min, log s_max]; a
// path with an entry that is not finite counts as 0.  So s always lies in [s_min, s_max] -- on a fall-back too -- and L' is finite
// whenever L_hat is.  p and log s are stored back on every path: on a fall-back they are the (mended) entry values.
// step_size == 0: s = 1, the two matrices are copied, p and log s are not touched and the row is neutral (flag 4 still reported).
//
// One 256-thread workgroup per instance.
//   load     L into LDS, all of it (64 KiB fp32), transposed and rotated -- element (i, j) at j * 128 + ((i + j) & 127) -- so that
//            the substitution reads a column with consecutive lanes on consecutive banks; the float4 loads of a row are coalesced
//   solve    wave 0 alone: lane l holds the residuals of rows l and l + 64 in registers; step j broadcasts r_j / L_jj with
//            v_readlane and every lane folds column j in: 128 dependent steps, no barrier inside
//   norms    |z|^2 and |p|^2 by wave_reduce.hpp's wave64_allsum: no atomics, no LDS traffic
//   scale    all four waves stream L_hat -> L_out and Sigma_hat -> Sigma_out as float4, elementwise: zeros stay exact zeros and a
//            symmetric Sigma_hat stays symmetric bit for bit
// L_out may be L_prev (every read of L_prev precedes the barrier every store follows) and Sigma_out may be Sigma_hat (elementwise).
#include "covo_common.hpp"
#include "wave_reduce.hpp"

namespace {

constexpr int CP_N = COVO_NA;  // 128
constexpr int CP_THREADS = 256;
constexpr size_t CP_LDS_BYTES = (size_t)CP_N * CP_N * sizeof(float);  // 64 KiB

__device__ __forceinline__ int cp_at(int i, int j) { return j * CP_N + ((i + j) & (CP_N - 1)); }
__device__ __forceinline__ bool cp_finite(double v) { return fabs(v) < __builtin_inf(); }  // (false for a NaN)

__global__ __launch_bounds__(CP_THREADS) void cma_path_kernel(const CmaPathDesc d)
{
    extern __shared__ __align__(16) float cp_L[];  // [128][128], cp_at
    __shared__ double cp_s;                        // the step size the scaling applies
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int e = blockIdx.x;
    const size_t mat = (size_t)e * CP_N * CP_N;
    const int shape_fell_back = (d.shape_rows != nullptr && d.shape_rows[(size_t)e * COVO_SIGMA_ADAPT_FLOATS] != 0.0f) ? 4 : 0;

    if (!d.step_size) {  // (uniform)
        if (tid == 0) {
            float4 *row = reinterpret_cast<float4 *>(d.rows_out + (size_t)e * COVO_CMA_FLOATS);
            row[0] = make_float4(1.f, 0.f, 0.f, 0.f);
            row[1] = make_float4(0.f, 0.f, 0.f, (float)shape_fell_back);
            cp_s = 1.0;
        }
    } else {
        // ---- load: thread t takes the float4 at row idx / 32, columns 4 (idx % 32) ..
        const float *Lg = d.L_prev + mat;
        for (int idx = tid; idx < CP_N * (CP_N / 4); idx += CP_THREADS) {
            const int i = idx >> 5, k4 = (idx & 31) * 4;
            const float4 v = *reinterpret_cast<const float4 *>(Lg + (size_t)i * CP_N + k4);
            cp_L[cp_at(i, k4 + 0)] = v.x;
            cp_L[cp_at(i, k4 + 1)] = v.y;
            cp_L[cp_at(i, k4 + 2)] = v.z;
            cp_L[cp_at(i, k4 + 3)] = v.w;
        }
        __syncthreads();
        if (wave == 0) {
            const float *aux = d.aux + (size_t)e * d.aux_stride;
            const double W = (double)aux[CP_N], ess = (double)d.ess[(size_t)e * d.ess_stride];
            const double d0 = (double)aux[lane], d1 = (double)aux[lane + 64];
            const double g0 = (double)cp_L[cp_at(lane, lane)], g1 = (double)cp_L[cp_at(lane + 64, lane + 64)];
            bool good = W > 0.0 && cp_finite(W) && cp_finite(ess);
            good = good && __ballot(cp_finite(d0) && cp_finite(d1) && g0 > 0.0 && cp_finite(g0) && g1 > 0.0 && cp_finite(g1)) == ~0ull;
            // ---- solve: r holds d - (columns folded in so far) z
            double r0 = d0, r1 = d1, z0 = 0.0, z1 = 0.0;
            for (int j = 0; j < 64; ++j) {
                const double zj = wr::bcast_lane(r0, j) / (double)cp_L[cp_at(j, j)];
                if (lane == j) z0 = zj;
                if (lane > j) r0 = fma(-(double)cp_L[cp_at(lane, j)], zj, r0);
                r1 = fma(-(double)cp_L[cp_at(lane + 64, j)], zj, r1);
            }
            for (int j = 64; j < CP_N; ++j) {
                const double zj = wr::bcast_lane(r1, j - 64) / (double)cp_L[cp_at(j, j)];
                if (lane == j - 64) z1 = zj;
                if (lane > j - 64) r1 = fma(-(double)cp_L[cp_at(lane + 64, j)], zj, r1);
            }
            good = good && __ballot(cp_finite(z0) && cp_finite(z1)) == ~0ull;
            double *pg = d.p + (size_t)e * CP_N;
            double p0 = pg[lane], p1 = pg[lane + 64];
            double ls = d.log_s[e];
            // the state as a caller may hand it over: a path with an entry that is not finite counts as 0, so does such a log s, and
            // log s is held inside its bounds before anything uses it -- also on a fall-back, which scales by exp(log s)
            if (__ballot(cp_finite(p0) && cp_finite(p1)) != ~0ull) p0 = p1 = 0.0;
            if (!cp_finite(ls)) ls = 0.0;
            ls = fmin(fmax(ls, (double)d.log_s_min), (double)d.log_s_max);
            int flags = shape_fell_back;
            double znorm = 0.0, mu_eff = 0.0, cs = 0.0, ds = 0.0;
            if (good) {  // (uniform: ballots and broadcast words)
                const double n = (double)CP_N;
                znorm = sqrt(wr::wave64_allsum(z0 * z0 + z1 * z1));
                mu_eff = fmin(fmax(ess, 1.0), (double)d.n_samples);
                cs = (mu_eff + 2.0) / (n + mu_eff + 5.0);
                ds = (double)d.damping * (1.0 + 2.0 * fmax(0.0, sqrt((mu_eff - 1.0) / (n + 1.0)) - 1.0) + cs);
                const double keep = 1.0 - cs, gain = sqrt(cs * (2.0 - cs) * mu_eff);
                p0 = keep * p0 + gain * z0;
                p1 = keep * p1 + gain * z1;
            } else {
                flags |= 1;
            }
            const double pnorm = sqrt(wr::wave64_allsum(p0 * p0 + p1 * p1));
            if (good) {
                const double n = (double)CP_N, chi = sqrt(n) * (1.0 - 1.0 / (4.0 * n) + 1.0 / (21.0 * n * n));
                const double raw = ls + (cs / ds) * (pnorm / chi - 1.0);
                ls = fmin(fmax(raw, (double)d.log_s_min), (double)d.log_s_max);
                if (ls != raw) flags |= 2;
            }
            // (on a fall-back these are the entry values again, bit for bit unless the lines above had to mend them)
            pg[lane] = p0;
            pg[lane + 64] = p1;
            const double sv = exp(ls);
            if (lane == 0) {
                d.log_s[e] = ls;
                float4 *row = reinterpret_cast<float4 *>(d.rows_out + (size_t)e * COVO_CMA_FLOATS);
                row[0] = make_float4((float)sv, (float)ls, (float)pnorm, (float)znorm);
                row[1] = make_float4((float)mu_eff, (float)cs, (float)ds, (float)flags);
                cp_s = sv;
            }
        }
    }
    __syncthreads();
    // ---- scale: L' = fp32(s L_hat), Sigma' = fp32(s^2 Sigma_hat)
    const double sv = cp_s, sv2 = sv * sv;
    const float4 *Lh = reinterpret_cast<const float4 *>(d.L_hat + mat), *Sh = reinterpret_cast<const float4 *>(d.Sigma_hat + mat);
    float4 *Lo = reinterpret_cast<float4 *>(d.L_out + mat), *So = reinterpret_cast<float4 *>(d.Sigma_out + mat);
    for (int idx = tid; idx < CP_N * (CP_N / 4); idx += CP_THREADS) {
        const float4 l = Lh[idx], c = Sh[idx];
        Lo[idx] = make_float4((float)(sv * (double)l.x), (float)(sv * (double)l.y), (float)(sv * (double)l.z), (float)(sv * (double)l.w));
        So[idx] = make_float4((float)(sv2 * (double)c.x), (float)(sv2 * (double)c.y), (float)(sv2 * (double)c.z), (float)(sv2 * (double)c.w));
    }
}

// the state of a reset and the step that follows it: L = sigma I, Sigma = sigma^2 I (sigma^2 rounded once from fp64), p = 0,
// log s = 0, the neutral row; any of the targets may be null
__global__ __launch_bounds__(CP_THREADS) void cma_reset_kernel(const float sigma, float *L, float *Sigma, double *p, double *log_s, float *rows)
{
    const int tid = threadIdx.x, e = blockIdx.x;
    const size_t mat = (size_t)e * CP_N * CP_N;
    const float s2 = (float)((double)sigma * (double)sigma);
    for (int idx = tid; idx < CP_N * (CP_N / 4); idx += CP_THREADS) {
        const int i = idx >> 5, k4 = (idx & 31) * 4, q = i - k4;  // the diagonal lies in this float4 iff 0 <= q < 4
        if (L) reinterpret_cast<float4 *>(L + mat)[idx] = make_float4(q == 0 ? sigma : 0.f, q == 1 ? sigma : 0.f, q == 2 ? sigma : 0.f, q == 3 ? sigma : 0.f);
        if (Sigma) reinterpret_cast<float4 *>(Sigma + mat)[idx] = make_float4(q == 0 ? s2 : 0.f, q == 1 ? s2 : 0.f, q == 2 ? s2 : 0.f, q == 3 ? s2 : 0.f);
    }
    if (p && tid < CP_N) p[(size_t)e * CP_N + tid] = 0.0;
    if (log_s && tid == 0) log_s[e] = 0.0;
    if (rows && tid == 0) {
        float4 *row = reinterpret_cast<float4 *>(rows + (size_t)e * COVO_CMA_FLOATS);
        row[0] = make_float4(1.f, 0.f, 0.f, 0.f);
        row[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

}  // namespace

int launch_cma_reset(float sample_sigma, int batch, float *L, float *Sigma, double *p, double *log_s, float *rows, hipStream_t s)
{
    hipLaunchKernelGGL(cma_reset_kernel, dim3(batch), dim3(CP_THREADS), 0, s, sample_sigma, L, Sigma, p, log_s, rows);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_cma_path(const CmaPathDesc &d, hipStream_t s)
{
    static unsigned long long attr_devices = 0;  // (per device: covo_first_on_device)
    if (covo_first_on_device(attr_devices)) {
        COVO_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(cma_path_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)CP_LDS_BYTES));
    }
    hipLaunchKernelGGL(cma_path_kernel, dim3(d.batch), dim3(CP_THREADS), CP_LDS_BYTES, s, d);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
