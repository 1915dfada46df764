// sigma_nodes.hip -- covo-online in spline-node space (covo_set_step_sigma_nodes, covo_sigma_nodes, covo_noise_factor_philox;
// DESIGN.md 4.30): CoVO's optimal covariance of the NODE-parameterised problem J(mu + (W (x) I_4) e), and the sampler for its factor.
//
//   R_M   = P^T sym(R) P,   P = W (x) I_4 [128][d],  d = 4 M,  W [32][M] the interpolation weights (controllers/_options.py: node_basis)
//   Sig_M = optimize_sigma(R_M) in d dimensions (covo.py:116-132 with element_num = d): log det Sig_M = 2 d log sigma
//   L_M   = chol(Sig_M),  G = fp32(P L_M) [128][d],  a_cov = fp32(P Sig_M P^T) [128][128] of rank d
//   a[h][n] = clip(mu[h] + G[(h, .), :] eps(n)),  eps = the first M normal4 of the stream noise_nodes / the block-diagonal kernel draw
//
// sigma_nodes_kernel: one 256-thread workgroup per instance, fp64, everything in LDS (d <= 64: 134 KiB of the CU's 160), ONE launch
// in the place of the Sigma chain and its finalize launch.  R is read once, in four 32-row chunks; P^T R P is accumulated per chunk
// (T = R_chunk P, then A += P_chunk^T T) in plain fp64 FMAs -- under 1 M multiply-adds -- and symmetrised afterwards, which is
// P^T sym(R) P up to rounding and symmetric bit for bit.  The eigensolver is sigma.hip's one-sided (Hestenes) cyclic block Jacobi on
// R_M + shift I (Gershgorin shift: eigenvalues >= 1, lam_k = |g_k| - shift, one matrix stored) at a run-time d: M column blocks of 4, a
// block pair in the registers of a 16-lane group (lane l owns rows l + 16 i), block round-robin over M blocks padded to an even count
// -- the partner of the phantom block has a bye: it loads zeros for it, rotates by the identity and stores nothing.  Then the spectrum
// map, Sig_M = H H^T (bit-symmetric: entry (r, c) and (c, r) run the same fma chain), the LDS Cholesky (chol_lds.hpp where d is a
// multiple of 8, the plain right-looking one else), G, P Sig_M P^T (lower triangle computed, mirrored) and the side row.
//
// Fallback, decided here and reported in the side row's flags, never an error: an R_M that is not finite, a sweep limit reached, a
// factor with a non-positive pivot -> that instance gets Sig_M = sigma^2 I_d.  Plain arithmetic on whatever R holds: nothing faults.
//
// LDS banks: the work matrices are column-major with stride 64 doubles; a 16-lane group reads 16 consecutive doubles of one column
// (conflict-free inside the group), two groups of one 32-lane half may meet on a bank (2-way) -- the sweep is latency-bound at these
// sizes (at most 8 of 16 groups busy), so the columns are not padded.  All LDS is dynamic, every carve offset a multiple of 16 bytes.
#include "covo_common.hpp"
#include <cstdlib>
#include "wave_reduce.hpp"
#include "chol_lds.hpp"
#include "rng_device.hpp"

constexpr int SN_THREADS = 256;
constexpr int SN_LD = 64;          // column stride of the d x d work matrices (doubles)
constexpr int SN_WLD = 16;         // row stride of W in LDS: Wl[h][m], zero for m >= M
constexpr int SN_MAX_SWEEPS = 16;
constexpr double SN_TOL = 1e-12;   // |g_p.g_q| <= tol |g_p||g_q| for every pair of a whole sweep (sigma.hip: SG_TOL)
// LDS carve (doubles): Wl, C (Jacobi work matrix, then L_M), S (P^T R P, then Sig_M), scratch (R chunk + T chunk; later Sig_M P^T), vec
constexpr int SN_OFF_W = 0;
constexpr int SN_OFF_C = SN_OFF_W + COVO_H * SN_WLD;
constexpr int SN_OFF_S = SN_OFF_C + SN_LD * SN_LD;
constexpr int SN_OFF_X = SN_OFF_S + SN_LD * SN_LD;
constexpr int SN_X_DOUBLES = 64 * COVO_NA;  // >= 32 x 128 (R chunk) + 32 x 64 (T chunk)
constexpr int SN_OFF_V = SN_OFF_X + SN_X_DOUBLES;
constexpr int SN_LDS_DOUBLES = SN_OFF_V + 4 * 64;

// the plain right-looking Cholesky of sigma.hip (cholesky_lds), for the d that are no multiple of 8
__device__ void sn_cholesky_plain(double *A, int n, int tid)
{
    for (int j = 0; j < n; ++j) {
        __syncthreads();
        const double djj = sqrt(A[j * SN_LD + j]);
        const double inv = 1.0 / djj;
        __syncthreads();
        for (int i = j + tid; i < n; i += SN_THREADS) A[j * SN_LD + i] = (i == j) ? djj : A[j * SN_LD + i] * inv;
        __syncthreads();
        const int m = n - j - 1;
        for (int e = tid; e < m * m; e += SN_THREADS) {
            const int c = j + 1 + e / m, i = j + 1 + e % m;
            if (i >= c) A[c * SN_LD + i] -= A[j * SN_LD + i] * A[j * SN_LD + c];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(SN_THREADS) void sigma_nodes_kernel(const double *__restrict__ Rin, const double *__restrict__ Wdev, int M,
                                                                 float sample_sigma, double *__restrict__ SigmaM_out,
                                                                 float *__restrict__ G_out, float *__restrict__ Sigma_out,
                                                                 float *__restrict__ rows_out)
{
    extern __shared__ __attribute__((aligned(16))) double sn_sm[];
    double *Wl = sn_sm + SN_OFF_W, *Cm = sn_sm + SN_OFF_C, *Sm = sn_sm + SN_OFF_S, *Xs = sn_sm + SN_OFF_X, *vec = sn_sm + SN_OFF_V;
    double *lam = vec + 64, *lgo = vec + 128, *fk = vec + 192;
    const int tid = threadIdx.x, d = 4 * M;
    const size_t inst = blockIdx.x;
    const double *__restrict__ R = Rin + inst * COVO_NA * COVO_NA;

    for (int e = tid; e < COVO_H * SN_WLD; e += SN_THREADS) {
        const int h = e / SN_WLD, m = e % SN_WLD;
        Wl[e] = m < M ? Wdev[h * M + m] : 0.0;
    }
    for (int e = tid; e < SN_LD * SN_LD; e += SN_THREADS) Cm[e] = 0.0;

    // ---- A = P^T R P, four chunks of 32 rows of R (8 stages): T = R_chunk P [32][d], A += P_chunk^T T
    double accA[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) accA[k] = 0.0;
    double *Rc = Xs, *Tc = Xs + 32 * COVO_NA;  // [32][128], [32][64]
    for (int q = 0; q < 4; ++q) {
        __syncthreads();  // (the previous chunk's readers are through; first pass: Wl is complete)
        for (int e = tid; e < 32 * COVO_NA; e += SN_THREADS) Rc[e] = R[(size_t)q * 32 * COVO_NA + e];
        __syncthreads();
        for (int e = tid; e < 32 * d; e += SN_THREADS) {
            const int rr = e / d, b = e - rr * d, mp = b >> 2, j = b & 3;
            double s = 0.0;
            for (int hp = 0; hp < COVO_H; ++hp) s = fma(Rc[rr * COVO_NA + 4 * hp + j], Wl[hp * SN_WLD + mp], s);
            Tc[rr * 64 + b] = s;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int e = tid + SN_THREADS * k;
            if (e < d * d) {
                const int a = e / d, b = e - a * d, m = a >> 2, i = a & 3;
                double s = accA[k];
#pragma unroll
                for (int hh = 0; hh < 8; ++hh) s = fma(Wl[(8 * q + hh) * SN_WLD + m], Tc[(4 * hh + i) * 64 + b], s);
                accA[k] = s;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int e = tid + SN_THREADS * k;
        if (e < d * d) Sm[(e / d) * SN_LD + e % d] = accA[k];
    }
    __syncthreads();
    // ---- R_M = (A + A^T) / 2 into the work matrix (column-major; rows and columns >= d stay zero), finite?, Gershgorin shift
    int bad = 0;
    for (int e = tid; e < d * d; e += SN_THREADS) {
        const int c = e / d, r = e - c * d;
        const double v = 0.5 * (Sm[r * SN_LD + c] + Sm[c * SN_LD + r]);
        bad |= !(fabs(v) < __builtin_inf());
        Cm[c * SN_LD + r] = v;
    }
    const int nonfinite = __syncthreads_or(bad);
    if (tid < d) {
        double s = 0.0;
        for (int r = 0; r < d; ++r) s += fabs(Cm[tid * SN_LD + r]);
        vec[tid] = s;
    }
    __syncthreads();
    double shift = 0.0;
    for (int i = 0; i < d; ++i) shift = fmax(shift, vec[i]);
    shift += 1.0;
    __syncthreads();
    if (tid < d) Cm[tid * SN_LD + tid] += shift;
    __syncthreads();

    int flags = nonfinite ? COVO_SIGMA_NODES_NONFINITE : 0, sweeps = 0;
    double lam_min = __builtin_nan(""), lam_max = __builtin_nan(""), f_max = 0.0, f_min = 0.0, log_det = 0.0;
    if (!nonfinite) {
        // ---- one-sided cyclic block Jacobi (sigma.hip's sweep at a run-time size): NBe blocks with the phantom, NBe / 2 block pairs
        // per round on as many 16-lane groups, NBe - 1 rounds per sweep
        const int slot = tid >> 4, l16 = tid & 15;
        const int NBe = (M + 1) & ~1, nslots = NBe >> 1;
        auto rotate4 = [&](double *x0, double *y0, double &ax0, double &ay0, double *x1, double *y1, double &ax1, double &ay1, double *x2,
                           double *y2, double &ax2, double &ay2, double *x3, double *y3, double &ax3, double &ay3) -> bool {
            double *xs[4] = {x0, x1, x2, x3}, *ys[4] = {y0, y1, y2, y3};
            double *als[4] = {&ax0, &ax1, &ax2, &ax3}, *bes[4] = {&ay0, &ay1, &ay2, &ay3};
            double ga[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ga[r] = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) ga[r] = fma(xs[r][i], ys[r][i], ga[r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) ga[r] = wr::row16_allsum(ga[r]);  // (a group is a DPP row: VALU only, every lane the same bits)
            bool any = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double al = *als[r], be = *bes[r];
                const bool live = ga[r] * ga[r] > (SN_TOL * SN_TOL) * al * be;  // uniform within the group; false against a zero column
                any |= live;
                const float zeta = (float)(be - al) * __builtin_amdgcn_rcpf(2.0f * (float)ga[r]);
                float tf = __builtin_copysignf(1.0f, zeta) *
                           __builtin_amdgcn_rcpf(__builtin_fabsf(zeta) + __builtin_amdgcn_sqrtf(fmaf(zeta, zeta, 1.0f)));
                tf = live ? tf : 0.0f;
                const double t = (double)tf;
                const double u = fma(t, t, 1.0);
                double c = (double)__builtin_amdgcn_rsqf((float)u);
                c = c * fma(-0.5 * u, c * c, 1.5);
                c = c * fma(-0.5 * u, c * c, 1.5);
                const double sn = c * t;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double xi = xs[r][i], yi = ys[r][i];
                    xs[r][i] = c * xi - sn * yi;
                    ys[r][i] = sn * xi + c * yi;
                }
                const double cc = c * c, ss = sn * sn, cs2 = 2.0 * c * sn * ga[r];
                *als[r] = cc * al - cs2 + ss * be;
                *bes[r] = ss * al + cs2 + cc * be;
            }
            return any;
        };
        int any = 1;
        for (int sweep = 0; sweep < SN_MAX_SWEEPS && any; ++sweep) {
            if (tid < d) {  // refresh the squared norms once per sweep
                double s2 = 0.0;
                for (int r = 0; r < d; ++r) s2 = fma(Cm[tid * SN_LD + r], Cm[tid * SN_LD + r], s2);
                vec[tid] = s2;
            }
            __syncthreads();
            bool rotated = false;
            for (int round = 0; round < NBe - 1; ++round) {
                int P = M, Q = M;  // (M: the phantom block -- also what the idle groups hold)
                if (slot == 0) {
                    P = round;
                    Q = NBe - 1;
                } else if (slot < nslots) {
                    P = (round + slot) % (NBe - 1);
                    Q = (round - slot + (NBe - 1)) % (NBe - 1);
                }
                const bool hasP = P < M, hasQ = Q < M;
                double X[4][4], Y[4][4], nx[4], ny[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    nx[a] = hasP ? vec[4 * P + a] : 0.0;
                    ny[a] = hasQ ? vec[4 * Q + a] : 0.0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        X[a][i] = hasP ? Cm[(4 * P + a) * SN_LD + l16 + 16 * i] : 0.0;
                        Y[a][i] = hasQ ? Cm[(4 * Q + a) * SN_LD + l16 + 16 * i] : 0.0;
                    }
                }
                if (round == 0) {  // pairs inside each block, once per sweep
                    rotated |= rotate4(X[0], X[1], nx[0], nx[1], X[2], X[3], nx[2], nx[3], Y[0], Y[1], ny[0], ny[1], Y[2], Y[3], ny[2], ny[3]);
                    rotated |= rotate4(X[0], X[2], nx[0], nx[2], X[1], X[3], nx[1], nx[3], Y[0], Y[2], ny[0], ny[2], Y[1], Y[3], ny[1], ny[3]);
                    rotated |= rotate4(X[0], X[3], nx[0], nx[3], X[1], X[2], nx[1], nx[2], Y[0], Y[3], ny[0], ny[3], Y[1], Y[2], ny[1], ny[2]);
                }
                rotated |= rotate4(X[0], Y[0], nx[0], ny[0], X[1], Y[1], nx[1], ny[1], X[2], Y[2], nx[2], ny[2], X[3], Y[3], nx[3], ny[3]);
                rotated |= rotate4(X[0], Y[1], nx[0], ny[1], X[1], Y[2], nx[1], ny[2], X[2], Y[3], nx[2], ny[3], X[3], Y[0], nx[3], ny[0]);
                rotated |= rotate4(X[0], Y[2], nx[0], ny[2], X[1], Y[3], nx[1], ny[3], X[2], Y[0], nx[2], ny[0], X[3], Y[1], nx[3], ny[1]);
                rotated |= rotate4(X[0], Y[3], nx[0], ny[3], X[1], Y[0], nx[1], ny[0], X[2], Y[1], nx[2], ny[1], X[3], Y[2], nx[3], ny[2]);
#pragma unroll
                for (int a = 0; a < 4; ++a) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (hasP) Cm[(4 * P + a) * SN_LD + l16 + 16 * i] = X[a][i];
                        if (hasQ) Cm[(4 * Q + a) * SN_LD + l16 + 16 * i] = Y[a][i];
                    }
                    if (l16 == 0 && hasP) vec[4 * P + a] = nx[a];
                    if (l16 == 0 && hasQ) vec[4 * Q + a] = ny[a];
                }
                __syncthreads();
            }
            any = __syncthreads_or(rotated ? 1 : 0);
            sweeps = sweep + 1;
        }
        if (any) flags |= COVO_SIGMA_NODES_NO_CONVERGENCE;
        // ---- eigenvalues and the spectrum map (covo.py:118-128, element_num = d)
        if (tid < d) {
            double s = 0.0;
            for (int r = 0; r < d; ++r) s = fma(Cm[tid * SN_LD + r], Cm[tid * SN_LD + r], s);
            vec[tid] = sqrt(s);  // |g_k|
            lam[tid] = vec[tid] - shift;
        }
        __syncthreads();
        lam_min = lam[0];
        lam_max = lam[0];
        for (int i = 1; i < d; ++i) {
            lam_min = fmin(lam_min, lam[i]);
            lam_max = fmax(lam_max, lam[i]);
        }
        if (tid < d) lgo[tid] = log(lam[tid] + (-lam_min + 1e-2));
        __syncthreads();
        double sum_log_o = 0.0;
        for (int i = 0; i < d; ++i) sum_log_o += lgo[i];
        const double log_const = ((double)d * (log((double)sample_sigma) * 2.0) * 2.0 + sum_log_o) / (double)d;
        if (tid < d) fk[tid] = exp(0.5 * log_const - 0.5 * lgo[tid]);
        __syncthreads();
        f_max = f_min = fk[0];
        for (int i = 0; i < d; ++i) {
            f_max = fmax(f_max, fk[i]);
            f_min = fmin(f_min, fk[i]);
            log_det += 0.5 * log_const - 0.5 * lgo[i];
        }
        // h_k = g_k sqrt(f_k) / |g_k|;  Sig_M = H H^T
        for (int e = tid; e < d * d; e += SN_THREADS) {
            const int c = e / d, r = e - c * d;
            Cm[c * SN_LD + r] *= sqrt(fk[c]) / vec[c];
        }
        __syncthreads();
        for (int e = tid; e < d * d; e += SN_THREADS) {
            const int c = e / d, r = e - c * d;
            double s = 0.0;
            for (int k = 0; k < d; ++k) s = fma(Cm[k * SN_LD + r], Cm[k * SN_LD + c], s);
            Sm[c * SN_LD + r] = s;
        }
        __syncthreads();
        for (int e = tid; e < d * d; e += SN_THREADS) {
            const int c = e / d, r = e - c * d;
            Cm[c * SN_LD + r] = Sm[c * SN_LD + r];
        }
        // ---- L_M = chol(Sig_M) in place of the copy (both begin with a barrier); a pivot that is not positive shows on the diagonal
        if ((d & 7) == 0) chol_lds_fast(Cm, d, SN_LD, tid, SN_THREADS);
        else sn_cholesky_plain(Cm, d, tid);
        int badp = 0;
        if (tid < d) {
            const double dg = Cm[tid * SN_LD + tid];
            badp = !(dg > 0.0 && dg < __builtin_inf());
        }
        if (__syncthreads_or(badp)) flags |= COVO_SIGMA_NODES_PIVOT;
    }
    if (flags) {  // (uniform) the fallback: Sig_M = sigma^2 I_d, L_M = sigma I_d
        const double sg = (double)sample_sigma;
        __syncthreads();
        for (int e = tid; e < d * d; e += SN_THREADS) {
            const int c = e / d, r = e - c * d;
            Sm[c * SN_LD + r] = r == c ? sg * sg : 0.0;
            Cm[c * SN_LD + r] = r == c ? sg : 0.0;
        }
        f_max = f_min = sg * sg;
        log_det = 2.0 * (double)d * log(sg);
        __syncthreads();
    }
    // ---- outputs: Sig_M, G = fp32(P L_M), a_cov = fp32(P Sig_M P^T), the side row
    double *So = SigmaM_out + inst * (size_t)d * d;
    for (int e = tid; e < d * d; e += SN_THREADS) {
        const int r = e / d, c = e - r * d;
        So[e] = Sm[c * SN_LD + r];
    }
    float *Go = G_out + inst * (size_t)COVO_NA * d;
    for (int e = tid; e < COVO_NA * d; e += SN_THREADS) {
        const int row = e / d, c = e - row * d, h = row >> 2, i = row & 3;
        double s = 0.0;
        for (int m = 0; m < M; ++m) {
            const int lr = 4 * m + i;
            s = fma(Wl[h * SN_WLD + m], lr >= c ? Cm[c * SN_LD + lr] : 0.0, s);
        }
        Go[e] = (float)s;
    }
    if (Sigma_out != nullptr) {
        // Q = Sig_M P^T [d][128], then the lower triangle of P Q, mirrored: symmetric bit for bit
        for (int e = tid; e < d * COVO_NA; e += SN_THREADS) {
            const int a = e / COVO_NA, col = e - a * COVO_NA, hp = col >> 2, j = col & 3;
            double s = 0.0;
            for (int mp = 0; mp < M; ++mp) s = fma(Sm[(4 * mp + j) * SN_LD + a], Wl[hp * SN_WLD + mp], s);
            Xs[e] = s;
        }
        __syncthreads();
        float *Co = Sigma_out + inst * (size_t)COVO_NA * COVO_NA;
        for (int e = tid; e < COVO_NA * COVO_NA; e += SN_THREADS) {
            const int row = e / COVO_NA, col = e - row * COVO_NA;
            if (col > row) continue;
            const int h = row >> 2, i = row & 3;
            double s = 0.0;
            for (int m = 0; m < M; ++m) s = fma(Wl[h * SN_WLD + m], Xs[(4 * m + i) * COVO_NA + col], s);
            const float v = (float)s;
            Co[(size_t)row * COVO_NA + col] = v;
            Co[(size_t)col * COVO_NA + row] = v;
        }
    }
    if (rows_out != nullptr && tid == 0) {
        float *ro = rows_out + inst * COVO_SIGMA_NODES_FLOATS;
        ro[0] = (float)lam_min;
        ro[1] = (float)lam_max;
        ro[2] = (float)f_max;
        ro[3] = (float)f_min;
        ro[4] = (float)log_det;
        ro[5] = (float)sweeps;
        ro[6] = (float)flags;
        ro[7] = (float)d;
    }
}

int launch_sigma_nodes(const double *R, int batch, const double *W_dev, int M, float sample_sigma, double *SigmaM, float *G, float *Sigma,
                       float *rows, hipStream_t s)
{
    if (M < 2 || M > COVO_SIGMA_NODES_MAX || batch < 1 || R == nullptr || W_dev == nullptr || SigmaM == nullptr || G == nullptr) {
        covo_set_error("sigma_nodes: M=%d outside [2, %d], batch=%d, or a null buffer", M, COVO_SIGMA_NODES_MAX, batch);
        return COVO_E_BADARG;
    }
    const size_t lds = (size_t)SN_LDS_DOUBLES * sizeof(double);
    static unsigned long long attr_devices = 0;  // (per device: covo_first_on_device)
    if (covo_first_on_device(attr_devices)) {
        COVO_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(sigma_nodes_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds));
    }
    hipLaunchKernelGGL(sigma_nodes_kernel, dim3(batch), dim3(SN_THREADS), lds, s, R, W_dev, M, sample_sigma, SigmaM, G, Sigma, rows);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the sampler for a dense factor G [128][d]: noise_nodes.hip's form -- lane = sample, 256 consecutive samples per workgroup on
// blockIdx.x, HS = 32 / S consecutive stages per thread on blockIdx.y, instance on blockIdx.z (BATCHED: G, mu, keys and stripes per
// instance), G wave-uniform by scalar loads.  m is the outer loop (one normal4 live at a time); entry (h, i) accumulates
// fmaf(G[(h, i)][4 m + k], e_m[k], acc) for k = 0 .. 3, which over m is ONE ascending-c fmaf chain from 0: the chain of an entry knows
// neither S, N nor the grid, so every launch shape gives the same bits.  No scratch, no atomics, no LDS.
template <int HS, bool BATCHED>
__global__ __launch_bounds__(256) void noise_factor_kernel(const float *__restrict__ G, int M, const float *__restrict__ mu, uint32_t k0,
                                                           uint32_t k1, int64_t sample_offset, int N, float4 *__restrict__ a_out,
                                                           const uint32_t *__restrict__ dyn, int nanp)
{
    const int d = 4 * M;
    if (BATCHED) {
        const size_t z = blockIdx.z;
        G += z * (size_t)COVO_NA * d;
        mu += z * COVO_NA;
        a_out += z * ((size_t)COVO_H * N);
        dyn += z * 12;
    }
    if (dyn != nullptr) { k0 = dyn[0]; k1 = dyn[1]; }
    const int h0 = (int)blockIdx.y * HS;
    const float *Gh = G + (size_t)h0 * 4 * d;  // (uniform: scalar loads)
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= (size_t)N) return;
    const uint64_t id = (uint64_t)(sample_offset + (int64_t)n);
    float acc[HS][4];
#pragma unroll
    for (int j = 0; j < HS; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = 0.0f;
    for (int m = 0; m < M; ++m) {
        const float4 e = rngd::normal4((uint32_t)m, id, k0, k1);
        const float ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
        for (int j = 0; j < HS; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float *g = Gh + (size_t)(4 * j + i) * d + 4 * m;
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[j][i] = fmaf(g[k], ev[k], acc[j][i]);
            }
    }
#pragma unroll
    for (int j = 0; j < HS; ++j) {
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v = mu[(h0 + j) * 4 + i] + acc[j][i];
            o[i] = nanp ? qm::clip11_nan_(v) : qm::clip11_(v);
        }
        a_out[(size_t)(h0 + j) * N + n] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// S, the stage groups on the grid's y, chosen as noise_nodes.hip chooses it (two waves per SIMD where the launch allows);
// COVO_FACTOR_SPLIT = 1 | 2 | 4 | 8 overrides it (read at every call: the tests force two shapes in one process); the bits do not
// depend on it.
static int noise_factor_split(int N, int batch)
{
    const char *v = std::getenv("COVO_FACTOR_SPLIT");
    const int f = v ? std::atoi(v) : 0;
    if (f == 1 || f == 2 || f == 4 || f == 8) return f;
    const long long blocks = (long long)((N + 255) / 256) * batch;
    int S = 2;
    while (S < 8 && blocks * S < 512) S *= 2;
    return S;
}

int launch_noise_factor(const NoiseDesc &d, const float *G, int M, hipStream_t s)
{
    const int N = d.N;
    const int nanp = d.propagate_nan ? 1 : 0;
    if (M < 2 || M > COVO_SIGMA_NODES_MAX || G == nullptr || d.eps != nullptr || (d.batch > 1 && d.dyn == nullptr)) {
        covo_set_error("noise_factor: d=%d outside [8, %d] or no multiple of 4, a null factor, a materialised eps, or batch=%d without the "
                       "keys in device memory", 4 * M, 4 * COVO_SIGMA_NODES_MAX, d.batch);
        return COVO_E_BADARG;
    }
    const int S = noise_factor_split(N, d.batch);
    const dim3 grid((N + 255) / 256, S, d.batch);
    float4 *a = reinterpret_cast<float4 *>(d.a);
#define NF_GO(HS)                                                                                                                   \
    do {                                                                                                                            \
        if (d.batch > 1)                                                                                                            \
            hipLaunchKernelGGL((noise_factor_kernel<HS, true>), grid, dim3(256), 0, s, G, M, d.mu, 0u, 0u, d.sample_offset, N, a,  \
                               d.dyn, nanp);                                                                                        \
        else                                                                                                                        \
            hipLaunchKernelGGL((noise_factor_kernel<HS, false>), grid, dim3(256), 0, s, G, M, d.mu, d.key[0], d.key[1],            \
                               d.sample_offset, N, a, d.dyn, nanp);                                                                 \
    } while (0)
    if (S == 1) NF_GO(32);
    else if (S == 2) NF_GO(16);
    else if (S == 4) NF_GO(8);
    else NF_GO(4);
#undef NF_GO
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
