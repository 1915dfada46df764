// riccati.hip -- the regularised Newton direction of the Hessian's objective by a backward Riccati sweep (gfx950, fp64):
// covo_riccati / covo_riccati_refine / covo_set_step_riccati and their box forms (covo_riccati_box / covo_riccati_refine_box /
// covo_set_step_riccati_box), include/covo_hip.h.
//
// The Hessian's launches 1 | 2 (hessian_adj.hip: KB, then the chains with the hyper-dual workgroups) leave, for every stage k of the
// plan, A_k, B_k (WS_JF), the costate lam_k (WS_LAM) and the exact stage blocks M_k = Hess_z(r_k + lam_{k+1} . f_k) (WS_MXX, WS_MXU,
// WS_MUU).  A backward Riccati sweep over them is the block elimination of the reduced Hessian R = d^2 C / da^2, so its forward pass
// returns d = -(R + mu I)^-1 g without R, without Sigma and without a 128 x 128 factorisation -- and, by the way, the time-varying
// feedback gains K_k and the nominal states x_k along the plan (the ancillary LQR controller of a tube MPC).  In cost sign (C = -J:
// Mc = -M, g_k = -B_k^T lam_{k+1} as in cost_gradient.hip), P_32 = 0, p_32 = 0, k = 31 .. 0:
//     Qxx = Mcxx + A^T P A      Qux = Mcxu^T + B^T P A      Quu = Mcuu + B^T P B + mu I      Qu = g_k + B^T p
//     k_k = -Quu^-1 Qu          K_k = -Quu^-1 Qux           P <- sym(Qxx + Qux^T K_k)        p <- A^T p + Qux^T k_k
// (stage 31 has no A, B: action 31 reaches no reward, Quu_31 = mu I, K_31 = 0, d[124:] = 0).  R + mu I is positive definite exactly
// when all 32 pivots Quu_k are.
//
// One launch, one workgroup of eight waves per batch entry.  Wave j runs the whole sweep with mu_j = reg0 4^j: the ladder costs the
// time of one rung.  P lives in the MFMA C/D layout (lane (lo, hi), register r = P[4r + hi][lo]); being symmetric it is the A operand
// and the B operand of v_mfma_f64_16x16x4_f64 as it lies, so do T = P A and U = P B, and the 4-row results B^T T, B^T U leave the
// matrix core as the operands of the rank-4 update Qxx + Qux^T K.  p rides in column 0 of a tile next to -lam_{k+1} in column 1: one
// chain gives B^T p and g_k.  Quu is factored by an unpivoted 4 x 4 Cholesky, every lane the same fma chain on wave-uniform values; a
// pivot that is not a positive finite number fails the rung and ends its wave's sweep (the top rung goes on for the gradient's sake).
// The rung's K_k, k_k and g_k go to its slice of the sweep workspace.
// After one barrier the lowest rung whose 32 pivots were all positive runs the linear forward pass (dx_0 = 0, du_k = k_k + K_k dx_k,
// dx_{k+1} = A_k dx_k + B_k du_k) and writes d, K, kff, x and the side row {mu, rung, smallest pivot, flags}.  No rung positive
// definite: flag bit 3, d = 0, K = 0, rung = COVO_RICCATI_RUNGS.  Flag bit 0: g not finite (an entry of the plan that is not finite counts:
// the model's clip would hide it), bit 1: d not finite.
// Every sum has one order and every output one owner: a batch gives the bits of its singles.
//
// The box form (BOX; covo_riccati_box / covo_set_step_riccati_box): the stage problem is the QP  min 1/2 du^T Quu du + Qu^T du  on
// lo <= du <= hi, lo = -1 - clip(b_k), hi = 1 - clip(b_k) (an entry of the plan that is not finite: lo = hi = 0).  A coordinate is
// clamped when it sits on a bound and its multiplier (Quu du + Qu)_i pushes strictly outward; k_k is the bound itself there and
// the row of K_k is 0, the free coordinates solve the Schur system of the free block.  With clamped rows of K zero the recurrences
// of P and p above stay exact.  The rung is still judged by the pivots of the FULL Quu.  A stage whose unconstrained k_k is feasible
// keeps it and today's arithmetic (one wave-uniform test); otherwise the 80 other active sets are tried at once, one or two per
// lane -- a clamped row and column replaced by the identity, its entry held at the bound, the same unpivoted chain, then
// primal feasibility of the free and the multiplier's sign of the clamped coordinates -- the wave takes the lowest passing pattern by
// ballot (in exact arithmetic exactly one passes; none: the set the unconstrained k_k violates, and k_k clipped) and every lane
// solves that one for its column of Qux.  The stage's mask (bits 0-3: clamped at lo, 4-7: at hi) rides in lane k of the rung's wave.
#include <type_traits>

#include "covo_common.hpp"

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int RIC_RUNGS = COVO_RICCATI_RUNGS;  // 8
constexpr int RIC_STAGE = 72;                  // doubles per (rung, stage) of the sweep workspace: K [4][16], k [4], g [4]
constexpr int RIC_BLOCK = RIC_RUNGS * COVO_WAVE;

struct RicArgs {
    const double *ws;  // [batch][L.count] the Hessian workspace behind launches 1 | 2
    const float *a;    // [batch][128] the plan (the model's clip takes a NaN action for a bound: its gradient entry is reported as NaN)
    HessianWsLayout L;
    double *sw;        // [batch][RIC_RUNGS][H][RIC_STAGE]
    double reg0;
    double *g_out;     // [batch][128] or null
    double *d_out;     // [batch][128]
    double *K_out;     // [batch][H][4][16] or null
    double *kff_out;   // [batch][H][4] or null
    double *x_out;     // [batch][H][16] or null
    double *side_out;  // [batch][COVO_RICCATI_SIDE] or null
};
struct RicBoxArgs : RicArgs {
    int *masks_out;  // [batch][H] or null
};

__device__ __forceinline__ double ric_readlane(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ bool ric_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (false for NaN)
// LDS written by one lane of a wave and read by another of the same wave: DS operations of a wave complete in order, the compiler
// must keep them in order too
__device__ __forceinline__ void ric_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the operands of stage k as the lane holds them
struct RicOps {
    double a[4];    // A_k[4g + hi][lo]
    double bq[4];   // B_k[4g + hi][lo], lo < 4 (else 0)
    double mxx[4];  // -Mxx_k[4r + hi][lo]
    double mxu;     // -Mxu_k[lo][hi]
    double muu;     // -Muu_k[hi][lo], lo < 4
    double lam[4];  // -lam_{k+1}[4g + hi] on lo == 1 (else 0)
};

// Loads only: the values are touched one stage later (ric_finish), so a stage's loads stay in flight under the stage before it -- a
// sign flip or a select next to the load would put the wait for it there
template <int NX>
__device__ __forceinline__ RicOps ric_load(const double *__restrict__ ws, const HessianWsLayout &L, int k, int lo, int hi)
{
    constexpr int NZ = NX + 4;
    RicOps o;
    const double *__restrict__ jf = ws + L.jf + (size_t)k * NX * NZ;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int row = 4 * g + hi;
        const bool oka = row < NX && lo < NX, okb = row < NX && lo < 4;
        o.a[g] = jf[oka ? row * NZ + lo : 0];
        o.bq[g] = jf[okb ? row * NZ + NX + lo : 0];
        o.mxx[g] = ws[L.mxx + (size_t)k * 256 + row * 16 + lo];
        o.lam[g] = ws[L.lam + 16 * (k + 1) + row];
    }
    o.mxu = ws[L.mxu + (size_t)k * 64 + lo * 4 + hi];
    o.muu = ws[L.muu + (size_t)k * 16 + hi * 4 + (lo & 3)];
    return o;
}
template <int NX>
__device__ __forceinline__ RicOps ric_finish(const RicOps &r, int k, int lo, int hi)
{
    RicOps o;
    const bool dyn = k < COVO_H - 1;  // (stage 31 has no A, B: its slot of WS_JF is never written)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int row = 4 * g + hi;
        o.a[g] = (dyn && row < NX && lo < NX) ? r.a[g] : 0.0;
        o.bq[g] = (dyn && row < NX && lo < 4) ? r.bq[g] : 0.0;
        o.mxx[g] = -r.mxx[g];
        o.lam[g] = lo == 1 ? -r.lam[g] : 0.0;
    }
    o.mxu = -r.mxu;
    o.muu = lo < 4 ? -r.muu : 0.0;
    return o;
}

#define RIC_MFMA4(acc, A_, B_)                                                                       \
    do {                                                                                             \
        _Pragma("unroll") for (int g_ = 0; g_ < 4; ++g_)                                             \
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64((A_)[g_], (B_)[g_], acc, 0, 0, 0);            \
    } while (0)


// ---- the 4 x 4 part of a stage: wave-uniform or per-lane values alike
// unpivoted lower Cholesky of q (lower triangle) with the rows and columns cl names replaced by the identity: l, inv = 1 / diagonal
__device__ __forceinline__ void ric_chol_masked(const double (&q)[4][4], const bool (&cl)[4], double (&l)[4][4], double (&inv)[4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double s = cl[j] ? 1.0 : q[j][j];
#pragma unroll
        for (int t = 0; t < j; ++t) s = fma(-l[j][t], l[j][t], s);
        inv[j] = 1.0 / sqrt(s);
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            double r = (cl[i] || cl[j]) ? 0.0 : q[i][j];
#pragma unroll
            for (int t = 0; t < j; ++t) r = fma(-l[i][t], l[j][t], r);
            l[i][j] = r * inv[j];
        }
    }
}
// sol = -(L L^T)^-1 rhs: forward, then backward substitution
__device__ __forceinline__ void ric_solve_neg(const double (&l)[4][4], const double (&inv)[4], const double (&rhs)[4], double (&sol)[4])
{
    double y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double s = rhs[i];
#pragma unroll
        for (int t = 0; t < i; ++t) s = fma(-l[i][t], y[t], s);
        y[i] = s * inv[i];
    }
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int t = i + 1; t < 4; ++t) s = fma(-l[t][i], sol[t], s);
        sol[i] = s * inv[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sol[i] = -sol[i];
}
// the box QP's k under the active set cl (clamped at bd): the free block's right-hand side Qu_f + Quu_fc bd_c, the clamped entries bd
__device__ __forceinline__ void ric_box_solve(const double (&q)[4][4], const double (&qu)[4], const bool (&cl)[4], const double (&bd)[4],
                                              double (&l)[4][4], double (&inv)[4], double (&k)[4])
{
    ric_chol_masked(q, cl, l, inv);
    double rhs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double s = qu[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) s = (cl[c] && c != i) ? fma(c < i ? q[i][c] : q[c][i], bd[c], s) : s;
        rhs[i] = cl[i] ? 0.0 : s;
    }
    ric_solve_neg(l, inv, rhs, k);
#pragma unroll
    for (int i = 0; i < 4; ++i) k[i] = cl[i] ? bd[i] : k[i];
}
// The active set of a stage whose unconstrained k0 leaves the box -> its pattern sum_i t_i 3^i, t_i = 0 free | 1 at lo | 2 at hi
// (wave-uniform); *fallback: no pattern passed.  Lane l tries patterns l + 1 and l + 65 (<= 80)
__device__ __forceinline__ int ric_box_pattern(const double (&q)[4][4], const double (&qu)[4], const double (&lo4)[4],
                                               const double (&hi4)[4], const double (&k0)[4], int lane, bool *fallback)
{
    unsigned long long pass[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = lane + 1 + 64 * h;
        const int t[4] = {p % 3, (p / 3) % 3, (p / 9) % 3, (p / 27) % 3};
        bool cl[4];
        double bd[4], l[4][4], inv[4], k[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            cl[i] = t[i] != 0;
            bd[i] = t[i] == 1 ? lo4[i] : hi4[i];
        }
        ric_box_solve(q, qu, cl, bd, l, inv, k);
        bool okp = p <= 80;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double m = qu[i];  // the multiplier (Quu k + Qu)_i
#pragma unroll
            for (int j = 0; j < 4; ++j) m = fma(j <= i ? q[i][j] : q[j][i], k[j], m);
            const bool free_ok = k[i] >= lo4[i] && k[i] <= hi4[i];
            okp = okp && (t[i] == 0 ? free_ok : (t[i] == 1 ? m > 0.0 : m < 0.0));
        }
        pass[h] = __ballot(okp);
    }
    int pat;
    *fallback = false;
    if (pass[0] != 0ull) pat = __ffsll((long long)pass[0]);            // (bit l: pattern l + 1)
    else if (pass[1] != 0ull) pat = 64 + __ffsll((long long)pass[1]);
    else {
        *fallback = true;
        pat = 0;
        int w3 = 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pat += w3 * (k0[i] < lo4[i] ? 1 : (k0[i] > hi4[i] ? 2 : 0));
            w3 *= 3;
        }
    }
    return __builtin_amdgcn_readfirstlane(pat);
}

template <int NX, bool BOX>
__device__ __forceinline__ void riccati_body(const std::conditional_t<BOX, RicBoxArgs, RicArgs> &A, int b, int tid, double (*sP)[16][17], double *sx, double *sdu,
                                             double *spiv, int *sok)
{
    constexpr int NZ = NX + 4, HH = COVO_H;
    const int lane = tid & (COVO_WAVE - 1), lo = lane & 15, hi = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double *__restrict__ ws = A.ws + (size_t)b * A.L.count;
    double *__restrict__ sw = A.sw + ((size_t)b * RIC_RUNGS + w) * HH * RIC_STAGE;
    const double mu = A.reg0 * (double)(1 << (2 * w));

    // ---- the backward sweep of rung w
    f64x4 P = {0.0, 0.0, 0.0, 0.0};  // P_{k+1}[4r + hi][lo]
    f64x4 pv = {0.0, 0.0, 0.0, 0.0};  // p_{k+1}[4r + hi] on lo == 0
    bool ok = true;
    double minpiv = __builtin_inf();
    // BOX: the plan's entries lane and lane + 64 (stage k's four are read by readlane: no load inside the sweep), lane k's stage mask
    [[maybe_unused]] float pl0 = 0.0f, pl1 = 0.0f;
    [[maybe_unused]] int mymask = 0;
    if constexpr (BOX) {
        pl0 = A.a[(size_t)b * COVO_NA + lane];
        pl1 = A.a[(size_t)b * COVO_NA + COVO_WAVE + lane];
    }
    RicOps raw = ric_load<NX>(ws, A.L, HH - 1, lo, hi);
    for (int k = HH - 1; k >= 0; --k) {
        const RicOps cur = ric_finish<NX>(raw, k, lo, hi);
        if (k > 0) raw = ric_load<NX>(ws, A.L, k - 1, lo, hi);  // in flight under this stage
        const f64x4 zero = {0.0, 0.0, 0.0, 0.0};
        f64x4 T = zero, U = zero;
        RIC_MFMA4(T, P, cur.a);   // P A
        RIC_MFMA4(U, P, cur.bq);  // P B (columns 0 .. 3)
        f64x4 Qxx = {cur.mxx[0], cur.mxx[1], cur.mxx[2], cur.mxx[3]};
        RIC_MFMA4(Qxx, cur.a, T);  // Mcxx + A^T P A
        f64x4 Qux = {cur.mxu, 0.0, 0.0, 0.0};
        RIC_MFMA4(Qux, cur.bq, T);  // register 0: Qux[hi][lo]
        f64x4 Quu = {cur.muu + ((lo == hi) ? mu : 0.0), 0.0, 0.0, 0.0};
        RIC_MFMA4(Quu, cur.bq, U);  // register 0, lo < 4: Quu[hi][lo]
        f64x4 v;
#pragma unroll
        for (int g = 0; g < 4; ++g) v[g] = lo == 0 ? pv[g] : cur.lam[g];
        f64x4 Atv = zero, Btv = zero;
        RIC_MFMA4(Atv, cur.a, v);   // column 0: A^T p
        RIC_MFMA4(Btv, cur.bq, v);  // register 0: (B^T p)[hi] on lo == 0, g_k[hi] on lo == 1
        // the 4 x 4 part: wave-uniform values, every lane the same chain
        double q[4][4], gk[4], qu[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) q[i][j] = ric_readlane(Quu[0], 16 * i + j);
            gk[i] = ric_readlane(Btv[0], 16 * i + 1);
            qu[i] = gk[i] + ric_readlane(Btv[0], 16 * i);
        }
        double l[4][4], inv[4];
        bool stage_ok = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double s = q[j][j];
#pragma unroll
            for (int t = 0; t < j; ++t) s = fma(-l[j][t], l[j][t], s);
            stage_ok = stage_ok && s > 0.0 && ric_finite(s);
            minpiv = (ok && stage_ok) ? fmin(minpiv, s) : minpiv;
            inv[j] = 1.0 / sqrt(s);
#pragma unroll
            for (int i = j + 1; i < 4; ++i) {
                double r = q[i][j];
#pragma unroll
                for (int t = 0; t < j; ++t) r = fma(-l[i][t], l[j][t], r);
                l[i][j] = r * inv[j];
            }
        }
        ok = ok && stage_ok;
        // a failed rung ends here and leaves its SIMD to the rungs still running (two waves share one).  The top rung alone goes on:
        // g_k does not depend on mu, and its slice is where the gradient comes from when no rung is positive definite
        if (!ok && w != RIC_RUNGS - 1) break;
        // the lane's column of Qux, and Qu: forward, then backward substitution
        double rhs[2][4], sol[2][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rhs[0][i] = __shfl(Qux[0], 16 * i + lo, COVO_WAVE);
            rhs[1][i] = qu[i];
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            double y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double s = rhs[c][i];
#pragma unroll
                for (int t = 0; t < i; ++t) s = fma(-l[i][t], y[t], s);
                y[i] = s * inv[i];
            }
#pragma unroll
            for (int i = 3; i >= 0; --i) {
                double s = y[i];
#pragma unroll
                for (int t = i + 1; t < 4; ++t) s = fma(-l[t][i], sol[c][t], s);
                sol[c][i] = s * inv[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) sol[c][i] = -sol[c][i];
        }
        if constexpr (BOX) {
            // the stage's box (wave-uniform); the unconstrained k_k inside it: nothing more to do
            double lo4[4], hi4[4];
            bool inside = true;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int at = (4 * k + i) & (COVO_WAVE - 1);
                const float pa = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(k < 16 ? pl0 : pl1), at));  // (the words: readlane is an int builtin)
                const bool fin = ric_finite((double)pa);
                const double bc = fmin(fmax((double)pa, -1.0), 1.0);
                lo4[i] = fin ? -1.0 - bc : 0.0;
                hi4[i] = fin ? 1.0 - bc : 0.0;
                inside = inside && sol[1][i] >= lo4[i] && sol[1][i] <= hi4[i];
            }
            if (__builtin_amdgcn_readfirstlane((int)inside) == 0) {
                double qf[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) qf[i][j] = j <= i ? q[i][j] : 0.0;
                }
                bool fallback;
                const int pat = ric_box_pattern(qf, qu, lo4, hi4, sol[1], lane, &fallback);
                const int t[4] = {pat % 3, (pat / 3) % 3, (pat / 9) % 3, (pat / 27) % 3};
                bool cl[4];
                double bd[4], lm[4][4], im[4];
                int m = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    cl[i] = t[i] != 0;
                    bd[i] = t[i] == 1 ? lo4[i] : hi4[i];
                    m |= t[i] == 1 ? (1 << i) : (t[i] == 2 ? (16 << i) : 0);
                }
                ric_box_solve(qf, qu, cl, bd, lm, im, sol[1]);
                if (fallback) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) sol[1][i] = fmin(fmax(sol[1][i], lo4[i]), hi4[i]);
                }
                // the free rows of K under the same factor, the clamped ones exactly 0
                double rk[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) rk[i] = cl[i] ? 0.0 : rhs[0][i];
                ric_solve_neg(lm, im, rk, sol[0]);
#pragma unroll
                for (int i = 0; i < 4; ++i) sol[0][i] = cl[i] ? 0.0 : sol[0][i];
                mymask = lane == k ? m : mymask;
            }
        }
        // K[hi][lo] and k[hi] as the B operands of the rank-4 updates
        const double Kop = hi == 0 ? sol[0][0] : (hi == 1 ? sol[0][1] : (hi == 2 ? sol[0][2] : sol[0][3]));
        const double kk = hi == 0 ? sol[1][0] : (hi == 1 ? sol[1][1] : (hi == 2 ? sol[1][2] : sol[1][3]));
        const double kop = lo == 0 ? kk : 0.0;
        double *__restrict__ slice = sw + (size_t)k * RIC_STAGE;
        slice[hi * 16 + lo] = Kop;
        if (lo == 0) slice[64 + hi] = kk;
        if (lo == 1) slice[68 + hi] = Btv[0];
        f64x4 Pn = Qxx;
        Pn = __builtin_amdgcn_mfma_f64_16x16x4f64(Qux[0], Kop, Pn, 0, 0, 0);  // Qxx + Qux^T K
        pv = __builtin_amdgcn_mfma_f64_16x16x4f64(Qux[0], kop, Atv, 0, 0, 0);  // column 0: A^T p + Qux^T k
        // P <- (P + P^T) / 2 through the wave's LDS tile
        ric_wave_sync();
#pragma unroll
        for (int r = 0; r < 4; ++r) sP[w][4 * r + hi][lo] = Pn[r];
        ric_wave_sync();
#pragma unroll
        for (int r = 0; r < 4; ++r) P[r] = 0.5 * (Pn[r] + sP[w][lo][4 * r + hi]);
    }
    if (lane == 0) {
        sok[w] = ok ? 1 : 0;
        spiv[w] = minpiv;
    }
    __syncthreads();
    int win = RIC_RUNGS;
#pragma unroll
    for (int j = RIC_RUNGS - 1; j >= 0; --j) win = sok[j] ? j : win;
    const bool none = win == RIC_RUNGS;
    if (w != (none ? RIC_RUNGS - 1 : win)) return;

    // ---- the forward pass of the winning rung (no rung: the top rung's gradient, everything else zero)
    double *__restrict__ d_out = A.d_out + (size_t)b * COVO_NA;
    const double *__restrict__ jf = ws + A.L.jf;
    if constexpr (BOX) {
        if (A.masks_out != nullptr && lane < HH) A.masks_out[(size_t)b * HH + lane] = none ? 0 : mymask;
    }
    // the copies first: independent loads, all in flight together
    if (A.K_out != nullptr) {
        double kv[HH];
#pragma unroll
        for (int k = 0; k < HH; ++k) kv[k] = sw[(size_t)k * RIC_STAGE + lane];
#pragma unroll
        for (int k = 0; k < HH; ++k) A.K_out[((size_t)b * HH + k) * 64 + lane] = none ? 0.0 : kv[k];
    }
    if (A.x_out != nullptr) {
#pragma unroll
        for (int i = lane; i < HH * 16; i += COVO_WAVE) A.x_out[(size_t)b * HH * 16 + i] = (i & 15) < NX ? ws[A.L.x + i] : 0.0;
    }
    // what stage k reads from memory -- row (lane & 3) of K_k with k_k and g_k, row lane of [A_k B_k], the plan's entry -- is loaded a
    // stage ahead and not touched before its stage
    struct Fwd {
        double K[16], kf, gk, row[NZ];
        float a;
    };
    const int q = lane & 3, xr = lane < NX ? lane : 0;
    auto load = [&](int k) {
        Fwd f;
        const double *__restrict__ slice = sw + (size_t)k * RIC_STAGE;
        const double *__restrict__ row = jf + ((size_t)(k < HH - 1 ? k : 0) * NX + xr) * NZ;
#pragma unroll
        for (int j = 0; j < 16; ++j) f.K[j] = slice[q * 16 + j];
        f.kf = slice[64 + q];
        f.gk = slice[68 + q];
#pragma unroll
        for (int j = 0; j < NZ; ++j) f.row[j] = row[j];
        f.a = A.a[(size_t)b * COVO_NA + 4 * k + q];
        return f;
    };
    if (lane < 16) sx[lane] = 0.0;
    bool gbad = false, dbad = false;
    Fwd nf = load(0);
    for (int k = 0; k < HH; ++k) {
        const Fwd f = nf;
        if (k + 1 < HH) nf = load(k + 1);
        ric_wave_sync();
        if (lane < 4) {
            double du = f.kf;
#pragma unroll
            for (int j = 0; j < 16; ++j) du = fma(f.K[j], sx[j], du);
            if (none) du = 0.0;
            double gk = f.gk;
            if (!ric_finite((double)f.a)) gk = __builtin_nan("");
            sdu[lane] = du;
            d_out[4 * k + lane] = du;
            if (A.g_out != nullptr) A.g_out[(size_t)b * COVO_NA + 4 * k + lane] = gk;
            if (A.kff_out != nullptr) A.kff_out[((size_t)b * HH + k) * 4 + lane] = none ? 0.0 : f.kf;
            gbad = gbad || !ric_finite(gk);
            dbad = dbad || !ric_finite(du);
        }
        ric_wave_sync();
        double xn = 0.0;
        if (lane < NX && k < HH - 1) {
#pragma unroll
            for (int j = 0; j < NX; ++j) xn = fma(f.row[j], sx[j], xn);
#pragma unroll
            for (int c = 0; c < 4; ++c) xn = fma(f.row[NX + c], sdu[c], xn);
        }
        ric_wave_sync();
        if (lane < 16) sx[lane] = xn;
    }
    const int flags = (__any(gbad) ? 1 : 0) | (__any(dbad) ? 2 : 0) | (none ? 8 : 0);
    if (lane == 0 && A.side_out != nullptr) {
        double *__restrict__ side = A.side_out + (size_t)b * COVO_RICCATI_SIDE;
        side[0] = none ? 0.0 : mu;
        side[1] = (double)win;
        side[2] = none ? 0.0 : spiv[win];
        side[3] = (double)flags;
    }
}

template <int NX, bool BOX>
__global__ __launch_bounds__(RIC_BLOCK) void riccati_sweep_kernel(const std::conditional_t<BOX, RicBoxArgs, RicArgs> A)
{
    __shared__ double sP[RIC_RUNGS][16][17];
    __shared__ double sx[16], sdu[4], spiv[RIC_RUNGS];
    __shared__ int sok[RIC_RUNGS];
    riccati_body<NX, BOX>(A, (int)blockIdx.x, (int)threadIdx.x, sP, sx, sdu, spiv, sok);
}

// ---- host
// the Hessian workspace of launches 1 | 2, then the sweep's slices
size_t riccati_workspace_bytes(int batch)
{
    return hessian_workspace_bytes(batch) + (size_t)batch * RIC_RUNGS * COVO_H * RIC_STAGE * sizeof(double);
}

// d: the Hessian's descriptor (R and stats are not read: launch 8 never runs); o: what the sweep writes
int launch_riccati(const HessianDesc &d, double reg0, const RiccatiOut &o, void *workspace, hipStream_t s)
{
    if (!(reg0 > 0.0) || !(reg0 < 1e300)) {
        covo_set_error("riccati: reg0=%g must be a positive finite number", reg0);
        return COVO_E_BADARG;
    }
    DebugMasks dbg;
    dbg.hess = 1 | 2;
    if (int rc = launch_hessian(d, workspace, s, dbg)) return rc;
    const covo_env_params &p = *d.params;
    const bool fs = p.disturb_kind == COVO_DISTURB_DRAG || p.disturb_kind == COVO_DISTURB_MIXED;
    RicBoxArgs A;
    A.ws = reinterpret_cast<const double *>(workspace);
    A.a = d.a_mean;
    A.L = hessian_workspace_layout(fs);
    A.sw = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + hessian_workspace_bytes(d.batch));
    A.reg0 = reg0;
    A.g_out = o.g;
    A.d_out = o.d;
    A.K_out = o.K;
    A.kff_out = o.kff;
    A.x_out = o.x;
    A.side_out = o.side;
    A.masks_out = o.masks;
    const RicArgs &A0 = A;
    if (o.box) {
        if (fs) hipLaunchKernelGGL((riccati_sweep_kernel<16, true>), dim3(d.batch), dim3(RIC_BLOCK), 0, s, A);
        else hipLaunchKernelGGL((riccati_sweep_kernel<13, true>), dim3(d.batch), dim3(RIC_BLOCK), 0, s, A);
    } else {
        if (fs) hipLaunchKernelGGL((riccati_sweep_kernel<16, false>), dim3(d.batch), dim3(RIC_BLOCK), 0, s, A0);
        else hipLaunchKernelGGL((riccati_sweep_kernel<13, false>), dim3(d.batch), dim3(RIC_BLOCK), 0, s, A0);
    }
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
