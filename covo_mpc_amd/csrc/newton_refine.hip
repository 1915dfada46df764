// newton_refine.hip -- a Newton line search on the mean a control step has just committed (gfx950): covo_newton_refine /
// covo_set_step_refine, include/covo_hip.h.
//
// covo-online samples from Sigma = c (R + delta I)^(-1/2), so (R + delta I)^-1 = Sigma^2 / c^2 and the regularised Newton direction
// at the committed mean b needs no factorisation:  d = -Sigma (Sigma g) / c^2,  g = grad C(b) (cost_gradient.hip).  Seventeen
// candidates per instance, each [H][4]:
//   0        clip(b)
//   1 .. 16  fp32(clip(b + alpha_j d)), alpha_j = 2^(3 - j): 4, 2, 1, ..., 2^-13
// every one rolled out by the rollout's own stage functions with exactly the inputs the step's sample rollouts had, as the update
// arbiter's are (update_arbiter.hip).  A NaN cost counts as +inf, equal costs resolve to the lowest candidate: the mean stays unless a
// candidate is strictly cheaper under the step's own sampling objective.  g, d or c^2 not finite: no candidate exists, the mean stays
// and the row's flags say which (bit 0: g, 1: d, 2: c^2).
//
// One launch, one workgroup of three waves per instance (after_step.hpp), eager, behind the update arbiter and ahead of the plan / fan:
//   phase 0  the per-step scalars (after_derive); g -> LDS; t = Sigma g, d = -(Sigma t) / c^2: Sigma fp32 as the step left it, row i by
//            one lane, k ascending, fp64 fma; t and d in LDS; the action image [H][64] float4 (lanes above 16 copy lane 0).  With the
//            direction supplied (RefineArgs::dir, riccati.hip: d = -(R + mu I)^-1 g by the sweep) the two mat-vecs are skipped and
//            nothing of Sigma or c is read; the row then ends {.., mu, bits(flags | rung << 8)}, flags bit 3 the sweep's
//   phase 1  rp3_stages with A_LDS, N = 64, PLAN = 3 on the image
//   phase 2  one lane decides; choice j >= 1 writes the candidate as it was rolled out (clipped) into a_mean, choice 0 writes nothing;
//            the row {cost_base, cost_chosen, bits(choice), alpha, |g|_2, g.d, 0, bits(flags)}.
// c^2 of a step: sigma^4 det(R + delta I)^(1/n) = sigma^4 exp(2 sumlogB / n) from the Sigma chain's own log-determinant slot of this
// step (sigma_ns.hip: SC_SUMLOGB; the chain's scale cancels: c = cz sqrt(scale)); stand-alone: the caller's 1 / c^2.
// With closed-loop candidates supplied (RefineArgs::extra, feedback_rollout.hip: the sweep's gains around the nonlinear plant at the
// same 16 step sizes) image lanes 17 .. 32 take those sequences as they are -- clipped fp32 already -- and 33 candidates compete; one
// the generator flagged invalid costs +inf.  Ties go to the lowest index: a closed-loop candidate wins only when strictly cheaper than
// every open-loop one.  choice is then 0 .. 32, alpha = 2^(3 - j) of either family, and a second row per instance says how the two
// families fared: {cheapest of 0 .. 16, cheapest valid closed-loop (+inf: none), bits(index of the former), bits(index of the latter,
// 0: none), that candidate's max |K dx|_inf, bits(its clipped count), bits(16-bit mask of invalid closed-loop candidates), 0}.  Flags
// set: no candidate beyond 0 of either family, the second row {cost_base, +inf, 0 ...}.
#include "after_step.hpp"
#include "wave_reduce.hpp"

constexpr int NR_BLOCK = 3 * COVO_WAVE;
constexpr int NR_CH = 2;
constexpr int NR_CAND = COVO_REFINE_CANDIDATES;  // 17
constexpr int NR_CAND_FB = COVO_FEEDBACK_CANDIDATES;  // 33: with the closed-loop family

struct RefineArgs {
    AfterHead head;         // R: the step's sample rollout (no samples: the image is the kernel's own)
    const double *g;        // [128] the gradient at a_mean
    const float *Sigma;     // [128][128] the covariance the step sampled from
    const double *inv_c2;   // the caller's 1 / c^2, or null: ...
    const double *sumlogB;  // ... the chain's sum_i log diag(chol(R + delta I)) of this instance's matrix
    float sample_sigma;
    float *a_mean;          // [128] in: the committed mean; out: the chosen candidate
    float *row_out;         // [COVO_REFINE_FLOATS] or null
    float *costs_out;       // [NR_CAND] or null
    int nanp;
    const double *dir;      // [128] the direction supplied (riccati.hip), or null: d from Sigma and c^2 as above ...
    const double *dir_side; // ... with the sweep's side row {mu, rung, smallest pivot, flags}
    const float *extra;     // [16][128] the closed-loop candidates (feedback_rollout.hip), or null: 17 candidates ...
    const float *extra_aux; // ... [16][4] their aux rows {max |K dx|_inf, bits(clipped), bits(first invalid k, -1: none), 0}
    float *fb_row_out;      // ... [COVO_FEEDBACK_FLOATS] or null
};

struct RefNoPos {  // (update_arbiter.hip: ArbNoPos)
    float unused_[1][9];
    __device__ float (&operator[](int))[1][9] { return unused_; }
};
struct RefLds {
    float4 a[COVO_H][COVO_WAVE];  // 32 KiB: the action image
    Rp3Lds<NR_CH> rings;          // 9 KiB
    RefNoPos p;
    double g[COVO_NA], t[COVO_NA], d[COVO_NA];  // 3 KiB
    double red[2][2];             // |g|^2 and g.d of the two waves that own rows
    uint32_t dyn[12];
    DynBlock kb[4];
    float cost[COVO_WAVE];
    int choice;
};

// row i of Sigma times x (LDS), k ascending, one fma per element
__device__ __forceinline__ double refine_row_dot(const float *__restrict__ Sigma, int i, const double *x)
{
    const float4 *__restrict__ r4 = reinterpret_cast<const float4 *>(Sigma + (size_t)i * COVO_NA);
    double s = 0.0;
#pragma unroll 8
    for (int q = 0; q < COVO_NA / 4; ++q) {
        const float4 v = r4[q];
        s = fma((double)v.x, x[4 * q + 0], s);
        s = fma((double)v.y, x[4 * q + 1], s);
        s = fma((double)v.z, x[4 * q + 2], s);
        s = fma((double)v.w, x[4 * q + 3], s);
    }
    return s;
}
__device__ __forceinline__ bool refine_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (false for NaN)

template <bool ROLL, int REWARD, int FDIST, bool BATCHED>
__global__ __launch_bounds__(NR_BLOCK) void newton_refine_kernel(const RefineArgs P_, const RefineArgs *__restrict__ batch, const AfterDyn dyn)
{
    RefineArgs Pb;
    if (BATCHED) {
        Pb = batch[blockIdx.x];
        after_rebase_head(P_.head, Pb.head);
        Pb.g = rebase_global(P_.g, Pb.g);
        Pb.Sigma = rebase_global(P_.Sigma, Pb.Sigma);
        Pb.inv_c2 = rebase_global(P_.inv_c2, Pb.inv_c2);
        Pb.sumlogB = rebase_global(P_.sumlogB, Pb.sumlogB);
        Pb.a_mean = rebase_global(P_.a_mean, Pb.a_mean);
        Pb.row_out = rebase_global(P_.row_out, Pb.row_out);
        Pb.costs_out = rebase_global(P_.costs_out, Pb.costs_out);
        Pb.dir = rebase_global(P_.dir, Pb.dir);
        Pb.dir_side = rebase_global(P_.dir_side, Pb.dir_side);
        Pb.extra = rebase_global(P_.extra, Pb.extra);
        Pb.extra_aux = rebase_global(P_.extra_aux, Pb.extra_aux);
        Pb.fb_row_out = rebase_global(P_.fb_row_out, Pb.fb_row_out);
    }
    const RefineArgs &P = BATCHED ? Pb : P_;
    __shared__ RefLds S;
    const int tid = threadIdx.x, lane = tid & (COVO_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool has_row = P_.row_out != nullptr, has_costs = P_.costs_out != nullptr;  // (all instances alike)
    const bool fb = P_.extra != nullptr, has_fb_row = fb && P_.fb_row_out != nullptr;

    // ---- phase 0
    after_derive(tid, P.head, dyn, BATCHED, S.kb, S.dyn);
    const bool supplied = P_.dir != nullptr;  // (all instances alike)
    double inv_c2;
    if (supplied) {
        inv_c2 = 1.0;  // (never used: no Sigma, no c)
    } else if (P_.inv_c2 != nullptr) {
        inv_c2 = P.inv_c2[0];
    } else {
        const double s2 = (double)P.sample_sigma * (double)P.sample_sigma;
        inv_c2 = 1.0 / (s2 * s2 * exp(2.0 * P.sumlogB[0] / (double)COVO_NA));
    }
    const bool row = tid < COVO_NA;  // waves 0 and 1: one row of Sigma each
    double gi = 0.0;
    if (row) {
        gi = P.g[tid];
        S.g[tid] = gi;
    }
    double di = 0.0;
    if (supplied) {
        if (row) {
            di = P.dir[tid];
            S.d[tid] = di;
        }
    } else {
        __syncthreads();
        if (row) S.t[tid] = refine_row_dot(P.Sigma, tid, S.g);
        __syncthreads();
        if (row) {
            di = -refine_row_dot(P.Sigma, tid, S.t) * inv_c2;
            S.d[tid] = di;
        }
    }
    if (wave < 2) {
        const double gg = wr::wave64_allsum(gi * gi), gd = wr::wave64_allsum(gi * di);
        if (lane == 0) {
            S.red[wave][0] = gg;
            S.red[wave][1] = gd;
        }
    }
    // (__syncthreads_or is a logical or: one per bit; the first is also the barrier behind S.d)
    const int flags = (__syncthreads_or(row && !refine_finite(gi)) ? 1 : 0) | (__syncthreads_or(row && !refine_finite(di)) ? 2 : 0) |
                      (!(refine_finite(inv_c2) && inv_c2 > 0.0) ? 4 : 0) | (supplied ? ((int)P.dir_side[3] & 8) : 0);
    {
        const float4 *__restrict__ am4 = reinterpret_cast<const float4 *>(P.a_mean);
        const int nanp = P_.nanp;
        for (int i = tid; i < COVO_H * COVO_WAVE; i += NR_BLOCK) {
            const int k = i >> 6, l = i & (COVO_WAVE - 1);
            float4 v = am4[k];
            if (fb && l >= NR_CAND && l < NR_CAND_FB && flags == 0) {
                v = reinterpret_cast<const float4 *>(P.extra)[(l - NR_CAND) * COVO_H + k];
            } else if (l >= 1 && l < NR_CAND && flags == 0) {
                const double alpha = __builtin_ldexp(1.0, 3 - l);
                const float b[4] = {v.x, v.y, v.z, v.w};
                float o[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double x = fma(alpha, S.d[4 * k + q], (double)b[q]);
                    o[q] = (float)((nanp && x != x) ? x : qm::clip11_(x));
                }
                v = make_float4(o[0], o[1], o[2], o[3]);
            } else if (nanp) {
                v.x = qm::clip11_nan_(v.x); v.y = qm::clip11_nan_(v.y); v.z = qm::clip11_nan_(v.z); v.w = qm::clip11_nan_(v.w);
            } else {
                v.x = qm::clip11_(v.x); v.y = qm::clip11_(v.y); v.z = qm::clip11_(v.z); v.w = qm::clip11_(v.w);
            }
            S.a[k][l] = v;
        }
    }
    __syncthreads();
    RolloutArgs A = after_rollout_args(P.head, S.dyn);
    A.N = COVO_WAVE;  // the image holds one full group: every lane is a sample of its own
    A.clip = 0;
    A.cost = nullptr;  // (PLAN = 3: stage R stores nothing)
    A.groupmin = nullptr;

    // ---- phase 1: the candidates' rollouts (covo.py:227-263)
    float cost = 0.0f;
    bool valid = false;
    int n = 0;
    rp3_stages<false, ROLL, NR_CH, -1, false, true, REWARD, FDIST, true, RefNoPos, COVO_H, 3>(A, S.rings, S.p, wave, 0, 0, lane,
                                                                                               &S.a[0][0], cost, valid, n);
    if (wave == 2) {
        // (a closed-loop sequence the generator flagged: first invalid k >= 0)
        if (fb && flags == 0 && lane >= NR_CAND && lane < NR_CAND_FB &&
            __float_as_int(P.extra_aux[(lane - NR_CAND) * COVO_FEEDBACK_AUX_FLOATS + 2]) >= 0)
            cost = __builtin_inff();
        S.cost[lane] = cost;
    }
    __syncthreads();

    // ---- phase 2: the decision, the row, the mean
    if (tid == 0) {
        const float inf = __builtin_inff();
        int choice = 0;
        float cb = inf;
        const int ncand = flags == 0 ? (fb ? NR_CAND_FB : NR_CAND) : 1;
        for (int q = 0; q < ncand; ++q) {
            const float c = S.cost[q];
            if (c < cb) {  // (a NaN cost never wins; equal costs keep the lower candidate)
                cb = c;
                choice = q;
            }
        }
        S.choice = choice;
        if (has_row) {
            const double gg = S.red[0][0] + S.red[1][0], gd = S.red[0][1] + S.red[1][1];
            const float alpha = choice >= 1 ? __builtin_ldexpf(1.0f, 3 - (choice >= NR_CAND ? choice - (NR_CAND - 1) : choice)) : 0.0f;
            const float w6 = supplied ? (float)P.dir_side[0] : 0.0f;
            const int w7 = supplied ? (flags | ((int)P.dir_side[1] << 8)) : flags;
            const float out[COVO_REFINE_FLOATS] = {S.cost[0], S.cost[choice], __int_as_float(choice), alpha,
                                                   (float)sqrt(gg),  (float)gd,      w6,                    __int_as_float(w7)};
#pragma unroll
            for (int j = 0; j < COVO_REFINE_FLOATS; ++j) P.row_out[j] = out[j];
        }
        if (has_fb_row) {  // how the two families fared, by the rule above within each
            int io = 0, ic = 0, bad = 0;
            float co = inf, cc = inf;
            for (int q = 0; q < (flags == 0 ? NR_CAND : 1); ++q)
                if (S.cost[q] < co) {
                    co = S.cost[q];
                    io = q;
                }
            for (int q = NR_CAND; q < ncand; ++q) {
                if (__float_as_int(P.extra_aux[(q - NR_CAND) * COVO_FEEDBACK_AUX_FLOATS + 2]) >= 0) bad |= 1 << (q - NR_CAND);
                if (S.cost[q] < cc) {
                    cc = S.cost[q];
                    ic = q;
                }
            }
            const float *aux = P.extra_aux + (ic ? ic - NR_CAND : 0) * COVO_FEEDBACK_AUX_FLOATS;
            const float out[COVO_FEEDBACK_FLOATS] = {co, cc, __int_as_float(io), __int_as_float(ic), ic ? aux[0] : 0.0f, ic ? aux[1] : 0.0f,
                                                     __int_as_float(bad), 0.0f};
#pragma unroll
            for (int j = 0; j < COVO_FEEDBACK_FLOATS; ++j) P.fb_row_out[j] = out[j];
        }
    }
    if (has_costs && tid >= COVO_WAVE && tid < COVO_WAVE + (fb ? NR_CAND_FB : NR_CAND)) P.costs_out[tid - COVO_WAVE] = S.cost[tid - COVO_WAVE];
    __syncthreads();
    const int choice = S.choice;
    if (choice != 0 && tid < COVO_H) reinterpret_cast<float4 *>(P.a_mean)[tid] = S.a[tid][choice];
}

// ---- host
static void fill_refine_args(RefineArgs &P, covo_ctx *h, const PlanInstDesc &d, RolloutClip clip, const RefineDesc &r)
{
    std::memset(&P, 0, sizeof(P));
    after_fill_head(P.head, h, d, clip, false);
    P.g = r.g;
    P.Sigma = r.Sigma;
    P.inv_c2 = r.inv_c2;
    P.sumlogB = r.sumlogB;
    P.sample_sigma = r.sample_sigma;
    P.a_mean = d.a_mean_out;
    P.row_out = r.row_out;
    P.costs_out = r.costs_out;
    P.nanp = covo_propagate_nan(h) ? 1 : 0;
    P.dir = r.dir;
    P.dir_side = r.dir_side;
    P.extra = r.extra;
    P.extra_aux = r.extra_aux;
    P.fb_row_out = r.extra ? r.fb_row_out : nullptr;
}

// covo_newton_refine: one instance, the caller's buffers and shared vector (d.derive_keys = 0), the clip covo_rollout_cost applies
int launch_newton_refine_one(covo_ctx *h, const PlanInstDesc &d, RolloutClip clip, const RefineDesc &r, hipStream_t s)
{
    if (int rc = after_check_tables(&d, 1, "newton refine")) return rc;
    RefineArgs P;
    fill_refine_args(P, h, d, clip, r);
    AFTER_DISPATCH(newton_refine_kernel, NR_BLOCK, P, (const RefineArgs *)nullptr, 1, after_dyn_single(d, -1), s);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

// inst / r: n_inst instances of ONE step that has just been enqueued (launch_update_arbiter's descriptors) and what each refines with
int launch_newton_refine(covo_ctx *h, const PlanInstDesc *inst, const RefineDesc *r, int n_inst, bool batched, hipStream_t s)
{
    if (int rc = after_check_tables(inst, n_inst, "newton refine")) return rc;
    if (!batched) {
        RefineArgs P;
        fill_refine_args(P, h, inst[0], ROLLOUT_CLIP_TRUSTED, r[0]);
        AFTER_DISPATCH(newton_refine_kernel, NR_BLOCK, P, (const RefineArgs *)nullptr, 1, after_dyn_single(inst[0], -1), s);
    } else {
        std::vector<RefineArgs> now(n_inst);
        for (int e = 0; e < n_inst; ++e) fill_refine_args(now[e], h, inst[e], ROLLOUT_CLIP_TRUSTED, r[e]);
        ArgBlockCache &c = after_state(h)->refine;
        if (int rc = c.sync_upload(now.data(), now.size() * sizeof(RefineArgs), sizeof(RefineArgs), s)) return rc;
        AFTER_DISPATCH(newton_refine_kernel, NR_BLOCK, now[0], (const RefineArgs *)c.dev, n_inst, after_dyn_batched(-1), s);
    }
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
