// feedback_rollout.hip -- closed-loop action sequences under the gains of the Riccati sweep (gfx950): covo_feedback_rollout /
// covo_riccati_refine_feedback / covo_set_step_riccati_feedback, include/covo_hip.h.
//
// The sweep (riccati.hip) leaves, per instance, the gains K_k [4][16], the feed-forward terms kff_k [4] and the nominal states xb_k [16]
// along the plan b.  The forward pass of DDP / iLQR at step size alpha, the nonlinear plant in the loop, x_0 the state's 13 numbers
// (pos, vel, quat, omega) in fp32:
//     for k = 0 .. 31:
//         dx_j = (double)x_k[j] - xb_k[j],                                   j = 0 .. 12  (raw coordinates: plain quaternion components)
//         v_i  = fma(alpha, kff_k[i], (double)b_k[i]);  v_i = fma(K_k[i][j], dx_j, v_i),  j ascending
//         u_k[i] = (float)clip(v_i, -1, 1)
//         x_{k+1} = qm::dyn_step<float, float>(x_k, u_k, consts, force_k)
// force_k is what the step's sample rollouts apply at step k: the state's own f_disturb at k = 0, then the shared vector (FDIST 0) or
// row k of the step's table (FDIST 1).  No reward, no termination: the kernel only produces actions, newton_refine.hip judges them.
// K = 0 gives fp32(clip(fma(alpha, kff, b))): the open-loop candidate along kff, bit for bit.
// A v_i that is not finite makes the sequence invalid: the aux row says at which k, and from there on the sequence is clip(b).
//   aux row  float[4] = {max over k of |K_k dx_k|_inf -- the feedback term as it entered the action, v_i - fma(alpha, kff_k[i], b_k[i]);
//                        bits(number of components with |v| > 1); bits(first k with a v that is not finite, -1: none); 0}
//            (the first two over the stages before the sequence became invalid)
//
// One launch, one workgroup of ONE wave per instance, lane = step size (lanes at and above n_alpha idle): the 32 stages are a dependent
// chain, so the aim is latency.  K, xb, kff and b are wave-uniform: staged in LDS once (23 KiB, every load in flight together), then
// read as broadcasts ahead of their use -- stage k + 1's rows are loaded while stage k's plant step runs.  Phase 0 is the
// after-step frame's (after_step.hpp): the shared vector from the raw controller key, per-instance argument blocks through rebase_global.
#include "after_step.hpp"

constexpr int FB_BLOCK = COVO_WAVE;
constexpr int FB_NX = 13;

struct FeedbackArgs {
    AfterHead head;     // R: the step's sample rollout (state, model constants, disturbance table)
    const float *b;     // [128] the plan the sweep ran at
    const double *K;    // [H][4][16]
    const double *kff;  // [H][4]
    const double *x;    // [H][16]
    float *a_out;       // [n_alpha][128]
    float *aux_out;     // [n_alpha][4]
    int n_alpha;
};
struct FeedbackAlphas {
    double v[COVO_FEEDBACK_MAX_ALPHAS];
};

struct FbLds {
    double K[COVO_H][4][16];  // 16 KiB
    double x[COVO_H][16];     // 4 KiB
    double kff[COVO_H][4];    // 1 KiB
    float4 b[COVO_H];         // 512 B
    float4 f[COVO_H];         // 512 B: FDIST 1, the step's table
    double alpha[COVO_WAVE];  // 512 B: the step sizes (from the kernel arguments: nothing the loop waits for is then a vector-memory load,
                              // and its stores stay in flight -- on gfx9 loads and stores share one counter)
    uint32_t dyn[12];
    DynBlock kb[4];
};

// what stage k reads from LDS, loaded under the plant's step of stage k - 1 and not touched before its stage
struct FbStage {
    double K[4][FB_NX], x[FB_NX], kff[4];
    float4 b, f;
};
template <int FDIST>
__device__ __forceinline__ FbStage fb_load(const FbLds &S, int k)
{
    FbStage f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < FB_NX; ++j) f.K[i][j] = S.K[k][i][j];
#pragma unroll
    for (int j = 0; j < FB_NX; ++j) f.x[j] = S.x[k][j];
#pragma unroll
    for (int i = 0; i < 4; ++i) f.kff[i] = S.kff[k][i];
    f.b = S.b[k];
    f.f = FDIST == 1 ? S.f[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return f;
}
__device__ __forceinline__ bool fb_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (false for NaN)

template <int FDIST, bool BATCHED>
__global__ __launch_bounds__(FB_BLOCK) void feedback_rollout_kernel(const FeedbackArgs P_, const FeedbackArgs *__restrict__ batch,
                                                                    const AfterDyn dyn, const FeedbackAlphas alphas)
{
    FeedbackArgs Pb;
    if (BATCHED) {
        Pb = batch[blockIdx.x];
        after_rebase_head(P_.head, Pb.head);
        Pb.b = rebase_global(P_.b, Pb.b);
        Pb.K = rebase_global(P_.K, Pb.K);
        Pb.kff = rebase_global(P_.kff, Pb.kff);
        Pb.x = rebase_global(P_.x, Pb.x);
        Pb.a_out = rebase_global(P_.a_out, Pb.a_out);
        Pb.aux_out = rebase_global(P_.aux_out, Pb.aux_out);
    }
    const FeedbackArgs &P = BATCHED ? Pb : P_;
    __shared__ FbLds S;
    const int lane = threadIdx.x;

    // ---- phase 0: the per-step scalars; the sweep's outputs -> LDS
    after_derive(lane, P.head, dyn, BATCHED, S.kb, S.dyn);
    {
        const double2 *__restrict__ K2 = reinterpret_cast<const double2 *>(P.K);
        const double2 *__restrict__ x2 = reinterpret_cast<const double2 *>(P.x);
        double2 *sK = reinterpret_cast<double2 *>(&S.K[0][0][0]), *sx = reinterpret_cast<double2 *>(&S.x[0][0]);
#pragma unroll
        for (int i = 0; i < COVO_H * 64 / 2 / FB_BLOCK; ++i) sK[i * FB_BLOCK + lane] = K2[i * FB_BLOCK + lane];
#pragma unroll
        for (int i = 0; i < COVO_H * 16 / 2 / FB_BLOCK; ++i) sx[i * FB_BLOCK + lane] = x2[i * FB_BLOCK + lane];
        reinterpret_cast<double2 *>(&S.kff[0][0])[lane] = reinterpret_cast<const double2 *>(P.kff)[lane];
        if (lane < COVO_H) S.b[lane] = reinterpret_cast<const float4 *>(P.b)[lane];
        if (FDIST == 1 && lane < COVO_H) S.f[lane] = P.head.R.f_tab[lane];
        S.alpha[lane] = alphas.v[lane];
    }
    __syncthreads();

    const float *__restrict__ st = P.head.R.state;
    const qm::Consts<float> c = P.head.R.c;
    qm::State<float> s;
    s.px = st[ST_POS + 0]; s.py = st[ST_POS + 1]; s.pz = st[ST_POS + 2];
    s.vx = st[ST_VEL + 0]; s.vy = st[ST_VEL + 1]; s.vz = st[ST_VEL + 2];
    s.qx = st[ST_QUAT + 0]; s.qy = st[ST_QUAT + 1]; s.qz = st[ST_QUAT + 2]; s.qw = st[ST_QUAT + 3];
    s.ox = st[ST_OMEGA + 0]; s.oy = st[ST_OMEGA + 1]; s.oz = st[ST_OMEGA + 2];
    const float f0x = st[ST_FDIST + 0], f0y = st[ST_FDIST + 1], f0z = st[ST_FDIST + 2];
    const float fsx = __uint_as_float(S.dyn[2]), fsy = __uint_as_float(S.dyn[3]), fsz = __uint_as_float(S.dyn[4]);
    const int n_alpha = P_.n_alpha;  // (all instances alike)
    const bool live = lane < n_alpha;
    const double alpha = S.alpha[live ? lane : 0];
    float4 *__restrict__ out = reinterpret_cast<float4 *>(P.a_out + (size_t)(live ? lane : 0) * COVO_NA);

    // ---- the 32 stages
    double gain_max = 0.0;
    int n_clip = 0, bad_k = -1;
    FbStage f = fb_load<FDIST>(S, 0);
#pragma unroll 1
    for (int k = 0; k < COVO_H; ++k) {
        const double xs[FB_NX] = {s.px, s.py, s.pz, s.vx, s.vy, s.vz, s.qx, s.qy, s.qz, s.qw, s.ox, s.oy, s.oz};
        double dx[FB_NX];
#pragma unroll
        for (int j = 0; j < FB_NX; ++j) dx[j] = xs[j] - f.x[j];
        const float bk[4] = {f.b.x, f.b.y, f.b.z, f.b.w};
        double v[4];
        float u[4];
        bool fin = true;
        double gain = 0.0;
        int nc = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double v0 = fma(alpha, f.kff[i], (double)bk[i]);
            v[i] = v0;
#pragma unroll
            for (int j = 0; j < FB_NX; ++j) v[i] = fma(f.K[i][j], dx[j], v[i]);
            fin = fin && fb_finite(v[i]);
            gain = fmax(gain, fabs(v[i] - v0));
            nc += fabs(v[i]) > 1.0 ? 1 : 0;
        }
        if (bad_k < 0 && !fin) bad_k = k;
        const bool ok = bad_k < 0;
        gain_max = ok ? fmax(gain_max, gain) : gain_max;
        n_clip += ok ? nc : 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = ok ? (float)qm::clip11_(v[i]) : qm::clip11_(bk[i]);
        if (live) out[k] = make_float4(u[0], u[1], u[2], u[3]);
        const float fx = k == 0 ? f0x : (FDIST == 1 ? f.f.x : fsx);
        const float fy = k == 0 ? f0y : (FDIST == 1 ? f.f.y : fsy);
        const float fz = k == 0 ? f0z : (FDIST == 1 ? f.f.z : fsz);
        // the next stage's rows into the registers this stage's chain has just released: in flight under the plant's step (a second
        // copy of the 73 doubles does not fit the 256 VGPRs a VALU instruction can name and would travel through the AGPRs)
        __builtin_amdgcn_sched_barrier(0);
        if (k + 1 < COVO_H) f = fb_load<FDIST>(S, k + 1);
        __builtin_amdgcn_sched_barrier(0);
        qm::dyn_step<float, float>(s, u[0], u[1], u[2], u[3], c, fx, fy, fz);
    }
    if (live) {
        float *__restrict__ aux = P.aux_out + (size_t)lane * COVO_FEEDBACK_AUX_FLOATS;
        aux[0] = (float)gain_max;
        aux[1] = __int_as_float(n_clip);
        aux[2] = __int_as_float(bad_k);
        aux[3] = 0.0f;
    }
}

// ---- host
static int fill_feedback_args(FeedbackArgs &P, covo_ctx *h, const PlanInstDesc &d, const FeedbackDesc &f)
{
    const int kind = d.params->disturb_kind;
    if (kind == COVO_DISTURB_DRAG || kind == COVO_DISTURB_MIXED) {
        covo_set_error("feedback rollout: disturb_kind=%d (drag / mixed) is a 16-state plant -- its force is a state of the sweep and a "
                       "per-sample quantity of the rollout; the closed-loop generator carries the 13-state plants only", kind);
        return COVO_E_BADARG;
    }
    std::memset(&P, 0, sizeof(P));
    after_fill_head(P.head, h, d, ROLLOUT_CLIP_TRUSTED, false);
    P.b = f.b;
    P.K = f.K;
    P.kff = f.kff;
    P.x = f.x;
    P.a_out = f.a_out;
    P.aux_out = f.aux_out;
    P.n_alpha = f.n_alpha;
    return 0;
}

template <bool BATCHED>
static void feedback_dispatch(const FeedbackArgs &P, const FeedbackArgs *batch, int n, const AfterDyn &dyn, const FeedbackAlphas &al,
                              hipStream_t s)
{
    if (P.head.R.fdist == 1) hipLaunchKernelGGL((feedback_rollout_kernel<1, BATCHED>), dim3(n), dim3(FB_BLOCK), 0, s, P, batch, dyn, al);
    else hipLaunchKernelGGL((feedback_rollout_kernel<0, BATCHED>), dim3(n), dim3(FB_BLOCK), 0, s, P, batch, dyn, al);
}

static int feedback_alphas(FeedbackAlphas &al, const double *alphas, int n_alpha)
{
    if (alphas == nullptr || n_alpha < 1 || n_alpha > COVO_FEEDBACK_MAX_ALPHAS) {
        covo_set_error("feedback rollout: n_alpha=%d outside [1, %d] (or alphas is null)", n_alpha, COVO_FEEDBACK_MAX_ALPHAS);
        return COVO_E_BADARG;
    }
    std::memset(&al, 0, sizeof(al));
    for (int j = 0; j < n_alpha; ++j) al.v[j] = alphas[j];
    return 0;
}

// covo_feedback_rollout: one instance, the caller's buffers and shared vector (d.derive_keys = 0)
int launch_feedback_rollout_one(covo_ctx *h, const PlanInstDesc &d, const FeedbackDesc &f, const double *alphas, hipStream_t s)
{
    if (int rc = after_check_tables(&d, 1, "feedback rollout")) return rc;
    FeedbackAlphas al;
    if (int rc = feedback_alphas(al, alphas, f.n_alpha)) return rc;
    FeedbackArgs P;
    if (int rc = fill_feedback_args(P, h, d, f)) return rc;
    feedback_dispatch<false>(P, nullptr, 1, after_dyn_single(d, -1), al, s);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

// inst / f: n_inst instances of ONE step that has just been enqueued (launch_newton_refine's descriptors), every one at the ladder's
// 16 step sizes 2^(3 - j), j = 1 .. 16
int launch_feedback_rollout(covo_ctx *h, const PlanInstDesc *inst, const FeedbackDesc *f, int n_inst, bool batched, hipStream_t s)
{
    if (int rc = after_check_tables(inst, n_inst, "feedback rollout")) return rc;
    double ladder[COVO_FEEDBACK_LADDER];
    for (int j = 1; j <= COVO_FEEDBACK_LADDER; ++j) ladder[j - 1] = std::ldexp(1.0, 3 - j);
    FeedbackAlphas al;
    if (int rc = feedback_alphas(al, ladder, COVO_FEEDBACK_LADDER)) return rc;
    if (!batched) {
        FeedbackArgs P;
        if (int rc = fill_feedback_args(P, h, inst[0], f[0])) return rc;
        feedback_dispatch<false>(P, nullptr, 1, after_dyn_single(inst[0], -1), al, s);
    } else {
        std::vector<FeedbackArgs> now(n_inst);
        for (int e = 0; e < n_inst; ++e)
            if (int rc = fill_feedback_args(now[e], h, inst[e], f[e])) return rc;
        ArgBlockCache &c = after_state(h)->feedback;
        if (int rc = c.sync_upload(now.data(), now.size() * sizeof(FeedbackArgs), sizeof(FeedbackArgs), s)) return rc;
        feedback_dispatch<true>(now[0], (const FeedbackArgs *)c.dev, n_inst, after_dyn_batched(-1), al, s);
    }
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
