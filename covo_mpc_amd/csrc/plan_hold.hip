// plan_hold.hip -- the hold step of a plan-hold schedule (gfx950): covo_plan_hold / covo_set_step_plan_hold, include/covo_hip.h.
//
// A plan step (age 0) is the control step as it always was; its Riccati sweep (riccati.hip) leaves the gains K_k [4][16], the
// feed-forward terms kff_k [4] and the nominal states xb_k [16] along the mean b it ran at, and plan_latch_kernel keeps b and the time
// word of the state the step planned from.  A hold step (age j >= 1) samples nothing: it applies stage j of that law to the measured
// state x (pos, vel, quat, omega: 13 raw coordinates, fp32),
//     dx_c = (double)x[c] - xb_j[c];  v0_i = fma(alpha, kff_j[i], (double)b_j[i]);  v_i = v0_i, v_i = fma(K_j[i][c], dx_c, v_i), c ascending
//     u_i  = (float)clip(v_i, -1, 1)
// -- the arithmetic of feedback_rollout.hip's stage, restated (stage 0 on the start state is that generator's first action bit for
// bit: tests/test_gpu_plan_hold.py) -- and then does, in place, what the begin work of a step would have done to the controller
// state: a_mean <- [a_mean[1:], a_mean[31]], MPPI's 32 covariance blocks likewise, and finally a_mean[0] <- u.
// Decided on the device, reported in the row, none an error:
//   bit 0  the sweep is flagged (its side row, when given: no rung positive definite -- K = kff = 0 then anyway --, g or d not
//          finite): u = clip(b_j)
//   bit 1  a v_i that is not finite (bit 0 clear): all four components are clip(b_j)
//   bit 2  the state's time word is not t_plan + j (an auto-reset, an episode end: the plan belongs to another trajectory): the
//          feedback term is dropped, u = (float)clip(v0)
//   hold row  float[8] = {bits(j), alpha, max_i |v_i - v0_i| (0 when the feedback term is not applied), bits(number of components whose
//             applied command exceeds 1 in magnitude), bits(flags), |dx_pos|_2, bits(the state's time word), 0}
//
// One launch, one workgroup of ONE wave per instance; the aim is latency: every load -- one stage of K, xb, kff, b, 13 state floats
// and the time word, alpha, the 128 mean floats, MPPI's 512 covariance floats -- is issued before the first use, the shift goes
// registers -> stores (in place: all lanes of the one wave have loaded before any stores).  Lane i & 3 carries chain i (the quads
// repeat each other: no divergence, the loads are broadcasts).  Batched instances take their argument block from device memory,
// pointers through rebase_global, as feedback_rollout_kernel does; the stage and the log's row index are kernel arguments, so the
// blocks of a steady-state schedule never change.
#include "after_step.hpp"

constexpr int PH_BLOCK = COVO_WAVE;
constexpr int PH_NX = 13;

__device__ __forceinline__ bool ph_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (false for NaN)

template <bool BATCHED>
__global__ __launch_bounds__(PH_BLOCK) void plan_hold_kernel(const HoldDesc P_, const HoldDesc *__restrict__ batch, const int stage,
                                                             const int log_index)
{
    HoldDesc Pb;
    if (BATCHED) {
        Pb = batch[blockIdx.x];
        Pb.state = rebase_global(P_.state, Pb.state);
        Pb.b = rebase_global(P_.b, Pb.b);
        Pb.K = rebase_global(P_.K, Pb.K);
        Pb.kff = rebase_global(P_.kff, Pb.kff);
        Pb.x = rebase_global(P_.x, Pb.x);
        Pb.alpha = rebase_global(P_.alpha, Pb.alpha);
        Pb.t_plan = rebase_global(P_.t_plan, Pb.t_plan);
        Pb.side = rebase_global(P_.side, Pb.side);
        Pb.a_mean_src = rebase_global(P_.a_mean_src, Pb.a_mean_src);
        Pb.a_mean = rebase_global(P_.a_mean, Pb.a_mean);
        Pb.a_cov = rebase_global(P_.a_cov, Pb.a_cov);
        Pb.u_out = rebase_global(P_.u_out, Pb.u_out);
        Pb.row_out = rebase_global(P_.row_out, Pb.row_out);
        Pb.log = rebase_global(P_.log, Pb.log);
    }
    const HoldDesc &P = BATCHED ? Pb : P_;
    // (what is attached is the same for all instances)
    const bool has_t = P_.t_plan != nullptr, has_side = P_.side != nullptr, has_mean = P_.a_mean != nullptr, has_cov = P_.a_cov != nullptr;
    const int lane = threadIdx.x, i = lane & 3;

    // ---- every load
    const double *__restrict__ Kr = P.K + ((size_t)stage * 4 + i) * 16;
    const double *__restrict__ xr = P.x + (size_t)stage * 16;
    double k[PH_NX], xb[PH_NX];
#pragma unroll
    for (int c = 0; c < PH_NX; ++c) k[c] = Kr[c];
#pragma unroll
    for (int c = 0; c < PH_NX; ++c) xb[c] = xr[c];
    const double kf = P.kff[stage * 4 + i];
    const float bj = P.b[stage * 4 + i];
    const float *__restrict__ st = P.state;
    float xs[PH_NX];
#pragma unroll
    for (int c = 0; c < PH_NX; ++c) xs[c] = st[c];
    const int t_state = reinterpret_cast<const int *>(st)[ST_TIME];
    const float alpha = P.alpha[0];
    const int t_plan = has_t ? P.t_plan[0] : 0;
    const double side_flags = has_side ? P.side[3] : 0.0;
    const int hs = lane < COVO_H - 1 ? lane + 1 : COVO_H - 1;  // lanes 0 .. 31: the stage that moves to stage `lane`
    float4 mean = make_float4(0.0f, 0.0f, 0.0f, 0.0f), cov0 = mean, cov1 = mean;
    if (has_mean && lane < COVO_H) mean = reinterpret_cast<const float4 *>(P.a_mean_src)[hs];
    if (has_cov) {  // float4 q of block m lies at 4 m + q; the lane owns float4s `lane` and `lane + 64`
        const int m0 = lane >> 2, m1 = (lane + 64) >> 2, q = lane & 3;
        cov0 = reinterpret_cast<const float4 *>(P.a_cov)[4 * (m0 + 1) + q];  // (m0 + 1 <= 16)
        cov1 = reinterpret_cast<const float4 *>(P.a_cov)[4 * (m1 < COVO_H - 1 ? m1 + 1 : COVO_H - 1) + q];
    }

    // ---- the law at stage j
    double dx[PH_NX];
#pragma unroll
    for (int c = 0; c < PH_NX; ++c) dx[c] = (double)xs[c] - xb[c];
    const double v0 = fma((double)alpha, kf, (double)bj);
    double v = v0;
#pragma unroll
    for (int c = 0; c < PH_NX; ++c) v = fma(k[c], dx[c], v);
    const bool flagged = side_flags != 0.0;
    const bool mismatch = has_t && t_state != t_plan + stage;
    const double cmd = mismatch ? v0 : v;
    const bool fin = __all(ph_finite(cmd) ? 1 : 0) != 0;
    const bool plan_only = flagged || !fin;  // clip(b_j)
    const double applied = plan_only ? (double)bj : cmd;
    const float u = plan_only ? qm::clip11_(bj) : (float)qm::clip11_(cmd);
    const int flags = (flagged ? 1 : 0) | ((!flagged && !fin) ? 2 : 0) | (mismatch ? 4 : 0);
    double gain = (plan_only || mismatch) ? 0.0 : fabs(v - v0);
    gain = fmax(gain, __shfl_xor(gain, 1));
    gain = fmax(gain, __shfl_xor(gain, 2));
    const int n_clip = __popcll(__ballot(fabs(applied) > 1.0 ? 1 : 0) & 0xFull);
    const double dpos = sqrt(fma(dx[2], dx[2], fma(dx[1], dx[1], dx[0] * dx[0])));

    // ---- stores: the shifted controller state, the action, the row
    const float u0 = __shfl(u, 0), u1 = __shfl(u, 1), u2 = __shfl(u, 2), u3 = __shfl(u, 3);
    if (has_mean && lane < COVO_H) reinterpret_cast<float4 *>(P.a_mean)[lane] = lane == 0 ? make_float4(u0, u1, u2, u3) : mean;
    if (has_cov) {
        reinterpret_cast<float4 *>(P.a_cov)[lane] = cov0;
        reinterpret_cast<float4 *>(P.a_cov)[lane + 64] = cov1;
    }
    if (P_.u_out != nullptr && lane < COVO_DU) P.u_out[lane] = u;
    if (lane < COVO_HOLD_FLOATS) {
        const float w = lane == 0   ? __int_as_float(stage)
                        : lane == 1 ? alpha
                        : lane == 2 ? (float)gain
                        : lane == 3 ? __int_as_float(n_clip)
                        : lane == 4 ? __int_as_float(flags)
                        : lane == 5 ? (float)dpos
                        : lane == 6 ? __int_as_float(t_state)
                                    : 0.0f;
        if (P_.row_out != nullptr) P.row_out[lane] = w;
        if (P_.log != nullptr && log_index >= 0) P.log[(size_t)log_index * COVO_HOLD_FLOATS + lane] = w;
    }
}

// the latch of a plan step, between its sweep and what follows it: b (the mean the sweep ran at, which the line search is about to
// overwrite) and the time word of the state the step planned from; the step's hold row {0, 0, 0, 0, 0, 0, bits(time), 0}
template <bool BATCHED>
__global__ __launch_bounds__(PH_BLOCK) void plan_latch_kernel(const LatchDesc P_, const LatchDesc *__restrict__ batch, const int log_index)
{
    LatchDesc Pb;
    if (BATCHED) {
        Pb = batch[blockIdx.x];
        Pb.a_mean = rebase_global(P_.a_mean, Pb.a_mean);
        Pb.state = rebase_global(P_.state, Pb.state);
        Pb.b_out = rebase_global(P_.b_out, Pb.b_out);
        Pb.t_out = rebase_global(P_.t_out, Pb.t_out);
        Pb.row_out = rebase_global(P_.row_out, Pb.row_out);
        Pb.log = rebase_global(P_.log, Pb.log);
    }
    const LatchDesc &P = BATCHED ? Pb : P_;
    const int lane = threadIdx.x;
    const int t = reinterpret_cast<const int *>(P.state)[ST_TIME];
    if (lane < COVO_H) reinterpret_cast<float4 *>(P.b_out)[lane] = reinterpret_cast<const float4 *>(P.a_mean)[lane];
    if (lane == COVO_H) P.t_out[0] = t;
    if (lane < COVO_HOLD_FLOATS) {
        const float w = lane == 6 ? __int_as_float(t) : 0.0f;
        if (P_.row_out != nullptr) P.row_out[lane] = w;
        if (P_.log != nullptr && log_index >= 0) P.log[(size_t)log_index * COVO_HOLD_FLOATS + lane] = w;
    }
}

// ---- host
// d: n_inst instances, all alike in what is attached (null or not); batched: the blocks go through device memory -- the handle's
// schedule (primitive = false) and the stateless entry (primitive = true) keep a cache each, so that neither makes the other upload
int launch_plan_hold(covo_ctx *h, const HoldDesc *d, int n_inst, bool batched, bool primitive, int stage, int log_index, hipStream_t s)
{
    if (stage < 0 || stage >= COVO_H || n_inst < 1 || n_inst > COVO_MAX_ENVS) {
        covo_set_error("plan hold: stage=%d outside [0, %d) or n_inst=%d outside (0, %d]", stage, COVO_H, n_inst, COVO_MAX_ENVS);
        return COVO_E_BADARG;
    }
    if (!batched) {
        hipLaunchKernelGGL(plan_hold_kernel<false>, dim3(1), dim3(PH_BLOCK), 0, s, d[0], (const HoldDesc *)nullptr, stage, log_index);
    } else {
        ArgBlockCache &c = primitive ? after_state(h)->hold_primitive : after_state(h)->hold;
        if (int rc = c.sync_upload(d, (size_t)n_inst * sizeof(HoldDesc), sizeof(HoldDesc), s)) return rc;
        hipLaunchKernelGGL(plan_hold_kernel<true>, dim3(n_inst), dim3(PH_BLOCK), 0, s, d[0], (const HoldDesc *)c.dev, stage, log_index);
    }
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_plan_latch(covo_ctx *h, const LatchDesc *d, int n_inst, bool batched, int log_index, hipStream_t s)
{
    if (!batched) {
        hipLaunchKernelGGL(plan_latch_kernel<false>, dim3(1), dim3(PH_BLOCK), 0, s, d[0], (const LatchDesc *)nullptr, log_index);
    } else {
        ArgBlockCache &c = after_state(h)->latch;
        if (int rc = c.sync_upload(d, (size_t)n_inst * sizeof(LatchDesc), sizeof(LatchDesc), s)) return rc;
        hipLaunchKernelGGL(plan_latch_kernel<true>, dim3(n_inst), dim3(PH_BLOCK), 0, s, d[0], (const LatchDesc *)c.dev, log_index);
    }
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
