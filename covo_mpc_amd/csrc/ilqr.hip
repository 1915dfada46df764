// ilqr.hip -- what a control step without samples needs around the Riccati line search (gfx950): COVO_MODE_ILQR / covo_set_step_ilqr,
// include/covo_hip.h.
//
// An iLQR step is   b_0 = shift(a_mean);   b_{j+1} = riccati line search at b_j, j < k;   a_mean <- b_k   -- the k iterations are the
// launches of riccati_after (step.hip) as they stand: Hessian KB -> chains -> sweep -> [latch] -> [generator] -> line search, all on
// the step's one state with the step's one raw key.  Two small kernels frame them:
//
//   ilqr_begin_kernel   the begin work of every step, without a sample buffer in sight: the mean shifted IN PLACE (or from the caller's
//                       input mean into the handle's), the per-step scalars derived from the raw key exactly as step_begin_kernel /
//                       batch_mode_begin_kernel derive them (step_begin_derive: act key to dyn[0..1], the shared vector to [2..4], the
//                       raw key parked at [10..11], where the disturbance tables and the after-step frame read it).  The sampling
//                       begin kernels leave the shifted mean in a scratch of their own for the noise kernels; here the line search
//                       refines a_mean itself, so the shift has to land there.  One wave per instance: every lane has loaded its two
//                       floats before any lane stores (in place is safe).
//   ilqr_tally_kernel   behind every iteration's line search: the instance's Riccati row and feedback row into slot j of the
//                       per-iteration logs, and the summary row
//                           float[8] = {row_0.cost_base, row_j.cost_chosen, bits(iterations with choice != 0),
//                                       bits(first j with choice 0; k: none), bits(iterations with choice > 16),
//                                       bits(OR of the rows' flag words), |g|_2 of the last iteration, 0}
//                       updated in place (iteration 0 starts it).  One workgroup of ONE wave per instance, lane = word of the row;
//                       batched instances take their argument block from device memory, pointers through rebase_global, as
//                       plan_latch_kernel does; j and k are kernel arguments, so the blocks of a steady-state schedule never change.
#include "after_step.hpp"

constexpr int IL_BLOCK = COVO_WAVE;

struct IlqrKeys {
    uint32_t w[COVO_MAX_ENVS][2];  // instance e's raw rng_act
};

__global__ __launch_bounds__(IL_BLOCK) void ilqr_begin_kernel(const float *__restrict__ a_mean_src, float *a_mean, uint32_t *__restrict__ dyn,
                                                              const IlqrKeys keys, const int derive_keys, const float shared_noise_scale)
{
    const int e = blockIdx.x, lane = threadIdx.x;
    const float *src = a_mean_src + (size_t)e * COVO_NA;
    float *dst = a_mean + (size_t)e * COVO_NA;
    // floats `lane` and `lane + 64` of the shifted mean: [a_mean[1:], a_mean[31]]
    const int i0 = lane, i1 = lane + COVO_WAVE;
    const float v0 = src[i0 + COVO_DU];  // (i0 + 4 <= 67)
    const float v1 = src[i1 < COVO_NA - COVO_DU ? i1 + COVO_DU : i1];
    if (lane < 4) {
        DynBlock blk;
#pragma unroll
        for (int w = 0; w < 12; ++w) blk.w[w] = 0u;
        blk.w[0] = keys.w[e][0];
        blk.w[1] = keys.w[e][1];
        step_begin_derive(lane, blk, derive_keys, shared_noise_scale, dyn + 12 * e);
    }
    dst[i0] = v0;
    dst[i1] = v1;
}

template <bool BATCHED>
__global__ __launch_bounds__(IL_BLOCK) void ilqr_tally_kernel(const IlqrTallyDesc P_, const IlqrTallyDesc *__restrict__ batch, const int j,
                                                              const int k)
{
    IlqrTallyDesc Pb;
    if (BATCHED) {
        Pb = batch[blockIdx.x];
        Pb.row = rebase_global(P_.row, Pb.row);
        Pb.fb_row = rebase_global(P_.fb_row, Pb.fb_row);
        Pb.rows_log = rebase_global(P_.rows_log, Pb.rows_log);
        Pb.fb_log = rebase_global(P_.fb_log, Pb.fb_log);
        Pb.summary = rebase_global(P_.summary, Pb.summary);
        Pb.masks = rebase_global(P_.masks, Pb.masks);
        Pb.box_log = rebase_global(P_.box_log, Pb.box_log);
    }
    const IlqrTallyDesc &P = BATCHED ? Pb : P_;
    // (what is attached is the same for all instances)
    const bool has_fb = P_.fb_row != nullptr, has_rows = P_.rows_log != nullptr, has_fb_log = P_.fb_log != nullptr, has_sum = P_.summary != nullptr;
    const int lane = threadIdx.x, w = lane & 7;  // (the octets repeat each other: the loads are broadcasts)
    const float r = P.row[w];
    const float f = has_fb ? P.fb_row[w] : 0.0f;
    const float prev = (has_sum && j > 0) ? P.summary[w] : 0.0f;
    if (lane < COVO_RICCATI_FLOATS) {
        if (has_rows) P.rows_log[(size_t)j * COVO_RICCATI_FLOATS + lane] = r;
        if (has_fb_log) P.fb_log[(size_t)j * COVO_FEEDBACK_FLOATS + lane] = f;
    }
    // the box sweep's clamped coordinates: lane k < H holds stage k's mask, one ballot per bit
    if (P_.box_log != nullptr) {
        const int m = lane < COVO_H ? P.masks[lane] : 0;
        int n = 0;
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) n += __popcll(__ballot((m >> bit) & 1));
        if (lane == 0) P.box_log[j] = n;
    }
    if (!has_sum) return;
    const int choice = __float_as_int(__shfl(r, 2));
    const int flags = __float_as_int(__shfl(r, 7));
    const float gnorm = __shfl(r, 4);  // (all lanes active: not inside the select below)
    const int pi = __float_as_int(prev);
    const int fixed_prev = j > 0 ? pi : k;
    const float out = w == 0   ? (j > 0 ? prev : r)                                             // row_0.cost_base
                      : w == 1 ? r                                                               // row_j.cost_chosen
                      : w == 2 ? __int_as_float(pi + (choice != 0 ? 1 : 0))
                      : w == 3 ? __int_as_float((fixed_prev == k && choice == 0) ? j : fixed_prev)
                      : w == 4 ? __int_as_float(pi + (choice > COVO_REFINE_CANDIDATES - 1 ? 1 : 0))
                      : w == 5 ? __int_as_float(pi | flags)
                      : w == 6 ? gnorm                                                           // |g|_2
                               : 0.0f;
    if (lane < COVO_ILQR_FLOATS) P.summary[lane] = out;
}

// ---- host
// the begin work of n_inst dense instances: a_mean_src / a_mean [n][128], dyn [n][12], keys [n][2] (host)
int launch_ilqr_begin(const float *a_mean_src, float *a_mean, uint32_t *dyn, const uint32_t *keys, int n_inst, int derive_keys,
                      float shared_noise_scale, hipStream_t s)
{
    IlqrKeys k;
    std::memset(&k, 0, sizeof(k));
    for (int e = 0; e < n_inst; ++e) {
        k.w[e][0] = keys[2 * e];
        k.w[e][1] = keys[2 * e + 1];
    }
    hipLaunchKernelGGL(ilqr_begin_kernel, dim3(n_inst), dim3(IL_BLOCK), 0, s, a_mean_src, a_mean, dyn, k, derive_keys, shared_noise_scale);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

// iteration j of k of the handle's n_inst instances (no-op with nothing attached); batched: the blocks go through device memory
int launch_ilqr_tally(covo_ctx *h, int n_inst, bool batched, int j, int k, hipStream_t s)
{
    const bool box = covo_box_on(h) && h->ilqr_box != nullptr;  // (covo_set_step_ilqr_box: the count needs the box sweep's masks)
    if (h->ilqr_rows == nullptr && h->ilqr_fb_rows == nullptr && h->ilqr_summary == nullptr && !box) return 0;
    IlqrTallyDesc d[COVO_MAX_ENVS];
    const size_t log = (size_t)COVO_MAX_STEP_ITERS * COVO_RICCATI_FLOATS;
    for (int e = 0; e < n_inst; ++e) {
        d[e].row = h->riccati_out + (size_t)e * COVO_RICCATI_FLOATS;
        d[e].fb_row = covo_feedback_on(h) ? h->feedback_out + (size_t)e * COVO_FEEDBACK_FLOATS : nullptr;
        d[e].rows_log = h->ilqr_rows ? h->ilqr_rows + (size_t)e * log : nullptr;
        d[e].fb_log = h->ilqr_fb_rows ? h->ilqr_fb_rows + (size_t)e * log : nullptr;
        d[e].summary = h->ilqr_summary ? h->ilqr_summary + (size_t)e * COVO_ILQR_FLOATS : nullptr;
        d[e].masks = box ? h->box_masks + (size_t)e * COVO_H : nullptr;
        d[e].box_log = box ? h->ilqr_box + (size_t)e * COVO_MAX_STEP_ITERS : nullptr;
    }
    if (!batched) {
        hipLaunchKernelGGL(ilqr_tally_kernel<false>, dim3(1), dim3(IL_BLOCK), 0, s, d[0], (const IlqrTallyDesc *)nullptr, j, k);
    } else {
        ArgBlockCache &c = after_state(h)->ilqr;
        if (int rc = c.sync_upload(d, (size_t)n_inst * sizeof(IlqrTallyDesc), sizeof(IlqrTallyDesc), s)) return rc;
        hipLaunchKernelGGL(ilqr_tally_kernel<true>, dim3(n_inst), dim3(IL_BLOCK), 0, s, d[0], (const IlqrTallyDesc *)c.dev, j, k);
    }
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
