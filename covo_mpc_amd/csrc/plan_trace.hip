// plan_trace.hip -- the flight recorder of a control step (gfx950): the controller's own plan and, inside an episode driver, the
// trace row of the step (covo_set_step_plan / covo_set_episode_trace, include/covo_hip.h).
//
// The plan of a step: a_plan = clip(a_new, -1, 1) with a_new the mean the step has just left in a_mean (covo.py:275, mppi.py:116,
// before the next step's shift), rolled out from the state the step planned from (covo.py:198) with exactly the inputs the step's
// sample rollouts had -- model constants, reward, rollover switch, trajectory window, discount and the same disturbance: the one
// shared vector of NONE / GAUSSIAN (0 under deterministic=True, MPPI's dyn_noise_scale * normal from the step key), or the step's
// per-step table of PERIODIC / SIN / DRAG / MIXED.  cost_plan is what the rollout kernel gives that action sequence, pos_plan[k]
// the position after rollout step k (the reference's `poses`, covo.py:234-237, for one sample).
//
// One launch per control step, one workgroup of three waves per instance, eager, behind the step and in front of the env step:
//   phase 0  the per-step scalars from the raw controller key (step_begin.hpp: step_begin_derive, as the fused small step derives
//            them per workgroup) and a_plan as a one-sample action image in LDS ([H][64] float4, every lane the same stripe)
//   phase 1  the rollout's own three stage waves on it (rollout_pipe.hpp: rp3_stages with A_LDS, N = 1, the instantiation the
//            step's reward / disturbance / rollover selects; PLAN: stage T's lane 0 also stores its new position per step).  Always
//            the general discount path: fma(discount^k, r, acc) is acc + r bit for bit at discount 1 (rollout_launch.hpp)
//   phase 2  the plan row {cost_plan, 0, 0, 0, pos_plan[H][3]} and, with a trace attached, the trace row {true state[32], noisy
//            state[32], u = a_new[0][0..3], plan row}: the PRE-step state of the env step that follows.
// The row index travels as a kernel argument, so nothing is captured and no step graph changes.  BATCHED: workgroup e takes its
// argument block from device memory (pointers through rebase_global, as step_small_kernel<..., BATCHED> does).
#include "after_step.hpp"

constexpr int PT_BLOCK = 3 * COVO_WAVE;
constexpr int PT_CH = 2;

struct PlanArgs {
    AfterHead head;           // R: the plan rollout, N = 1
    const float *a_mean;      // [128] the mean the step left
    const float *state_true;  // trace: the true state [32], or null
    float *plan_out;          // this instance's row of the plan buffer [COVO_PLAN_FLOATS], or null
    float *trace;             // this instance's trace rows [stride][COVO_TRACE_FLOATS], or null
    int nanp;
    int pad_;
};

// what rp3_stages<..., PLAN> takes in place of the statistics scratch: stage T's lane 0 writes pos[k]; the subscript only lets
// the (never instantiated at run time, STATS = false) statistics code of the stage compile
struct PlanPos {
    float pos[COVO_H][3];
    float unused_[1][9];
    __device__ float (&operator[](int))[1][9] { return unused_; }
};
struct PlanLds {
    float4 a[COVO_H][COVO_WAVE];  // 32 KiB: a_plan as the action image of one 64-sample group
    Rp3Lds<PT_CH> rings;          // 9 KiB
    PlanPos p;
    uint32_t dyn[12];
    DynBlock kb[4];               // after_derive's
    float cost;
};

template <bool ROLL, int REWARD, int FDIST, bool BATCHED>
__global__ __launch_bounds__(PT_BLOCK) void plan_trace_kernel(const PlanArgs P_, const PlanArgs *__restrict__ batch, const AfterDyn dyn)
{
    PlanArgs Pb;
    if (BATCHED) {
        Pb = batch[blockIdx.x];
        after_rebase_head(P_.head, Pb.head);
        Pb.a_mean = rebase_global(P_.a_mean, Pb.a_mean);
        Pb.state_true = rebase_global(P_.state_true, Pb.state_true);
        Pb.plan_out = rebase_global(P_.plan_out, Pb.plan_out);
        Pb.trace = rebase_global(P_.trace, Pb.trace);
    }
    const PlanArgs &P = BATCHED ? Pb : P_;
    __shared__ PlanLds S;
    const int tid = threadIdx.x, lane = tid & (COVO_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool has_plan = P_.plan_out != nullptr, has_trace = P_.trace != nullptr && dyn.row >= 0;  // (all instances alike)
    float *trow = has_trace ? P.trace + (size_t)dyn.row * COVO_TRACE_FLOATS : nullptr;

    // ---- phase 0
    after_derive(tid, P.head, dyn, BATCHED, S.kb, S.dyn);
    const float4 *__restrict__ am4 = reinterpret_cast<const float4 *>(P.a_mean);
    for (int i = tid; i < COVO_H * COVO_WAVE; i += PT_BLOCK) {
        float4 v = am4[i >> 6];
        if (P.nanp) { v.x = qm::clip11_nan_(v.x); v.y = qm::clip11_nan_(v.y); v.z = qm::clip11_nan_(v.z); v.w = qm::clip11_nan_(v.w); }
        else { v.x = qm::clip11_(v.x); v.y = qm::clip11_(v.y); v.z = qm::clip11_(v.z); v.w = qm::clip11_(v.w); }
        S.a[i >> 6][i & (COVO_WAVE - 1)] = v;
    }
    __syncthreads();
    RolloutArgs A = after_rollout_args(P.head, S.dyn);
    A.cost = has_plan ? P.plan_out : trow + 68;  // (stage R stores the one cost itself; phase 2 writes the same value again)

    // ---- phase 1: the plan rollout (covo.py:227-263 for the one sample a_plan)
    float cost = 0.0f;
    bool valid = false;
    int n = 0;
    rp3_stages<false, ROLL, PT_CH, -1, false, true, REWARD, FDIST, true, PlanPos, COVO_H, 1>(A, S.rings, S.p, wave, 0, 0, lane,
                                                                                                &S.a[0][0], cost, valid, n);
    if (wave == 2 && lane == 0) S.cost = cost;
    __syncthreads();

    // ---- phase 2: the rows
    if (tid < COVO_PLAN_FLOATS) {
        const float v = tid == 0 ? S.cost : (tid < 4 ? 0.0f : S.p.pos[(tid - 4) / 3][(tid - 4) % 3]);
        if (has_plan) P.plan_out[tid] = v;
        if (has_trace) trow[68 + tid] = v;
    }
    if (has_trace) {
        const int j = tid - 128;  // wave 2: the states travel as bit patterns (the time word is an integer)
        if (j >= 0 && j < COVO_STATE_FLOATS) {
            reinterpret_cast<uint32_t *>(trow)[j] = reinterpret_cast<const uint32_t *>(P.state_true)[j];
            reinterpret_cast<uint32_t *>(trow)[COVO_STATE_FLOATS + j] = reinterpret_cast<const uint32_t *>(A.state)[j];
        } else if (j >= COVO_STATE_FLOATS && j < COVO_STATE_FLOATS + COVO_DU) {
            trow[2 * COVO_STATE_FLOATS + (j - COVO_STATE_FLOATS)] = P.a_mean[j - COVO_STATE_FLOATS];  // u: what env_step_kernel reads
        }
    }
}

// ---- host
static void fill_plan_args(PlanArgs &P, covo_ctx *h, const PlanInstDesc &d, int e, const float *states_true)
{
    std::memset(&P, 0, sizeof(P));
    after_fill_head(P.head, h, d, ROLLOUT_CLIP_TRUSTED, false);  // one sample, its image is clipped in phase 0; the kernel sets A.cost
    P.a_mean = d.a_mean;
    P.state_true = states_true ? states_true + (size_t)e * COVO_STATE_FLOATS : nullptr;
    P.plan_out = h->plan_out ? h->plan_out + (size_t)e * COVO_PLAN_FLOATS : nullptr;
    P.trace = covo_eplog_inst(h, COVO_EPLOG_TRACE, e, COVO_TRACE_FLOATS);
    P.nanp = covo_propagate_nan(h) ? 1 : 0;
}

// inst: n_inst instances of ONE step, all alike in reward, rollover switch and disturbance kind (the step's own checks);
// states_true: [n_inst][32] for the trace row (trace_index >= 0), else null.  batched: the argument blocks go through device
// memory, re-uploaded (behind a stream synchronisation, outside the steady state) only when they differ from the last launch's.
int launch_plan_trace(covo_ctx *h, const PlanInstDesc *inst, int n_inst, bool batched, const float *states_true, int trace_index,
                      hipStream_t s)
{
    const bool trace = h->eplog[COVO_EPLOG_TRACE].log != nullptr && trace_index >= 0;
    if (h->plan_out == nullptr && !trace) return 0;
    const int row = trace ? trace_index : -1;
    if (int rc = after_check_tables(inst, n_inst, "plan trace")) return rc;
    if (!batched) {
        PlanArgs P;
        fill_plan_args(P, h, inst[0], 0, trace ? states_true : nullptr);
        AFTER_DISPATCH(plan_trace_kernel, PT_BLOCK, P, (const PlanArgs *)nullptr, 1, after_dyn_single(inst[0], row), s);
    } else {
        std::vector<PlanArgs> now(n_inst);
        for (int e = 0; e < n_inst; ++e) fill_plan_args(now[e], h, inst[e], e, trace ? states_true : nullptr);
        ArgBlockCache &c = after_state(h)->plan;
        if (int rc = c.sync_upload(now.data(), now.size() * sizeof(PlanArgs), sizeof(PlanArgs), s)) return rc;
        AFTER_DISPATCH(plan_trace_kernel, PT_BLOCK, now[0], (const PlanArgs *)c.dev, n_inst, after_dyn_batched(row), s);
    }
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
