// update_arbiter.hip -- the update arbiter of a control step (gfx950): the step commits the best of {softmax mean, old plan, best
// sample} instead of the softmax mean unchecked (covo_arbitrate / covo_set_step_arbiter / covo_set_episode_arbiter_log,
// include/covo_hip.h).
//
// Three candidates per instance, each [H][4]:
//   0  the softmax mean the step has just left in a_mean (covo.py:275, mppi.py:116)
//   1  the nominal: the shifted mean the step sampled around (covo.py:201-203)
//   2  the best sample a[:, n*, :], n* = argmin_n cost[n] over the step's own costs (NaN skipped, equal costs -> lowest n; all NaN:
//      the candidate is absent, n* = -1)
// Candidates 0 and 1 are clipped to [-1, 1] for evaluation only (as the plan is, plan_trace.hip); every candidate is rolled out by
// the rollout's own stage functions with exactly the inputs the step's sample rollouts had.  mask bit c enables candidate c; a
// masked-out or absent candidate costs +inf, a NaN cost counts as +inf, equal costs resolve to the lowest candidate, all +inf -> 0.
// Choice 0 leaves a_mean alone, 1 writes the nominal (unclipped), 2 writes a[:, n*, :].
//
// One launch, one workgroup of three waves per instance, eager, behind the step and ahead of the plan / fan launches:
//   phase 0  the per-step scalars from the raw controller key (step_begin.hpp: step_begin_derive); the argmin over cost[0..N): 16-byte
//            loads where aligned, one 64-bit key {order-preserving cost bits, index} per sample so that one `min` carries the
//            tie-break, reduced in the wave (wave_reduce.hpp) and across the three waves through LDS; the LDS action image [H][64]
//            float4: lane 0 = clip(candidate 0), lane 1 = clip(candidate 1), lanes >= 2 = candidate 2
//   phase 1  the rollout's three stage waves on the image (rollout_pipe.hpp: rp3_stages with A_LDS, N = 64, the general discount
//            path as in plan_trace.hip; PLAN = 3: no positions, stage R hands its costs back)
//   phase 2  one lane decides; the workgroup writes the chosen candidate's 128 floats into a_mean (nothing for choice 0) and the
//            arbiter row {cost_softmax, cost_nominal, cost_best, cost_chosen, bits(choice), bits(n_best), 0, 0}.
// The row index of the episode log travels as a kernel argument: nothing is captured, no step graph changes.  BATCHED: workgroup e
// takes its argument block from device memory (pointers through rebase_global, as sample_fan_kernel does).
#include "after_step.hpp"
#include "wave_reduce.hpp"

constexpr int UA_BLOCK = 3 * COVO_WAVE;
constexpr int UA_CH = 2;

struct ArbArgs {
    AfterHead head;          // R: the step's sample rollout with a and N; R.clip applies to candidate 2's stripe
    const float *cost;       // [N] the step's costs
    const float *a_nominal;  // [128] the shifted mean the step sampled around
    float *a_mean;           // [128] in: the softmax mean; out: the chosen candidate
    float *row_out;          // this instance's [COVO_ARB_FLOATS] of the arbiter buffer, or null
    float *arblog;           // this instance's [stride][COVO_ARB_FLOATS] of the episode log, or null
    int mask;
    int nanp;
};

// what rp3_stages<..., PLAN = 3> takes in place of the statistics scratch: never touched; the subscript only lets the (never
// instantiated at run time, STATS = false) statistics code of the stage compile
struct ArbNoPos {
    float unused_[1][9];
    __device__ float (&operator[](int))[1][9] { return unused_; }
};
struct ArbLds {
    float4 a[COVO_H][COVO_WAVE];  // 32 KiB: the action image of the one 64-sample group
    Rp3Lds<UA_CH> rings;          // 9 KiB
    ArbNoPos p;
    float4 raw[3][COVO_H];        // the candidates as they are committed (unclipped)
    uint32_t dyn[12];
    DynBlock kb[4];
    unsigned long long red[3];
    float cost[COVO_WAVE];
    int choice;
};

// the argmin key of sample i: cost bits in an order-preserving unsigned form above the index; NaN -> the largest key
__device__ __forceinline__ unsigned long long arb_key(float v, int i)
{
    if (!(v == v)) return ~0ull;
    if (v == 0.0f) v = 0.0f;  // -0 and +0 are one cost
    uint32_t u = __float_as_uint(v);
    u = (u >> 31) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (uint32_t)i;
}
__device__ __forceinline__ unsigned long long arb_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

template <bool ROLL, int REWARD, int FDIST, bool BATCHED>
__global__ __launch_bounds__(UA_BLOCK) void update_arbiter_kernel(const ArbArgs P_, const ArbArgs *__restrict__ batch, const AfterDyn dyn)
{
    ArbArgs Pb;
    if (BATCHED) {
        Pb = batch[blockIdx.x];
        after_rebase_head(P_.head, Pb.head);
        Pb.head.R.a = rebase_global(P_.head.R.a, Pb.head.R.a);
        Pb.cost = rebase_global(P_.cost, Pb.cost);
        Pb.a_nominal = rebase_global(P_.a_nominal, Pb.a_nominal);
        Pb.a_mean = rebase_global(P_.a_mean, Pb.a_mean);
        Pb.row_out = rebase_global(P_.row_out, Pb.row_out);
        Pb.arblog = rebase_global(P_.arblog, Pb.arblog);
    }
    const ArbArgs &P = BATCHED ? Pb : P_;
    __shared__ ArbLds S;
    const int tid = threadIdx.x, lane = tid & (COVO_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = P_.head.R.N, mask = P_.mask;  // (all instances alike)
    const bool has_row = P_.row_out != nullptr, has_log = P_.arblog != nullptr && dyn.row >= 0;

    // ---- phase 0
    after_derive(tid, P.head, dyn, BATCHED, S.kb, S.dyn);
    {  // the argmin of the step's costs
        const float *__restrict__ c = P.cost;
        int head = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(c) & 15u)) & 15u) >> 2);  // floats in front of the first 16-byte line
        head = head < N ? head : N;
        const int nb = (N - head) >> 2, tail = head + 4 * nb;
        unsigned long long best = ~0ull;
        if (tid < head) best = arb_key(c[tid], tid);
        const float4 *__restrict__ c4 = reinterpret_cast<const float4 *>(c + head);
        constexpr int UA_INFLIGHT = 8;  // 16-byte loads a lane issues before it looks at the first: one workgroup has to cover the latency itself
        const float qnan = __builtin_nanf("");
        for (int j0 = tid; j0 < nb; j0 += UA_BLOCK * UA_INFLIGHT) {
            float4 v[UA_INFLIGHT];
#pragma unroll
            for (int u = 0; u < UA_INFLIGHT; ++u) {
                const int j = j0 + u * UA_BLOCK;
                v[u] = j < nb ? c4[j] : make_float4(qnan, qnan, qnan, qnan);
            }
#pragma unroll
            for (int u = 0; u < UA_INFLIGHT; ++u) {
                const int i = head + 4 * (j0 + u * UA_BLOCK);
                best = arb_min(best, arb_min(arb_min(arb_key(v[u].x, i), arb_key(v[u].y, i + 1)),
                                             arb_min(arb_key(v[u].z, i + 2), arb_key(v[u].w, i + 3))));
            }
        }
        if (tail + tid < N) best = arb_min(best, arb_key(c[tail + tid], tail + tid));
        best = wr::wave64_allmin_u64(best);
        if (lane == 0) S.red[wave] = best;
    }
    __syncthreads();
    const unsigned long long best = arb_min(S.red[0], arb_min(S.red[1], S.red[2]));
    const int n_best = best == ~0ull ? -1 : (int)(uint32_t)best;
    {
        const float4 *__restrict__ am4 = reinterpret_cast<const float4 *>(P.a_mean);
        const float4 *__restrict__ nom4 = reinterpret_cast<const float4 *>(P.a_nominal);
        const float4 *__restrict__ a4 = P.head.R.a;
        const int clip = P_.head.R.clip, nanp = P_.nanp;
        for (int i = tid; i < COVO_H * COVO_WAVE; i += UA_BLOCK) {
            const int k = i >> 6, l = i & (COVO_WAVE - 1);
            float4 v;
            if (l == 0) v = am4[k];
            else if (l == 1) v = nom4[k];
            else if (n_best >= 0) v = a4[(size_t)k * N + n_best];
            else v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (l < 3) S.raw[l][k] = v;
            const int how = l < 2 ? (nanp ? 2 : 1) : clip;
            if (how == 1) { v.x = qm::clip11_(v.x); v.y = qm::clip11_(v.y); v.z = qm::clip11_(v.z); v.w = qm::clip11_(v.w); }
            else if (how == 2) { v.x = qm::clip11_nan_(v.x); v.y = qm::clip11_nan_(v.y); v.z = qm::clip11_nan_(v.z); v.w = qm::clip11_nan_(v.w); }
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
    rp3_stages<false, ROLL, UA_CH, -1, false, true, REWARD, FDIST, true, ArbNoPos, COVO_H, 3>(A, S.rings, S.p, wave, 0, 0, lane,
                                                                                               &S.a[0][0], cost, valid, n);
    if (wave == 2) S.cost[lane] = cost;
    __syncthreads();

    // ---- phase 2: the decision, the mean, the row
    float *lrow = has_log ? P.arblog + (size_t)dyn.row * COVO_ARB_FLOATS : nullptr;
    if (tid == 0) {
        const float inf = __builtin_inff();
        float c[3];
        c[0] = (mask & 1) ? S.cost[0] : inf;
        c[1] = (mask & 2) ? S.cost[1] : inf;
        c[2] = ((mask & 4) && n_best >= 0) ? S.cost[2] : inf;
        int choice = 0;
        float cb = inf;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (c[q] < cb) {  // (a NaN cost never wins; equal costs keep the lower candidate)
                cb = c[q];
                choice = q;
            }
        }
        S.choice = choice;
        const float row[COVO_ARB_FLOATS] = {c[0], c[1], c[2], c[choice], __int_as_float(choice), __int_as_float(n_best), 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < COVO_ARB_FLOATS; ++j) {
            if (has_row) P.row_out[j] = row[j];
            if (has_log) lrow[j] = row[j];
        }
    }
    __syncthreads();
    const int choice = S.choice;
    if (choice != 0 && tid < COVO_H) reinterpret_cast<float4 *>(P.a_mean)[tid] = S.raw[choice][tid];
}

// the nominal of the env-batched fused step (step_small.hip keeps its shifted mean in LDS only): shift(a_mean) (covo.py:201-203)
// per instance, ahead of the step
__global__ void arbiter_nominal_kernel(const float *__restrict__ a_mean, float *__restrict__ nominal)
{
    const int e = blockIdx.x, i = threadIdx.x;
    nominal[e * COVO_NA + i] = (i < COVO_NA - COVO_DU) ? a_mean[e * COVO_NA + i + COVO_DU] : a_mean[e * COVO_NA + i];
}

// ---- host
// the handle's after-step state (after_step.hpp) goes: the three launches' argument blocks and the nominals
void after_state_destroy(covo_ctx *h)
{
    AfterState *as = reinterpret_cast<AfterState *>(h->after);
    if (!as) return;
    for (ArgBlockCache *c : {&as->arbiter, &as->plan, &as->fan, &as->refine, &as->feedback, &as->hold, &as->hold_primitive, &as->latch, &as->ilqr, &as->est, &as->est_primitive, &as->obs, &as->obs_primitive}) (void)hipFree(c->dev);
    (void)hipFree(as->nominal);
    delete as;
    h->after = nullptr;
}

int launch_arbiter_nominal(covo_ctx *h, const float *a_mean, int n_inst, hipStream_t s, const float **nominal_out)
{
    AfterState *as = after_state(h);
    if (as->nominal == nullptr) COVO_CHECK_HIP(hipMalloc(&as->nominal, (size_t)COVO_MAX_ENVS * COVO_NA * sizeof(float)));
    if (a_mean != nullptr) {
        hipLaunchKernelGGL(arbiter_nominal_kernel, dim3(n_inst), dim3(COVO_NA), 0, s, a_mean, as->nominal);
        COVO_CHECK_HIP(hipGetLastError());
    }
    if (nominal_out) *nominal_out = as->nominal;
    return 0;
}

static void fill_arb_args(ArbArgs &P, covo_ctx *h, const PlanInstDesc &d, RolloutClip clip, int mask, float *row_out, float *arblog)
{
    std::memset(&P, 0, sizeof(P));
    after_fill_head(P.head, h, d, clip, true);
    P.cost = d.cost;
    P.a_nominal = d.a_nominal;
    P.a_mean = d.a_mean_out;
    P.row_out = row_out;
    P.arblog = arblog;
    P.mask = mask;
    P.nanp = covo_propagate_nan(h) ? 1 : 0;
}

// covo_arbitrate: one instance, the caller's buffers and shared vector (d.derive_keys = 0), the clip covo_rollout_cost applies
int launch_update_arbiter_one(covo_ctx *h, const PlanInstDesc &d, RolloutClip clip, int mask, float *row_out, hipStream_t s)
{
    if (int rc = after_check_tables(&d, 1, "update arbiter")) return rc;
    ArbArgs P;
    fill_arb_args(P, h, d, clip, mask, row_out, nullptr);
    AFTER_DISPATCH(update_arbiter_kernel, UA_BLOCK, P, (const ArbArgs *)nullptr, 1, after_dyn_single(d, -1), s);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

// inst: n_inst instances of ONE step that has just been enqueued (launch_plan_trace's descriptors, with a, N, cost, a_nominal and
// a_mean_out).  The stripes come from the step's own noise launch: already clipped.  batched: the argument blocks go through device
// memory, re-uploaded (behind a stream synchronisation, outside the steady state) only when they differ from the last launch's.
int launch_update_arbiter(covo_ctx *h, const PlanInstDesc *inst, int n_inst, bool batched, int log_index, hipStream_t s)
{
    if (!covo_arb_on(h)) return 0;
    const int row = (h->eplog[COVO_EPLOG_ARB].log != nullptr && log_index >= 0) ? log_index : -1;
    if (int rc = after_check_tables(inst, n_inst, "update arbiter")) return rc;
    auto fill = [&](ArbArgs &P, int e) {
        fill_arb_args(P, h, inst[e], ROLLOUT_CLIP_TRUSTED, h->arb_mask, h->arb_out + (size_t)e * COVO_ARB_FLOATS,
                      covo_eplog_inst(h, COVO_EPLOG_ARB, e, COVO_ARB_FLOATS));
    };
    if (!batched) {
        ArbArgs P;
        fill(P, 0);
        AFTER_DISPATCH(update_arbiter_kernel, UA_BLOCK, P, (const ArbArgs *)nullptr, 1, after_dyn_single(inst[0], row), s);
    } else {
        std::vector<ArbArgs> now(n_inst);
        for (int e = 0; e < n_inst; ++e) fill(now[e], e);
        ArgBlockCache &c = after_state(h)->arbiter;
        if (int rc = c.sync_upload(now.data(), now.size() * sizeof(ArbArgs), sizeof(ArbArgs), s)) return rc;
        AFTER_DISPATCH(update_arbiter_kernel, UA_BLOCK, now[0], (const ArbArgs *)c.dev, n_inst, after_dyn_batched(row), s);
    }
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
