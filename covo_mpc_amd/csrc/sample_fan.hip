// sample_fan.hip -- the sample fan of a control step (gfx950): K of the step's N sampled rollouts as trajectories
// (covo_rollout_fan / covo_set_step_fan / covo_set_episode_fan, include/covo_hip.h).
//
// The fan of one instance: K rows {cost_s, bits(int32 n_s), 0, 0, pos_s[H][3]}, the layout of a plan row.  n_s is the local sample
// the row was taken from (the caller's idx clamped into [0, N), or the stride (s N) / K), pos_s[k] its position after rollout step k
// (the reference's poses[k, n_s], covo.py:234-237 / mppi.py:77-80; they keep integrating after done), cost_s what the rollout's
// stage functions give the action stripe a[:, n_s, :] with the step's own inputs -- the value the step's rollout left in cost[n_s],
// bit for bit.
//
// One launch, one workgroup of three waves per instance, eager, behind the step (and behind the plan launch, if attached):
//   phase 0  the per-step scalars from the raw controller key (step_begin.hpp: step_begin_derive; the stand-alone entry passes its
//            shared vector through with derive_keys = 0), the sample of every lane, and the gather a[t][n_lane] into the LDS action
//            image [H][64] float4.  Lanes >= K take lane K - 1's stripe and are never stored.
//   phase 1  the rollout's own three stage waves on the image (rollout_pipe.hpp: rp3_stages with A_LDS, N = 64, the general
//            discount path as in plan_trace.hip; PLAN = 2: stage T stores every lane's new position per step to an LDS tile
//            [H][3][64], stage R hands its costs back instead of storing them)
//   phase 2  the K rows, coalesced, to the step's fan buffer and / or row `log_index` of the episode's fan log.
// The row index travels as a kernel argument, so nothing is captured and no step graph changes.  BATCHED: workgroup e takes its
// argument block from device memory (pointers through rebase_global, as plan_trace_kernel does).
#include "after_step.hpp"

constexpr int SF_BLOCK = 3 * COVO_WAVE;
constexpr int SF_CH = 2;

struct FanArgs {
    AfterHead head;      // R: the step's sample rollout with a and N
    const int32_t *idx;  // [K] the caller's sample indices, or null: the stride
    float *fan_out;      // this instance's [K][COVO_FAN_FLOATS] of the fan buffer, or null
    float *fanlog;       // this instance's [stride][K][COVO_FAN_FLOATS] of the episode log, or null
    int K;
    int pad_;
};

// what rp3_stages<..., PLAN = 2> takes in place of the statistics scratch: stage T's lane l writes pos[k][.][l]; the subscript
// only lets the (never instantiated at run time, STATS = false) statistics code of the stage compile
struct FanPos {
    float pos[COVO_H][3][COVO_WAVE];  // 24 KiB: conflict-free stores (lane = bank), phase 2 reads them row by row
    float unused_[1][9];
    __device__ float (&operator[](int))[1][9] { return unused_; }
};
struct FanLds {
    float4 a[COVO_H][COVO_WAVE];  // 32 KiB: the action image of the fan's one 64-sample group
    Rp3Lds<SF_CH> rings;          // 9 KiB
    FanPos p;
    uint32_t dyn[12];
    DynBlock kb[4];
    float cost[COVO_WAVE];
    int n[COVO_WAVE];
};

template <bool ROLL, int REWARD, int FDIST, bool BATCHED>
__global__ __launch_bounds__(SF_BLOCK) void sample_fan_kernel(const FanArgs P_, const FanArgs *__restrict__ batch, const AfterDyn dyn)
{
    FanArgs Pb;
    if (BATCHED) {
        Pb = batch[blockIdx.x];
        after_rebase_head(P_.head, Pb.head);
        Pb.head.R.a = rebase_global(P_.head.R.a, Pb.head.R.a);
        Pb.idx = rebase_global(P_.idx, Pb.idx);
        Pb.fan_out = rebase_global(P_.fan_out, Pb.fan_out);
        Pb.fanlog = rebase_global(P_.fanlog, Pb.fanlog);
    }
    const FanArgs &P = BATCHED ? Pb : P_;
    __shared__ FanLds S;
    const int tid = threadIdx.x, lane = tid & (COVO_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = P_.K, N = P_.head.R.N;  // (all instances alike)
    const bool has_fan = P_.fan_out != nullptr, has_log = P_.fanlog != nullptr && dyn.row >= 0;
    const bool has_idx = P_.idx != nullptr;

    // ---- phase 0
    after_derive(tid, P.head, dyn, BATCHED, S.kb, S.dyn);
    if (wave == 1) {  // the sample of every lane: lanes >= K repeat lane K - 1's
        const int s = lane < K ? lane : K - 1;
        int n;
        if (has_idx) {
            n = P.idx[s];
            n = n < 0 ? 0 : (n > N - 1 ? N - 1 : n);
        } else {
            n = (int)(((long long)s * N) / K);
        }
        S.n[lane] = n;
    }
    __syncthreads();
    {
        const float4 *__restrict__ a4 = P.head.R.a;
        const int clip = P_.head.R.clip;
        for (int i = tid; i < COVO_H * COVO_WAVE; i += SF_BLOCK) {
            const int k = i >> 6, l = i & (COVO_WAVE - 1);
            float4 v = a4[(size_t)k * N + S.n[l]];
            if (clip == 1) { v.x = qm::clip11_(v.x); v.y = qm::clip11_(v.y); v.z = qm::clip11_(v.z); v.w = qm::clip11_(v.w); }
            else if (clip == 2) { v.x = qm::clip11_nan_(v.x); v.y = qm::clip11_nan_(v.y); v.z = qm::clip11_nan_(v.z); v.w = qm::clip11_nan_(v.w); }
            S.a[k][l] = v;
        }
    }
    __syncthreads();
    RolloutArgs A = after_rollout_args(P.head, S.dyn);
    A.N = COVO_WAVE;  // the image holds one full group: every lane is a sample of its own
    A.clip = 0;
    A.cost = nullptr;  // (PLAN = 2: stage R stores nothing)
    A.groupmin = nullptr;

    // ---- phase 1: the fan's rollouts (covo.py:227-263 for the samples n_lane)
    float cost = 0.0f;
    bool valid = false;
    int n = 0;
    rp3_stages<false, ROLL, SF_CH, -1, false, true, REWARD, FDIST, true, FanPos, COVO_H, 2>(A, S.rings, S.p, wave, 0, 0, lane,
                                                                                             &S.a[0][0], cost, valid, n);
    if (wave == 2) S.cost[lane] = cost;
    __syncthreads();

    // ---- phase 2: the rows
    float *lrow = has_log ? P.fanlog + (size_t)dyn.row * K * COVO_FAN_FLOATS : nullptr;
    for (int i = tid; i < K * COVO_FAN_FLOATS; i += SF_BLOCK) {
        const int s = i / COVO_FAN_FLOATS, j = i - s * COVO_FAN_FLOATS;
        float v;
        if (j == 0) v = S.cost[s];
        else if (j == 1) v = __int_as_float(S.n[s]);
        else if (j < 4) v = 0.0f;
        else v = S.p.pos[(j - 4) / 3][(j - 4) % 3][s];
        if (has_fan) P.fan_out[i] = v;
        if (has_log) lrow[i] = v;
    }
}

// ---- host
static void fill_fan_args(FanArgs &P, covo_ctx *h, const PlanInstDesc &d, RolloutClip clip, const int32_t *idx, int K, float *fan_out,
                          float *fanlog)
{
    std::memset(&P, 0, sizeof(P));
    after_fill_head(P.head, h, d, clip, true);
    P.idx = idx;
    P.fan_out = fan_out;
    P.fanlog = fanlog;
    P.K = K;
}

// covo_rollout_fan: one instance, the caller's buffers and shared vector (d.derive_keys = 0), the clip covo_rollout_cost applies
int launch_sample_fan_one(covo_ctx *h, const PlanInstDesc &d, RolloutClip clip, const int32_t *idx, int K, float *fan_out, hipStream_t s)
{
    if (int rc = after_check_tables(&d, 1, "sample fan")) return rc;
    FanArgs P;
    fill_fan_args(P, h, d, clip, idx, K, fan_out, nullptr);
    AFTER_DISPATCH(sample_fan_kernel, SF_BLOCK, P, (const FanArgs *)nullptr, 1, after_dyn_single(d, -1), s);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

// inst: n_inst instances of ONE step that has just been enqueued (launch_plan_trace's descriptors, with a and N).  The stripes
// come from the step's own noise launch: already clipped.  batched: the argument blocks go through device memory, re-uploaded
// (behind a stream synchronisation, outside the steady state) only when they differ from the last launch's.
int launch_sample_fan(covo_ctx *h, const PlanInstDesc *inst, int n_inst, bool batched, int log_index, hipStream_t s)
{
    const bool log = h->eplog[COVO_EPLOG_FAN].log != nullptr && log_index >= 0;
    if (h->fan_out == nullptr && !log) return 0;
    const int K = h->fan_K, row = log ? log_index : -1;
    if (int rc = after_check_tables(inst, n_inst, "sample fan")) return rc;
    auto fill = [&](FanArgs &P, int e) {
        fill_fan_args(P, h, inst[e], ROLLOUT_CLIP_TRUSTED, h->fan_idx ? h->fan_idx + (size_t)e * K : nullptr, K,
                      h->fan_out ? h->fan_out + (size_t)e * K * COVO_FAN_FLOATS : nullptr, covo_eplog_inst(h, COVO_EPLOG_FAN, e, K * COVO_FAN_FLOATS));
    };
    if (!batched) {
        FanArgs P;
        fill(P, 0);
        AFTER_DISPATCH(sample_fan_kernel, SF_BLOCK, P, (const FanArgs *)nullptr, 1, after_dyn_single(inst[0], row), s);
    } else {
        std::vector<FanArgs> now(n_inst);
        for (int e = 0; e < n_inst; ++e) fill(now[e], e);
        ArgBlockCache &c = after_state(h)->fan;
        if (int rc = c.sync_upload(now.data(), now.size() * sizeof(FanArgs), sizeof(FanArgs), s)) return rc;
        AFTER_DISPATCH(sample_fan_kernel, SF_BLOCK, now[0], (const FanArgs *)c.dev, n_inst, after_dyn_batched(row), s);
    }
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
