// after_step.hpp -- the frame the eager launches that follow a control step share (gfx950): the update arbiter
// (update_arbiter.hip), the Newton refinement (newton_refine.hip), the plan / episode trace (plan_trace.hip) and the sample fan
// (sample_fan.hip), in the order plan_after (step.hip) issues them from the AfterFrame that covo_plan_after_step /
// covo_plan_after_batched build for the step.
//
// Each is one launch per control step with one workgroup of three waves per instance:
//   phase 0  the per-step scalars from the raw controller key (after_derive) next to the kernel's own action image in LDS
//   phase 1  the rollout's three stage waves on that image (rollout_pipe.hpp: rp3_stages<..., PLAN = 1 | 2 | 3>) with the inputs
//            the step's sample rollouts had (after_rollout_args)
//   phase 2  the kernel's own rows.
// What all of them take the same way lives here: the head of the argument block and its rebase (BATCHED: workgroup e takes its
// block from device memory, pointers through rebase_global, as step_small_kernel<..., BATCHED> does), the per-step kernel
// arguments (AfterDyn: the row index travels there, so nothing is captured and no step graph changes), the choice of the launch
// variant, and the device copy of a batched step's argument blocks.  A further after-step launch starts from this file: an
// argument struct that begins with AfterHead, a kernel <ROLL, REWARD, FDIST, BATCHED> with its own LDS struct and phases, an
// ArgBlockCache of its own in AfterState.
#pragma once
#include <cstring>
#include <type_traits>
#include <vector>
#include "rollout_common.hpp"
#include "step_begin.hpp"

// the first member of PlanArgs / FanArgs / ArbArgs / RefineArgs / FeedbackArgs
struct AfterHead {
    RolloutArgs R;            // the step's sample rollout: noisy state, trajectories, model, discount, disturbance table; with the
                              // samples (fan, arbiter) a, N and R.clip: how phase 0 clips the stripes it gathers
    const uint32_t *key_mem;  // the raw rng_act of the step in device memory (batched steps), or null: AfterDyn's
    int derive_keys;
    float shared_noise_scale;
};
// what changes from step to step: kernel arguments of the eager launch
struct AfterDyn {
    uint32_t key[2];       // single step: the raw rng_act
    uint32_t f_shared[3];  // single step with derive_keys = 0: the caller's shared vector (float bits)
    int row;               // row of the episode's trace / log this step writes; < 0: none
};

// BATCHED: the pointers of the head a workgroup has loaded from its block, re-expressed on the kernel arguments' (each kernel adds
// the pointers of its own)
__device__ __forceinline__ void after_rebase_head(const AfterHead &P_, AfterHead &Pb)
{
    Pb.R.state = rebase_global(P_.R.state, Pb.R.state);
    Pb.R.pos_traj = rebase_global(P_.R.pos_traj, Pb.R.pos_traj);
    Pb.R.vel_traj = rebase_global(P_.R.vel_traj, Pb.R.vel_traj);
    Pb.R.f_tab = rebase_global(P_.R.f_tab, Pb.R.f_tab);
    Pb.key_mem = rebase_global(P_.key_mem, Pb.key_mem);
}

// phase 0, threads 0..3: the per-step scalars (step_begin.hpp: step_begin_derive, as the fused small step derives them per
// workgroup) into dyn_out[12].  kb[4]: the scalars' input block in LDS, one copy per deriving thread (indexed at run time: not in
// registers)
__device__ __forceinline__ void after_derive(const int tid, const AfterHead &P, const AfterDyn &dyn, const bool batched, DynBlock *kb4,
                                             uint32_t *dyn_out)
{
    if (tid < 4) {
        DynBlock &kb = kb4[tid];
#pragma unroll
        for (int i = 0; i < 12; ++i) kb.w[i] = 0u;
        if (batched) {
            kb.w[0] = P.key_mem[0];
            kb.w[1] = P.key_mem[1];
        } else {
            kb.w[0] = dyn.key[0];
            kb.w[1] = dyn.key[1];
            kb.w[2] = dyn.f_shared[0];
            kb.w[3] = dyn.f_shared[1];
            kb.w[4] = dyn.f_shared[2];
        }
        step_begin_derive(tid, kb, P.derive_keys, P.shared_noise_scale, dyn_out);
    }
}

// behind the barrier that ends phase 0: the rollout's arguments with the shared vector after_derive left in LDS
__device__ __forceinline__ RolloutArgs after_rollout_args(const AfterHead &P, const uint32_t *dyn_lds)
{
    RolloutArgs A = P.R;
    A.f_shared_dev = nullptr;
    A.f_shared[0] = __uint_as_float(dyn_lds[2]);
    A.f_shared[1] = __uint_as_float(dyn_lds[3]);
    A.f_shared[2] = __uint_as_float(dyn_lds[4]);
    return A;
}

// ---- host
// the head of one instance's argument block (the caller has zeroed the block: it is compared bytewise).  The kernels leave no
// costs, minima or records.  with_samples: the step's stripes and sample count; else one sample (the plan's image)
static inline void after_fill_head(AfterHead &H, covo_ctx *h, const PlanInstDesc &d, RolloutClip clip, bool with_samples)
{
    RolloutDesc ro;
    ro.state = d.state;
    ro.pos_traj = d.pos_traj;
    ro.vel_traj = d.vel_traj;
    ro.T = d.T;
    ro.params = d.params;
    ro.f_tab = d.f_tab;
    ro.a = with_samples ? d.a : nullptr;
    ro.N = with_samples ? d.N : 1;
    ro.discount = h->cfg.discount;
    ro.xcd_groups = 1;
    ro.clip = clip;
    fill_rollout_args(H.R, ro, 1);
    H.R.xcd_remap = 0;
    H.key_mem = d.key_mem;
    H.derive_keys = d.derive_keys;
    H.shared_noise_scale = d.shared_noise_scale;
}

static inline int after_check_tables(const PlanInstDesc *inst, int n_inst, const char *who)
{
    for (int e = 0; e < n_inst; ++e) {
        if (inst[e].params->disturb_kind >= COVO_DISTURB_PERIODIC && inst[e].f_tab == nullptr) {
            covo_set_error("%s: disturb_kind=%d needs the step's per-step disturbance table", who, inst[e].params->disturb_kind);
            return COVO_E_BADARG;
        }
    }
    return 0;
}

// the per-step kernel arguments of a launch that is not batched: the key and the shared vector as covo_mpc_step got them
static inline AfterDyn after_dyn_single(const PlanInstDesc &d, int row)
{
    AfterDyn dyn;
    dyn.key[0] = d.key[0];
    dyn.key[1] = d.key[1];
    std::memcpy(dyn.f_shared, d.f_shared, sizeof(dyn.f_shared));
    dyn.row = row;
    return dyn;
}
// ... and of a batched one: every instance's key lies in device memory (AfterHead::key_mem)
static inline AfterDyn after_dyn_batched(int row) { return AfterDyn{{0u, 0u}, {0u, 0u, 0u}, row}; }

// the launch variant the step's reward / disturbance / rollover switch selects (all instances alike: the step's own checks), as
// integral constants handed to go(roll, reward, fdist, batched)
template <class Go>
static inline void after_pick_variant(const RolloutArgs &R, bool batched, Go go)
{
    auto with_fdist = [&](auto roll, auto reward, auto b) {
        if (R.fdist == 0) go(roll, reward, std::integral_constant<int, 0>(), b);
        else if (R.fdist == 1) go(roll, reward, std::integral_constant<int, 1>(), b);
        else go(roll, reward, std::integral_constant<int, 2>(), b);
    };
    auto with_reward = [&](auto roll, auto b) {
        if (R.reward == COVO_REWARD_REALWORLD) with_fdist(roll, std::integral_constant<int, 1>(), b);
        else with_fdist(roll, std::integral_constant<int, 0>(), b);
    };
    auto with_roll = [&](auto b) {
        if (R.rollover) with_reward(std::true_type(), b);
        else with_reward(std::false_type(), b);
    };
    if (batched) with_roll(std::true_type());
    else with_roll(std::false_type());
}
// kernel<ROLL, REWARD, FDIST, BATCHED>(P, batch, dyn) on n workgroups; batch == null: not batched, P is the one instance's block,
// else P = the first instance's (a macro: a __global__ template cannot be passed as a template argument)
#define AFTER_DISPATCH(kernel, BLOCK, P, batch, n, dyn, s)                                                                              \
    after_pick_variant((P).head.R, (batch) != nullptr, [&](auto roll, auto reward, auto fdist, auto batched) {                          \
        hipLaunchKernelGGL((kernel<decltype(roll)::value, decltype(reward)::value, decltype(fdist)::value, decltype(batched)::value>), \
                           dim3(n), dim3(BLOCK), 0, s, P, batch, dyn);                                                                  \
    })

// The device copy of a batched step's argument blocks, COVO_MAX_ENVS of them, allocated at the first upload.  A steady-state step
// builds the same blocks as the one before it and uploads nothing
struct ArgBlockCache {
    void *dev = nullptr;
    std::vector<char> host;  // what dev holds

    // dev = the `bytes` at `now` (blocks of block_bytes each).  Only when they differ from what dev holds: behind a synchronisation
    // of the stream -- the launches that read the old blocks are done
    int sync_upload(const void *now, size_t bytes, size_t block_bytes, hipStream_t s)
    {
        if (host.size() == bytes && std::memcmp(host.data(), now, bytes) == 0) return 0;
        COVO_CHECK_HIP(hipStreamSynchronize(s));
        host.clear();
        if (dev == nullptr) COVO_CHECK_HIP(hipMalloc(&dev, (size_t)COVO_MAX_ENVS * block_bytes));
        COVO_CHECK_HIP(hipMemcpy(dev, now, bytes, hipMemcpyHostToDevice));
        host.assign(static_cast<const char *>(now), static_cast<const char *>(now) + bytes);
        return 0;
    }
};

// covo_ctx::after.  One cache per launch: with a shared one every launch of a batched step would overwrite the mirror the next
// compares against, and every step would synchronise and upload
struct AfterState {
    ArgBlockCache arbiter, plan, fan, refine, feedback;
    ArgBlockCache hold, hold_primitive, latch;  // plan_hold.hip: a batched hold step's blocks, covo_plan_hold's, a batched plan step's latch
    ArgBlockCache ilqr;                         // ilqr.hip: a batched iLQR step's tally blocks
    ArgBlockCache est, est_primitive;           // state_estimator.hip: an episode driver's batched launch, covo_estimate's
    ArgBlockCache obs, obs_primitive;           // force_observer.hip: an episode driver's batched launch, covo_observe_force's
    float *nominal = nullptr;  // [COVO_MAX_ENVS][128] the update arbiter's nominals of the env-batched fused step
};
static inline AfterState *after_state(covo_ctx *h)
{
    if (h->after == nullptr) h->after = new AfterState();
    return reinterpret_cast<AfterState *>(h->after);
}
