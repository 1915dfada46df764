// step_small.hip -- the WHOLE control step of the precomputed-Sigma controllers as ONE launch, for small sample counts (gfx950).
//
// SURVEY.md 8f-2 (GEMM -> clip -> rollout -> online softmax in one launch) where it pays: covo-offline and MPPI at N <= 16 384
// (BASELINE configs[0], [1]; the 8 192-sample shards of config [3]).  There the staged step is four launch boundaries
// (begin | noise | rollout + records | merge: 18 us at N = 1 024, 25 us at N = 8 192) around ~1 us of matrix work and a ~5 us
// rollout chain; at N = 65 536 the same fusion was built in round 2 and bought nothing (MFMA and VALU time add up on a SIMD,
// DESIGN.md 4.2) -- the gain here is the removed boundaries, not pipe overlap.  One workgroup = one 64-sample group = four waves:
//
//   phase 0  what step_begin_kernel does, per workgroup: shifted mean (covo.py:201-203) -> LDS; sampling key / MPPI's shared
//            disturbance from the raw rng_act (step_begin.hpp); the factor: covo-offline L_table[state.time] staged into the
//            padded LDS image (noise_gemm_body.hpp), MPPI the 32 4x4 block factors of the SHIFTED covariance (mppi.py:43-61)
//   phase 1  the group's actions a = clip(mu + L eps) (covo.py:212-224, mppi.py:53-66): covo-offline as the noise GEMM's two
//            32-sample tiles, each split over two waves (row tiles {0, 3} / {1, 2}) with in-register Philox -- the SAME device
//            functions and MFMA order as noise_gemm_kernel's SPLIT shape; MPPI per lane -> LDS [H][64] float4 (and the `a` work
//            buffer in HBM, write-only)
//   phase 2  the three-stage rollout pipeline (rollout_pipe.hpp: rp3_stages) on waves 0-2, stage A reading its stripes from
//            LDS; wave 3 shares the barriers
//   phase 3  the workgroup's online-softmax record (rollout_record, stripes from LDS) published with coherent stores; the
//            workgroup that takes the last ticket merges all records (softmax_merge.hpp: merge_body, the arithmetic of
//            merge_kernel) into the new mean -- or, on a sample-sharded rank, into the rank's record --, and shifts MPPI's
//            covariances in place (every workgroup has read them by then).
//
// Bit-identical to the staged step (same device functions, same record order, same merge): tests/test_gpu_parity.py
// test_small_fused_step_equals_staged.  Not taken (the staged launches run): position statistics, the per-step disturbance
// tables, the realworld reward, MPPI's covariance adaptation, more than 256 groups, the debug phase timers.
// Reference: quadjax/controllers/covo.py:201-278, mppi.py:43-129.
#include <cstring>
#include "rollout_common.hpp"
#include "noise_gemm_body.hpp"
#include "softmax_merge.hpp"
#include "step_begin.hpp"
#include "step_small.hpp"

constexpr int SS_BLOCK = 256;
constexpr int SS_CH = 2;

struct SmallLds {
    float4 a[COVO_H][COVO_WAVE];  // 32 KiB: the group's clipped actions, [t][sample]
    Rp3Lds<SS_CH> rings;          // 9 KiB
    float mus[COVO_NA];           // shifted mean
    uint32_t dyn[12];             // {key0, key1, f_shared[3], ...} as step_begin_kernel leaves them
    float rec_m[1], rec_s[1];
    __attribute__((aligned(16))) float rec_v[1][COVO_NA];
    int last;
    float mppi_L[COVO_H][16];     // MPPI: the block factors of the shifted covariance
};
// the padded image of L (covo-offline, phase 0/1) and the merge's scratch (phase 3) share the tail of the dynamic LDS
constexpr size_t SS_LDS_GEMM = sizeof(SmallLds) + (size_t)COVO_NA * NG_LDA * sizeof(float);
constexpr size_t SS_LDS_MPPI = sizeof(SmallLds) + sizeof(MergeLds);
static_assert(sizeof(MergeLds) <= (size_t)COVO_NA * NG_LDA * sizeof(float), "merge scratch must fit the factor image");

// BATCHED (the env-batched step, covo_mpc_step_batched_mode): grid = (groups per instance, instances).  Workgroup row y does for
// instance y what the single launch does for its one instance; instance y's argument block -- own state, trajectories, model
// constants, mean, covariances or factor table, work buffers, records, ticket -- is batch[y] in device memory (wave-uniform scalar
// loads), P_ is instance 0's block as a kernel argument and only anchors the pointers' address space (rebase_global).  Every
// quantity that counts workgroups (record index, ticket wrap, the merge's record count, the group mapping) is blockIdx.x /
// gridDim.x, i.e. per instance: instance y's step is bit-identical to the single launch on it.  The per-step keys come from
// device memory: dyn_mem = that instance's RAW rng_act (batch_set_dyn_kernel), derived per workgroup like an eager single step.
// DIAG (covo_set_step_diag): the record stage also leaves the group's diagnostic record, the last workgroup's merge also writes the
// instance's COVO_DIAG_FLOATS (row y of the caller's buffer); their LDS scratch is the rollout's rings, idle after phase 2.
template <bool MPPI, bool DISC1, bool ROLL, bool BATCHED = false, bool DIAG = false>
__global__ __launch_bounds__(SS_BLOCK) void step_small_kernel(const SmallStepArgs P_, const SmallStepArgs *__restrict__ batch)
{
    SmallStepArgs Pb;
    if (BATCHED) {
        Pb = batch[blockIdx.y];
        Pb.R.state = rebase_global(P_.R.state, Pb.R.state);
        Pb.R.pos_traj = rebase_global(P_.R.pos_traj, Pb.R.pos_traj);
        Pb.R.vel_traj = rebase_global(P_.R.vel_traj, Pb.R.vel_traj);
        Pb.R.a = rebase_global(P_.R.a, Pb.R.a);
        Pb.R.cost = rebase_global(P_.R.cost, Pb.R.cost);
        Pb.R.records = rebase_global(P_.R.records, Pb.R.records);
        Pb.R.merge_ticket = rebase_global(P_.R.merge_ticket, Pb.R.merge_ticket);
        Pb.R.merge_out = rebase_global(P_.R.merge_out, Pb.R.merge_out);
        if (DIAG) {
            Pb.R.diag_rec = rebase_global(P_.R.diag_rec, Pb.R.diag_rec);
            Pb.R.diag_out = rebase_global(P_.R.diag_out, Pb.R.diag_out);
        }
        Pb.a_mean_in = rebase_global(P_.a_mean_in, Pb.a_mean_in);
        Pb.L_table = rebase_global(P_.L_table, Pb.L_table);
        Pb.mppi_cov = rebase_global(P_.mppi_cov, Pb.mppi_cov);
        Pb.dyn_mem = rebase_global(P_.dyn_mem, Pb.dyn_mem);
        Pb.a_mean_shift_out = nullptr;  // (the merge blends with the shifted mean in LDS; nobody else reads it)
        Pb.pass = P_.pass;
    }
    const SmallStepArgs &P = BATCHED ? Pb : P_;
    extern __shared__ __attribute__((aligned(16))) unsigned char ss_raw[];
    SmallLds &S = *reinterpret_cast<SmallLds *>(ss_raw);
    float *Ls = reinterpret_cast<float *>(ss_raw + sizeof(SmallLds));       // [128][NG_LDA] (covo-offline)
    MergeLds &M = *reinterpret_cast<MergeLds *>(ss_raw + sizeof(SmallLds));  // phase 3
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    RolloutArgs A = P.R;
    const int N = A.N;

    // ---- phase 0
    const float *__restrict__ a_mean = P.a_mean_in;
    const int pass = P.pass;  // (wave-uniform: a kernel argument)
    // the raw key of this pass where no begin launch has left the step's scalars: the caller's (pass 0), or the previous pass's
    // advanced.  Every deriving thread of every workgroup has loaded it before any workgroup takes its ticket, and only the workgroup
    // with the last ticket stores the pass's key back
    uint32_t raw_key[2] = {0u, 0u};
    if (tid < COVO_NA) {
        if (!BATCHED && P.dyn_mem != nullptr) {  // (a captured graph: the begin launch has shifted the mean of THIS replay; a_mean_in is not baked in)
            S.mus[tid] = P.a_mean_shift_out[tid];
        } else {
            const float v = (pass == 0 && tid < COVO_NA - COVO_DU) ? a_mean[tid + COVO_DU] : a_mean[tid];  // covo.py:201-203
            S.mus[tid] = v;
            if (blockIdx.x == 0 && P.a_mean_shift_out != nullptr) P.a_mean_shift_out[tid] = v;
        }
    } else if (tid < COVO_NA + 4) {
        if (BATCHED) {  // no begin launch: the instance's raw rng_act lies in device memory, every workgroup derives from it
            DynBlock kb;
#pragma unroll
            for (int i = 0; i < 12; ++i) kb.w[i] = 0u;
            const uint32_t p0 = P.dyn_mem[0], p1 = P.dyn_mem[1];
            if (pass > 0) {
                step_begin_derive_next(tid - COVO_NA, p0, p1, P.shared_noise_scale, S.dyn, raw_key);
            } else {
                raw_key[0] = kb.w[0] = p0;
                raw_key[1] = kb.w[1] = p1;
                step_begin_derive(tid - COVO_NA, kb, 1, P.shared_noise_scale, S.dyn);
            }
        } else if (P.dyn_mem != nullptr) {  // a captured graph: the begin launch has left the step's scalars in device memory
            const int q = tid - COVO_NA;
            if (q == 0) { S.dyn[0] = P.dyn_mem[0]; S.dyn[1] = P.dyn_mem[1]; }
            else S.dyn[1 + q] = P.dyn_mem[1 + q];
        } else if (pass > 0) {  // an eager iterated step: the previous pass's last workgroup has left its raw key at key_io
            const uint32_t p0 = P.key_io[0], p1 = P.key_io[1];
            step_begin_derive_next(tid - COVO_NA, p0, p1, P.shared_noise_scale, S.dyn, raw_key);
        } else {
            raw_key[0] = P.blk.w[0];
            raw_key[1] = P.blk.w[1];
            step_begin_derive(tid - COVO_NA, P.blk, P.derive_keys, P.shared_noise_scale, S.dyn);
        }
    }
    if (MPPI) {
        if (tid >= SS_BLOCK - COVO_H) {  // the last 32 threads: block t of the SHIFTED covariance = old block t + 1 (mppi.py:43-49)
            const int t = tid - (SS_BLOCK - COVO_H);
            // (pass >= 1 of an iterated step: pass 0's last workgroup has shifted the blocks already)
            const float *src = P.mppi_cov + 16 * ((pass == 0 && t < COVO_H - 1) ? t + 1 : t);
            float blk[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) blk[i] = src[i];
            mppi_factor_block(blk, &S.mppi_L[t][0]);
        }
    } else {
        const float *L = P.L_table;
        int t = __float_as_int(A.state[ST_TIME]);  // covo.py:107-108, clamped like a JAX gather
        t = t < 0 ? 0 : (t > P.n_table - 1 ? P.n_table - 1 : t);
        L += (size_t)t * COVO_NA * COVO_NA;
        ng_stage_factor<SS_BLOCK>(L, Ls, tid);
    }
    __syncthreads();
    const uint32_t k0 = S.dyn[0], k1 = S.dyn[1];
    // the rollouts' one shared disturbance vector (free.py:66-70 from the shared step key; 0 under deterministic = True)
    A.f_shared_dev = nullptr;
    A.f_shared[0] = __uint_as_float(S.dyn[2]);
    A.f_shared[1] = __uint_as_float(S.dyn[3]);
    A.f_shared[2] = __uint_as_float(S.dyn[4]);

    // which 64-sample group: the staged rollout's mapping (rollout_pipe3_kernel with one group per workgroup), so that record
    // i of this launch is record i of that one and the merge adds them in the same order
    int group = blockIdx.x;
    if (A.xcd_remap) {
        const int x = blockIdx.x & 7, m = (int)(blockIdx.x >> 3), q = A.xcd_remap;
        group = q * (x + 8 * (m / q)) + (m % q);
    }

    // ---- phase 1: the group's actions
    float4 *__restrict__ a_out = const_cast<float4 *>(A.a);
    if (MPPI) {
        // lane = sample, wave w takes steps 8 w .. 8 w + 7 (noise_blockdiag_kernel<PHILOX>'s arithmetic)
        const int n_raw = group * COVO_WAVE + lane;
        const int n = n_raw < N ? n_raw : N - 1;
#pragma unroll 2
        for (int i = 0; i < COVO_H / 4; ++i) {
            const int t = wave * (COVO_H / 4) + i;
            const float4 e = rngd::normal4((uint32_t)t, (uint64_t)(P.sample_offset + (int64_t)n), k0, k1);
            const float ev[4] = {e.x, e.y, e.z, e.w};
            float o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float acc = 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) acc = fmaf((k <= r) ? S.mppi_L[t][r * 4 + k] : 0.0f, ev[k], acc);
                const float mt = S.mus[4 * t + r];
                o[r] = P.nanp ? qm::clip11_nan_(mt + acc) : qm::clip11_(mt + acc);  // mppi.py:66
            }
            const float4 v = make_float4(o[0], o[1], o[2], o[3]);
            S.a[t][lane] = v;
            if (n_raw < N) a_out[(size_t)t * N + n_raw] = v;
        }
    } else {
        const int j = lane & 31, kh = lane >> 5;
        const int tl = wave >> 1;  // which of the group's two 32-sample tiles
        const int n_raw = group * COVO_WAVE + tl * 32 + j;
        const int row = n_raw < N ? n_raw : N - 1;
        const uint64_t id = (uint64_t)(P.sample_offset + row);
        const float *__restrict__ La = Ls + j * NG_LDA + kh;
        f32x16 acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[rt][e] = 0.0f;
        auto store_rt = [&](int rt) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int t = 8 * rt + 2 * g + kh;
                const float4 m4 = *reinterpret_cast<const float4 *>(S.mus + 4 * t);
                float4 v;
                if (P.nanp) {  // COVO_FLAG_PROPAGATE_NAN (covo.py:224 under jnp.clip)
                    v.x = qm::clip11_nan_(m4.x + acc[rt][4 * g + 0]);
                    v.y = qm::clip11_nan_(m4.y + acc[rt][4 * g + 1]);
                    v.z = qm::clip11_nan_(m4.z + acc[rt][4 * g + 2]);
                    v.w = qm::clip11_nan_(m4.w + acc[rt][4 * g + 3]);
                } else {
                    v.x = qm::clip11_(m4.x + acc[rt][4 * g + 0]);
                    v.y = qm::clip11_(m4.y + acc[rt][4 * g + 1]);
                    v.z = qm::clip11_(m4.z + acc[rt][4 * g + 2]);
                    v.w = qm::clip11_(m4.w + acc[rt][4 * g + 3]);
                }
                S.a[t][tl * 32 + j] = v;
                if (n_raw < N) a_out[(size_t)t * N + n_raw] = v;
            }
        };
        // noise_gemm_kernel's sequence for the row-tile set of this wave (work item 2 tile + half: odd -> {1, 2}, even -> {0, 3})
        auto seq = [&](auto mtag) {
            constexpr int MK = decltype(mtag)::value;
            BGroup b = gen_group(id, 0, kh, k0, k1);
            mfma_group<0, MK>(La, b, acc);
            if (MK & 1) store_rt(0);
            if (MK >> 1) b = gen_group(id, 1, kh, k0, k1);
            mfma_group<1, MK>(La, b, acc);
            if (MK & 2) store_rt(1);
            if (MK >> 2) b = gen_group(id, 2, kh, k0, k1);
            mfma_group<2, MK>(La, b, acc);
            if (MK & 4) store_rt(2);
            if (MK >> 3) b = gen_group(id, 3, kh, k0, k1);
            mfma_group<3, MK>(La, b, acc);
            if (MK & 8) store_rt(3);
        };
        if (wave & 1) seq(RtMask<6>());
        else seq(RtMask<9>());
    }
    __syncthreads();

    // ---- phase 2: the rollout (covo.py:227-263), stripes from LDS
    float cost = 0.0f;
    bool valid = false;
    int n = 0;
    float dummy_st[1][1][9];
    if (wave < 3)
        rp3_stages<DISC1, ROLL, SS_CH, -1, false, true, 0, 0, true>(A, S.rings, dummy_st, wave, 0, group, lane, &S.a[0][0], cost, valid, n);
    else
        rp3_idle_barriers<SS_CH>();

    // ---- phase 3: this group's record, then the last workgroup's merge (covo.py:266-278)
    const bool carrier = wave == 2;
    static_assert(sizeof(Rp3Lds<SS_CH>) >= (3 * MG_VWAVES + MG_DIAG_REC) * sizeof(float), "diagnostic scratch must fit the rings");
    float(*diag_red)[MG_VWAVES] = reinterpret_cast<float(*)[MG_VWAVES]>(&S.rings);
    float(*diag_wave)[MG_DIAG_REC] = reinterpret_cast<float(*)[MG_DIAG_REC]>(reinterpret_cast<float *>(&S.rings) + 3 * MG_VWAVES);
    if (DIAG)
        rollout_record<SS_BLOCK / COVO_WAVE, 1, true, true>(A, cost, valid && carrier, n, 0, carrier, lane, blockIdx.x, S.rec_m, S.rec_s,
                                                            S.rec_v, &S.a[0][0], true, diag_wave);
    else
        rollout_record<SS_BLOCK / COVO_WAVE, 1, true>(A, cost, valid && carrier, n, 0, carrier, lane, blockIdx.x, S.rec_m, S.rec_s,
                                                      S.rec_v, &S.a[0][0], true);
    // the write-through stores of the record are acknowledged before the ticket; the last workgroup merges (softmax_merge.hpp)
    A.merge_mean_old = S.mus;
    if (DIAG) rollout_merge_last_diag<SS_BLOCK>(A, M, S.last, diag_red);
    else rollout_merge_last<SS_BLOCK>(A, M, S.last);
    if (!S.last) return;
    // an iterated step: the merge's cost minimum (the minimum over the merging waves' minima, softmax_merge.hpp phase 1) to this
    // pass's slot of the iteration log, and the pass's raw key to where the next pass and the recorder's launches read it
    if (P.iter_out != nullptr && tid == 0) {
        float m = M.redm[0];
#pragma unroll
        for (int i = 1; i < SS_BLOCK / COVO_WAVE; ++i) m = fminf(m, M.redm[i]);
        P.iter_out[pass] = m;
    }
    if (P.key_io != nullptr && tid == COVO_NA) {
        P.key_io[0] = raw_key[0];
        P.key_io[1] = raw_key[1];
    }
    if (MPPI && pass == 0) {  // the in-place shift of a_cov (mppi.py:43-49): every workgroup took its factors from the old blocks long ago
        float blk[16];
        const int t = tid;
        if (t < COVO_H) {
            const float *src = P.mppi_cov + 16 * ((t < COVO_H - 1) ? t + 1 : t);
#pragma unroll
            for (int i = 0; i < 16; ++i) blk[i] = src[i];
        }
        __syncthreads();
        if (t < COVO_H) {
#pragma unroll
            for (int i = 0; i < 16; ++i) P.mppi_cov[16 * t + i] = blk[i];
        }
    }
}

// why the step (args, params) cannot run as the one fused launch, in words a caller can act on; null: it can
const char *step_small_refusal(const covo_ctx *h, const covo_env_params &p, const covo_step_args &a)
{
    if (a.mode != COVO_MODE_COVO_OFFLINE && a.mode != COVO_MODE_MPPI) return "the mode is neither MPPI nor covo-offline";
    if (a.mode == COVO_MODE_MPPI && a.gamma_sigma != 0.0f)                     // second moments: reduce.hip's own stage 1
        return "gamma_sigma != 0 (MPPI's covariance adaptation)";
    if (a.pos_stats != nullptr) return "position statistics are requested";    // covo.py:281's statistics: the STATS rollout
    if (p.reward_kind != COVO_REWARD_PENYAW) return "reward_kind is not COVO_REWARD_PENYAW (the realworld reward)";
    if (p.disturb_kind != COVO_DISTURB_NONE && p.disturb_kind != COVO_DISTURB_GAUSSIAN)  // per-step tables
        return "disturb_kind needs per-step tables (only COVO_DISTURB_NONE and COVO_DISTURB_GAUSSIAN)";
    const int ng = (a.n_samples + COVO_WAVE - 1) / COVO_WAVE;
    if (ng < 1 || ng > h->max_red_blocks || ng > 256) return "n_samples is outside [1, 16384] (at most 256 groups of 64 samples)";
    return nullptr;
}

bool step_small_eligible(const covo_ctx *h, const covo_env_params &p, const covo_step_args &a)
{
    return step_small_refusal(h, p, a) == nullptr;
}

static void fill_small_args(SmallStepArgs &P, covo_ctx *h, const covo_env_params &p, const covo_step_args &a, const float *state,
                            float *a_mean_shift, const DynBlock *blk, const uint32_t *dyn_mem, float shared_noise_scale,
                            unsigned *ticket, float *records, float *diag_rec, float *diag_out, int pass, uint32_t *key_io, float *iter_out)
{
    std::memset(&P, 0, sizeof(P));
    P.pass = pass;
    P.key_io = key_io;
    P.iter_out = iter_out;
    RolloutDesc ro;
    ro.state = state;
    ro.pos_traj = a.pos_traj;
    ro.vel_traj = a.vel_traj;
    ro.T = a.T;
    ro.params = &p;
    ro.a = a.a;
    ro.N = a.n_samples;
    ro.discount = h->cfg.discount;
    ro.cost = a.cost;
    ro.records = records;
    ro.lam = h->cfg.lam;
    ro.diag_rec = diag_out ? diag_rec : nullptr;
    ro.xcd_groups = a.mode == COVO_MODE_MPPI ? 4 : 0;
    ro.clip = ROLLOUT_CLIP_TRUSTED;  // the stripes come straight from this launch's own clipped draw
    fill_rollout_args(P.R, ro, 1);
    P.R.merge_ticket = ticket;
    P.R.merge_final = a.partial_out == nullptr;
    P.R.merge_out = a.partial_out ? a.partial_out : a.a_mean;
    P.R.merge_gamma = a.gamma_mean;
    P.R.diag_out = diag_out;
    P.a_mean_in = a.a_mean_in ? a.a_mean_in : a.a_mean;
    P.a_mean_shift_out = a_mean_shift;
    P.L_table = a.L_table;
    P.n_table = a.n_table;
    P.mppi_cov = a.mode == COVO_MODE_MPPI ? a.a_cov : nullptr;
    P.sample_offset = a.sample_offset;
    if (blk != nullptr) P.blk = *blk;
    P.dyn_mem = dyn_mem;
    P.derive_keys = a.derive_keys;
    P.shared_noise_scale = shared_noise_scale;
    P.nanp = covo_propagate_nan(h) ? 1 : 0;
}

// the dynamic LDS above 64 KB is a per-device opt-in of every instantiation
static int small_attrs_once()
{
    static unsigned long long attr_devices = 0;  // (per device: covo_first_on_device)
    if (covo_first_on_device(attr_devices)) {
#define SS_ATTR2(MPPI, D, R, B, G) COVO_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(step_small_kernel<MPPI, D, R, B, G>), \
                                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)(MPPI ? SS_LDS_MPPI : SS_LDS_GEMM)))
#define SS_ATTR1(MPPI, D, R, B) SS_ATTR2(MPPI, D, R, B, false); SS_ATTR2(MPPI, D, R, B, true)
#define SS_ATTR(MPPI, D, R) SS_ATTR1(MPPI, D, R, false); SS_ATTR1(MPPI, D, R, true)
        SS_ATTR(false, false, false); SS_ATTR(false, false, true); SS_ATTR(false, true, false); SS_ATTR(false, true, true);
        SS_ATTR(true, false, false); SS_ATTR(true, false, true); SS_ATTR(true, true, false); SS_ATTR(true, true, true);
#undef SS_ATTR
#undef SS_ATTR1
#undef SS_ATTR2
    }
    return 0;
}

template <bool BATCHED>
static int small_go(const SmallStepArgs &P, const SmallStepArgs *batch, int nb, bool mppi, bool disc1, hipStream_t s)
{
    const int ng = (P.R.N + COVO_WAVE - 1) / COVO_WAVE;
    const bool roll = P.R.rollover != 0;
    const bool diag = P.R.diag_out != nullptr;  // (all instances of a batch alike)
#define SS_GO1(MPPI, D, R, G) hipLaunchKernelGGL((step_small_kernel<MPPI, D, R, BATCHED, G>), dim3(ng, nb), dim3(SS_BLOCK), MPPI ? SS_LDS_MPPI : SS_LDS_GEMM, s, P, batch)
#define SS_GO(MPPI, D, R) do { if (diag) SS_GO1(MPPI, D, R, true); else SS_GO1(MPPI, D, R, false); } while (0)
    if (mppi) {
        if (disc1) { if (roll) SS_GO(true, true, true); else SS_GO(true, true, false); }
        else       { if (roll) SS_GO(true, false, true); else SS_GO(true, false, false); }
    } else {
        if (disc1) { if (roll) SS_GO(false, true, true); else SS_GO(false, true, false); }
        else       { if (roll) SS_GO(false, false, true); else SS_GO(false, false, false); }
    }
#undef SS_GO
#undef SS_GO1
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_step_small(covo_ctx *h, const covo_env_params &p, const covo_step_args &a, const float *state, float *a_mean_shift,
                      const DynBlock *blk, const uint32_t *dyn_mem, float shared_noise_scale, unsigned *ticket, hipStream_t s,
                      int pass, uint32_t *key_io, float *iter_slot)
{
    SmallStepArgs P;
    fill_small_args(P, h, p, a, state, a_mean_shift, blk, dyn_mem, shared_noise_scale, ticket, h->ws_partials, h->ws_diag_rec,
                    a.partial_out == nullptr ? covo_diag_target(h) : nullptr, pass, key_io, iter_slot ? iter_slot - pass : nullptr);
    int rc = small_attrs_once();
    if (rc) return rc;
    return small_go<false>(P, nullptr, 1, a.mode == COVO_MODE_MPPI, h->cfg.discount == 1.0f, s);
}

// ---- the env-batched form: one argument block per instance in device memory (step.hip keeps the host and device arrays)
size_t step_small_args_bytes(int n) { return (size_t)n * sizeof(SmallStepArgs); }

void step_small_fill_args(covo_ctx *h, void *out, int index, const covo_env_params &p, const covo_step_args &a, const uint32_t *raw_key_mem,
                          float shared_noise_scale, unsigned *ticket, float *records, float *diag_rec, float *diag_out, float *iter_out)
{
    // (an iterated step walks the instance's raw key in place: the key upload of the next step overwrites it)
    fill_small_args(reinterpret_cast<SmallStepArgs *>(out)[index], h, p, a, a.state, nullptr, nullptr, raw_key_mem, shared_noise_scale,
                    ticket, records, diag_rec, diag_out, 0, iter_out ? const_cast<uint32_t *>(raw_key_mem) : nullptr, iter_out);
}

// all instances alike in mode, sample count, reward, rollover flag and disturbance kind (the caller has checked): instance 0 picks
// the variant
int launch_step_small_batched(covo_ctx *h, const void *args_host, const void *args_dev, int n, bool mppi, hipStream_t s, int pass)
{
    int rc = small_attrs_once();
    if (rc) return rc;
    SmallStepArgs P0 = *reinterpret_cast<const SmallStepArgs *>(args_host);
    P0.pass = pass;
    return small_go<true>(P0, reinterpret_cast<const SmallStepArgs *>(args_dev), n, mppi, h->cfg.discount == 1.0f, s);
}
