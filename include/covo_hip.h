/* covo_hip.h -- C ABI of libcovo_hip.so: the MI355X (gfx950) sampling-MPC inner loop.
 *
 * The reference (LeCAR-Lab/CoVO-MPC, package quadjax) has NO plugin/FFI boundary for
 * this path: it is pure Python-on-JAX and the boundary is the Python controller
 * protocol quadjax/controllers/base.py:5-19.  This header is therefore the
 * build-defined C ABI that covo_mpc_amd's Python controllers (the mirror of
 * quadjax.controllers) bind with ctypes; each entry point cites the reference
 * lines whose XLA-lowered ops it replaces.  INTEGRATION.md shows the ctypes stub
 * a quadjax maintainer would add.
 *
 * Conventions
 *   - extern "C", every function returns int: 0 = ok, otherwise a COVO_E_* code
 *     (negative) or a hipError_t (positive); covo_last_error() gives the text.
 *   - All tensor arguments are CALLER-OWNED DEVICE pointers (torch data_ptr()),
 *     fp32, contiguous, unless marked [host].  The library owns only the opaque
 *     handle and a small device workspace allocated in covo_create().
 *   - Every launch goes to the caller's hipStream_t (passed as void*); there are
 *     no hidden synchronisations or allocations on these paths (graph-capturable).
 *   - A handle is single-threaded and bound to the device current at creation.
 *
 * Data layouts in HBM
 *   state    float[COVO_STATE_FLOATS]: the (noisy) env state the controller plans
 *            from (quadjax/controllers/covo.py:198), packed as
 *            pos[0:3] vel[3:6] quat_xyzw[6:10] omega[10:13] f_disturb[13:16]
 *            pos_tar[16:19] vel_tar[19:22] acc_tar[22:25] time(int32 bits)[25]
 *   traj     pos_traj / vel_traj: float[T][3] reference trajectory (EnvState3D)
 *   eps      float[N][n]      standard-normal draws, sample-major, n = H*du = 128
 *   a        float[H][N][4]   clipped sampled actions in "stripe" order: one
 *            float4 (thrust, wx, wy, wz) per (step, sample); a wave of the rollout
 *            kernel reads one contiguous 1 KiB stripe per step.
 *   cost     float[N]
 *   partial  float[COVO_PARTIAL_FLOATS] = {m, s, v[128], pad}: online-softmax
 *            record of one shard (m = min cost, s = sum w, v = sum w*a).  The two
 *            pad floats only round the record up to 16 bytes: no entry writes them
 *            or lets them reach a result; they keep what the caller's buffer held.
 */
#ifndef COVO_HIP_H
#define COVO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COVO_ABI_VERSION 10

#define COVO_H 32            /* horizon (compile-time in the fused kernels)          */
#define COVO_DU 4            /* action dim, quadjax/envs/quadrotor.py:198            */
#define COVO_NA (COVO_H * COVO_DU) /* n = 128 flattened actions, index 4*t + d        */
#define COVO_STATE_FLOATS 32
#define COVO_PARTIAL_FLOATS 132
#define COVO_POS_STATS_DOUBLES (COVO_H * 6) /* per step: sum(pos-c)[3], sum((pos-c)^2)[3] */
#define COVO_DIAG_FLOATS 8   /* per-step sampling diagnostics of one instance (covo_set_step_diag)                       */

#define COVO_FLAG_ACTIONS_CLIPPED 1 /* covo_config.flags: every `a` handed to covo_rollout_cost is already
                                       clipped to [-1,1] (true for covo_noise_* outputs): skip step_env's re-clip */

#define COVO_FLAG_NO_GRAPH 2         /* covo_config.flags: covo_mpc_step always launches eagerly (no hipGraph) */
#define COVO_FLAG_SHARED_DEVICE 4    /* covo_config.flags: other processes / streams compete for this GPU: no launch may depend on
                                        its workgroups being co-resident (the Sigma chain then runs every phase as its own
                                        launch instead of folding them into two persistent launches).  Set it as well when TWO
                                        HANDLES of one process run covo-online / covo_sigma steps concurrently on different
                                        streams: two persistent launches side by side can hold the workgroup slots each other's
                                        missing workgroups need (their barriers then time out: COVO_DEVSTAT_GRID_BARRIER).  Steps on
                                        one stream, and any number of handles used one after the other, need nothing. */

#define COVO_FLAG_PROPAGATE_NAN 8    /* covo_config.flags: the action clips (covo.py:224, mppi.py:66, quadrotor.py:223,258) keep a NaN
                                        like jnp.clip = minimum(maximum(x, lo), hi) does.  Default (flag off): the kernels clip with
                                        v_med3 / maxNum / minNum, where a NaN operand loses -- a NaN sample becomes -1.
                                        The one place quadjax produces NaNs by itself on this path: covo-offline on `hovering`, whose
                                        Sigma-table row 0 is NaN (norm'(0)); there quadjax's mean is NaN from the first step on, and
                                        with this flag so is this library's; without it the episode carries on. */

#define COVO_MODE_MPPI 0
#define COVO_MODE_COVO_ONLINE 1
#define COVO_MODE_COVO_OFFLINE 2

#define COVO_E_BADARG (-1)
#define COVO_E_NOHANDLE (-2)
#define COVO_E_UNSUPPORTED (-3)
#define COVO_E_DEVICE (-4)           /* a kernel of an EARLIER call on this handle reported a failure (covo_device_status) */

#define COVO_RANK_RECORD_FLOATS (COVO_PARTIAL_FLOATS + 2 * COVO_POS_STATS_DOUBLES) /* 516: the record one rank of a sample-sharded
                                        step contributes to the exchange: {m, s, v[128], pad[2]} + the 192 fp64 position sums of
                                        covo.py:281 (zeros when not requested): ONE message of 2 064 bytes per rank and step */
#define COVO_COV_FLOATS (COVO_H * 10)  /* MPPI's covariance adaptation (mppi.py:119-125): the 10 second moments i <= j of the 4 action
                                        components of every step, sum_n w_n d_i d_j about the shifted OLD mean */
#define COVO_RANK_RECORD_COV_FLOATS (COVO_PARTIAL_FLOATS + COVO_COV_FLOATS + 2 * COVO_POS_STATS_DOUBLES) /* 836: the rank record of a
                                        sample-sharded MPPI step with gamma_sigma != 0: {m, s, v[128], pad[2]} + 320 second moments +
                                        the 192 fp64 position sums -- still ONE message (3 344 bytes) per rank and step */
#define COVO_EXCHANGE_HANDLE_BYTES 128 /* opaque inter-process handle of a rank's exchange buffer (covo_exchange_create): the hipIpc
                                        handle + whether the buffer is fine-grained + the PCI bus id of its device */

#define COVO_DEVSTAT_EXCHANGE 2      /* covo_exchange_records: a peer's record did not arrive within the exchange's time-out
                                        (covo_exchange_set_timeout, default 60 s); the gathered records are NaN */
#define COVO_DEVSTAT_ADJOINT 4       /* covo_hessian / covo_mpc_step: a hyper-dual workgroup of the adjoint Hessian's chain launch
                                        gave up waiting for a costate row of the same launch (0.2 s: the costate workgroup was not
                                        co-resident); that call's Hessian, Sigma and L are NaN */
#define COVO_DEVSTAT_GRID_BARRIER 1  /* a grid barrier of the Sigma chain's persistent launches timed out (its workgroups were not
                                        co-resident within 0.2 s: GPU shared with other work); that call's Sigma / L are NaN */

/* covo_env_params.reward_kind: which reward Quad3D binds to env.reward_fn (quadjax/envs/quadrotor.py:49-84) */
#define COVO_REWARD_PENYAW 0     /* tracking_penyaw_reward_fn (dynamics/utils.py:285-294): tasks tracking, tracking_zigzag, hovering */
#define COVO_REWARD_REALWORLD 1  /* tracking_realworld_reward_fn (utils.py:297-313): task tracking_slow */

/* covo_env_params.disturb_kind: Quad3D(disturb_type=...) -> get_quadrotor_1st_order_dyn (dynamics/free.py:8-72) */
#define COVO_DISTURB_NONE 0      /* free.py:72 */
#define COVO_DISTURB_GAUSSIAN 1  /* free.py:66-70: dyn_noise_scale * normal(key, (3,)); 0 under deterministic=True (quadrotor.py:234) */
#define COVO_DISTURB_PERIODIC 2  /* free.py:10-24: redrawn uniform(-scale, scale) when time % period == 0, held otherwise */
#define COVO_DISTURB_SIN 3       /* free.py:27-38: a function of time and disturb_params */
#define COVO_DISTURB_DRAG 4      /* free.py:41-47: -|scale| rel |rel| / 1.5^2, rel = vel - disturb_params[:3] / 2 (per sample) */
#define COVO_DISTURB_MIXED 5     /* free.py:50-56: (drag + sin + periodic) / 3 */

/* covo_env_params.reset_traj: the trajectory generator Quad3D binds to self.generate_traj (quadjax/envs/quadrotor.py:49-84), i.e.
 * what reset_env (quadrotor.py:265-312, 363-370) draws when BaseEnvironment.step auto-resets a finished episode
 * (quadjax/envs/base.py:22-40).  COVO_TRAJ_NONE switches the device env's auto-reset off (done is logged, the state flies on). */
#define COVO_TRAJ_NONE 0
#define COVO_TRAJ_FIXED 1        /* generate_fixed_traj (dynamics/utils.py:49-53): task hovering; T = max_steps_in_episode rows of 0 */
#define COVO_TRAJ_LISSA 2        /* generate_lissa_traj (utils.py:87-130): task tracking; T = max_steps_in_episode + 50 */
#define COVO_TRAJ_LISSA_SLOW 3   /* generate_lissa_traj_slow (utils.py:133-180): task tracking_slow; T = max_steps_in_episode + 50 */
#define COVO_TRAJ_ZIGZAG 4       /* generate_zigzag_traj (utils.py:183-251): task tracking_zigzag; T = (max_steps_in_episode / 40 + 1) * 40 */

/* covo_disturb_table key threading (who calls step_env with which key) */
#define COVO_DISTURB_KEYS_SHARED 0    /* every step uses the SAME step key: the controllers' rollouts (covo.py:225,231; mppi.py:69,74) */
#define COVO_DISTURB_KEYS_HESSIAN 1   /* per step rng_k, key = split(key); step_env(rng_k): get_hessian (covo.py:150-153) */
#define COVO_DISTURB_KEYS_NOMINAL 2   /* per step _, key = split(key); rng_step, key = split(key): covo-offline's nominal rollout (covo.py:58-70) */

typedef struct covo_ctx *covo_handle_t;

/* Rollout-relevant subset of EnvParams3D (quadjax/dynamics/dataclass.py:40-100). [host] */
typedef struct covo_env_params {
    float max_thrust;       /* .8   */
    float max_torque[3];    /* 9e-3, 9e-3, 2e-3 (cancels: quadrotor.py:260 * free.py:122) */
    float max_omega[3];     /* 10, 10, 3 */
    float dt;               /* .02  */
    float g;                /* 9.81 */
    float m;                /* .027 */
    float action_scale;     /* 1    */
    float alpha_bodyrate;   /* .5   */
    int32_t max_steps_in_episode; /* 300 */
    float pos_limit;        /* 3.0, quadrotor.py:484 */
    int32_t rollover_terminate; /* 1: is_terminal also fires on quat[3] < cos(pi/4) or any |omega| > 100 (quadrotor.py:486-490),
                                 *    i.e. Quad3D(disable_rollover_terminate=False), the constructor's default; quadjax's main()
                                 *    builds its env with disable_rollover_terminate=True (quadrotor.py:779) -> 0 */
    int32_t reward_kind;        /* COVO_REWARD_*: env.reward_fn (quadrotor.py:56,66,73,82) */
    int32_t disturb_kind;       /* COVO_DISTURB_*: Quad3D(disturb_type=...) (quadrotor.py:35,87-89) */
    int32_t disturb_period;     /* 50   (dataclass.py:86) */
    float disturb_scale;        /* .2   (dataclass.py:87) */
    float disturb_params[6];    /* 0    (dataclass.py:88; domain randomisation / reset draw them, quadrotor.py:151,171) */
    float dyn_noise_scale;      /* .05  (dataclass.py:93): scale of the gaussian model (zeroed by deterministic=True) */
    /* ---- auto-reset of the device env (covo_env_step*, covo_run_episode*; base.py:22-40).  Ignored by every other entry point. */
    int32_t reset_traj;         /* COVO_TRAJ_*; COVO_TRAJ_NONE (0) = no auto-reset */
    int32_t reserved0;          /* 0 */
    double reset_dt;            /* dt as the trajectory generators receive it (quadrotor.py:52,60,68,77: the host's double .02) */
    double reset_disturb_scale; /* f_disturb ~ U(-s, s) at reset (quadrotor.py:300-305): the host's double .2 */
} covo_env_params;

typedef struct covo_config {
    int32_t n_local;        /* samples handled by this handle (this rank's shard)  */
    int32_t H;              /* must equal COVO_H                                   */
    int32_t du;             /* must equal COVO_DU                                  */
    float lam;              /* temperature lambda, controllers/covo.py:266         */
    float discount;         /* controllers/covo.py:258                             */
    int32_t flags;          /* COVO_FLAG_* bits                                    */
} covo_config;

const char *covo_last_error(void);
int covo_abi_version(void);

/* Replaces nothing in the reference: lifetime of the opaque handle + workspace. */
int covo_create(const covo_config *cfg, covo_handle_t *out);
int covo_destroy(covo_handle_t h);

/* Sticky device-side status of the handle: COVO_DEVSTAT_* bits raised by kernels of earlier (asynchronous) calls, read from
 * host-mapped memory without synchronising.  While it is non-zero every compute entry point returns COVO_E_DEVICE instead of
 * enqueueing more work on poisoned data; clear != 0 resets it (after the caller has dealt with the failed step, e.g. by
 * re-creating the handle with COVO_FLAG_SHARED_DEVICE).  Returns the status before clearing, or COVO_E_NOHANDLE. */
int covo_device_status(covo_handle_t h, int32_t clear);

/* Counter-based N(0,1) fill (Philox4x32-10 + Box-Muller) keyed by
 * (key0, key1, global sample id, column): results do not depend on how samples are
 * sharded.  Stands in for jax.random.split + normal inside
 * jax.random.multivariate_normal (controllers/covo.py:212-220, mppi.py:53-65);
 * jax's threefry bitstream is unpinned/unavailable, so the stream is build-defined.
 * eps_out: float[n_samples][n_cols], rows = global ids sample_offset .. +n_samples. */
int covo_randn(covo_handle_t h, uint32_t key0, uint32_t key1, int64_t sample_offset, int32_t n_samples,
               int32_t n_cols, float *eps_out, void *stream);

/* The same draws from jax.random's OWN bitstream (threefry2x32-20, jax 0.4.x default layout), so that a
 * JAX-equipped machine can replay a run without shipping epsilon:  row n of eps_out (float[n_samples][128]) is
 *   mppi == 0:  jax.random.normal(jax.random.split(act_key, n_total)[sample_offset + n], (128,))        (covo.py:213-220)
 *   mppi != 0:  concat_t jax.random.normal(jax.random.split(jax.random.split(act_key, n_total)[..], H)[t], (4,))  (mppi.py:53-60)
 * with act_key = (key0, key1).  Twin of covo_mpc_amd/random_jax.py, which is pinned to the Random123 threefry vectors and to
 * the values jax's documentation prints; ~2x the cost of covo_randn, meant for replay / parity runs (the kernel-by-kernel
 * path), not for the fused step. */
int covo_randn_jax(covo_handle_t h, uint32_t key0, uint32_t key1, int64_t n_total, int64_t sample_offset, int32_t n_samples,
                   int32_t mppi, float *eps_out, void *stream);

/* a = clip(mu + L eps, -1, 1): jax.random.multivariate_normal's `mean + factor @ eps`
 * followed by jnp.clip (controllers/covo.py:215-224).  fp32 MFMA GEMM
 * (v_mfma_f32_32x32x2_f32; each dot product is an ascending-k fmaf chain, bit-exact).
 * L: float[128][128] row-major lower-triangular Cholesky factor of a_cov (entries
 * above the diagonal are ignored); mu: float[128]; eps: float[N][128]; a_out: float[H][N][4]. */
int covo_noise_gemm(covo_handle_t h, const float *L, const float *mu, const float *eps, int32_t N, float *a_out,
                    void *stream);

/* Same, with epsilon drawn inside the kernel (never written to HBM): row n of the virtual eps matrix is
 * the covo_randn row of global sample id sample_offset + n for the same key -- bit-identical to
 * covo_randn followed by covo_noise_gemm. */
int covo_noise_gemm_philox(covo_handle_t h, const float *L, const float *mu, uint32_t key0, uint32_t key1,
                           int64_t sample_offset, int32_t N, float *a_out, void *stream);

/* MPPI's per-step sampling (controllers/mppi.py:53-66): a[t] = clip(mu[t] + Ls[t] eps[t]).
 * Ls: float[H][4][4] lower factors; eps: float[N][H][4]; a_out: float[H][N][4]. */
int covo_noise_blockdiag(covo_handle_t h, const float *Ls, const float *mu, const float *eps, int32_t N,
                         float *a_out, void *stream);

int covo_noise_blockdiag_philox(covo_handle_t h, const float *Ls, const float *mu, uint32_t key0, uint32_t key1,
                                int64_t sample_offset, int32_t N, float *a_out, void *stream);

/* The fused N x H rollout: lax.scan(H) of vmap(N) Quad3D.step_env + done-freeze +
 * discounted cost (controllers/covo.py:227-263, mppi.py:71-106; envs/quadrotor.py:215-263,
 * 479-490; dynamics/free.py:74-155; dynamics/utils.py:266-294).  Per-sample state lives in
 * registers / LDS; only cost[N] (+ one min per 64-sample wave) is written.  Actions are re-clipped like
 * step_env does unless the handle was created with COVO_FLAG_ACTIONS_CLIPPED.  Termination follows
 * params->rollover_terminate (quadrotor.py:479-490).
 * The disturbance acting during rollout step 0 is the state's own f_disturb; for steps k >= 1 (free.py:147) it follows
 * params->disturb_kind:
 *   NONE / GAUSSIAN: f_disturb_shared [host float[3]]: the single vector every sample and step receives from the shared
 *     step_key (0 for CoVO's deterministic=True; dyn_noise_scale * normal for MPPI); NULL = 0.
 *   PERIODIC / SIN / DRAG / MIXED: f_disturb_steps [DEVICE float[COVO_H][4]], the table covo_disturb_table builds
 *     (COVO_DISTURB_KEYS_SHARED): row k = {g_k[3], c_k}, f_k = c_drag * drag(vel_{k-1}) + c_k * f_{k-1} + g_k with
 *     c_drag = 1 (DRAG), 1/3 (MIXED), 0 otherwise -- PERIODIC and SIN are wave-uniform per step (c_k = 0, g_k = the force
 *     itself: no per-sample work), DRAG and MIXED keep a per-sample force.  f_disturb_shared is then ignored.
 * pos_stats (nullable): double[COVO_H*6] accumulators, zeroed by the call, receiving
 *   per-step sum(pos - pos0) and sum((pos - pos0)^2) over samples of the post-step
 *   positions (controllers/covo.py:234-237,281); pos0 = state pos.
 * groupmin (nullable): float[ceil(N/64)] minimum of cost over each group of 64 consecutive samples. */
int covo_rollout_cost(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                      const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                      const float *a, int32_t N, float *cost_out, float *groupmin, double *pos_stats, void *stream);

/* The per-step disturbance table of a rollout that starts at `state` (DEVICE float[batch][COVO_STATE_FLOATS]; it supplies
 * time and, for PERIODIC's hold, f_disturb): out [DEVICE float[batch][COVO_H][4]], rows as described at covo_rollout_cost,
 * for params->disturb_kind = PERIODIC / SIN / DRAG / MIXED (NONE: zeros; GAUSSIAN: g_k = dyn_noise_scale * normal unless
 * `deterministic`).  The uniform draws of PERIODIC / MIXED (free.py:16-21) come from the key step_env would hand to
 * disturb_func -- disturb_key = split(split(split(k)[1])[0])[0] for step_env(k) (quadrotor.py:262, free.py:136,144) -- with k
 * threaded as `key_mode` (COVO_DISTURB_KEYS_*) says from the batch entry's key: keys_dev [DEVICE uint32[batch][2]] or, when
 * NULL, (key0, key1) for every entry.  Philox keys / host formulas of covo_mpc_amd/random.py (the stream is build-defined). */
int covo_disturb_table(covo_handle_t h, const covo_env_params *params, const float *state, int32_t batch,
                       const uint32_t *keys_dev, uint32_t key0, uint32_t key1, int32_t key_mode, int32_t deterministic,
                       float *out, void *stream);

/* controllers/covo.py:281 (mppi.py:134) from the sums covo_rollout_cost / covo_mpc_step leave in pos_stats (after the
 * all-reduce when the samples are sharded): pos_mean[k][i] = pos0[i] + S1/n, pos_std[k][i] = sqrt(max(S2/n - (S1/n)^2, 0))
 * (ddof 0), both float[COVO_H][3]; n_total = the global sample count.  One launch instead of the caller's elementwise ops. */
int covo_pos_info(covo_handle_t h, const double *pos_stats, const float *state, int64_t n_total, float *pos_mean_out,
                  float *pos_std_out, void *stream);

/* softmax weights + weighted sum as ONE online-softmax record of this shard
 * (controllers/covo.py:266-272 before normalisation): two-stage wavefront reduction.
 * groupmin (nullable): the per-64-sample minima covo_rollout_cost left for exactly this
 *   cost/N (saves one pass over cost); recomputed internally when null.
 * partial_out: float[COVO_PARTIAL_FLOATS]; floats 130 and 131 (the pad) are not written. */
int covo_softmax_reduce(covo_handle_t h, const float *cost, const float *a, int32_t N, const float *groupmin,
                        float *partial_out, void *stream);

/* Single-shard finish: covo_softmax_reduce + covo_merge(G=1) without materialising the record:
 * a_mean_out = gamma_mean * sum_n w_n a_n + (1-gamma_mean) * a_mean_old (covo.py:266-275). */
int covo_softmax_update(covo_handle_t h, const float *cost, const float *a, int32_t N, const float *groupmin,
                        const float *a_mean_old, float gamma_mean, float *a_mean_out, void *stream);

/* MPPI with covariance adaptation (controllers/mppi.py:109-125, gamma_sigma != 0; quadjax's own factory fixes gamma_sigma = 0,
 * envs/quadrotor.py:715): the update of covo_softmax_update plus
 *   a_cov_out[t] = gamma_sigma sum_n w_n (a_n[t] - a_mean_out[t]) (a_n[t] - a_mean_out[t])^T + (1 - gamma_sigma) a_cov_old[t]
 * with the NEW mean, as the reference does.  a_cov_*: float[H][4][4] (a_cov_old already shifted, mppi.py:43-49); in place allowed.
 * The weighted second moments are accumulated about a_mean_old (the mean the samples were drawn around).  Single shard. */
int covo_softmax_update_cov(covo_handle_t h, const float *cost, const float *a, int32_t N, const float *groupmin,
                            const float *a_mean_old, float gamma_mean, const float *a_cov_old, float gamma_sigma,
                            float *a_mean_out, float *a_cov_out, void *stream);

/* The same on sample-sharded ranks (round 4): covo_softmax_reduce_cov leaves this rank's UNNORMALISED record
 * {m, s, v[128], pad[2], S2[320]} (S2 = the weighted second moments about a_mean_old, which every rank shares) in the first
 * COVO_PARTIAL_FLOATS + COVO_COV_FLOATS floats of record_out -- a COVO_RANK_RECORD_COV_FLOATS rank record whose last 192 doubles are
 * the position sums (or zeros); after ONE exchange of the G records (all-gather, or covo_exchange_records_cov)
 * covo_merge_ranks_cov forms the new mean and the adapted covariances identically on every rank and, if asked, adds the position sums. */
int covo_softmax_reduce_cov(covo_handle_t h, const float *cost, const float *a, int32_t N, const float *groupmin,
                            const float *a_mean_old, float *record_out, void *stream);
int covo_merge_ranks_cov(covo_handle_t h, const float *records /* [G][COVO_RANK_RECORD_COV_FLOATS] */, int32_t G,
                         const float *a_mean_old, float gamma_mean, const float *a_cov_old, float gamma_sigma, float *a_mean_out,
                         float *a_cov_out, double *pos_stats_out, void *stream);

/* Merge G shard records (this GPU's, or the all-gathered records of all ranks), normalise,
 * blend with the old mean (controllers/covo.py:270-275):
 *   a_mean_out = gamma_mean * (sum_g v_g e^{-(m_g-m)/lam}) / (sum_g s_g e^{-(m_g-m)/lam})
 *              + (1-gamma_mean) * a_mean_old.         a_mean_*: float[128] (index 4t+d). */
int covo_merge(covo_handle_t h, const float *partials, int32_t G, const float *a_mean_old, float gamma_mean,
               float *a_mean_out, void *stream);

/* Sample-sharded step: merge the all-gathered RANK records (float[G][COVO_RANK_RECORD_FLOATS]: rank g's
 * covo_mpc_step wrote its {m, s, v} to partial_out = record and its position sums to pos_stats = record + COVO_PARTIAL_FLOATS)
 * like covo_merge, and (pos_stats_out != NULL) sum the ranks' position sums into pos_stats_out [double[COVO_POS_STATS_DOUBLES]]
 * for covo_pos_info -- the statistics travel in the same message as the softmax partial, not in a second collective. */
int covo_merge_ranks(covo_handle_t h, const float *records, int32_t G, const float *a_mean_old, float gamma_mean,
                     float *a_mean_out, double *pos_stats_out, void *stream);

/* covo_merge_ranks over all-gathered records of `record_floats` floats each: COVO_RANK_RECORD_FLOATS, or
 * COVO_RANK_RECORD_COV_FLOATS -- the records of a core built for MPPI's covariance adaptation that runs a step with
 * gamma_sigma == 0: {m, s, v[128], pad[2]} in front, the 320 second-moment slots unused, the position sums at the END of the
 * wider record.  Any other record_floats is refused. */
int covo_merge_ranks_wide(covo_handle_t h, const float *records, int32_t G, int32_t record_floats, const float *a_mean_old,
                          float gamma_mean, float *a_mean_out, double *pos_stats_out, void *stream);

/* The exchange of the rank records as direct peer writes instead of a collective (exchange.hip).  Setup, once:
 * every rank calls covo_exchange_create (allocates its buffer, returns its inter-process handle), the G handles are
 * all-gathered by the caller (any transport: they are 64 opaque bytes), every rank calls covo_exchange_connect with all G of
 * them (rank order).  Per step: covo_exchange_records enqueues, on `stream`, the push of this rank's record into every peer's
 * buffer and the wait for all G records, which land in gathered_out [float[G][COVO_RANK_RECORD_FLOATS], device]; no host
 * synchronisation.  A peer that does not deliver within the time-out (covo_exchange_set_timeout; default 60 s, or
 * COVO_EXCHANGE_TIMEOUT_S at covo_exchange_create) raises COVO_DEVSTAT_EXCHANGE and leaves NaN records.  With a
 * connected exchange covo_run_episode also runs on sample-sharded handles (args->partial_out = this rank's record).
 * covo_exchange_connect returns COVO_E_UNSUPPORTED, before mapping anything, when two ranks sit on DIFFERENT devices and either
 * buffer is coarse-grained (the fine-grained allocation failed): remote xGMI writes into it would not be guaranteed visible.
 * NOT measured over xGMI (the build pool has single-GPU boxes): the host mirror keeps the collective unless asked. */
int covo_exchange_create(covo_handle_t h, int32_t world, int32_t rank, void *handle_out /* [host COVO_EXCHANGE_HANDLE_BYTES] */);
int covo_exchange_connect(covo_handle_t h, const void *handles /* [host world x COVO_EXCHANGE_HANDLE_BYTES] */);
int covo_exchange_set_timeout(covo_handle_t h, double seconds);
int covo_exchange_records(covo_handle_t h, const float *record, float *gathered_out, void *stream);
/* the same for the COVO_RANK_RECORD_COV_FLOATS record kind (gathered_out: float[G][COVO_RANK_RECORD_COV_FLOATS]) */
int covo_exchange_records_cov(covo_handle_t h, const float *record, float *gathered_out, void *stream);

/* PCI bus id ("0000:c1:00.0") of HIP device `device` of this process -> out (NUL-terminated, len >= 16): the PHYSICAL identity
 * of a GPU.  Device indices are per-process (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES renumber them: every isolated rank sees
 * index 0), so ranks that must know whether they share a GPU compare this, not the index. */
int covo_device_bus_id(int32_t device, char *out, int32_t len);

/* a_mean <- [a_mean[1:], a_mean[-1]] (controllers/covo.py:201-203).  in != out. */
int covo_shift_mean(covo_handle_t h, const float *a_mean_in, float *a_mean_out, void *stream);

/* Exact Hessian of the CoVO objective -(sum_k r(s_k) + r(s_0)) w.r.t. the flattened mean
 * actions: jax.jacfwd(jax.jacfwd(get_cumulated_cost)) of controllers/covo.py:134-185
 * (deterministic, no discount, no done-freeze), fp64.  Second-order adjoint: one hyper-dual evaluation of
 * the step model per (time, pair of step inputs), a costate and a sensitivity recursion, and
 * sum_k S_k^T M_k S_k on the matrix cores (hessian_adj.hip).  May (re)allocate scratch, with a stream sync,
 * the first time a batch size is seen.  R_out: double[batch][128][128]; state/a_mean are strided by
 * COVO_STATE_FLOATS / 128 per batch entry; traj is shared.  The reward is params->reward_kind's.
 * f_disturb_steps [DEVICE float[batch][COVO_H][4], nullable]: covo_disturb_table(COVO_DISTURB_KEYS_HESSIAN, deterministic = 1)
 * -- required for params->disturb_kind PERIODIC / SIN / DRAG / MIXED (get_hessian's deterministic=True only switches the
 * gaussian model off, quadrotor.py:234-235); NULL = no force after step 0.  DRAG / MIXED make the force part of the
 * differentiated state: those two run the kernels' 16-component instantiation (state + force; hessian_adj.hip adj16). */
int covo_hessian(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                 const covo_env_params *params, const float *a_mean, const float *f_disturb_steps, int32_t batch,
                 double *R_out, void *stream);

/* The same Hessian by one hyper-dual ROLLOUT per unordered pair of actions (hessian.hip): ~4x slower,
 * derived independently; kept as the cross-check of covo_hessian. */
int covo_hessian_pairs(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                       const covo_env_params *params, const float *a_mean, const float *f_disturb_steps, int32_t batch,
                       double *R_out, void *stream);

/* CoVO's optimal covariance (controllers/covo.py:116-132) and the lower Cholesky factor
 * jax.random.multivariate_normal takes of it (covo.py:216-218).  The reference's
 *   eigh -> shift spectrum to min 1e-2 -> U diag(exp(log_s)) U^T (det = sigma^(2n)) -> symmetrise
 * is the matrix function Sigma = c (R + delta I)^(-1/2), delta = 1e-2 - lambda_min(R); it is evaluated
 * WITHOUT an eigendecomposition (fp64 MFMA GEMM pipeline: repeated squaring + Rayleigh-Ritz for
 * lambda_min, coupled Newton-Schulz for the inverse square root, Cholesky for log det; sigma_ns.hip)
 * and agrees with LAPACK eigh to ~1e-15.  Sigma is rounded to fp32 (the reference's a_cov dtype)
 * before its Cholesky factor is taken.  May (re)allocate scratch, with a stream sync, the first time a
 * batch size is seen.
 * R: double[batch][128][128]; Sigma_out: float[batch][128][128] (nullable);
 * L_out: float[batch][128][128] lower-triangular. */
int covo_sigma(covo_handle_t h, const double *R, int32_t batch, float sample_sigma, float *Sigma_out,
               float *L_out, void *stream);

/* Same result by an explicit symmetric eigendecomposition (one-sided cyclic block Jacobi, fp64, one
 * workgroup per matrix; sigma.hip).  Slower (latency of 10-12 sweeps); kept as an independent check. */
int covo_sigma_jacobi(covo_handle_t h, const double *R, int32_t batch, float sample_sigma, float *Sigma_out,
                      float *L_out, void *stream);

/* ---- Experiment switches of ONE handle (round 6; rounds 1-5 kept them process-global).  A new handle takes its defaults from the
 * environment (COVO_FUSE_SMALL, COVO_STREAM_GEMM, COVO_FOLD_BEGIN, COVO_NS_DEFLATE, COVO_NS_MERGED; csrc/step.hip:
 * covo_default_opts); the setters below change them for THAT handle only and make it re-capture its step graphs at the next step.
 * They exist for A/B measurements and the parity tests: every pair of settings gives the same bits unless stated otherwise.
 * A handle is single-threaded (as every entry point that takes one). */

/* 0: covo-offline / MPPI steps of <= 256 sample groups run their staged launches (begin | noise | rollout + records | merge)
 * instead of the ONE fused launch of csrc/step_small.hip (the default where eligible). */
int covo_debug_set_fuse_small(covo_handle_t h, int on);

/* 0: covo-online's noise GEMM runs as a launch of its own behind the Sigma chain (rounds 1-4) instead of streamed under the
 * factorisation inside the chain's finalize launch (the default for one matrix on a GPU of one's own).  Same actions, a_cov and
 * means bit for bit. */
int covo_debug_set_stream_gemm(covo_handle_t h, int on);

/* 0: eager covo-online steps keep the begin launch (mean shift, key derivation, sequence bump) instead of folding its work into the
 * Hessian's first launch (the default; every launch of a folded step reads args->state where it lies instead of the handle's
 * fixed-address copy).  Same bits (tests/test_gpu_parity.py::test_folded_begin_equals_the_begin_launch). */
int covo_debug_set_fold_begin(covo_handle_t h, int on);

/* Debug aid: copy `count` doubles from offset `offset_doubles` of the Sigma pipeline's scratch (layout in
 * sigma_ns.hip: 11 matrices [batch][128][128], then 3 712 doubles of slots per matrix -- SC_* in sigma_ns.hip: lambda_min, delta,
 * scale, the iterate the result was taken from, iteration counts, barrier status ... --, then the filter's iterate buffers) to
 * `out` (device or pinned host). */
int covo_debug_sigma_workspace(covo_handle_t h, double *out, int64_t offset_doubles, int64_t count, void *stream);
/* 0 switches the deflation of the bottom eigenpair in the eigh-free Sigma chain off (sigma_ns.hip: the Newton-Schulz iteration then
 * runs on B itself, ~2 iterations more); default on.  Results agree to fp64 rounding either way (not bit for bit: another
 * iteration sequence). */
int covo_debug_set_ns_deflate(covo_handle_t h, int on);
/* 0: the one-matrix Sigma chain runs its two persistent launches (squarings with the evaluations inside | Newton-Schulz iterations)
 * as TWO launches (rounds 4-5) instead of one whose iteration workgroups wait inside for the chain's result (csrc/sigma_ns.hip:
 * ns_chain_kernel; the default for covo-online steps on a GPU of one's own; COVO_NS_MERGED=0 in the environment).  Same Sigma and L
 * bit for bit. */
int covo_debug_set_ns_merged(covo_handle_t h, int on);
/* 1 makes the Sigma chain's persistent launches behave as if their workgroups had NOT all landed on one XCD (sigma_ns.hip: every
 * access stays an agent-scope atomic, COH_AGENT) -- the fallback of the placement check, which no MI355X box takes by itself; 0
 * (default): as detected.  Same Sigma and L bit for bit. */
int covo_debug_set_ns_coherence(covo_handle_t h, int force_agent);
int covo_debug_hess_workspace(covo_handle_t h, double *out, int64_t offset_doubles, int64_t count, void *stream);

/* Per-step sampling diagnostics (ABI 10; off by default, and off changes nothing a caller can observe).  With a buffer attached,
 * every control step of this handle -- covo_mpc_step (all modes, staged and fused, eager and graph), covo_mpc_step_batched,
 * covo_mpc_step_batched_mode and the steps of the three episode drivers -- also writes COVO_DIAG_FLOATS floats per instance, over
 * the step's N samples with costs c_n as the rollout wrote them, m = min c_n, w_n = exp(-(c_n - m) / lambda):
 *   [0] ess            (sum w)^2 / sum w^2      (1: the update follows one sample; N: the costs do not discriminate)
 *   [1] cost_min       m
 *   [2] cost_weighted  sum w c / sum w
 *   [3] cost_mean      sum c / N
 *   [4] weight_sum     sum w
 *   [5] n_samples      N as a float
 *   [6], [7]           reserved, written as 0
 * The sums are formed by the launches that form the update itself (stage-1 records and their merge), in a fixed order; every
 * other output of the step is bit-identical to the same call without diagnostics.
 * covo_set_step_diag: diag = DEVICE float[n_inst][COVO_DIAG_FLOATS], row e = instance e of a batched step (a single step writes
 *   row 0); NULL = off.  A batched step with more instances than n_inst is refused.
 * covo_set_episode_diag_log: log = DEVICE float[n_inst][stride][COVO_DIAG_FLOATS]; step k of an episode driver's segment writes
 *   instance e's row to log[e][log_index + k] (covo_run_episode: log_index = 0, one instance) from the device, between that
 *   control step and its env step; NULL = off.  A segment that would leave the log is refused.
 * A change of where the steps write (attach, detach, another buffer) makes the handle re-capture its step graphs at the next
 * call, like a covo_debug_set_* switch.  Out of scope: a sample-sharded step (partial_out != NULL) with diagnostics attached is
 * refused -- the rank records carry no diagnostic sums. */
int covo_set_step_diag(covo_handle_t h, float *diag, int32_t n_inst);
int covo_set_episode_diag_log(covo_handle_t h, float *log, int32_t stride);

/* The ESS floor: a per-step temperature solved on the device from the step's costs (additive to ABI 10: COVO_HAS_ESS_FLOOR; off
 * by default, and off changes nothing a caller can observe).  With the handle's configured temperature lam0 (covo_config.lam),
 * costs c_n as the rollout wrote them, m = min c_n, w_n(lam) = expf((m - c_n) * (1 / lam)) in fp32 and
 * ESS(lam) = (sum w)^2 / sum w^2 (non-decreasing in lam):
 *   ESS(lam0) >= ess_min   lam_eff = lam0 exactly: the floor is inactive
 *   otherwise              lam_eff solves ESS(lam) = ess_min on (lam0, 3 (max finite c - m)], to the resolution of fp32 temperatures
 * The bracket holds the solution for 1 <= ess_min <= N / 2; a step whose ess_min lies outside is refused.  The step's weights,
 * its mean update, MPPI's covariance adaptation and the diagnostics use lam_eff; actions, costs, Sigma, L and the key chain are those
 * of the same step without a floor.  Per instance the solver leaves float[COVO_LAM_FLOATS]:
 *   [0] lam_eff   [1] 1 / lam_eff (what the update's launches multiply by)   [2] ESS(lam0)   [3] ESS evaluations taken (<= 64)
 * covo_set_step_ess_floor: ess_min = 0 turns the floor off; lam_out = DEVICE float[n_inst][COVO_LAM_FLOATS] (row e = instance e of a
 *   batched step, a single step writes row 0), or NULL for a buffer the handle owns.  Covered: covo_mpc_step (all modes, eager and
 *   graph), covo_mpc_step_batched and the episode drivers that call them; such a step runs staged -- rollout, solver, stage 1 and
 *   merge reading 1 / lam_eff from device memory -- so one captured graph serves every step.  Attaching, detaching or changing
 *   ess_min makes the handle re-capture its step graphs, like covo_set_step_diag.  Refused before any launch: a sample-sharded step
 *   (partial_out != NULL), and covo_mpc_step_batched_mode / covo_run_episode_batched_mode in the MPPI and covo-offline modes (their
 *   fused launch needs the temperature before all costs exist, and there is no staged batched fallback).
 * covo_ess_lambda: the solver alone on the caller's costs, DEVICE float[n_inst][n_samples] -> out = DEVICE
 *   float[n_inst][COVO_LAM_FLOATS]; it forms the cost minima itself. */
#define COVO_HAS_ESS_FLOOR 1
#define COVO_LAM_FLOATS 4
int covo_set_step_ess_floor(covo_handle_t h, float ess_min, float *lam_out, int32_t n_inst);
int covo_ess_lambda(covo_handle_t h, const float *cost, int32_t n_samples, int32_t n_inst, float lam0, float ess_min, float *out, void *stream);

/* The annealed MPPI step: a per-pass noise schedule and weights on standardised costs (additive to ABI 10: COVO_HAS_STEP_ANNEAL; off
 * by default, and off changes nothing a caller can observe).  For an MPPI step of k = iters passes (covo_set_step_iters):
 *   schedule   sigma_table = HOST float[n_pass][32], formed by the caller (the Python layer: fp32(sigma0 beta_pass^i beta_stage^(31 - h)),
 *              in fp64, rounded once).  Pass i samples a = clip(mu_i + sigma[i][h] eps) stage by stage: one launch behind the pass's
 *              begin launch writes the block factors sigma[i][h] I_4 and a_cov[h] = fp32(sigma[i][h]^2) I_4.  eps, the key walk and
 *              mu_i are those of the same step without the attachment; a_cov on input is ignored, on output it is the last pass's.
 *   temp > 0   with F the finite costs of the pass: mean = sum_F c / |F|, std = sqrt(sum_F (c - mean)^2 / |F|) (two passes, fp64),
 *              lam_eff = fp32(temp std); the update is the softmax update at lam_eff through the ESS floor's staged launches.
 *              Fallback to the configured lam, decided on the device: |F| < 2, std == 0, or lam_eff not a normal fp32 number.
 *              The row: float[COVO_LAM_FLOATS] = {lam_eff, 1 / lam_eff (the correctly rounded fp32 quotient, as the ESS floor's row),
 *              (float)std, bits(int32 |F| | fallback << 31)}.
 *   temp = 0   every pass updates at the configured lam; no solver runs.
 * covo_set_step_anneal: a NULL table with temp = 0 turns it off.  rows_out = DEVICE float[n_inst][n_pass][COVO_LAM_FLOATS] (row (e, i):
 *   instance e's pass i; temp > 0 only), or NULL.  The last pass's row is also the handle's temperature row: COVO_EPLOG_LAM logs it.
 *   The table is copied into device memory the handle owns; any change makes the handle re-capture its step graphs.
 *   Refused at the step, before any launch: a mode other than COVO_MODE_MPPI; n_pass != the step's iters; gamma_sigma != 0 (the
 *   schedule owns a_cov); temp > 0 together with the ESS floor or the elite-set update; a sample-sharded step; the env-batched fused
 *   launch (the staged batch, covo_set_step_batched_staged, takes it).
 * covo_cost_standardise: the solver alone on the caller's costs, DEVICE float[n_inst][n_samples] -> out = DEVICE
 *   float[n_inst][COVO_LAM_FLOATS]. */
#define COVO_HAS_STEP_ANNEAL 1
int covo_set_step_anneal(covo_handle_t h, const float *sigma_table, int32_t n_pass, float temp, float *rows_out, int32_t n_inst);
int covo_cost_standardise(covo_handle_t h, const float *cost, int32_t n_samples, int32_t n_inst, float lam0, float temp, float *out, void *stream);

/* Spline nodes for the annealed MPPI step: perturbations that are smooth over the horizon, drawn in 4 n_nodes dimensions instead of
 * 128 (additive to ABI 10: COVO_HAS_STEP_NODES; off by default, and off changes nothing a caller can observe).  With M = n_nodes nodes
 * spread over the 32 stages, W[h][m] the interpolation weight of node m at stage h and sigma_n[i][m] the schedule over the nodes,
 *   basis_table = HOST float[n_pass][32][n_nodes], B[i][h][m] = fp32(sigma_n[i][m] W[h][m]), formed by the caller (the Python layer:
 *              fp64, rounded once).  Pass i samples a[h] = clip(mu_i[h] + sum_m B[i][h][m] e_m), e_m = the m-th normal4 of the stream
 *              the step without nodes draws its 32 from (same key walk), the sum an ascending-m fmaf chain from 0 per component.
 *              The mean, the update and every later launch are untouched: only the perturbations are splines.
 *   schedule   covo_set_step_anneal's table must then hold the stages' MARGINAL standard deviations sigma_e[i][h] =
 *              fp32(sqrt(sum_m B[i][h][m]^2)): its launch writes a_cov[h] = fp32(sigma_e^2) I_4, which is only the 4 x 4 block diagonal
 *              of the sampled covariance (B B^T) (x) I_4 of rank 4 n_nodes.  n_nodes = 32 with B[i] = diag(sigma[i]) is the step
 *              without nodes, bit for bit.
 * covo_set_step_nodes: the table is copied into device memory the handle owns; NULL turns it off; any change makes the handle
 *   re-capture its step graphs.  Refused at the step, before any launch: no schedule attached (covo_set_step_anneal with a table);
 *   n_pass != the schedule's; n_nodes outside [2, 32]; and whatever the schedule refuses.
 * covo_step_nodes: what is attached -> *n_pass, *n_nodes (both 0: nothing).
 * covo_noise_nodes_philox: the sampler alone, basis = DEVICE float[32][n_nodes], otherwise covo_noise_blockdiag_philox's arguments. */
#define COVO_HAS_STEP_NODES 1
int covo_set_step_nodes(covo_handle_t h, const float *basis_table, int32_t n_pass, int32_t n_nodes);
int covo_step_nodes(covo_handle_t h, int32_t *n_pass, int32_t *n_nodes);
int covo_noise_nodes_philox(covo_handle_t h, const float *basis, int32_t n_nodes, const float *mu, uint32_t key0, uint32_t key1,
                            int64_t sample_offset, int32_t N, float *a_out, void *stream);

/* covo-online in spline-node space: the optimal covariance of the node-parameterised problem (additive to ABI 10:
 * COVO_HAS_SIGMA_NODES; off by default, and off changes nothing a caller can observe).  With M nodes, W = double[32][M] their
 * interpolation weights (rows sum to 1), P = W (x) I_4 [128][d] and d = 4 M <= 64, a covo-online step (every pass of an iterated one)
 * forms, per instance and in ONE launch of one workgroup (csrc/sigma_nodes.hip), from the Hessian R at its shifted mean
 *   R_M     = P^T ((R + R^T) / 2) P                        fp64 [d][d], symmetric bit for bit
 *   Sigma_M = optimize_sigma(R_M) with element_num = d     eigenpairs (lam, U), o = lam - lam_min + 1e-2,
 *             log_s = ((4 d log sigma + sum log o) / d) / 2 - (log o) / 2, Sigma_M = U diag(exp(log_s)) U^T: log det Sigma_M = 2 d log sigma
 *   L_M     = the lower Cholesky factor of Sigma_M (fp64),  G = fp32(P L_M) float[128][d], summed in fp64 and rounded once
 *   a_cov   = fp32(P Sigma_M P^T) float[128][128], of rank d, symmetric bit for bit
 * and samples a[h][n][i] = clip(mu[h][i] + acc), acc ONE ascending-c fmaf chain from 0 over G[(h, i)][c] eps_c, c < d, eps_c component
 * c mod 4 of the (c div 4)-th normal4 of the stream covo_noise_blockdiag_philox draws its 32 from (same key walk); every launch shape
 * gives the same bits.  The Sigma chain, its finalize launch and the noise GEMM do not run in such a step; everything behind the
 * sampler is untouched.  Fallback, decided on the device and reported in the side row, never an error: an R_M that is not finite, a
 * Jacobi that has not converged at its sweep limit, a factor with a non-positive pivot -- that instance samples from sigma^2 I_d.
 * rows: DEVICE float[n_inst][COVO_SIGMA_NODES_FLOATS] = {lam_min, lam_max of R_M, largest, smallest eigenvalue of Sigma_M,
 *   log det Sigma_M, sweeps, flags (COVO_SIGMA_NODES_*), d}, instance e's row of every step (lam_* are NaN when R_M was not finite).
 * covo_set_step_sigma_nodes: W is copied into device memory the handle owns; NULL turns it off; any change makes the handle
 *   re-capture its step graphs.  Refused: M outside [2, COVO_SIGMA_NODES_MAX], a W entry that is not finite, n_inst outside
 *   (0, COVO_MAX_ENVS]; at the step, before any launch: a mode other than covo-online, a Sigma period > 1, Sigma adapt, the Newton
 *   refinement (its direction needs the full-rank Sigma), a sample-sharded step, more instances than rows.
 * covo_step_sigma_nodes: what is attached -> *M (0: nothing); SigmaM_out / G_out (DEVICE, nullable): copies of the n_inst instances'
 *   Sigma_M double[n_inst][d][d] and G float[n_inst][128][d] of the last step, enqueued on `stream`.
 * covo_sigma_nodes: the first launch alone on the caller's R = DEVICE double[batch][128][128] and W_dev = DEVICE double[32][M].
 * covo_noise_factor_philox: the sampler alone, G = DEVICE float[128][d], d = 8, 12, .., 64, otherwise covo_noise_nodes_philox's
 *   arguments. */
#define COVO_HAS_SIGMA_NODES 1
#define COVO_SIGMA_NODES_MAX 16
#define COVO_SIGMA_NODES_FLOATS 8
#define COVO_SIGMA_NODES_NONFINITE 1
#define COVO_SIGMA_NODES_NO_CONVERGENCE 2
#define COVO_SIGMA_NODES_PIVOT 4
int covo_set_step_sigma_nodes(covo_handle_t h, const double *W, int32_t M, float *rows, int32_t n_inst);
int covo_step_sigma_nodes(covo_handle_t h, int32_t *M, double *SigmaM_out, float *G_out, int32_t n_inst, void *stream);
int covo_sigma_nodes(covo_handle_t h, const double *R, int32_t batch, const double *W_dev, int32_t M, float sample_sigma,
                     double *SigmaM_out, float *G_out, float *Sigma_out, float *rows_out, void *stream);
int covo_noise_factor_philox(covo_handle_t h, const float *G, int32_t d, const float *mu, uint32_t key0, uint32_t key1,
                             int64_t sample_offset, int32_t N, float *a_out, void *stream);

/* The elite-set update: exact top-K selection on the device, the cross-entropy method's update rule (additive to ABI 10:
 * COVO_HAS_ELITE_UPDATE; off by default, and off changes nothing a caller can observe).  Per instance and per pass, with the costs
 * c_n as the rollout wrote them, key(n) = (u(c_n) << 32) | n: u is the order-preserving unsigned form of the fp32 bits (sign bit
 * set for c >= 0, all bits inverted for c < 0; -0 and +0 are one cost), a NaN cost has u = 0xFFFFFFFF; the index in the low word
 * makes the keys distinct.  The ELITE SET is the K samples of smallest key: equal costs go to the lowest indices, NaN costs last,
 * +inf is an ordinary large cost, and the set has exactly K members for every input.  The update is the step's own update with the
 * weights w_n = 1 for the elites and 0 otherwise:
 *   new mean   gamma_mean * (sum over the elites of a_n / K) + (1 - gamma_mean) * shifted old mean
 *   MPPI with gamma_sigma != 0: the elites' second moments through the same covariance merge as the softmax weights' -- the
 *              cross-entropy method's refit, smoothed by gamma_sigma; covo-online / covo-offline keep their Sigma / L
 * Actions, costs, Sigma, L, the key chain and sampling are those of the same step without it.  With diagnostics attached: ess and
 * weight_sum are K, cost_weighted is the elites' mean cost, cost_min / cost_mean are as before.  The arbiter's candidate 0 is the
 * elite mean; with iterations per step every pass selects again.  If the smallest cost is not finite the new mean is NaN.
 * Per instance the selector leaves float[COVO_ELITE_FLOATS]:
 *   [0] bits(uint32: the threshold key's cost word)   [1] bits(uint32: the threshold key's index word)   [2] cost_min
 *   [3] cost_kth, the K-th smallest cost   [4] K   [5] the elites whose cost word is the threshold's   [6..7] 0
 * so that the elite set is {n : key(n) <= threshold}.
 * covo_set_step_elite: K = 0 turns it off; rows_out = DEVICE float[n_inst][COVO_ELITE_FLOATS] (row e = instance e of a batched
 *   step, a single step writes row 0), or NULL for a buffer the handle owns.  Covered: covo_mpc_step (all modes, eager and graph),
 *   covo_mpc_step_batched and the episode drivers that call them; such a step runs staged -- rollout, selector, stage 1 with 0/1
 *   weights, the merges of the softmax update -- so one captured graph serves every step.  Attaching, detaching or another K makes
 *   the handle re-capture its step graphs, like covo_set_step_ess_floor.  Refused before any launch, with a message that names the
 *   condition: K outside [1, n_samples]; n_inst outside (0, COVO_MAX_ENVS]; the elite set together with an ESS floor (both define
 *   the weights); a sample-sharded step (partial_out != NULL); covo_mpc_step_batched_mode / covo_run_episode_batched_mode in the
 *   MPPI and covo-offline modes (their fused launch needs the weights before all costs exist, and there is no staged batched
 *   fallback).
 * covo_elite_select: the selector alone on the caller's costs, DEVICE float[n_inst][n_samples] -> out = DEVICE
 *   float[n_inst][COVO_ELITE_FLOATS]. */
#define COVO_HAS_ELITE_UPDATE 1
#define COVO_ELITE_FLOATS 8
int covo_set_step_elite(covo_handle_t h, int32_t K, float *rows_out, int32_t n_inst);
int covo_elite_select(covo_handle_t h, const float *cost, int32_t n_samples, int32_t n_inst, int32_t K, float *out, void *stream);

/* The flight recorder: the plan of a control step and the trace of an episode (additive to ABI 10: COVO_HAS_PLAN_TRACE; off by
 * default, and off changes nothing a caller can observe).
 * The PLAN of a step, for one instance: a_plan = clip(a_new, -1, 1), a_new the mean the step leaves in a_mean (covo.py:275,
 * mppi.py:116; before the next step's shift), rolled out from the state the step planned from with exactly the inputs the step's
 * sample rollouts had -- covo_env_params, trajectory window, discount and the same disturbance (NONE / GAUSSIAN: the step's one
 * shared vector, 0 under deterministic = 1; PERIODIC / SIN / DRAG / MIXED: the step's per-step table):
 *   plan row  float[COVO_PLAN_FLOATS] = {cost_plan, 0, 0, 0, pos_plan[COVO_H][3]}: cost_plan is what covo_rollout_cost gives that
 *             one action sequence (done-freeze and discount included; formed by the rollout kernel's own stage functions, bit for
 *             bit), pos_plan[k] the position AFTER rollout step k (covo.py:234-237's poses; they keep integrating after done).
 *   trace row float[COVO_TRACE_FLOATS] = [0..31] true state, [32..63] noisy state, [64..67] u = a_new[0][0..3], [68..167] the
 *             step's plan row -- both states as they are between the control step and its env step, i.e. the PRE-step state of
 *             the env step that follows (state layout above; word 25 is the int32 time).
 * One extra eager launch per step for all instances (csrc/plan_trace.hip), behind the step; no captured step graph changes.
 * covo_set_step_plan: plan = DEVICE float[n_inst][COVO_PLAN_FLOATS]; every control step of the handle -- covo_mpc_step (all
 *   modes, staged and fused, eager and graph), covo_mpc_step_batched, covo_mpc_step_batched_mode and the steps of the three episode
 *   drivers -- also writes row e for instance e (a single step: row 0); NULL = off.  A batched step with more instances than
 *   n_inst is refused.
 * covo_set_episode_trace: trace = DEVICE float[n_inst][stride][COVO_TRACE_FLOATS]; step k of an episode driver's segment writes
 *   instance e's row to trace[e][log_index + k] (covo_run_episode: log_index = 0, one instance); NULL = off.  A segment that would
 *   leave the trace is refused.
 * Every other output of a step (u, a_mean, a_cov, costs, diagnostics, the env log, the key chain) is bit-identical with either
 * attached or not.  Out of scope: a sample-sharded step (partial_out != NULL) with either attached is refused -- a rank holds only
 * its shard's record until the exchange. */
#define COVO_HAS_PLAN_TRACE 1
#define COVO_PLAN_FLOATS  100   /* {cost_plan, 0, 0, 0, pos_plan[COVO_H][3]} */
#define COVO_TRACE_FLOATS 168   /* [0..31] true state  [32..63] noisy state  [64..67] u
                                   [68..167] the step's plan row (COVO_PLAN_FLOATS) */
int covo_set_step_plan(covo_handle_t h, float *plan, int32_t n_inst);       /* DEVICE float[n_inst][COVO_PLAN_FLOATS];  NULL = off */
int covo_set_episode_trace(covo_handle_t h, float *trace, int32_t stride);  /* DEVICE float[n_inst][stride][COVO_TRACE_FLOATS]; NULL = off */
/* The sample fan: K of a step's N sampled rollouts as trajectories (additive to ABI 10: COVO_HAS_SAMPLE_FAN; off by default, and
 * off changes nothing a caller can observe).  For one instance, a step with N samples and a fan size 1 <= K <= min(COVO_FAN_MAX, N):
 *   fan       float[K][COVO_FAN_FLOATS], row s = {cost_s, bits(int32 n_s), 0, 0, pos_s[COVO_H][3]} -- the layout of a plan row.
 *             n_s: the local sample the row was taken from -- idx[s] clamped into [0, N) (duplicates allowed), or, with idx = NULL,
 *             the stride (s * N) / K in integer arithmetic.  pos_s[k]: the position of sample n_s AFTER rollout step k
 *             (covo.py:234-237's poses[k, n_s]; they keep integrating after done).  cost_s: what the rollout kernel's own stage
 *             functions give the action stripe a[:, n_s, :] with exactly the inputs of the step's sample rollouts (noisy state,
 *             trajectory window, covo_env_params, discount, the same disturbance as for the plan) -- equal to cost[n_s] bit for bit.
 * One extra eager launch per step for all instances (csrc/sample_fan.hip), behind the step and the plan launch; no captured step
 * graph changes, and every other output of a step is bit-identical with the fan attached or not.
 * covo_rollout_fan: stateless, the arguments of covo_rollout_cost; idx = DEVICE int32[K] or NULL; fan_out = DEVICE
 *   float[K][COVO_FAN_FLOATS].  Run it behind covo_rollout_cost on the same `a` to get the trajectories of chosen samples.
 * covo_set_step_fan: fan = DEVICE float[n_inst][K][COVO_FAN_FLOATS], idx = DEVICE int32[n_inst][K] or NULL (read by every step's
 *   launch: the caller may rewrite it between steps); every control step of the handle -- covo_mpc_step (all modes, staged and
 *   fused, eager and graph), covo_mpc_step_batched, covo_mpc_step_batched_mode and the steps of the three episode drivers -- also
 *   writes instance e's fan (a single step: instance 0); fan = NULL: off.
 * covo_set_episode_fan: fanlog = DEVICE float[n_inst][stride][K][COVO_FAN_FLOATS] with the K (and idx) of covo_set_step_fan, which
 *   must be called first (fan = NULL there with K > 0 keeps K and idx for the log alone); step k of an episode driver's segment
 *   writes instance e's fan to fanlog[e][log_index + k] (covo_run_episode: log_index = 0, one instance); NULL = off.
 * Refused before any launch, with a message that names the condition: K outside [1, COVO_FAN_MAX]; a step with n_samples < K; a
 * batched step with more instances than n_inst; an episode segment that would leave the log; a sample-sharded step
 * (partial_out != NULL) -- a rank's `a` holds its shard only. */
#define COVO_HAS_SAMPLE_FAN 1
#define COVO_FAN_FLOATS 100   /* {cost_s, bits(int32 n_s), 0, 0, pos_s[COVO_H][3]} */
#define COVO_FAN_MAX    64
int covo_rollout_fan(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                     const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                     const float *a, int32_t N, const int32_t *idx, int32_t K, float *fan_out, void *stream);
int covo_set_step_fan(covo_handle_t h, float *fan, const int32_t *idx, int32_t K, int32_t n_inst);
int covo_set_episode_fan(covo_handle_t h, float *fanlog, int32_t stride);
/* The update arbiter: a control step commits the best of {softmax mean, old plan, best sample} (additive to ABI 10:
 * COVO_HAS_UPDATE_ARBITER; off by default, and off changes nothing a caller can observe).  Per instance and control step, three
 * candidates, each [COVO_H][4]:
 *   0  softmax mean  the a_mean the step has just written (covo.py:275 / mppi.py:116)
 *   1  nominal       the shifted mean the step sampled around (what covo_shift_mean gives the step's input mean)
 *   2  best sample   a[:, n*, :] with n* = argmin_n cost[n] over the step's own costs; NaN costs are skipped, equal costs resolve to
 *                    the lowest index; all NaN: the candidate is absent and n* = -1
 * Candidates 0 and 1 are clipped to [-1, 1] for evaluation only.  Every enabled candidate is rolled out by the rollout kernel's own
 * stage functions with exactly the inputs of the step's sample rollouts (noisy state, trajectory window, covo_env_params, discount,
 * the same disturbance as for the plan).  mask bit c enables candidate c; a masked-out or absent candidate has cost +inf.  choice =
 * the enabled candidate of least cost (a NaN cost counts as +inf, equal costs resolve to the lowest candidate number, all +inf: 0).
 * Choice 0 leaves a_mean untouched; 1 writes the nominal, unclipped; 2 writes a[:, n*, :].  Nothing else of the step changes.
 *   row  float[COVO_ARB_FLOATS] = {cost_softmax, cost_nominal, cost_best, cost_chosen, bits(int32 choice), bits(int32 n_best), 0, 0}
 * One extra eager launch per step for all instances (csrc/update_arbiter.hip), behind the step and ahead of the plan and fan
 * launches: the plan, the trace's u and an episode driver's env step see the arbitrated mean.  No captured step graph changes.
 * covo_arbitrate: stateless, the arguments of covo_rollout_fan plus cost = DEVICE float[N], a_nominal = DEVICE float[128],
 *   a_mean_inout = DEVICE float[128], row_out = DEVICE float[COVO_ARB_FLOATS].
 * covo_set_step_arbiter: rows = DEVICE float[n_inst][COVO_ARB_FLOATS]; every control step of the handle -- covo_mpc_step (all modes,
 *   staged and fused, eager and graph), covo_mpc_step_batched, covo_mpc_step_batched_mode and the steps of the three episode
 *   drivers -- arbitrates and writes instance e's row (a single step: instance 0); rows = NULL: off, the episode log with it.
 * covo_set_episode_arbiter_log: log = DEVICE float[n_inst][stride][COVO_ARB_FLOATS], after covo_set_step_arbiter; step k of an
 *   episode driver's segment writes instance e's row to log[e][log_index + k] (covo_run_episode: log_index = 0); NULL = off.
 * Refused before any launch, with a message that names the condition: mask outside [1, 7]; n_inst outside (0, COVO_MAX_ENVS]; a
 * batched step with more instances than n_inst; an episode segment that would leave the log; a sample-sharded step
 * (partial_out != NULL) -- a rank's `a` and `cost` hold its shard only. */
#define COVO_HAS_UPDATE_ARBITER 1
#define COVO_ARB_FLOATS 8
int covo_set_step_arbiter(covo_handle_t h, float *rows, int32_t mask, int32_t n_inst);
int covo_set_episode_arbiter_log(covo_handle_t h, float *log, int32_t stride);

/* Iterations per control step: K sample-rollout-update passes per call (additive to ABI 10: COVO_HAS_STEP_ITERS; off by default,
 * and off changes nothing a caller can observe, graph cache keys included).  A control step with raw key rng_act runs K passes on
 * its one noisy state, trajectory window and parameter set:
 *   pass 0      today's step with key_0 = rng_act: it shifts the mean (MPPI: and a_cov).
 *   pass j >= 1 today's step without the shift -- its starting mean is the mean pass j - 1 committed (after the ESS floor and the
 *               arbiter, where attached), MPPI's a_cov is not shifted again -- with the raw key
 *               key_j = split(split(key_{j-1})[0])[0] (what is left of the previous raw key after a pass has taken act_key and
 *               step_key from it), walked in device memory, and with the gamma_mean blend against its own starting mean.
 * covo-online recomputes Hessian, Sigma and L at every pass's starting mean; covo-offline reuses L_table[clamp(time)]; MPPI with
 * gamma_sigma != 0 adapts a_cov in every pass.  The ESS floor and the update arbiter run in every pass (the arbiter's nominal is
 * the pass's starting mean); a_mean, a_cov, a, cost, the diagnostics, plan, fan, temperature and arbiter rows describe the LAST pass.
 * iter_log = DEVICE float[n_inst][iters]: entry (e, j) is the minimum sample cost of instance e's pass j, stored by that pass's merge.
 * iters = 1 or iter_log = NULL: off.  Every step entry point enqueues the K passes (one captured graph holds all of them; with the
 * arbiter attached the passes are enqueued eagerly around its launch); the episode drivers enqueue K passes, then the env step.
 * Refused with COVO_E_BADARG before any launch: iters outside [1, COVO_MAX_STEP_ITERS]; a sample-sharded step (partial_out != NULL)
 * with iters > 1; derive_keys = 0 with iters > 1; covo_debug_time_* with iters > 1; the env-batched MPPI / covo-offline step with
 * iters > 1 AND the arbiter. */
#define COVO_HAS_STEP_ITERS 1
#define COVO_MAX_STEP_ITERS 16
int covo_set_step_iters(covo_handle_t h, int32_t iters, float *iter_log, int32_t n_inst);

/* The Sigma period: covo-online reuses a shifted Sigma between refreshes (additive to ABI 10: COVO_HAS_SIGMA_PERIOD; off by default,
 * and off changes nothing a caller can observe: every launch is the one made without it).  With period = m the handle keeps an AGE:
 *   age 0            a REFRESH step: exactly the covo-online step (Hessian, Sigma chain, factor); it leaves its factor L on the handle.
 *   age 1 .. m - 1   a REUSE step: no Hessian, no Sigma chain.  With Sigma = L L^T the covariance the previous step sampled from
 *                    (n = 128 = 32 stages of 4 actions), it samples from Sigma' = c S(Sigma):
 *                      S(Sigma)[s][t] = Sigma[s + 1][t + 1] for stages s, t <= 30 (the trailing 124 x 124 block, moved up as the mean is),
 *                      S(Sigma)[31][31] = Sigma[31][31] (the new last stage takes the old last stage's marginal),
 *                      S(Sigma)[31][t] = S(Sigma)[t][31] = 0 for t <= 30,
 *                      c the scalar with log det Sigma' = 2 n log sample_sigma (optimize_sigma's volume constraint).
 *                    Its factor L' is the rank-4 Cholesky update of L[4:, 4:] by the columns of L[4:, 0:4], next to the factor of
 *                    L[124:, :] L[124:, :]^T, scaled by sqrt(c) (sigma_shift.hip); a_cov of the step is Sigma', the actions are
 *                    clip(shifted mean + L' eps) with the in-kernel Philox draw of the step's act key; rollout and update are the
 *                    step's own.  Under iterations per step no pass of a reuse step runs a Hessian or a Sigma chain: all sample from L'.
 * The age advances with every enqueued step (the episode drivers advance it as they enqueue; an env-batched step shares one age) and
 * wraps at m.  A handle without a valid factor -- no step yet, another sample_sigma, another instance count -- refreshes.  A device-side
 * auto-reset of an instance does not force a refresh: its next samples come from a stale but valid covariance.
 * covo_set_step_sigma_period: 1 <= period <= COVO_MAX_SIGMA_PERIOD (1 = off); sets the age to 0.  Refused before any launch, at the
 *   step: a period above 1 on a step whose mode is not covo-online (covo_mpc_step, covo_run_episode, covo_mpc_step_batched_mode,
 *   covo_run_episode_batched_mode); a sample-sharded step (partial_out != NULL).  The refresh step and the reuse step each have their
 *   captured graph.  The phase timers (covo_debug_time_*) replay a refresh step's launches.
 * covo_step_sigma_age: *next_age = the age the next step is scheduled at, *last_age = the age the last enqueued step ran at (either
 *   may be NULL).
 * covo_sigma_shift: the shift alone.  L_in = DEVICE float[batch][128][128] (the lower triangle is read), Sigma_out, L_out = DEVICE
 *   float[batch][128][128], all 16-byte aligned; L_out may be L_in.  L_out's strict upper triangle and Sigma_out's cross block are
 *   exact zeros, Sigma_out is symmetric bit for bit.
 * covo_debug_sigma_factor (test hook): the factor(s) L the last single (batched = 0) or env-batched (batched = 1) covo-online step of
 *   the handle sampled from -- what the next reuse step shifts -- copied to the DEVICE buffer out (count floats, at most 128 * 128 per
 *   instance). */
#define COVO_HAS_SIGMA_PERIOD 1
#define COVO_MAX_SIGMA_PERIOD 64
int covo_set_step_sigma_period(covo_handle_t h, int32_t period);
int covo_step_sigma_age(covo_handle_t h, int32_t *next_age, int32_t *last_age);
int covo_sigma_shift(covo_handle_t h, const float *L_in, int32_t batch, float sample_sigma, float *Sigma_out, float *L_out, void *stream);
int covo_debug_sigma_factor(covo_handle_t h, int32_t batched, float *out, int64_t count, void *stream);

/* The posterior covariance: the weighted 128 x 128 sample covariance of a step's own samples under the step's own weights (additive
 * to ABI 10: COVO_HAS_POST_COV; off by default, and off changes nothing a caller can observe: no launch is added).  Per instance, with
 *   x_i[4 t + d] = a[t][i][d]  the step's clipped samples, the ones its update used,
 *   mu                         the mean the step sampled around (the shifted mean; a later pass of an iterated step: the mean the pass
 *                              before it committed),
 *   w_i                        the weight the step's own update gave sample i -- exp(-(c_i - c_min) / lam), at lam_eff under the ESS
 *                              floor, 1 on the selector's set and 0 elsewhere under the elite-set update -- and 0 for a cost that is
 *                              not finite,
 *   W = sum w_i, y_i = x_i - mu, d = sum w_i y_i / W:      C = sum w_i y_i y_i^T / W - d d^T.
 * C is symmetric bit for bit; mu + d is the softmax mean the step forms at gamma_mean = 1; W = 0 gives C = 0 and d = 0.  For a locally
 * quadratic cost with Hessian H and samples from N(mu, Sigma), C estimates (Sigma^-1 + H / lam)^-1.
 * covo_set_step_post_cov: cov = DEVICE float[n_inst][128][128] (NULL = off), aux = DEVICE float[n_inst][COVO_POST_AUX_FLOATS]:
 *   {d[128], W, 0, 0, 0}.  Every later step of the handle fills row e with instance e's matrix by two eager launches behind the step
 *   and its update arbiter, plan and fan launches (no captured step graph changes); under iterations per step the last pass's.  Refused
 *   before any launch, at the step: a sample-sharded step (partial_out != NULL); the env-batched MPPI / covo-offline step
 *   (covo_mpc_step_batched_mode, covo_run_episode_batched_mode), whose one fused launch keeps the samples in LDS; more instances than
 *   n_inst.
 * covo_weighted_cov: the same two launches on the caller's buffers.  a = DEVICE float[n_inst][H][n_samples][4] (16-byte aligned), cost =
 *   DEVICE float[n_inst][n_samples], mu = DEVICE float[n_inst][128]; elite_K = 0: softmax weights at lam > 0; 1 <= elite_K <= n_samples:
 *   the elite set of covo_elite_select (lam is not read; n_inst <= COVO_MAX_ENVS). */
#define COVO_HAS_POST_COV 1
#define COVO_POST_AUX_FLOATS 132
int covo_set_step_post_cov(covo_handle_t h, float *cov, float *aux, int32_t n_inst);
int covo_weighted_cov(covo_handle_t h, const float *a, const float *cost, const float *mu, int32_t n_samples, int32_t n_inst, float lam,
                      int32_t elite_K, float *cov_out, float *aux_out, void *stream);

/* Sigma adapt: the reuse steps of a Sigma period blend the posterior covariance into the covariance they shift (additive to ABI 10:
 * COVO_HAS_SIGMA_ADAPT; off by default, and off changes nothing a caller can observe: every launch is the one made without it).  With
 * L the factor on the handle the previous step sampled from, Sigma = L L^T, C the posterior covariance the previous step's after-step
 * launches left in the attached covo_set_step_post_cov target, S the shift of the Sigma period and 0 < gamma < 1, a reuse step samples
 * from
 *   Sigma' = c M,   M = (1 - gamma) S(Sigma) + gamma S(C),   c the scalar with log det Sigma' = 2 n log sample_sigma
 * -- S applied to C exactly as to Sigma -- and L' is the lower Cholesky factor of Sigma' (sigma_adapt.hip: M formed in fp64 from the
 * handle's L, never from the caller's a_cov; factored in LDS; L' and Sigma' rounded to fp32 once each).  This is the full-matrix form
 * of MPPI's per-block gamma_sigma blend and of CMA's rank-mu update.  C is used as it stands: it is central about mu + d, the
 * posterior mean at gamma_mean = 1, and no d d^T correction is made for gamma_mean != 1 or for an arbitrated mean.  The lower triangle
 * of C is read, rows and columns 4 .. 127 of it.  W = 0 in the previous step gives C = 0 and hence the plain shift (c absorbs 1 - gamma).
 * Guard: M is positive definite whenever C is positive semidefinite.  If the factorisation of M leaves a pivot that is not finite or
 * not positive, or a log det that is not finite (C not finite, or indefinite), the instance's output is exactly that of gamma = 0,
 * its row records the fallback, and the other instances of the batch are unaffected.  Refresh steps do not adapt.
 * covo_set_step_sigma_adapt: 0 < gamma < 1 and rows_out = DEVICE float[n_inst][COVO_SIGMA_ADAPT_FLOATS] (16-byte aligned), instance
 *   e's {fallback (0 / 1), c, log det M, 0} of every reuse step, {0, 1, 0, 0} after a refresh step; gamma = 0 or rows_out = NULL: off.
 *   Sets the age to 0 and drops the captured step graphs; so does (re-)attaching the covo_set_step_post_cov target while it is on.
 *   Refused before any launch, at the step: no covo_set_step_post_cov target, or fewer instances there or in rows_out than the step
 *   has; a step whose mode is not covo-online; a sample-sharded step; a period of 1.  Under iterations per step the passes j >= 1
 *   sample from the same L', and the next reuse step reads the last pass's C.
 * covo_sigma_adapt: the kernel alone.  L_in, C = DEVICE float[batch][128][128] (the lower triangles are read), 0 <= gamma < 1 (0: C is
 *   not read -- the fallback's own result, the same matrix as covo_sigma_shift's by another route), Sigma_out, L_out = DEVICE
 *   float[batch][128][128], rows_out = DEVICE float[batch][COVO_SIGMA_ADAPT_FLOATS] or NULL, all 16-byte aligned; L_out may be L_in.
 *   L_out's strict upper triangle and Sigma_out's cross block are exact zeros, Sigma_out is symmetric bit for bit. */
#define COVO_HAS_SIGMA_ADAPT 1
#define COVO_SIGMA_ADAPT_FLOATS 4
int covo_set_step_sigma_adapt(covo_handle_t h, float gamma, float *rows_out /* DEVICE float[n_inst][4]; NULL = off */, int32_t n_inst);
int covo_sigma_adapt(covo_handle_t h, const float *L_in, const float *C, int32_t batch, float gamma, float sample_sigma, float *Sigma_out,
                     float *L_out, float *rows_out, void *stream);

/* Episode logs of the rows the step attachments above leave on the handle (additive to ABI 10: COVO_HAS_EPISODE_ROWS; off by
 * default, and off changes nothing a caller can observe: no launch is added).  Every step overwrites its attachments' rows; an episode
 * driver (covo_run_episode, covo_run_episode_batched, covo_run_episode_batched_mode) with one of these logs attached copies the rows of
 * every step it enqueues into the log, bit for bit, by ONE eager launch per step for all attached kinds and instances
 * (csrc/episode_rows.hip), behind the step and its after-step launches and ahead of the env step.  No captured step graph changes.
 *   kind                  row                                  the step attachment it follows
 *   COVO_EPLOG_LAM        float[COVO_LAM_FLOATS]               covo_set_step_ess_floor's solver row
 *   COVO_EPLOG_ELITE      float[COVO_ELITE_FLOATS]             covo_set_step_elite's selector row
 *   COVO_EPLOG_ITERS      float[iters]                         covo_set_step_iters' row (the width is the attached iters)
 *   COVO_EPLOG_SIGMA      float[COVO_SIGMA_LOG_FLOATS]         {age the step ran at (covo_step_sigma_age's last_age, as a float), fallback,
 *                                                              c, log det M}: the last three are covo_set_step_sigma_adapt's row, {0, 1, 0}
 *                                                              without Sigma adapt; needs a Sigma period above 1
 *   COVO_EPLOG_POST_AUX   float[COVO_POST_AUX_FLOATS]          covo_set_step_post_cov's side row
 *   COVO_EPLOG_POST_COV   float[128][128]                      covo_set_step_post_cov's matrix
 * Under iterations per step the rows are the last pass's (the iters row holds every pass).
 * covo_set_episode_rows: log = DEVICE float[n_inst][stride][width]; step k of an episode driver's segment writes instance e's row to
 *   log[e][log_index + k] (covo_run_episode: log_index = 0); NULL = off.  A row is copied with 16-byte accesses when its width is a
 *   multiple of 4 floats and both addresses are 16-byte aligned, else float by float.
 * Refused before any launch, with a message that names the condition: kind outside [0, COVO_EPLOG_KINDS); stride <= 0 with a log; a
 * kind whose step attachment is off (the message names the covo_set_step_* call to make first); an episode segment that would leave
 * the log; a sample-sharded step (partial_out != NULL).  Detaching a step attachment drops its log; so does covo_set_step_iters with
 * another iters. */
#define COVO_HAS_EPISODE_ROWS 1
#define COVO_SIGMA_LOG_FLOATS 4
#define COVO_EPLOG_LAM       0
#define COVO_EPLOG_ELITE     1
#define COVO_EPLOG_ITERS     2
#define COVO_EPLOG_SIGMA     3
#define COVO_EPLOG_POST_AUX  4
#define COVO_EPLOG_POST_COV  5
#define COVO_EPLOG_KINDS     6
int covo_set_episode_rows(covo_handle_t h, int32_t kind, float *log, int32_t stride);
int covo_arbitrate(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                   const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps, const float *a,
                   const float *cost, int32_t N, const float *a_nominal, float *a_mean_inout, int32_t mask, float *row_out,
                   void *stream);

/* The Newton refinement: a gradient-based line search on the mean a covo-online step has just committed (additive to ABI 10:
 * COVO_HAS_NEWTON_REFINE; off by default, and off changes nothing a caller can observe: no launch is added).
 * covo-online samples from Sigma = c (R + delta I)^(-1/2), so (R + delta I)^-1 = Sigma^2 / c^2 and the regularised Newton direction at
 * the committed mean b is d = -Sigma (Sigma g) / c^2 with g the gradient of the Hessian's own objective at b.  The candidates clip(b)
 * and fp32(clip(b + alpha_j d)), alpha_j = 2^(3 - j), j = 1 .. 16, are rolled out with the inputs the step's sample rollouts had
 * (csrc/newton_refine.hip); a NaN cost counts as +inf, equal costs resolve to the lowest candidate, so the mean changes only for a
 * strictly cheaper candidate; g, d or c^2 not finite: the mean stays.
 *   row  float[COVO_REFINE_FLOATS] = {cost_base, cost_chosen, bits(int32 choice), alpha (0 for choice 0), |g|_2, g.d, 0,
 *        bits(int32 flags)}; flags bit 0: g not finite, bit 1: d not finite, bit 2: c^2 not finite or not positive
 * covo_cost_gradient: g_out = DEVICE double[batch][128], the gradient of covo_hessian's objective at a = DEVICE float[batch][128]
 *   (first-order adjoint, fp64, csrc/cost_gradient.hip; the arguments of covo_hessian).  Rows 124 .. 127 are exactly 0.  It uses a
 *   workspace of its own: covo_hessian's results and the step's Hessian are untouched.
 * covo_newton_refine: stateless, n_inst instances with the rollout inputs of covo_arbitrate (state = DEVICE float[n_inst][32],
 *   f_disturb_steps / f_tab_hessian = DEVICE float[n_inst][H][4] or NULL; trajectories, params and f_disturb_shared shared);
 *   g = DEVICE double[n_inst][128] or NULL: computed here at a_mean with f_tab_hessian (covo_cost_gradient's launches);
 *   a_mean = DEVICE float[n_inst][128] in / out; Sigma = DEVICE float[n_inst][128][128], 16-byte aligned; inv_c2 = DEVICE double[n_inst],
 *   1 / c^2; rows_out = DEVICE float[n_inst][COVO_REFINE_FLOATS]; costs_out = DEVICE float[n_inst][COVO_REFINE_CANDIDATES] or NULL.
 * covo_set_step_refine: rows = DEVICE float[n_inst][COVO_REFINE_FLOATS]; every covo-online control step of the handle --
 *   covo_mpc_step, covo_mpc_step_batched, the episode drivers -- then ends with three eager launches behind the update arbiter's
 *   and ahead of the plan's and the fan's: the gradient's two at the committed mean with the step's Hessian table, then the line search
 *   with the step's Sigma and c^2 = sigma^4 det(R + delta I)^(1/n) from the Sigma chain's own log-determinant.  Under iterations per
 *   step every pass runs it and the row is the last pass's.  No captured step graph changes.
 * Refused before any launch, with a message that names the condition: a step that is not covo-online; a Sigma period above 1 (a reuse
 *   step has no R); a sample-sharded step (partial_out != NULL); more instances than rows; a_cov not 16-byte aligned. */
#define COVO_HAS_NEWTON_REFINE 1
#define COVO_REFINE_FLOATS 8
#define COVO_REFINE_CANDIDATES 17
int covo_cost_gradient(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                       const covo_env_params *params, const float *a, const float *f_disturb_steps, int32_t batch, double *g_out,
                       void *stream);
int covo_newton_refine(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                       const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                       const float *f_tab_hessian, const double *g, float *a_mean, const float *Sigma, const double *inv_c2,
                       int32_t n_inst, float *rows_out, float *costs_out, void *stream);
int covo_set_step_refine(covo_handle_t h, float *rows /* DEVICE [n_inst][COVO_REFINE_FLOATS]; NULL = off */, int32_t n_inst);

/* The Riccati refinement: the same line search for every sampling controller (additive to ABI 10: COVO_HAS_RICCATI_REFINE; off by
 * default, and off changes nothing a caller can observe: no launch is added).
 * The Hessian's first two launches leave A_k, B_k, the costate and the exact stage blocks M_k = Hess_z(r_k + lam_{k+1} . f_k) of every
 * stage of the plan.  A backward Riccati sweep over them (csrc/riccati.hip, fp64) is the block elimination of the reduced Hessian R:
 * its forward pass returns d = -(R + mu I)^-1 g with neither R, Sigma nor a 128 x 128 factorisation, next to the time-varying
 * feedback gains K_k, the feed-forward terms k_k and the nominal states x_k (du_k = k_k + K_k dx_k: the ancillary LQR controller along
 * the plan).  mu is the lowest rung of the ladder reg0 4^j, j = 0 .. COVO_RICCATI_RUNGS - 1, at which all 32 pivots Quu_k -- unpivoted
 * 4 x 4 Cholesky factorisations -- are positive, which is exactly where R + mu I is positive definite.
 *   side row  double[COVO_RICCATI_SIDE] = {mu, rung, smallest pivot of that rung, flags}; flags bit 0: g not finite (an entry of a that is not finite counts), bit 1: d
 *             not finite, bit 3: no rung positive definite -- then d = 0, K = 0, k = 0, mu = 0 and rung = COVO_RICCATI_RUNGS
 *   row       float[COVO_RICCATI_FLOATS] = {cost_base, cost_chosen, bits(int32 choice), alpha (0 for choice 0), |g|_2, g.d, mu,
 *             bits(int32 flags | rung << 8)}: a refine row whose last two words say what the sweep did
 * covo_riccati: the stand-alone sweep at a = DEVICE float[batch][128] with the arguments of covo_hessian (f_tab_hessian = DEVICE
 *   float[batch][H][4] or NULL); d_out = DEVICE double[batch][128] (rows 124 .. 127 are 0; a component whose action saturates is 0);
 *   K_out = DEVICE double[batch][H][4][16] (columns at and above the state dimension -- 13, or 16 for drag / mixed -- are 0), kff_out =
 *   DEVICE double[batch][H][4], x_out = DEVICE double[batch][H][16], rows_out = DEVICE double[batch][COVO_RICCATI_SIDE]; each of the
 *   four may be NULL.
 * covo_riccati_refine: stateless, covo_newton_refine without Sigma and c: the Hessian's two launches and the sweep at a_mean, then the
 *   line search of covo_newton_refine with that direction -- the candidates clip(a_mean) and fp32(clip(a_mean + 2^(3 - j) d)),
 *   j = 1 .. 16, rolled out with the inputs of covo_arbitrate, the first cheapest committed to a_mean (16-byte aligned, in / out);
 *   rows_out = DEVICE float[n_inst][COVO_RICCATI_FLOATS], costs_out = DEVICE float[n_inst][COVO_REFINE_CANDIDATES] or NULL.
 * covo_set_step_riccati: rows = DEVICE float[n_inst][COVO_RICCATI_FLOATS]; every control step of the handle -- MPPI, covo-offline and
 *   covo-online, refresh and reuse steps of a Sigma period alike, single and env-batched covo-online, the episode drivers -- then ends
 *   with eager launches behind the update arbiter's and ahead of the plan's and the fan's: the Hessian's first two at the committed
 *   mean (objective: the Hessian's -- no discount, no freeze, its disturbance table from the step's raw key), the sweep with
 *   reg0 = COVO_RICCATI_REG0, the line search.  Under iterations per step every pass runs them and the row is the last pass's.  The
 *   workspace is the refinement's own.  No captured step graph changes.
 * Refused before any launch, with a message that names the condition: a sample-sharded step (partial_out != NULL); the Newton
 *   refinement attached to the same handle; more instances than rows; the env-batched MPPI / covo-offline steps. */
#define COVO_HAS_RICCATI_REFINE 1
#define COVO_RICCATI_FLOATS 8
#define COVO_RICCATI_SIDE 4
#define COVO_RICCATI_RUNGS 8
#define COVO_RICCATI_REG0 1e-2
int covo_riccati(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                 const covo_env_params *params, const float *a, const float *f_tab_hessian, int32_t batch, double reg0, double *d_out,
                 double *K_out, double *kff_out, double *x_out, double *rows_out, void *stream);
int covo_riccati_refine(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                        const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                        const float *f_tab_hessian, float *a_mean, double reg0, int32_t n_inst, float *rows_out, float *costs_out,
                        void *stream);
int covo_set_step_riccati(covo_handle_t h, float *rows /* DEVICE [n_inst][COVO_RICCATI_FLOATS]; NULL = off */, int32_t n_inst);

/* Riccati feedback: closed-loop candidates under the sweep's gains (additive to ABI 10: COVO_HAS_RICCATI_FEEDBACK; off by default, and
 * off changes nothing a caller can observe: no launch, no allocation, no captured graph).
 * The sweep's K_k, k_k and nominal states xb_k are the forward pass of DDP / iLQR once the state deviation is taken from the nonlinear
 * plant instead of from A_k, B_k (csrc/feedback_rollout.hip).  For a step size alpha, from x_0 = the state's (pos, vel, quat, omega)
 * in fp32, k = 0 .. 31:
 *     dx_j = (double)x_k[j] - xb_k[j] (raw coordinates, j = 0 .. 12);  v_i = fma(alpha, k_k[i], (double)b_k[i]), then
 *     v_i = fma(K_k[i][j], dx_j, v_i) with j ascending;  u_k[i] = (float)clip(v_i, -1, 1);  x_{k+1} = the fp32 model step under the
 *     force the sample rollouts apply at step k (the state's own at k = 0, then the shared vector or row k of the step table).
 * K = 0 gives the open-loop candidate fp32(clip(b + alpha k)) bit for bit.  A v_i that is not finite makes the sequence invalid: from
 * that k on it is clip(b), and the line search gives it cost +inf.
 *   aux row       float[4] = {max over k of |K_k dx_k|_inf (the feedback term as it entered the action), bits(int32 number of components
 *                 with |v| > 1), bits(int32 first k with a v that is not finite, -1: none), 0}
 *   feedback row  float[COVO_FEEDBACK_FLOATS] = {cost of the cheapest of candidates 0 .. 16, cost of the cheapest valid closed-loop
 *                 candidate (+inf: none), bits(int32 index of the former), bits(int32 index of the latter, 0: none), that candidate's
 *                 max |K dx|_inf, bits(int32 its clipped count), bits(int32 16-bit mask of invalid closed-loop candidates), 0}
 * With the switch on the line search judges COVO_FEEDBACK_CANDIDATES = 33 sequences: 0 .. 16 as before (bit-identical, costs
 * included), 16 + j the closed-loop sequence at alpha_j = 2^(3 - j), j = 1 .. 16.  The first cheapest wins, so a closed-loop candidate
 * is committed only when strictly cheaper than every open-loop one; choice is 0 .. 32 and alpha is 2^(3 - j) of either family.  When
 * the sweep reports flags there are no candidates beyond 0 and the feedback row is {cost_base, +inf, 0, 0, 0, 0, 0, 0}.
 * covo_feedback_rollout: the generator alone, n_inst instances with the rollout inputs of covo_arbitrate (state = DEVICE
 *   float[n_inst][32] -- the start state need not be xb_0: that is the tube-MPC use; f_disturb_steps = DEVICE float[n_inst][H][4] or
 *   NULL); a = DEVICE float[n_inst][128], 16-byte aligned; K = DEVICE double[n_inst][H][4][16], kff = DEVICE double[n_inst][H][4],
 *   x = DEVICE double[n_inst][H][16] as covo_riccati leaves them; alphas = HOST double[n_alpha], 1 <= n_alpha <= 64;
 *   a_out = DEVICE float[n_inst][n_alpha][128]; aux_out = DEVICE float[n_inst][n_alpha][4].
 * covo_riccati_refine_feedback: covo_riccati_refine with the closed-loop family: the Hessian's two launches, the sweep, the generator,
 *   the line search; costs_out = DEVICE float[n_inst][COVO_FEEDBACK_CANDIDATES] or NULL, fb_rows_out = DEVICE
 *   float[n_inst][COVO_FEEDBACK_FLOATS].
 * covo_set_step_riccati_feedback: fb_rows = DEVICE float[n_inst][COVO_FEEDBACK_FLOATS]; every control step that runs the Riccati
 *   refinement then launches sweep | generator | line search, all eager.  No captured step graph changes.
 * Refused before any launch, with a message that names the condition: attached without covo_set_step_riccati on the handle, or with
 *   more instances than it has; drag / mixed (the 16-state plants: their force is a state of the sweep and a per-sample quantity of
 *   the rollout), in the stand-alone calls and at the step; more instances than rows. */
#define COVO_HAS_RICCATI_FEEDBACK 1
#define COVO_FEEDBACK_FLOATS 8
#define COVO_FEEDBACK_CANDIDATES 33
int covo_feedback_rollout(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                          const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps, const float *a,
                          const double *K, const double *kff, const double *x, const double *alphas /* HOST [n_alpha] */,
                          int32_t n_alpha, int32_t n_inst, float *a_out, float *aux_out, void *stream);
int covo_riccati_refine_feedback(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                                 const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                                 const float *f_tab_hessian, float *a_mean, double reg0, int32_t n_inst, float *rows_out,
                                 float *costs_out, float *fb_rows_out, void *stream);
int covo_set_step_riccati_feedback(covo_handle_t h, float *fb_rows /* DEVICE [n_inst][COVO_FEEDBACK_FLOATS]; NULL = off */,
                                   int32_t n_inst);
/* Test hook: the NEXT covo_riccati_refine_feedback on this handle overwrites entry `index` of instance `inst`'s gains K [H][4][16]
 * with `value` between the sweep and the generator (once) -- how a test hands the line search closed-loop candidates that are not
 * valid. */
int covo_debug_feedback_gain(covo_handle_t h, int32_t inst, int32_t index, double value);

/* Plan hold: replan every m-th control step, track the last plan under the sweep's gains between (additive to ABI 10:
 * COVO_HAS_PLAN_HOLD; a switch on top of covo_set_step_riccati; period 1, the default: off -- no launch, buffer or captured graph
 * differs).  Steps are counted from covo_set_step_plan_hold; the age of a step is (count) mod m, one age for all instances of a batch.
 * Age 0, a plan step: the control step as it is, every graph, attachment and output bit for bit.  Between the sweep and the line
 *   search one launch latches, per instance, the mean b the sweep ran at (the line search overwrites it) and the int32 time word of the
 *   state the step planned from; the sweep leaves K, kff, xb on the handle whether or not covo_set_step_riccati_feedback is on.
 * Age j >= 1, a hold step: no sampling step, no arbiter, refinement or fan launch; ONE launch for all instances (csrc/plan_hold.hip)
 *   computes, on the state the step would have read,
 *     dx_c = (double)x[c] - xb_j[c], c = 0 .. 12;  v0_i = fma(alpha, kff_j[i], (double)b_j[i]);  v_i = v0_i, then
 *     v_i = fma(K_j[i][c], dx_c, v_i) with c ascending;  u_i = (float)clip(v_i, -1, 1)
 *   -- stage j of covo_feedback_rollout's law, with alpha read from the handle's Riccati row (entry 3: 0 for choice 0) -- and then, in
 *   place, what the begin work of a step does: a_mean <- [a_mean[1:], a_mean[31]], MPPI's 32 blocks of a_cov likewise, finally
 *   a_mean[0] <- u.  The plan trace's launch runs behind it with the hold step's own inputs; every other attachment keeps the plan
 *   step's rows, the logs covo_set_episode_rows copies repeat them, logs written by their own launches leave the row unwritten.
 * Decided on the device, reported in the hold row, none an error (flags):
 *   bit 0  the sweep is flagged (its side row: no rung positive definite -- K = kff = 0 then anyway --, g or d not finite): u = clip(b_j)
 *   bit 1  a v_i that is not finite (and bit 0 clear): all four components are clip(b_j)
 *   bit 2  the state's time word differs from the latched one + j (a device auto-reset, an episode end): the feedback term is
 *          dropped, u = (float)clip(v0)
 *   hold row  float[COVO_HOLD_FLOATS] = {bits(int32 j), alpha, max_i |v_i - v0_i| (0 when the feedback term is not applied),
 *             bits(int32 number of components whose applied command exceeds 1 in magnitude), bits(int32 flags), |dx_pos|_2,
 *             bits(int32 the state's time word), 0}; a plan step writes {0, 0, 0, 0, 0, 0, bits(time), 0} from its latch.
 * covo_set_step_plan_hold: rows = DEVICE float[n_inst][COVO_HOLD_FLOATS] (NULL with period 1); the age goes back to 0.
 * covo_step_plan_age: the age the next step is scheduled at and the age the last one ran at (either pointer may be NULL).
 * covo_plan_hold: the hold step alone, stateless, n_inst instances: state = DEVICE float[n_inst][32]; b = DEVICE float[n_inst][128];
 *   K, kff, x as covo_riccati leaves them; side = covo_riccati's rows_out, DEVICE double[n_inst][4], or NULL (not flagged); alpha = DEVICE float, instance e's at alpha[e * alpha_stride]; stage in [0, H);
 *   t_plan = DEVICE int32[n_inst] or NULL (no time check); a_mean = DEVICE float[n_inst][128] or NULL and a_cov = DEVICE
 *   float[n_inst][H][4][4] or NULL, both in/out and 16-byte aligned; u_out = DEVICE float[n_inst][4]; rows_out = DEVICE
 *   float[n_inst][COVO_HOLD_FLOATS].
 * covo_set_episode_hold_log: log = DEVICE float[n_inst][stride][COVO_HOLD_FLOATS] (NULL: off); the hold launch, and the latch on
 *   plan steps, of an episode driver write instance e's row of step `index` to log[e][index] themselves.
 * Refused at the step, before any launch: period > 1 without covo_set_step_riccati; together with a Sigma period; drag / mixed (the
 *   16-state plants); more instances than rows; a_mean / a_mean_in / a_cov not 16-byte aligned; and whatever the Riccati refinement
 *   refuses (the env-batched MPPI / covo-offline steps, sample-sharded steps). */
#define COVO_HAS_PLAN_HOLD 1
#define COVO_HOLD_FLOATS 8
#define COVO_MAX_PLAN_HOLD 16
int covo_set_step_plan_hold(covo_handle_t h, int32_t period, float *rows /* DEVICE [n_inst][COVO_HOLD_FLOATS]; NULL with period 1 */,
                            int32_t n_inst);
int covo_step_plan_age(covo_handle_t h, int32_t *next_age, int32_t *last_age);
int covo_plan_hold(covo_handle_t h, const float *state, const float *b, const double *K, const double *kff, const double *x,
                   const double *side /* DEVICE [n_inst][4] or NULL */, const float *alpha /* DEVICE, one float per instance */, int32_t alpha_stride /* in floats */, int32_t stage,
                   const int32_t *t_plan /* DEVICE int32 per instance, or NULL: no time check */, float *a_mean /* in/out, nullable */,
                   float *a_cov /* in/out, nullable */, float *u_out, float *rows_out, int32_t n_inst, void *stream);
int covo_set_episode_hold_log(covo_handle_t h, float *log, int32_t stride);
/* Test hook: what the LAST plan step of this handle latched for its first n_inst instances, device -> device: b_out = DEVICE
 * float[n_inst][128], t_out = DEVICE int32[n_inst], and the sweep's K_out / kff_out / x_out = DEVICE double[n_inst][H][4][16] /
 * [n_inst][H][4] / [n_inst][H][16] -- what the hold steps that follow apply. */
int covo_debug_plan_latch(covo_handle_t h, int32_t n_inst, float *b_out, int32_t *t_out, double *K_out, double *kff_out, double *x_out,
                          void *stream);

/* The iLQR controller: Riccati sweeps and the closed-loop line search, nothing sampled (additive to ABI 10: COVO_HAS_ILQR; a fourth
 * step mode -- a handle never stepped in it launches, allocates and captures what it always did).  One control step in
 * COVO_MODE_ILQR, through covo_mpc_step / covo_run_episode (covo_step_args.mode) or covo_mpc_step_batched_mode /
 * covo_run_episode_batched_mode (covo_batch_mode_args.mode; the other fields of that struct are ignored), with k = the iteration
 * count of covo_set_step_iters (1 without it):
 *     b_0 = [a_mean[1:], a_mean[31]];   b_{j+1} = the Riccati line search at b_j, j = 0 .. k - 1;   a_mean <- b_k
 *   where an iteration is what covo_set_step_riccati [+ covo_set_step_riccati_feedback] enqueues behind a sampling step, launch for
 *   launch: Hessian blocks -> chains -> sweep -> [latch] -> [closed-loop generator] -> line search over 17 [33] candidates.  All k
 *   iterations see the step's one state, trajectory slices and raw key (derive_keys = 1: the disturbance inputs are derived from it
 *   on the device as a covo-online step derives them); the key is NOT walked between them as the passes of an iterated sampling step
 *   walk it -- the objective does not change inside a step, so row_{j+1}.cost_base == row_j.cost_chosen, and once an iteration commits
 *   choice 0 every later one does too.  a, cost, groupmin, a_cov, L_table, gamma_mean, sample_sigma are not read or written: no noise,
 *   sample rollout, update, Hessian GEMM, Sigma chain or arbiter launch runs.  Eager launches; the plan trace follows the last
 *   iteration.  The handle's Riccati and feedback rows describe the last iteration.
 * Under covo_set_step_plan_hold every m-th step is the step above; the latch, gains, alpha and side row of its LAST iteration are
 *   what the m - 1 hold steps between apply (the hold launch and its fall-backs are the ones of the sampling controllers).
 * covo_set_step_ilqr: the per-iteration logs.  rows = DEVICE float[n_inst][COVO_MAX_STEP_ITERS][COVO_RICCATI_FLOATS], fb_rows = DEVICE
 *   float[n_inst][COVO_MAX_STEP_ITERS][COVO_FEEDBACK_FLOATS] (slot j: iteration j's rows; zeros without the feedback rows), summary =
 *   DEVICE float[n_inst][COVO_ILQR_FLOATS] = {row_0.cost_base, row_{k-1}.cost_chosen, bits(int32 iterations with choice != 0),
 *   bits(int32 first j with choice 0; k: none), bits(int32 iterations with choice > 16), bits(OR of the rows' flag words),
 *   |g|_2 of the last iteration, 0}; any of the three may be NULL, all NULL (n_inst ignored) detaches.  One launch of one wave per
 *   instance behind every iteration's line search (csrc/ilqr.hip) fills them.
 * Refused at the step with COVO_E_BADARG, before any launch: no covo_set_step_riccati on the handle; covo_set_step_refine; an
 *   attached arbiter, sample fan, diagnostics buffer, ESS floor, elite set, posterior covariance, Sigma period or Sigma adapt; a
 *   sample-sharded step (partial_out != NULL); derive_keys = 0; more instances than log rows; and whatever the attachments in use
 *   refuse themselves (feedback rows and plan hold on drag / mixed).  covo_debug_time_step refuses the mode: its phase masks name
 *   sampling launches. */
#define COVO_HAS_ILQR 1
#define COVO_MODE_ILQR 3
#define COVO_ILQR_FLOATS 8
int covo_set_step_ilqr(covo_handle_t h, float *rows /* DEVICE [n_inst][16][8] or NULL */, float *fb_rows /* DEVICE [n_inst][16][8] or NULL */,
                       float *summary /* DEVICE [n_inst][COVO_ILQR_FLOATS] or NULL */, int32_t n_inst);
/* Test hook: the line search of iteration j of every later iLQR step also stores its candidates' costs, as covo_riccati_refine[_feedback]
 * stores them, to costs[e][j][0 .. 17 or 33) -- costs = DEVICE float[n_inst][COVO_MAX_STEP_ITERS][COVO_FEEDBACK_CANDIDATES]; NULL: off.  A
 * batched step then uploads its line search's argument blocks in every iteration. */
int covo_debug_ilqr_costs(covo_handle_t h, float *costs, int32_t n_inst);

/* The Riccati box: control-limited stages of the sweep (additive to ABI 10: COVO_HAS_RICCATI_BOX; off by default, and off means no
 * launch, buffer or kernel changes).  At stage k of rung mu, with bc = clip(b_k, -1, 1), lo = -1 - bc, hi = 1 - bc (an entry of the
 * plan that is not finite: lo = hi = 0), the sweep's 4 x 4 step becomes the box QP of control-limited DDP (Tassa, Mansard, Todorov 2014):
 *     k_k = argmin 1/2 du^T Quu du + Qu^T du   subject to   lo <= du <= hi        (Quu includes mu I)
 *   Coordinate i is clamped when k_k[i] sits on a bound and the multiplier (Quu k_k + Qu)[i] pushes strictly outward; there k_k[i] is
 *   the bound itself and row i of K_k is 0.  On the free set f, K_k[f] = -Quu_ff^-1 Qux_f.  The value recursion is unchanged (it stays
 *   exact with clamped rows of K zero), and so are the ladder's test -- the pivots of the FULL Quu -- the forward pass, d, x, the side
 *   row and the line search.  Every rung runs its own box sweep; a stage whose unconstrained step is feasible keeps it bit for bit.
 *   masks: int32[H] per entry, bits 0-3: coordinate i clamped at lo, bits 4-7: at hi, of the winning rung; zeros when no rung wins.
 * covo_riccati_box: covo_riccati over the box sweep; masks_out = DEVICE int32[batch][H] or NULL.
 * covo_riccati_refine_box: the stateless line search over the box sweep; feedback = 0: covo_riccati_refine's 17 candidates
 *   (fb_rows_out is not read), feedback != 0: covo_riccati_refine_feedback's 33; masks_out = DEVICE int32[n_inst][H] or NULL.
 * covo_set_step_riccati_box: a switch on top of covo_set_step_riccati; masks = DEVICE int32[n_inst][H].  Every sweep a step of the
 *   handle runs is then the box sweep -- the refinement behind an MPPI / covo-offline / covo-online step, every pass under
 *   covo_set_step_iters, the plan steps of covo_set_step_plan_hold, every iteration of an iLQR step, single and batched, steps and
 *   episode drivers alike -- and the masks of the last sweep stay in the buffer.  The 16-state plants (drag / mixed) are allowed: the
 *   box lives in the 4 x 4 part.  Refused before any launch, with a message that names the condition: attached without
 *   covo_set_step_riccati on the handle, or a step with more instances than rows.  A change of the switch drops the captured step
 *   graphs.
 * covo_set_step_ilqr_box: counts = DEVICE int32[n_inst][COVO_MAX_STEP_ITERS]; the tally launch of an iLQR step also files the number
 *   of clamped coordinates of iteration j's sweep in slot j (only while covo_set_step_riccati_box is on); NULL: off. */
#define COVO_HAS_RICCATI_BOX 1
int covo_riccati_box(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                     const covo_env_params *params, const float *a, const float *f_tab_hessian, int32_t batch, double reg0, double *d_out,
                     double *K_out, double *kff_out, double *x_out, double *rows_out, int32_t *masks_out, void *stream);
int covo_riccati_refine_box(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                            const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                            const float *f_tab_hessian, float *a_mean, double reg0, int32_t n_inst, float *rows_out, float *costs_out,
                            float *fb_rows_out, int32_t feedback, int32_t *masks_out, void *stream);
int covo_set_step_riccati_box(covo_handle_t h, int32_t *masks /* DEVICE [n_inst][H]; NULL = off */, int32_t n_inst);
int covo_set_step_ilqr_box(covo_handle_t h, int32_t *counts /* DEVICE [n_inst][COVO_MAX_STEP_ITERS]; NULL = off */, int32_t n_inst);

/* The CMA controller: a full 128 x 128 covariance learned from the samples, with cumulative step-size adaptation (additive to ABI 10:
 * COVO_HAS_CMA; a fifth step mode -- a handle never stepped in it launches, allocates and captures what it always did).  n = 128,
 * sigma0 = sample_sigma, S the Sigma period's shift.  Per instance the handle keeps the factor L the previous step sampled from (fp32,
 * step size included), the evolution path p (fp64 [128], in the caller's path_out) and log s (fp64), s the step size relative to sigma0.
 * A reset leaves L = sigma0 I, p = 0, log s = 0.  The first step after a reset samples from sigma0^2 I, adapts nothing and writes the
 * neutral row {1, 0, 0, 0, 0, 0, 0, 0}.  Every later step, before it samples:
 *   shape   Sigma_hat' = c ((1 - gamma) S(L L^T) + gamma S(C)), log det Sigma_hat' = 2 n log sigma0, L_hat' its factor: covo_sigma_adapt
 *           as it is, on the handle's L and the posterior covariance C the previous step left in the covo_set_step_post_cov target,
 *           into a second buffer; its fall-back (the gamma = 0 result) is kept and reported as flag 4
 *   step size (csrc/cma_path.hip, fp64): z = L^-1 d by forward substitution on the previous factor, d the previous step's mean
 *           displacement (the posterior side row); mu_eff = clamp(ess, 1, N), ess the previous step's diagnostics' ess (K under the
 *           elite set); c_s = (mu_eff + 2) / (n + mu_eff + 5); d_s = damping (1 + 2 max(0, sqrt((mu_eff - 1) / (n + 1)) - 1) + c_s);
 *           p <- (1 - c_s) p + sqrt(c_s (2 - c_s) mu_eff) z;   log s <- clamp(log s + (c_s / d_s) (|p| / chi_n - 1), log s_min, log s_max),
 *           chi_n = sqrt(n) (1 - 1/(4n) + 1/(21 n^2)).  p is not shifted: in whitened coordinates it is treated as isotropic.
 *   scale   L' = fp32(s L_hat') becomes the handle's factor, Sigma' = fp32(s^2 Sigma_hat') the step's a_cov, each rounded once; the
 *           strict upper triangle of L' stays exact zeros, Sigma' symmetric bit for bit
 *   and it samples clip(shift(mu) + L' eps) with the step's own in-kernel Philox draw; rollout, update, after-step and posterior
 *   launches are the existing ones.  Under covo_set_step_iters every pass samples from the step's one L'; the next step reads the last
 *   pass's C, d and ess.
 * Device-side fall-backs of the step size, reported in the row's flag word and never an error: 1 -- p and log s are left as they are
 *   (W is not a positive finite number, ess or an entry of d or z is not finite, or a diagonal entry of L is not positive and finite);
 *   2 -- the clamp was hit; 4 -- the shape kernel fell back.  The state is mended on entry: a log s that is not finite counts as 0 and
 *   is then held inside [log s_min, log s_max], a path with an entry that is not finite counts as 0; so s always lies in
 *   [s_min, s_max], on a fall-back too, and L' is finite whenever L_hat' is.
 * covo_set_step_cma: 0 <= gamma < 1; step_size = 0 keeps s = 1 (the kernel only copies; row and path stay neutral); damping > 0;
 *   0 < s_min <= 1 <= s_max; rows_out = DEVICE float[n_inst][COVO_CMA_FLOATS] = {s, log s, |p|, |z|, mu_eff, c_s, d_s, flags} (16-byte
 *   aligned; after a fall-back of kind 1 the entries |z| .. d_s are 0), path_out = DEVICE double[n_inst][128]: the handle's path lives
 *   there between steps -- read it, do not write it.  rows_out = NULL detaches.  Resets the state and drops the captured step graphs.
 * covo_cma_reset: the next step in COVO_MODE_CMA is a first step.
 * covo_cma_path: the step-size kernel alone on the caller's buffers.  L_prev, L_hat, Sigma_hat, L_out, Sigma_out = DEVICE
 *   float[batch][128][128]; aux = instance e's {d[128], W, ...} at aux + e * aux_stride floats; ess = instance e's at ess + e *
 *   ess_stride floats; shape_rows = covo_sigma_adapt's rows or NULL; p = DEVICE double[batch][128] and log_s = DEVICE double[batch],
 *   in place; rows_out as above.  Matrices and rows 16-byte aligned.  L_out may be L_prev and Sigma_out may be Sigma_hat.  It writes
 *   p and log_s (on a fall-back: their mended entry values), L_out, Sigma_out and rows_out, nothing else, and launches on hip_stream, the
 *   caller's stream (a hipStream_t as void *, like every other entry's `stream`).
 * COVO_MODE_CMA goes through covo_mpc_step and covo_run_episode.  Refused at the step with COVO_E_BADARG, before any launch: no
 *   covo_set_step_cma on the handle; no covo_set_step_post_cov or covo_set_step_diag target; a sample-sharded step; a Sigma period
 *   above 1; Sigma adapt or Sigma in node space attached; a_cov NULL or not 16-byte aligned; more instances than rows.
 * covo_debug_time_step refuses the mode, covo_debug_time_batched refuses while the batch's last step was one: a replayed copy would adapt.
 * The mode's number is 5: 4 stays an invalid mode. */
#define COVO_HAS_CMA 1
#define COVO_MODE_CMA 5
#define COVO_CMA_FLOATS 8
int covo_set_step_cma(covo_handle_t h, float gamma, int32_t step_size, float damping, float s_min, float s_max,
                      float *rows_out /* DEVICE [n_inst][COVO_CMA_FLOATS]; NULL = off */, double *path_out /* DEVICE [n_inst][128] */,
                      int32_t n_inst);
int covo_cma_reset(covo_handle_t h);
int covo_cma_path(covo_handle_t h, const float *L_prev, const float *aux, int32_t aux_stride, const float *ess, int32_t ess_stride,
                  const float *L_hat, const float *Sigma_hat, const float *shape_rows, int32_t batch, int32_t n_samples, int32_t step_size,
                  float damping, float s_min, float s_max, double *p, double *log_s, float *L_out, float *Sigma_out, float *rows_out,
                  void *hip_stream);
/* The state estimator: an extended Kalman filter between the env step and the control step (additive to ABI 10:
 * COVO_HAS_STATE_ESTIMATOR; csrc/state_estimator.hip).  One launch overwrites, IN PLACE, the 13 kinematic floats of the
 * packed state row the controller is about to read; no step path and no captured step graph changes; off unless attached.  fp64
 * throughout.  Per instance the filter keeps x [13] (pos, vel, quat, omega), P [13][13] (symmetric bit for bit), the force f_prev and
 * the time word t_prev of the row it last saw, and a valid bit, in the caller's buffers:
 *   xhat = DEVICE double[n_inst][COVO_EST_STATE_DOUBLES] (x, then f_prev), P = DEVICE double[n_inst][13][13],
 *   meta = DEVICE int32[n_inst][COVO_EST_META_INTS] = {valid, t_prev}, rows = DEVICE float[n_inst][COVO_EST_FLOATS].
 * R = diag(obs_std[group]^2), Q = diag(proc_std[group]^2), groups pos, vel, quat, omega; a NEGATIVE proc_std[1] means
 * dt force_std / m with the instance's own dt and m.  A call with the measured row z and the applied action u [4]:
 *   no valid state, or time(z) != t_prev + 1: x = (double)z[0:13], P = R, the row is left as measured; otherwise
 *   x- = f(x, clip(u), f_prev) (the model step of the rollouts in fp64, quaternion normalised on entry and exit), A = df/dx at x,
 *   P- = A P A^T + Q;  S = P- + R factored without pivoting, nu = z - x-, K = P- S^-1, x = x- + K nu,
 *   P = (I - K) P- (I - K)^T + K R K^T with the lower triangle mirrored;  row[0:13] = fp32(x), nothing else of the row changes;
 *   f_prev = z.f_disturb, t_prev = time(z).  The quaternion is neither renormalised nor sign-aligned.
 * Fall-backs, decided on the device, reported in the row's flag word, never an error: 1 -- initialised (no valid state); 2 --
 *   re-initialised (the time word); 4 -- one of the 13 measured coordinates is not finite: the row is untouched and the filter is
 *   invalidated; 8 -- a pivot of S is not positive and finite, or x / P has an entry that is not finite: re-initialised from z, the row
 *   untouched.
 * rows: {bits(flags), nu^T S^-1 nu, |nu_pos|, |x - z|_pos, P00 + P11 + P22, P33 + P44 + P55, smallest pivot of S, bits(time(z))}.
 * covo_set_step_estimator: covo_run_episode, covo_run_episode_batched and covo_run_episode_batched_mode enqueue the launch right behind
 *   their env step, whatever kind of step came before (a hold step included), on args->state[s] with u = the first four floats of
 *   each instance's a_mean.  rows = NULL detaches (the episode log with it).  obs_std, proc_std: [host] double[4].
 * covo_estimator_reset: the next launch of a driver treats every instance as one without a valid state.
 * covo_estimate: the launch alone on the caller's buffers: state_rows = DEVICE float[n_inst][32], in place; instance e's u at
 *   u + e * u_stride floats; params = [host] covo_env_params[n_inst]; reset > 0: every instance counts as one without a valid state;
 *   reset < 0: they do when covo_estimator_reset was called on the handle since its last launch (the flag is taken).
 *   It writes floats 0 .. 12 of each row, xhat, P, meta and rows, nothing else, and launches on hip_stream, the caller's stream (a
 *   hipStream_t as void *, like every other entry's `stream`).
 * covo_set_episode_estimator_log: log = DEVICE float[n_inst][stride][COVO_EST_LOG_FLOATS]; the launch of a driver's step t writes row
 *   first_row + t of every instance itself: the 13 measured floats, the 13 written floats, the row.  NULL: off.
 * Refused with COVO_E_BADARG before any launch: an obs_std entry that is not positive and finite; a proc_std entry that is negative
 *   (other than the marker) or not finite; force_std negative or not finite while the marker is set; more instances than rows;
 *   a sample-sharded episode step; a log with fewer rows than the episode segment needs; covo_set_step_estimator while a force
 *   observer (COVO_HAS_FORCE_OBSERVER, below) is attached to the handle: two filters must not write one row. */
#define COVO_HAS_STATE_ESTIMATOR 1
#define COVO_EST_FLOATS 8
#define COVO_EST_STATE_DOUBLES 16
#define COVO_EST_META_INTS 2
#define COVO_EST_LOG_FLOATS 34
int covo_set_step_estimator(covo_handle_t h, const double *obs_std, const double *proc_std, double force_std, double *xhat, double *P,
                            int32_t *meta, float *rows /* DEVICE [n_inst][COVO_EST_FLOATS]; NULL = off */, int32_t n_inst);
int covo_estimator_reset(covo_handle_t h);
int covo_estimate(covo_handle_t h, float *state_rows, const float *u, int32_t u_stride, const covo_env_params *params,
                  const double *obs_std, const double *proc_std, double force_std, double *xhat, double *P, int32_t *meta, float *rows,
                  int32_t n_inst, int32_t reset, void *hip_stream);
int covo_set_episode_estimator_log(covo_handle_t h, float *log, int32_t stride);
/* The force observer: a 16-state extended Kalman filter that estimates the disturbance force (additive to ABI 10:
 * COVO_HAS_FORCE_OBSERVER; csrc/force_observer.hip).  A second, independent filter launch next to the state
 * estimator's: it treats f_disturb as unknown, estimates it from the kinematic measurements alone and overwrites, IN PLACE, floats
 * 0 .. 15 of the packed state row the controller is about to read (the 13 kinematic floats and the three force slots).  The row's
 * force slots are never an input.  No step path and no captured step graph changes; off unless attached.  fp64 throughout.  Per
 * instance the filter keeps xi = (x [13], f [3]), P [16][16] (symmetric bit for bit), the time word t_prev of the row it last saw and
 * a valid bit, in the caller's buffers:
 *   xi = DEVICE double[n_inst][COVO_OBS_STATE_DOUBLES], P = DEVICE double[n_inst][16][16],
 *   meta = DEVICE int32[n_inst][COVO_OBS_META_INTS] = {valid, t_prev}, rows = DEVICE float[n_inst][COVO_OBS_FLOATS].
 * R = diag(obs_std[group]^2) over pos, vel, quat, omega; Q = diag(proc_std[group]^2 (13), force_walk_std^2 (3)).  A call with the
 * measured row z and the applied action u [4]:
 *   no valid state, or time(z) != t_prev + 1: x = (double)z[0:13], f = 0, P = diag(R, force_init_std^2 I3); row[13:16] = 0, row[0:13]
 *   is left as measured; otherwise
 *   x- = model(x, clip(u), f) (the model step of the rollouts in fp64, quaternion normalised on entry and exit), f- = f,
 *   A16 = d(x-, f-)/d(x, f) at xi, P- = A16 P A16^T + Q;  H = [I13 0], S = P-[0:13, 0:13] + R factored without pivoting, nu = z - x-,
 *   K = P-[:, 0:13] S^-1 (16 x 13), xi = xi- + K nu, P = (I - K H) P- (I - K H)^T + K R K^T with the lower triangle mirrored;
 *   row[0:16] = fp32(xi), nothing else of the row changes;  t_prev = time(z).  The quaternion is neither renormalised nor sign-aligned.
 * Fall-backs, decided on the device, reported in the row's flag word, never an error: 1 -- initialised (no valid state); 2 --
 *   re-initialised (the time word); 4 -- one of the 13 measured coordinates is not finite: the row is untouched and the filter is
 *   invalidated; 8 -- a pivot of S is not positive and finite, or xi / P has an entry that is not finite: re-initialised from z,
 *   row[0:13] untouched, the force slots 0.
 * rows: {bits(flags), nu^T S^-1 nu, |nu_pos|, |f^|, P00 + P11 + P22, P13,13 + P14,14 + P15,15, smallest pivot of S, bits(time(z))}.
 * covo_set_step_force_observer: covo_run_episode, covo_run_episode_batched and covo_run_episode_batched_mode enqueue the launch right
 *   behind their env step, whatever kind of step came before (a hold step included), on args->state[s] with u = the first four floats
 *   of each instance's a_mean.  rows = NULL detaches (the episode log with it).  obs_std, proc_std: [host] double[4].
 * covo_force_observer_reset: the next launch of a driver treats every instance as one without a valid state.
 * covo_observe_force: the launch alone on the caller's buffers: state_rows = DEVICE float[n_inst][32], in place; instance e's u at
 *   u + e * u_stride floats; params = [host] covo_env_params[n_inst]; reset > 0: every instance counts as one without a valid state;
 *   reset < 0: they do when covo_force_observer_reset was called on the handle since its last launch (the flag is taken).
 *   It writes floats 0 .. 15 of each row, xi, P, meta and rows, nothing else, and launches on hip_stream, the caller's stream (a
 *   hipStream_t as void *, like every other entry's `stream`).
 * covo_set_episode_force_observer_log: log = DEVICE float[n_inst][stride][COVO_OBS_LOG_FLOATS]; the launch of a driver's step t writes
 *   row first_row + t of every instance itself: the 16 measured floats (slots 13 .. 15: the TRUE force, as the env step left it), the
 *   16 floats the row holds behind the launch, the side row.  NULL: off.
 * Refused with COVO_E_BADARG before any launch: an obs_std entry that is not positive and finite; a proc_std entry, force_walk_std or
 *   force_init_std that is negative or not finite; more instances than rows; a sample-sharded episode step; a log with fewer rows than
 *   the episode segment needs; a state estimator attached to the same handle (and covo_set_step_estimator while an observer is
 *   attached): two filters must not write one row. */
#define COVO_HAS_FORCE_OBSERVER 1
#define COVO_OBS_FLOATS 8
#define COVO_OBS_STATE_DOUBLES 16
#define COVO_OBS_META_INTS 2
#define COVO_OBS_LOG_FLOATS 40
int covo_set_step_force_observer(covo_handle_t h, const double *obs_std, const double *proc_std, double force_walk_std,
                                 double force_init_std, double *xi, double *P, int32_t *meta,
                                 float *rows /* DEVICE [n_inst][COVO_OBS_FLOATS]; NULL = off */, int32_t n_inst);
int covo_force_observer_reset(covo_handle_t h);
int covo_observe_force(covo_handle_t h, float *state_rows, const float *u, int32_t u_stride, const covo_env_params *params,
                       const double *obs_std, const double *proc_std, double force_walk_std, double force_init_std, double *xi, double *P,
                       int32_t *meta, float *rows, int32_t n_inst, int32_t reset, void *hip_stream);
int covo_set_episode_force_observer_log(covo_handle_t h, float *log, int32_t stride);
/* Test hook: `count` doubles at `offset_doubles` of the Hessians of the LAST covo_mpc_step_batched on this handle
 * ([n_envs][128][128], the Sigma chain's input), copied to the HOST buffer `out` (asynchronously on `stream`). */
int covo_debug_batched_hessians(covo_handle_t h, double *out, int64_t offset_doubles, int64_t count, void *stream);

/* Profiling aid: covo_sigma for ONE matrix that also stores shader-clock ticks (s_memtime) at the kernel's
 * phase boundaries into ticks_out (device uint64[32]): [0] start, [1] loaded+shifted, [2+i] end of sweep i,
 * [20] sweeps done, [21] spectrum map, [22] H H^T, [23] Cholesky, [24] number of sweeps. */
int covo_sigma_profile(covo_handle_t h, const double *R, float sample_sigma, float *Sigma_out, float *L_out,
                       uint64_t *ticks_out, void *stream);

/* Everything one controller __call__ does between "shift the mean" and "new mean", for this handle's shard
 * of samples, in ONE call (controllers/covo.py:201-275, mppi.py:43-125):
 *   shift mean -> [online: Hessian -> optimal Sigma -> Cholesky | offline: L_table[state.time] | mppi: shift
 *   a_cov, factor the 4x4 blocks] -> in-kernel Philox draw + noise GEMM -> fused rollout -> softmax reduction
 *   -> (partial_out == NULL) new mean written back to a_mean, or (partial_out != NULL) this shard's record.
 * All pointers are device pointers that must stay valid and UNCHANGED from call to call for the sequence to be
 * captured into a hipGraph (second identical call) and replayed (later calls); changing any of them or
 * `params` falls back to eager launches and re-captures.  key0/key1, f_disturb_shared and `state` may change freely. */
typedef struct covo_step_args {
    int32_t mode;            /* COVO_MODE_* */
    int32_t n_samples;       /* <= n_local */
    int32_t T;               /* rows of pos_traj / vel_traj */
    int32_t n_table;         /* offline: rows of L_table */
    const float *state;      /* float[32], the noisy state (controllers/covo.py:198).  Must stay valid and unchanged until the step
                              * has run: eager covo-online steps read it where it lies from EVERY launch (the begin work rides in the
                              * Hessian's first launch, covo_debug_set_fold_begin); other steps copy it in their begin launch */
    const float *pos_traj;
    const float *vel_traj;
    float *a_mean;           /* float[128] in/out */
    float *a_mean_shift;     /* nullable: float[128] receives the shifted old mean (needed by covo_merge's blend) */
    float *a_cov;            /* online: float[128][128] Sigma out (nullable); mppi: float[H][4][4] in/out (shifted) */
    const float *L_table;    /* offline: float[n_table][128][128] lower Cholesky factors of a_cov_offline */
    float *a;                /* work: float[H][n_samples][4] */
    float *cost;             /* work: float[n_samples] */
    float *groupmin;         /* work: float[ceil(n_samples/64)]; scratch of the staged rollout -- a step may leave it unwritten (the
                              *    fused launches and the record-emitting rollout keep the minima in their records) */
    double *pos_stats;       /* nullable, as in covo_rollout_cost */
    float *partial_out;      /* nullable: this shard's record instead of finishing locally -- float[COVO_PARTIAL_FLOATS], or, MPPI with
                              *    gamma_sigma != 0, float[COVO_PARTIAL_FLOATS + COVO_COV_FLOATS] (with the second moments) */
    int64_t sample_offset;   /* global id of this shard's first sample */
    float gamma_mean;
    float sample_sigma;
    int32_t derive_keys;     /* 1: key0/key1 are the controller's raw rng_act; the sampling key (covo.py:212, mppi.py:53), the
                              *    rollouts' step key (covo.py:225, mppi.py:69) and everything drawn from it -- MPPI's shared
                              *    gaussian vector, the uniform draws of PERIODIC / MIXED, get_hessian's per-step keys
                              *    (covo.py:150-153, keyed by the raw rng_act) -- are derived on the device exactly as the Python
                              *    host does (random.py); f_disturb_shared is ignored.
                              * 0: key0/key1 = the sampling key; f_disturb_shared as given; PERIODIC / SIN / DRAG / MIXED need
                              *    derive_keys = 1 */
    int32_t rollout_deterministic; /* step_env's `deterministic` in the sampling rollouts: 1 for CoVO (covo.py:231), 0 for MPPI
                              *    (mppi.py:74): switches the GAUSSIAN model off (quadrotor.py:234-235) */
    float gamma_sigma;       /* MPPI: != 0 adapts a_cov in place after the mean update (mppi.py:119-125, covo_softmax_update_cov);
                              *    single shard */
    int32_t pad_;
    const float *a_mean_in;  /* nullable: the control_params.a_mean INPUT of this call when it does not live in `a_mean` (float[128],
                              *    read by the step's first launch only; covo.py:201 reads control_params.a_mean, :275 returns a new
                              *    one).  NULL: `a_mean` is read and then overwritten (a controller that carries its own mean).  Like
                              *    `state` it may change from call to call without invalidating the captured graph.  Must be NULL
                              *    for covo_run_episode (the episode carries the mean). */
} covo_step_args;

int covo_mpc_step(covo_handle_t h, const covo_env_params *params, const covo_step_args *args, uint32_t key0,
                  uint32_t key1, const float *f_disturb_shared /* [host float[3]] or NULL */, void *stream);

/* covo-online for n_envs INDEPENDENT env instances in one call / one hipGraph (BASELINE configs[4]; "replicas only": no
 * exchange between instances).  Every instance has its own noisy state, reference trajectory (T rows), parameters
 * (domain randomisation), mean and key; the Hessians and the Sigma chain of all instances run as ONE batched set of
 * launches, the sampling path (noise GEMM, rollout, softmax update) per instance.  Results per instance are bit-identical
 * to covo_mpc_step on that instance alone.  params: host array [n_envs]; keys: host uint32[n_envs][2], each the raw
 * rng_act of that instance's controller call (the sampling key is derived on the device, covo.py:212).  All instances
 * share reward_kind, rollover_terminate and disturb_kind (one kernel variant per launch); every disturbance model is
 * taken -- for PERIODIC / SIN / DRAG / MIXED the call builds each instance's per-step tables (covo_disturb_table's, SHARED
 * and HESSIAN key threading) from that instance's state, raw key and disturb_params inside the same graph. */
#define COVO_MAX_ENVS 64
typedef struct covo_batch_args {
    int32_t n_envs;          /* <= COVO_MAX_ENVS */
    int32_t n_samples;       /* per instance, <= n_local */
    int32_t T;               /* rows of every instance's pos_traj / vel_traj */
    int32_t pad_;
    const float *states;     /* float[n_envs][32] noisy states */
    const float *pos_traj;   /* float[n_envs][T][3] */
    const float *vel_traj;   /* float[n_envs][T][3] */
    float *a_mean;           /* float[n_envs][128] in/out */
    float *a_cov;            /* float[n_envs][128][128] Sigma out (nullable) */
    float *a;                /* work: float[n_envs][H][n_samples][4] */
    float *cost;             /* work: float[n_envs][n_samples] */
    float *groupmin;         /* work: float[n_envs][ceil(n_samples/64)]; scratch, as in covo_step_args: a step may leave it unwritten */
    float gamma_mean;
    float sample_sigma;
} covo_batch_args;

int covo_mpc_step_batched(covo_handle_t h, const covo_batch_args *args, const covo_env_params *params,
                          const uint32_t *keys, void *stream);

/* The env-batched step with a MODE: MPPI and covo-offline for n_envs independent instances next to covo-online, so that the three
 * controllers can be compared on the same instances (mppi.py:43-125, covo.py:201-278 per instance).
 * ABI choice: NEW entry points with an argument struct of their own.  covo_batch_args is unchanged, and a zeroed `pad_` in it
 * keeps meaning covo-online through covo_mpc_step_batched / covo_run_episode_batched (COVO_MODE_MPPI is 0: `pad_` could not
 * have become the mode).  Here `mode` is explicit:
 *   COVO_MODE_COVO_ONLINE   exactly covo_mpc_step_batched(h, &args->base, ...): the other fields are ignored.
 *   COVO_MODE_MPPI          base.a_cov = float[n_envs][H][4][4], in/out, shifted in place every step (mppi.py:43-49); the rollouts
 *                           are non-deterministic (mppi.py:74): under COVO_DISTURB_GAUSSIAN every instance draws its one shared
 *                           vector from its own key.  gamma_sigma must be 0.
 *   COVO_MODE_COVO_OFFLINE  L_table = instance e's float[n_table][128][128] lower factors at L_table + e * L_table_stride
 *                           (stride in floats; 0: all instances share one table), row clamp(state[e].time) per step (covo.py:107);
 *                           deterministic rollouts (covo.py:231).  base.a_cov is not touched.
 * MPPI and covo-offline run as ONE fused launch for all instances (csrc/step_small.hip with the instance as a grid dimension)
 * behind the key upload -- two launches per batched step, the fused one replayed from a hipGraph; instance e's new mean, action
 * buffer, costs (and MPPI's covariances) are bit-identical to covo_mpc_step on instance e alone.  base.groupmin is not used by
 * them (may be NULL).  Unless covo_set_step_batched_staged (below) is on there is no staged fallback: what the fused launch does
 * not take is refused before anything is launched, with a message that names the condition -- for every instance: reward_kind =
 * COVO_REWARD_PENYAW, disturb_kind NONE or GAUSSIAN, gamma_sigma == 0, n_samples <= 16 384 (256 groups of 64); all instances share
 * reward_kind, rollover_terminate and disturb_kind.
 * covo_debug_time_batched is refused after a step in these two modes (it replays covo-online's launch groups only; time the
 * fused launch with events around covo_mpc_step_batched_mode).
 * covo_run_episode_batched_mode = covo_run_episode_batched with the batched step in the chosen mode (same key threading, same
 * env step: it needs only a_mean[e][0..3]). */
typedef struct covo_batch_mode_args {
    covo_batch_args base;
    int32_t mode;            /* COVO_MODE_* */
    int32_t n_table;         /* offline: rows of every instance's L_table */
    const float *L_table;    /* offline: see above */
    int64_t L_table_stride;  /* offline: floats between consecutive instances' tables; 0 = one shared table */
    float gamma_sigma;       /* MPPI: must be 0 (the fused launch has no covariance adaptation) unless covo_set_step_batched_staged */
    int32_t pad_;
} covo_batch_mode_args;

int covo_mpc_step_batched_mode(covo_handle_t h, const covo_batch_mode_args *args, const covo_env_params *params,
                               const uint32_t *keys, void *stream);

/* The staged env-batched MPPI / covo-offline step (additive to ABI 10: COVO_HAS_BATCHED_STAGED; off by default, and off changes
 * nothing a caller can observe).  on != 0: covo_mpc_step_batched_mode and covo_run_episode_batched_mode run these two modes as the
 * launch sequence of a single staged step with the instance as a grid dimension -- per pass: begin | per-step disturbance tables |
 * sampling | rollout | update, one linear stream of launches behind the key upload, captured into a hipGraph on the second identical
 * call -- ALSO for a configuration the fused launch would take: one switch, one behaviour.  Instance e's new mean, action buffer,
 * costs, MPPI covariances and attachment rows are bit-identical to covo_mpc_step on instance e alone (and so, where the fused launch
 * applies, to the fused batched step) while the batched and the single rollout choose the same workgroup shape: n_envs *
 * ceil(n_samples / 64) < 1024, as for covo_mpc_step_batched; above, the update's sums are formed over other record boundaries and
 * agree to fp32 rounding.  It takes what the fused launch refuses: disturb_kind PERIODIC / SIN / DRAG / MIXED, the
 * realworld reward, MPPI's gamma_sigma != 0 (covo_batch_mode_args.gamma_sigma; a_cov[e] adapted in place, mppi.py:119-125),
 * n_samples up to the handle's n_local, the ESS floor, the elite-set update, the posterior covariance, and iterations per step
 * together with the update arbiter.  Its own refusals (COVO_E_BADARG before any launch, the message names the condition):
 * base.groupmin == NULL (the update reads the per-wave minima); gamma_sigma != 0 outside COVO_MODE_MPPI; gamma_sigma != 0 together
 * with the ESS floor or the elite-set update (those two covariance updates have no instance dimension); a sample-sharded handle;
 * instances that differ in reward_kind / rollover_terminate / disturb_kind, as for covo_mpc_step_batched.  covo_debug_time_batched
 * stays refused after such a step.  Changing the switch drops the handle's captured step graphs.  COVO_MODE_COVO_ONLINE ignores it. */
#define COVO_HAS_BATCHED_STAGED 1
int covo_set_step_batched_staged(covo_handle_t h, int32_t on);

/* Lower Cholesky factors of `batch` symmetric PD n x n fp32 matrices (1 <= n <= 128, row-major, densely packed), the
 * factorisation inside jax.random.multivariate_normal (covo.py:216, mppi.py:59).
 *  - The input is symmetrised as (A + A^T)/2 in fp64, so BOTH triangles of A are read; the factorisation runs in fp64 and
 *    is rounded once to fp32.  L_out receives the full n x n matrix: the factor in the lower triangle, +0.0f above it.
 *  - A and L_out must not alias (nor overlap between matrices of the batch); A is not written.
 *  - An input that is not positive definite is NOT detected: the status is 0 and non-finite entries appear from the failing
 *    pivot's column on, in that matrix only; the columns before it and the other matrices of the batch are unaffected.
 *  - n outside [1, 128], batch <= 0 or a null pointer: refused with a non-zero status, nothing is launched.
 * Pinned for every n and dispatch path by tests/test_gpu_cholesky.py against LAPACK on the same symmetrised fp64 image, rounded
 * to fp32: every entry within one fp32 ulp (plus a floor of 3.2e-12 max|L|), >= 99.9 % of the entries bit-identical (measured
 * on the MI355X: 2 790 700 entries of 2 004 matrices, one of them 1 ulp off, all others bit-identical). */
int covo_cholesky(covo_handle_t h, const float *A, int32_t n, int32_t batch, float *L_out, void *stream);

/* One closed-loop ENVIRONMENT step on the device: Quad3D.step_env + get_info for the controllers'
 * eval loop (envs/quadrotor.py:215-263, 314-361; dynamics/free.py:66-72, 114-202).  `state` (float[32], layout above) is
 * the true state, advanced in place; `noisy_state` receives the noisy copy of the NEW state (the controller's input);
 * `action` = float[4] on the device (the controller's u); `step_key` = uint32[2] on the HOST: the key Quad3D.step
 * receives -- the kernel derives the (disturbance, pos, vel, quat, omega) noise keys from it like the Python env; log (nullable) float[..][4] gets
 * {reward, err_pos, err_vel, done} of the PRE-step state at row log_index.  acc_traj: float[T][3].  Reward and disturbance
 * model (all six of free.py:9-72, the next step's force from the PRE-step state) follow params->reward_kind / disturb_kind.
 * AUTO-RESET (BaseEnvironment.step, quadjax/envs/base.py:22-40; params->reset_traj != COVO_TRAJ_NONE): when the PRE-step state is
 * terminal (quadrotor.py:479-490) the kernel stores what reset_env(key_reset) gives instead of the stepped state -- key_reset =
 * split(step_key)[1]; a NEW reference trajectory from params->reset_traj's generator written over pos_traj / vel_traj / acc_traj
 * (which are therefore written to, despite the const: T must be that generator's row count), the zero state with
 * f_disturb ~ U(-reset_disturb_scale, reset_disturb_scale), time 0, targets = row 0, and the noisy copy from reset_env's own
 * info key -- and the log row carries {reward of the pre-step state, err_pos, err_vel of the RESET state, 1}, which is what
 * eval_env records after env.step (quadrotor.py:531-538).  The controller's state carries on, as in the reference. */
int covo_env_step(covo_handle_t h, float *state, float *noisy_state, const float *pos_traj, const float *vel_traj,
                  const float *acc_traj, int32_t T, const covo_env_params *params, const float *action,
                  const uint32_t *step_key, int32_t noisy_on, float obs_noise_scale, float *log, int32_t log_index,
                  void *stream);

/* covo-offline's nominal trajectory (controllers/covo.py:58-99 with the PID law of controllers/pid.py:38-84 and the
 * expansion gains of covo.py:48-53): from `state0` (float[32], true reset state) `n_steps` PID-tracked,
 * NON-deterministic env steps (keys split from key0/key1 as the Python loop does) give states_out float[n_steps][32];
 * from each of them H deterministic PID steps give the nominal means a_means_out float[n_steps][128] -- the inputs of
 * the batched covo_hessian / covo_sigma that build the per-episode Sigma table.  `pid_params`: the parameters the PID
 * law uses (pid.py:33: the env's DEFAULT m, g, max_thrust, max_omega even under domain randomisation).  All disturbance
 * models of params->disturb_kind act in both loops (the nominal one is deterministic=True: GAUSSIAN off).
 * keys_out [DEVICE uint32[n_steps][2], nullable]: the scan's carry key at every start state = the key get_hessian receives
 * for that row (covo.py:77) -> covo_disturb_table(keys_dev = keys_out, COVO_DISTURB_KEYS_HESSIAN). */
int covo_pid_nominal(covo_handle_t h, const float *state0, const float *pos_traj, const float *vel_traj,
                     const float *acc_traj, int32_t T, const covo_env_params *params, const covo_env_params *pid_params,
                     float Kp, float Kd, float Kp_att, uint32_t key0, uint32_t key1, int32_t n_steps,
                     float *states_out, float *a_means_out, uint32_t *keys_out, void *stream);

/* A whole closed-loop episode segment with no host work between the steps (the reference traces
 * eval_env's run_one_step into one XLA program, envs/quadrotor.py:506-591): n_steps x { covo_mpc_step on the noisy state
 * -> covo_env_step with u = a_mean[0] }, keys threaded as run_one_step does (rng, rng_act, rng_step, _ = split(rng, 4);
 * rng, _ = split(rng)).  `args` as for covo_mpc_step with derive_keys = 1, partial_out = NULL and args->state = the
 * NOISY state buffer (float[32], rewritten by every env step); state_true float[32]; rng uint32[2] in/out (host);
 * log float[n_steps][4] (nullable).  Asynchronous: returns after enqueueing; one sync at the end of the episode. */
int covo_run_episode(covo_handle_t h, const covo_env_params *params, const covo_step_args *args, float *state_true,
                     const float *acc_traj, int32_t noisy_on, float obs_noise_scale, float *log, uint32_t *rng,
                     int32_t n_steps, void *stream);

/* BASELINE configs[4] end to end: the env step and the episode driver for n_envs INDEPENDENT, domain-randomised env instances
 * (quadrotor.py:132-171 samples each instance's parameters; :506-591 is the per-instance eval loop, which the reference reaches
 * through jax.vmap).  covo_env_step_batched = covo_env_step for every instance in ONE launch (workgroup e = instance e: its own
 * true state states[e], noisy copy noisy[e], trajectories [e][T][3], action a_mean[e][0..3], parameters params[e], key
 * step_keys[e]; log float[n_envs][log_stride][4], nullable); instance e's step is bit-identical to covo_env_step on it alone.
 * All instances share reward_kind, rollover_terminate, max_steps_in_episode and disturb_kind (as in covo_mpc_step_batched).
 * covo_run_episode_batched = n_steps x { covo_mpc_step_batched on the noisy states -> covo_env_step_batched }, every instance's
 * key chain threaded like run_one_step (rngs: host uint32[n_envs][2], in/out); args->states = the noisy states (rewritten by
 * every env step).  Asynchronous; one host sync per episode segment.  "Replicas only": instances shard over ranks with no
 * collective (bench.py --config envs). */
int covo_env_step_batched(covo_handle_t h, int32_t n_envs, float *states, float *noisy_states, const float *pos_traj,
                          const float *vel_traj, const float *acc_traj, int32_t T, const covo_env_params *params /* [n_envs] */,
                          const float *a_mean /* [n_envs][128] */, const uint32_t *step_keys /* host [n_envs][2] */,
                          int32_t noisy_on, float obs_noise_scale, float *log, int32_t log_stride, int32_t log_index, void *stream);
int covo_run_episode_batched(covo_handle_t h, const covo_batch_args *args, const covo_env_params *params /* [n_envs] */,
                             float *states_true /* [n_envs][32] */, const float *acc_traj /* [n_envs][T][3] */, int32_t noisy_on,
                             float obs_noise_scale, float *log /* [n_envs][log_stride][4], nullable */, int32_t log_stride,
                             int32_t log_index, uint32_t *rngs /* host [n_envs][2], in/out */, int32_t n_steps, void *stream);

int covo_run_episode_batched_mode(covo_handle_t h, const covo_batch_mode_args *args, const covo_env_params *params /* [n_envs] */,
                                  float *states_true /* [n_envs][32] */, const float *acc_traj /* [n_envs][T][3] */, int32_t noisy_on,
                                  float obs_noise_scale, float *log /* [n_envs][log_stride][4], nullable */, int32_t log_stride,
                                  int32_t log_index, uint32_t *rngs /* host [n_envs][2], in/out */, int32_t n_steps, void *stream);

/* Profiling aid: `reps` copies of the selected launches of one control step, captured into one hipGraph and
 * replayed; *us_out = GPU microseconds per copy.  step_mask bits: 1 shift_mean, 2 Hessian, 4 Sigma, 8 noise GEMM,
 * 16 rollout, 32 softmax update; hess_mask bits: the four kernels of the adjoint Hessian; sigma_stages 1..4:
 * prep+squarings, +Ritz, +Newton-Schulz, +finalize.  Uses the buffers in `args` exactly like covo_mpc_step -- and, like a
 * real step, MUTATES the controller state they hold: every replayed copy that includes the update writes args->a_mean, MPPI's
 * begin work / fused small step shifts args->a_cov in place once per copy (plus once for the scratch refresh an eager handle
 * needs first), and the handle's sequence number advances.  Time on a state you can afford to lose, or snapshot a_mean / a_cov
 * around the call (bench.py times after its value-bearing steps). */
int covo_debug_time_step(covo_handle_t h, const covo_env_params *params, const covo_step_args *args, int32_t step_mask,
                         int32_t hess_mask, int32_t sigma_stages, int32_t reps, float *us_out, void *stream);

/* The same for the LAST covo_mpc_step_batched call of the handle (all instances; the begin launch, bit 1, re-splits the keys and
 * is normally left out).  covo-online only: refused when no covo-online batched step has run (covo_mpc_step_batched_mode's MPPI /
 * covo-offline steps are one launch with nothing to select). */
int covo_debug_time_batched(covo_handle_t h, int32_t step_mask, int32_t reps, float *us_out, void *stream);

/* Test hook: a one-thread kernel on `stream` ORs `bits` into the handle's status word the way a failing kernel would
 * (device store to host-mapped memory); covo_device_status / COVO_E_DEVICE can then be exercised without starving a barrier. */
int covo_debug_raise_device_status(covo_handle_t h, int32_t bits, void *stream);

/* Profiling aid: covo_rollout_cost `reps` times back to back on `stream` between two events, three batches; us_out[0] =
 * mean GPU microseconds per launch over all batches, us_out[1] = the fastest batch's (what bench.py reports as
 * roofline.launch_us / launch_us_min: a Python loop of single calls is host-bound below ~10 us per launch).
 * with_records != 0: the variant covo_mpc_step runs -- every workgroup also leaves its online-softmax record
 * (rollout_pipe3_kernel<..., REC = true>).  Synchronises the stream.  Other arguments as covo_rollout_cost (no position
 * statistics). */
int covo_debug_time_rollout(covo_handle_t h, const float *state, const float *pos_traj, const float *vel_traj, int32_t T,
                            const covo_env_params *params, const float *f_disturb_shared, const float *f_disturb_steps,
                            const float *a, int32_t N,
                            float *cost_out, float *groupmin, int32_t with_records, int32_t reps, float *us_out /* [host float[2]] */,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif /* COVO_HIP_H */
