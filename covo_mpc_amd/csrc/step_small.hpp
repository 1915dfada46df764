// step_small.hpp -- interface of the fused small step (step_small.hip) towards step.hip.
#pragma once
#include "rollout_common.hpp"
#include "step_begin.hpp"

struct SmallStepArgs {
    RolloutArgs R;              // the rollout's argument block (state, trajectories, work buffers, records workspace, 1 / lambda,
                                // and where the last workgroup's merge goes: the new mean, or a sharded rank's merged record)
    const float *a_mean_in;     // control_params.a_mean of this call [128]
    float *a_mean_shift_out;    // receives the shifted old mean (the rank merge of a sharded step blends with it); with dyn_mem set it
                                // already HOLDS it (the begin launch of this graph replay) and is read instead of a_mean_in
    int n_table;
    const float *L_table;       // covo-offline: [n_table][128][128] lower factors
    float *mppi_cov;            // MPPI: a_cov [H][4][4], shifted in place by the launch's last workgroup
    int64_t sample_offset;
    DynBlock blk;               // eager launches: the per-step scalars as kernel arguments (step_begin.hpp) ...
    const uint32_t *dyn_mem;    // ... captured graphs: in device memory, left there by the begin launch (else null)
    int derive_keys;
    float shared_noise_scale;
    int nanp;
    // an iterated step (covo_set_step_iters; pass 0 with key_io and iter_out null is today's launch).  The BATCHED kernel reads `pass`
    // from its kernel argument (instance 0's block, patched per launch), the rest from the instance's own block
    int pass;                   // >= 1: no shift -- the starting mean is a_mean_in as it lies; MPPI's covariances stay as pass 0 shifted them
    uint32_t *key_io;           // where the step's raw key is walked in device memory: pass >= 1 reads the previous pass's raw key there
                                // and advances it (step_begin_advance); the last workgroup of every pass stores the pass's own
    float *iter_out;            // [iters]: the last workgroup stores the merge's cost minimum at [pass]
};

// can the step (args, params) run as the one fused launch?
bool step_small_eligible(const covo_ctx *h, const covo_env_params &p, const covo_step_args &a);
// state: the noisy state this launch reads (args.state, or the graph's fixed-address copy); blk / dyn_mem: exactly one non-null
int launch_step_small(covo_ctx *h, const covo_env_params &p, const covo_step_args &a, const float *state, float *a_mean_shift,
                      const DynBlock *blk, const uint32_t *dyn_mem, float shared_noise_scale, unsigned *ticket, hipStream_t s,
                      int pass = 0, uint32_t *key_io = nullptr, float *iter_slot = nullptr);
// why not, in words a caller can act on (null: eligible)
const char *step_small_refusal(const covo_ctx *h, const covo_env_params &p, const covo_step_args &a);
// The env-batched form (grid = groups per instance x instances): instance `index`'s argument block, described like a single step
// by (p, a) with a.state / a.a_mean / a.a_cov / a.L_table / a.a / a.cost its own buffers, into the host array `out`;
// raw_key_mem: DEVICE uint32[2], that instance's raw rng_act of the current step; ticket / records: its own arrival counter and
// [groups][COVO_PARTIAL_FLOATS] records; diag_rec / diag_out: its [groups][MG_DIAG_REC] diagnostic records and its row of the
// caller's diagnostic buffer (diag_out null: diagnostics off).  The device copy of the array is the launch's `args_dev`.
size_t step_small_args_bytes(int n);
void step_small_fill_args(covo_ctx *h, void *out, int index, const covo_env_params &p, const covo_step_args &a, const uint32_t *raw_key_mem,
                          float shared_noise_scale, unsigned *ticket, float *records, float *diag_rec, float *diag_out,
                          float *iter_out = nullptr);
int launch_step_small_batched(covo_ctx *h, const void *args_host, const void *args_dev, int n, bool mppi, hipStream_t s, int pass = 0);
