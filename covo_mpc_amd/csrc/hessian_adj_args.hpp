// hessian_adj_args.hpp -- what every translation unit that includes hessian_adj_body.hpp declares ahead of it (hessian_adj.hip: the
// Hessian's four kernels; cost_gradient.hip: KB again, for the first-order adjoint): the MFMA vector type, the kernels' argument
// block and the drag coefficient of the adj16 instantiation.
#pragma once
#include "covo_common.hpp"
#include <cstdlib>
#include <cstring>
#include "wave_reduce.hpp"
#include "sym_stats.hpp"
#include "disturb_model.hpp"
#include "step_begin.hpp"

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct AdjArgs {
    const float *state;     // [batch][COVO_STATE_FLOATS]
    const float *pos_traj;  // [T][3] shared
    const float *vel_traj;
    const float *a_mean;    // [batch][128]
    double *R;              // [batch][128][128]
    double *ws;             // [batch][WS_COUNT]
    int T;
    qm::Consts<double> c;            // shared model constants ...
    const qm::Consts<double> *cs;    // ... or one per batch entry (device, nullable): env instances with their own parameters
    size_t traj_stride;              // floats between the trajectories of consecutive batch entries (0: shared)
    SymStatsOut stats;               // rpart != null: KD also leaves the Sigma chain's input statistics of R there (every instance)
    const float4 *f_tab;             // [batch][H] per-step disturbance table (disturb.hip; wave-uniform kinds only) or null: no force after step 0
    int reward;                      // COVO_REWARD_*
    // adj16 only (drag / mixed: the force is part of the differentiated state); f_tab rows are then {g_k[3], c_k}
    double drag_k;                   // c_drag * (-|disturb_scale| / 1.5^2)   (free.py:41-47)
    double drag_off[3];              // disturb_params[:3] / 2
    const dm::Model *models;         // per batch entry next to cs (device, nullable): overrides drag_k / drag_off
    int *status;                     // the handle's sticky device status (nullable): COVO_DEVSTAT_ADJOINT when a costate wait times out
    // the step's begin work folded into KB (eager covo-online steps; launch_hessian's HessBegin): a_mean_raw != null -> KB reads the
    // UNSHIFTED mean through the shift's index map (covo.py:201-203) and its workgroup (0, 0) leaves what step_begin_kernel would
    // have left for the launches that follow: the shifted mean (a_mean points there: KC / KD read it a launch later), the per-step
    // scalars derived from the raw rng_act (step_begin.hpp) and the bumped sequence number
    const float *a_mean_raw;
    uint32_t *dyn_out;
    unsigned *seq;
    DynBlock blk;
    int derive_keys;
    float shared_noise_scale;
    int begin_pass;  // > 0 (pass of an iterated step, covo_set_step_iters): a_mean_raw is read as it lies, the raw key is dyn_out[10..11] advanced
    int scan_prefix;                 // KB forms its primal prefix by parallel scans (adj13; COVO_HESS_SCAN=0: the sequential rollout)
};

__host__ __device__ inline double adj_drag_coeff(const dm::Model &m)
{
    return -(m.kind == COVO_DISTURB_DRAG ? 1.0 : (m.kind == COVO_DISTURB_MIXED ? 1.0 / 3.0 : 0.0)) * fabs((double)m.scale) / 2.25;
}


// host: everything of the argument block that follows from the caller's descriptor alone -- the model, the trajectories, the mean, the
// tables -- with no begin work folded in, no statistics and no outputs (R, ws: the caller's).  fs: the adj16 instantiation runs
// (drag / mixed).  who: the entry point, for the error text
static inline int adj_args_from_desc(AdjArgs &A, const HessianDesc &d, const char *who, bool &fs)
{
    const covo_env_params &p = *d.params;
    const float *f_tab = d.f_tab;
    const void *consts_dev = d.consts_dev, *models_dev = d.models_dev;
    fs = p.disturb_kind == COVO_DISTURB_DRAG || p.disturb_kind == COVO_DISTURB_MIXED;
    if (fs && (consts_dev != nullptr) != (models_dev != nullptr)) {
        covo_set_error("%s: drag / mixed disturbance with per-instance constants needs the per-instance models too", who);
        return COVO_E_BADARG;
    }
    if ((fs || p.disturb_kind == COVO_DISTURB_PERIODIC || p.disturb_kind == COVO_DISTURB_SIN) && f_tab == nullptr) {
        covo_set_error("%s: disturb_kind=%d needs the per-step disturbance table (covo_disturb_table)", who, p.disturb_kind);
        return COVO_E_BADARG;
    }
    A.f_tab = (fs || p.disturb_kind == COVO_DISTURB_PERIODIC || p.disturb_kind == COVO_DISTURB_SIN) ? reinterpret_cast<const float4 *>(f_tab) : nullptr;
    const dm::Model m = dm::make_model(p);
    A.drag_k = adj_drag_coeff(m);
    for (int i = 0; i < 3; ++i) A.drag_off[i] = 0.5 * (double)m.dp[i];
    A.models = reinterpret_cast<const dm::Model *>(models_dev);
    A.reward = p.reward_kind;
    A.status = d.status_dev;
    A.state = d.state;
    A.pos_traj = d.pos_traj;
    A.vel_traj = d.vel_traj;
    A.a_mean = d.a_mean;
    A.a_mean_raw = nullptr;
    A.dyn_out = nullptr;
    A.seq = nullptr;
    std::memset(&A.blk, 0, sizeof(A.blk));
    A.derive_keys = 0;
    A.shared_noise_scale = 0.0f;
    A.begin_pass = 0;
    static const int scan_prefix = [] { const char *v = std::getenv("COVO_HESS_SCAN"); return v ? std::atoi(v) : 1; }();
    A.scan_prefix = scan_prefix;
    A.R = nullptr;
    A.ws = nullptr;
    A.T = d.T;
    A.c = make_consts<double>(p);
    A.cs = reinterpret_cast<const qm::Consts<double> *>(consts_dev);
    A.traj_stride = d.traj_stride;
    A.stats.rpart = nullptr;
    A.stats.fpart = nullptr;
    A.stats.diag = nullptr;
    A.stats.stride = 0;
    A.stats.flags = nullptr;
    A.stats.ready = nullptr;
    return 0;
}
