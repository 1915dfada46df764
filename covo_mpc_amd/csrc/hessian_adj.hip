// hessian_adj.hip -- exact Hessian of the CoVO rollout objective by the second-order adjoint (gfx950, fp64).
//
// Replaces jax.jacfwd(jax.jacfwd(get_cumulated_cost)) of quadjax/controllers/covo.py:134-185:
//     C(a) = -( sum_{k<H} r(s_k) + r(s_0) ),  s_{k+1} = step_env(s_k, a_k, deterministic=True)
// (no discount, no done-freeze; reward on the PRE-step state; r(s_0) constant).  R = d^2 C / da^2.
//
// hessian.hip (kept as covo_hessian_pairs) runs one hyper-dual ROLLOUT per pair (i, j): exact, but its critical
// path is 31 hyper-dual steps (~1500 fp64 instructions each, one wave issues ~1 per 5 cycles) = 80 us.
// The same matrix follows from ONE hyper-dual step per (time, pair of step inputs) plus two short
// linear recursions.  With z_k = (x_k, u_k) in R^17 (state 13, raw action 4), x_{k+1} = f_k(z_k),
// J = sum_{k>=1} r_k(x_k):
//     costate    lam_31 = grad r_31,   lam_k = grad r_k + A_k^T lam_{k+1}          (A_k = df_k/dx)
//     sensitivity S_0 = 0,  S_{k+1} = A_k S_k + B_k E_k                          (S_k = dx_k/da, 13 x 128)
//     d^2 J/da^2 = sum_k [S_k; E_k]^T  Hess_z( r_k(x) + lam_{k+1} . f_k(z) )  [S_k; E_k]
// (E_k selects the four actions of step k).  All derivatives of the step come from evaluating the SAME
// templated model (quad_model.hpp) on hyper-dual numbers, so every JAX AD convention it mirrors (clip ties,
// |x|', the double clip of quadrotor.py:223/:258) carries over.  Three launches (KM rides in KC's):
//   KB  32 waves: primal rollout to step k (plain fp64), then the step on first-order duals (17 seeds) -> A_k, B_k, grad r_k
//   KC  9 workgroups of four waves: the sensitivity recursion (8 column tiles of S held in MFMA C/D layout, which IS the B operand
//       of the next step: four dependent v_mfma_f64_16x16x4_f64 per step, nothing leaves the registers) and
//       the costate recursion (the same product with A^T) -- no sparsity assumptions.  Both are linear, so each runs as four
//       horizon segments (8, 8, 8, 7 steps) on the four waves of its workgroup at the same time, joined with one product per
//       boundary through LDS (hessian_adj_body.hpp: adj_chain_kernel; adj16 keeps the costate sequential)
//   KM  32 x 153 lanes, 32 more workgroups of KC's launch: one hyper-dual step per pair (a <= b) of step inputs, contracted with
//       lam_{k+1} as soon as the costate chain of the same launch has stored it -> M_k = Hess_z(r_k + lam_{k+1}.f_k)
//   KD  36 lower 16x16 tiles: sum_k S_k^T Mxx_k S_k on the matrix cores (v_mfma_f64_16x16x4_f64; the product
//       Mxx S leaves the MFMA in exactly the register layout the next MFMA wants as its B operand), the
//       action blocks Mxu, Muu added in the epilogue.  A NaN of the costate (norm'(0)) is laid over every tile, as the reference's AD has it
//       in every entry.
// Critical path: the primal prefix (five scan levels; drag / mixed: 30 plain steps) + 2 hyper-dual steps + an 8-step segment of
// each recursion, its joins and fills ~ 22 us.
// The kernels live in hessian_adj_body.hpp and are compiled twice: adj13 (x in R^13: the force of a step is a constant of that
// step -- none / gaussian / periodic / sin) and adj16 (x in R^16 = state + force: drag / mixed, whose next force depends on the
// PRE-step velocity and the current force; round 3 -- these two models used to take the 80 us per-pair kernel).
#include "covo_common.hpp"
#include "wave_reduce.hpp"
#include <cstdlib>
#include <cstring>
#include "sym_stats.hpp"
#include "disturb_model.hpp"
#include "step_begin.hpp"

#include "hessian_adj_args.hpp"

namespace {
namespace adj13 {
#define ADJ_NX 13
#define ADJ_FS 0
#include "hessian_adj_body.hpp"
#undef ADJ_NX
#undef ADJ_FS
}  // namespace adj13
namespace adj16 {
#define ADJ_NX 16
#define ADJ_FS 1
#include "hessian_adj_body.hpp"
#undef ADJ_NX
#undef ADJ_FS
}  // namespace adj16
}  // namespace


constexpr size_t WS_COUNT_MAX = adj16::WS_COUNT > adj13::WS_COUNT ? adj16::WS_COUNT : adj13::WS_COUNT;
size_t hessian_workspace_bytes(int batch) { return (size_t)batch * WS_COUNT_MAX * sizeof(double); }
// where launches 1 | 2 leave what a reader of the workspace needs (riccati.hip), by instantiation
HessianWsLayout hessian_workspace_layout(bool fs)
{
#define ADJ_LAYOUT(NS) HessianWsLayout{NS::NX, NS::WS_COUNT, NS::WS_X, NS::WS_JF, NS::WS_LAM, NS::WS_MXX, NS::WS_MXU, NS::WS_MUU}
    return fs ? ADJ_LAYOUT(adj16) : ADJ_LAYOUT(adj13);
#undef ADJ_LAYOUT
}

int launch_hessian(const HessianDesc &d, void *workspace, hipStream_t s, const DebugMasks &dbg)
{
    const HessBegin *begin = d.begin;
    const int batch = d.batch;
    AdjArgs A;
    bool fs;
    if (int rc = adj_args_from_desc(A, d, "hessian", fs)) return rc;
    if (begin != nullptr && batch == 1 && (dbg.hess & 1)) {
        A.a_mean_raw = begin->a_mean_raw;
        A.dyn_out = begin->dyn_out;
        A.seq = begin->seq;
        std::memcpy(&A.blk, begin->blk, sizeof(A.blk));
        A.derive_keys = begin->derive_keys;
        A.shared_noise_scale = begin->shared_noise_scale;
        A.begin_pass = begin->pass;
    }
    A.R = d.R;
    A.ws = reinterpret_cast<double *>(workspace);
    if (d.stats != nullptr) A.stats = *d.stats;
    // launch shapes: KB 32 waves; KC 9 chains + KM's 32 hyper-dual workgroups (which also contract with the costate); KD 36 tiles
    // batched: chains and hyper-dual workgroups as two launches (hessian_adj_body.hpp: adj_hd_kernel) -- 66.5 -> 62.5 us at 32 instances;
    // one instance keeps them in one launch (the hyper-dual workgroups start under the chains: 27.9 -> 25.7 us in round 3)
    const bool split_hd = batch >= 8;
#define ADJ_LAUNCH(NS, JAC)                                                                                                      \
    do {                                                                                                                         \
        if (dbg.hess & 1) hipLaunchKernelGGL(JAC, dim3(NS::HH, batch), dim3(64), 0, s, A);                                       \
        if ((dbg.hess & 2) && split_hd) {                                                                                        \
            hipLaunchKernelGGL(NS::adj_chain_kernel, dim3(9, batch), dim3(256), 0, s, A);                                        \
            hipLaunchKernelGGL(NS::adj_hd_kernel, dim3(NS::HH, batch), dim3(256), 0, s, A);                                      \
        } else if (dbg.hess & 2) hipLaunchKernelGGL(NS::adj_chain_kernel, dim3(9 + NS::HH, batch), dim3(256), 0, s, A);          \
        if (dbg.hess & 8) hipLaunchKernelGGL(NS::adj_gemm_kernel, dim3(36, batch), dim3(512), 0, s, A);                          \
    } while (0)
    if (fs) ADJ_LAUNCH(adj16, adj16::adj_jac_kernel<true>);
    else if (A.f_tab != nullptr) ADJ_LAUNCH(adj13, adj13::adj_jac_kernel<true>);
    else ADJ_LAUNCH(adj13, adj13::adj_jac_kernel<false>);
#undef ADJ_LAUNCH
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}

// host side of the per-instance constants: covo_env_params[n] -> qm::Consts<double>[n] (to be copied to the device)
size_t hessian_consts_bytes(int n) { return (size_t)n * sizeof(qm::Consts<double>); }
void hessian_fill_consts(const covo_env_params *params, int n, void *out)
{
    qm::Consts<double> *c = reinterpret_cast<qm::Consts<double> *>(out);
    for (int i = 0; i < n; ++i) c[i] = make_consts<double>(params[i]);
}
