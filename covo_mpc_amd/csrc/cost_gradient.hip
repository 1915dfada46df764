// cost_gradient.hip -- gradient of the CoVO rollout objective by the first-order adjoint (gfx950, fp64).
//
// The objective is the Hessian's (hessian_adj.hip): C(a) = -( sum_{k<H} r(s_k) + r(s_0) ), s_{k+1} = step_env(s_k, a_k,
// deterministic=True), no discount, no done-freeze, the Hessian's disturbance table.  With x_{k+1} = f_k(x_k, u_k), J = sum_{k>=1} r_k(x_k):
//     costate   lam_31 = grad r_31,   lam_k = grad r_k + A_k^T lam_{k+1}     (A_k = df_k/dx)
//     gradient  g_k = dC/du_k = -B_k^T lam_{k+1}                             (B_k = df_k/du), k = 0 .. 30;   g_31 = 0
// (the last action reaches no rewarded state).  Two launches:
//   KB  the Hessian's first kernel as it is (hessian_adj_body.hpp: adj_jac_kernel, no begin work folded in) into a workspace of the
//       gradient's own: A_k, B_k (WS_JF) and grad r_k (WS_GL)
//   KG  one wave per batch entry walks the costate down the horizon.  Lane c < NZ owns column c of df_k/dz: the sum over the rows
//       j = 0 .. NX-1 in ascending order, one fp64 fma each -- lam_k[c] = grad r_k[c] + sum for c < NX, g[4k + c - NX] = -sum for
//       c >= NX.  One order, one lane per output: a batch gives the bits of its singles, and the step's gradient (newton_refine.hip)
//       is this launch.
// The body is compiled a second time here, as hessian_adj.hip compiles it: adj13 (the force of a step is a constant of the step) and
// adj16 (drag / mixed: the force is part of the differentiated state).
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

// the costate walk of one batch entry.  ws: the entry's workspace as KB left it; g: its [128] of the output
template <int NX, int NZ, size_t WS_JF, size_t WS_GL>
__device__ __forceinline__ void cost_gradient_walk(const double *__restrict__ ws, double *__restrict__ g, int lane, double (*slam)[16])
{
    constexpr int HH = COVO_H, PF = 4;  // PF: steps whose column loads are in flight ahead of the one being summed
    const bool on = lane < NZ;
    const int c = on ? lane : 0;
    const double *__restrict__ jf = ws + WS_JF + c;  // column c: jf[(k * NX + j) * NZ]
    const double *__restrict__ gl = ws + WS_GL;
    double col[PF][NX], glk[PF];
    auto load = [&](int k) {  // (k is a compile-time number where this is called: the slot too)
#pragma unroll
        for (int j = 0; j < NX; ++j) col[k % PF][j] = jf[(size_t)(k * NX + j) * NZ];
        glk[k % PF] = gl[16 * k + (c < NX ? c : 0)];
    };
#pragma unroll
    for (int k = HH - 2; k > HH - 2 - PF; --k) load(k);
    if (lane < 16) slam[(HH - 1) & 1][lane] = lane < NX ? gl[16 * (HH - 1) + lane] : 0.0;
    if (lane >= 60) g[4 * (HH - 1) + lane - 60] = 0.0;
    __syncthreads();
#pragma unroll
    for (int k = HH - 2; k >= 0; --k) {
        const double *__restrict__ lam = slam[(k + 1) & 1];  // lam_{k+1}
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < NX; ++j) v = fma(col[k % PF][j], lam[j], v);
        const double lk = glk[k % PF] + v;
        if (k - PF >= 0) load(k - PF);
        if (on && c >= NX) g[4 * k + c - NX] = -v;
        if (lane < 16) slam[k & 1][lane] = lane < NX ? lk : 0.0;
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void cost_gradient_kernel(const double *__restrict__ ws, double *__restrict__ g_out, int fs)
{
    __shared__ double slam[2][16];
    const int b = blockIdx.x, lane = threadIdx.x;
    double *__restrict__ g = g_out + (size_t)b * COVO_NA;
    if (fs) cost_gradient_walk<adj16::NX, adj16::NZ, adj16::WS_JF, adj16::WS_GL>(ws + (size_t)b * adj16::WS_COUNT, g, lane, slam);
    else cost_gradient_walk<adj13::NX, adj13::NZ, adj13::WS_JF, adj13::WS_GL>(ws + (size_t)b * adj13::WS_COUNT, g, lane, slam);
}
}  // namespace

// KB addresses entry b at b * WS_COUNT of its instantiation; the sensitivities' part of a Hessian workspace is never written here
size_t cost_gradient_workspace_bytes(int batch)
{
    constexpr size_t n = adj16::WS_COUNT > adj13::WS_COUNT ? adj16::WS_COUNT : adj13::WS_COUNT;
    return (size_t)batch * n * sizeof(double);
}

// d: the Hessian's descriptor (R, stats and begin are not read); g_out [batch][128]
int launch_cost_gradient(const HessianDesc &d, double *g_out, void *workspace, hipStream_t s)
{
    AdjArgs A;
    bool fs;
    if (int rc = adj_args_from_desc(A, d, "cost gradient", fs)) return rc;
    A.status = nullptr;  // (KB raises nothing)
    A.ws = reinterpret_cast<double *>(workspace);
    const int batch = d.batch;
    if (fs) hipLaunchKernelGGL(adj16::adj_jac_kernel<true>, dim3(adj16::HH, batch), dim3(64), 0, s, A);
    else if (A.f_tab != nullptr) hipLaunchKernelGGL(adj13::adj_jac_kernel<true>, dim3(adj13::HH, batch), dim3(64), 0, s, A);
    else hipLaunchKernelGGL(adj13::adj_jac_kernel<false>, dim3(adj13::HH, batch), dim3(64), 0, s, A);
    hipLaunchKernelGGL(cost_gradient_kernel, dim3(batch), dim3(64), 0, s, A.ws, g_out, fs ? 1 : 0);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
