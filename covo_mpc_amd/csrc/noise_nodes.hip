// noise_nodes.hip -- the annealed step's spline-node sampler (covo_set_step_nodes, covo_noise_nodes_philox).
//
//   a[h][n] = clip(mu[h] + sum_{m < M} B[h][m] e_m(n)),   e_m(n) = normal4(counter m, sample n, the pass's act key)
//
// B [32][M] is one pass's slice of the host-made table B[i][h][m] = fp32(sigma_n[i][m] W[h][m]): W the interpolation weights of M
// nodes spread over the 32 stages, sigma_n the schedule over the nodes (controllers/_options.py: node_basis, node_schedule).  The
// perturbation of a sample is then a spline over the horizon drawn in 4 M dimensions; the mean stays a 128-vector, so everything
// behind the sampler reads a, cost and mu as ever.  e_m is entry [n, m, :] of the stream noise_blockdiag_kernel<PHILOX> draws from,
// and the sum is one ascending-m fmaf chain from 0 per component: at M = 32 with B = sigma I the result is that kernel's, bit for bit.
//
// Lane = sample, 256 consecutive samples per workgroup on blockIdx.x: a wave stores 1 KiB contiguous runs of a stage stripe, and a
// sample block has the producer workgroups the rollout's XCD mapping expects of MPPI (RolloutDesc::xcd_groups = 4).  blockIdx.y =
// stage group: HS = 32 / S consecutive stages per thread; every group redraws the M normal4 (m is the OUTER loop: one e_m is live at
// a time, M is a run-time value) and accumulates into HS x 4 registers.  B is wave-uniform: scalar loads, no LDS.  blockIdx.z =
// instance (BATCHED: table shared, mu / key block dyn + 12 z / stripes per instance).  The chain of entry (n, h) does not know S, N
// or the grid: every launch shape gives the same bits.  No scratch, no atomics, no flags, no pow.
#include "covo_common.hpp"
#include <cstdlib>
#include "rng_device.hpp"

template <int HS, bool BATCHED>
__global__ __launch_bounds__(256) void noise_nodes_kernel(const float *__restrict__ table, int pass, int M, const float *__restrict__ mu,
                                                          uint32_t k0, uint32_t k1, int64_t sample_offset, int N,
                                                          float4 *__restrict__ a_out, const uint32_t *__restrict__ dyn, int nanp)
{
    if (BATCHED) {
        const size_t z = blockIdx.z;
        mu += z * COVO_NA;
        a_out += z * ((size_t)COVO_H * N);
        dyn += z * 12;
    }
    if (dyn != nullptr) { k0 = dyn[0]; k1 = dyn[1]; }
    const int h0 = (int)blockIdx.y * HS;
    const float *B = table + ((size_t)pass * COVO_H + h0) * M;  // (uniform: scalar loads)
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= (size_t)N) return;
    const uint64_t id = (uint64_t)(sample_offset + (int64_t)n);
    float acc[HS][4];
#pragma unroll
    for (int j = 0; j < HS; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[j][c] = 0.0f;
    for (int m = 0; m < M; ++m) {
        const float4 e = rngd::normal4((uint32_t)m, id, k0, k1);
        const float ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
        for (int j = 0; j < HS; ++j) {
            const float b = B[j * M + m];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[j][c] = fmaf(b, ev[c], acc[j][c]);
        }
    }
#pragma unroll
    for (int j = 0; j < HS; ++j) {
        float o[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float v = mu[(h0 + j) * 4 + c] + acc[j][c];
            o[c] = nanp ? qm::clip11_nan_(v) : qm::clip11_(v);
        }
        a_out[(size_t)(h0 + j) * N + n] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// S, the stage groups on the grid's y: the smallest of 2, 4, 8 that gives the launch two waves per SIMD (4 S waves per sample block,
// 1 024 SIMDs), 8 where none does.  Every group redraws the M normal4, so S costs draws and buys resident waves: measured per N and M
// in DESIGN.md 4.29 (S = 8 up to N = 16 384, 4 at 32 768, 2 from 65 536 on; S = 1 lost at every size).  COVO_NODES_SPLIT = 1 | 2 | 4 | 8
// overrides it for that measurement (scripts/nodes_cost.py); the bits do not depend on it.
static int noise_nodes_split(int N, int batch)
{
    static const int forced = [] {
        const char *v = std::getenv("COVO_NODES_SPLIT");
        const int s = v ? std::atoi(v) : 0;
        return (s == 1 || s == 2 || s == 4 || s == 8) ? s : 0;
    }();
    if (forced) return forced;
    const long long blocks = (long long)((N + 255) / 256) * batch;
    int S = 2;
    while (S < 8 && blocks * S < 512) S *= 2;
    return S;
}

int launch_noise_nodes(const NoiseDesc &d, const float *table, int pass, int n_nodes, hipStream_t s)
{
    const int N = d.N;
    const int nanp = d.propagate_nan ? 1 : 0;
    if (n_nodes < 2 || n_nodes > COVO_H || table == nullptr || d.eps != nullptr || (d.batch > 1 && d.dyn == nullptr)) {
        covo_set_error("noise_nodes: n_nodes=%d outside [2, %d], a null table, a materialised eps, or batch=%d without the keys in device "
                       "memory", n_nodes, COVO_H, d.batch);
        return COVO_E_BADARG;
    }
    const int S = noise_nodes_split(N, d.batch);
    const dim3 grid((N + 255) / 256, S, d.batch);
    float4 *a = reinterpret_cast<float4 *>(d.a);
#define NN_GO(HS)                                                                                                                   \
    do {                                                                                                                            \
        if (d.batch > 1)                                                                                                            \
            hipLaunchKernelGGL((noise_nodes_kernel<HS, true>), grid, dim3(256), 0, s, table, pass, n_nodes, d.mu, 0u, 0u,          \
                               d.sample_offset, N, a, d.dyn, nanp);                                                                 \
        else                                                                                                                        \
            hipLaunchKernelGGL((noise_nodes_kernel<HS, false>), grid, dim3(256), 0, s, table, pass, n_nodes, d.mu, d.key[0], d.key[1], \
                               d.sample_offset, N, a, d.dyn, nanp);                                                                 \
    } while (0)
    if (S == 1) NN_GO(32);
    else if (S == 2) NN_GO(16);
    else if (S == 4) NN_GO(8);
    else NN_GO(4);
#undef NN_GO
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
