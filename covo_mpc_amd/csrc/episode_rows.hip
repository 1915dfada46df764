// episode_rows.hip -- the episode logs of the rows the step attachments leave on the handle (covo_set_episode_rows, include/covo_hip.h:
// COVO_HAS_EPISODE_ROWS, and covo_set_episode_diag_log).  The ESS floor, the elite set, the iterations, the Sigma period /
// Sigma adapt, the posterior covariance and the sampling diagnostics each keep ONE row per instance that every step overwrites (the
// copied kinds of covo_eplog_kinds, covo_common.hpp); an episode driver with a log attached copies the rows
// of the step it has just enqueued into row `index` of every instance's log: one eager launch per step for all attached kinds, behind
// the step's launches (its after-step frame included: that is where the posterior covariance is formed) and ahead of the env step.
// The row index and the Sigma age are plain kernel arguments: no captured step graph knows about the logs.
#include "covo_common.hpp"

#define EPR_THREADS 256
#define EPR_COV_CHUNKS 16  // workgroups per instance once the matrix log is attached: 16 384 floats = 4 096 float4 = 16 x 256 lanes

// one attached kind: instance e's source row src + e * width -> dst + (e * dst_stride_rows + index) * width.  age_col (the Sigma row,
// width 4): column 0 is the step's age; columns 1..3 are src[e][0..2] (Sigma adapt's {fallback, c, log det M}), {0, 1, 0} with src null
struct EpRowDesc {
    const float *src;
    float *dst;
    int width;
    int dst_stride_rows;
    int age_col;
    int vec4;  // width % 4 == 0 and both base addresses 16-byte aligned: every row of the kind is
};
struct EpRowTable {
    EpRowDesc d[COVO_EPLOG_KINDS + 1];  // the copied kinds of covo_eplog_kinds: the six of covo_set_episode_rows and the diagnostic log
};

// grid (chunks, n_inst, attached kinds).  Bit copies: the floats travel as 32-bit words (a NaN keeps its payload)
__global__ __launch_bounds__(EPR_THREADS) void episode_rows_kernel(EpRowTable tab, int index, float age)
{
    const EpRowDesc &d = tab.d[blockIdx.z];
    const int e = blockIdx.y, width = d.width;
    float *dst = d.dst + ((size_t)e * d.dst_stride_rows + index) * width;
    const int lane = blockIdx.x * EPR_THREADS + threadIdx.x, lanes = gridDim.x * EPR_THREADS;
    if (d.age_col) {
        if (lane == 0) {
            const float *src = d.src ? d.src + (size_t)e * COVO_SIGMA_ADAPT_FLOATS : nullptr;
            const uint4 row = {__float_as_uint(age), src ? __float_as_uint(src[0]) : 0u, src ? __float_as_uint(src[1]) : __float_as_uint(1.0f),
                               src ? __float_as_uint(src[2]) : 0u};
            if (d.vec4) {
                *reinterpret_cast<uint4 *>(dst) = row;
            } else {
                uint32_t *d1 = reinterpret_cast<uint32_t *>(dst);
                d1[0] = row.x;
                d1[1] = row.y;
                d1[2] = row.z;
                d1[3] = row.w;
            }
        }
        return;
    }
    const float *src = d.src + (size_t)e * width;
    if (d.vec4) {
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        for (int i = lane; i < width / 4; i += lanes) d4[i] = s4[i];
    } else {
        const uint32_t *s1 = reinterpret_cast<const uint32_t *>(src);
        uint32_t *d1 = reinterpret_cast<uint32_t *>(dst);
        for (int i = lane; i < width; i += lanes) d1[i] = s1[i];
    }
}

static inline bool epr_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

int launch_episode_rows(const covo_ctx *h, int n_inst, int index, int age, hipStream_t s)
{
    constexpr int COPIED = sizeof(EpRowTable::d) / sizeof(EpRowDesc);
    EpRowTable tab;
    int n = 0;
    for (int k = 0; k < COVO_EPLOG_ALL; ++k) {
        if (h->eplog[k].log == nullptr || covo_eplog_kinds[k].rows == nullptr) continue;
        const covo_eprows rows = covo_eplog_kinds[k].rows(h);
        const bool age_col = k == COVO_EPLOG_SIGMA;
        if (rows.src == nullptr && !age_col) {  // (the setters keep a log only next to its attachment)
            covo_set_error("covo_set_episode_rows: kind %d has a log but its step attachment left no rows", k);
            return COVO_E_BADARG;
        }
        if (n == COPIED) {
            covo_set_error("launch_episode_rows: EpRowTable holds %d of the copied kinds, kind %d is one more", COPIED, k);
            return COVO_E_BADARG;
        }
        EpRowDesc &d = tab.d[n++];
        d.src = rows.src;
        d.dst = h->eplog[k].log;
        d.width = rows.width;
        d.dst_stride_rows = h->eplog[k].stride;
        d.age_col = age_col ? 1 : 0;
        // every row of the kind starts a multiple of 4 floats from its base: aligned bases make aligned rows
        d.vec4 = (d.width % 4 == 0 && epr_aligned16(d.dst) && (d.src == nullptr || epr_aligned16(d.src))) ? 1 : 0;
    }
    if (n == 0) return 0;
    for (int k = n; k < COPIED; ++k) tab.d[k] = tab.d[0];  // never indexed (grid z = n); no indeterminate bytes in the argument
    const int chunks = h->eplog[COVO_EPLOG_POST_COV].log != nullptr ? EPR_COV_CHUNKS : 1;
    hipLaunchKernelGGL(episode_rows_kernel, dim3(chunks, n_inst, n), dim3(EPR_THREADS), 0, s, tab, index, (float)age);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
