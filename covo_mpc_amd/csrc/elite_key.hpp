// elite_key.hpp -- the sort key of the elite-set update (covo_set_step_elite), shared by the selector
// (elite_select.hip) and the 0/1-weight stage 1 (reduce_elite.hip): key(n) = (u(c_n) << 32) | n.
#pragma once
#include "covo_common.hpp"

// the cost word u: the fp32 bits in an order-preserving unsigned form, as update_arbiter.hip's arb_key builds it (-0 and +0 are one
// cost); a NaN cost -> 0xFFFFFFFF, above +inf (0xFF800000) and never the word of a number
__device__ __forceinline__ uint32_t elite_cost_word(float v)
{
    if (!(v == v)) return 0xFFFFFFFFu;
    if (v == 0.0f) v = 0.0f;
    const uint32_t u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
// the cost a word stands for (0xFFFFFFFF decodes to a NaN by itself: 0x7FFFFFFF)
__device__ __forceinline__ float elite_word_cost(uint32_t u) { return __uint_as_float((u >> 31) ? (u & 0x7FFFFFFFu) : ~u); }

// the selector's row of one instance (include/covo_hip.h: COVO_ELITE_FLOATS)
constexpr int ELITE_ROW_COST_WORD = 0, ELITE_ROW_INDEX_WORD = 1, ELITE_ROW_COST_MIN = 2, ELITE_ROW_COST_KTH = 3, ELITE_ROW_K = 4,
              ELITE_ROW_TIES = 5;
