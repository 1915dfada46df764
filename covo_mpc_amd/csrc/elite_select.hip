// elite_select.hip -- the elite-set update's selector (covo_set_step_elite, covo_elite_select).
//
// For the step's costs c_n and key(n) = (u(c_n) << 32) | n (elite_key.hpp) it finds the K-th smallest key exactly: the elite set is
// {n : key(n) <= threshold}, K members for every input -- equal costs go to the lowest indices, NaN costs last, +inf is a large cost.
// Radix select, most significant digit first, 8 bits per pass: a pass counts, over the samples whose key agrees with the digits
// fixed so far, the next digit into a 256-bin LDS histogram (integer atomicAdd), 256 threads scan the bins, and the bin that holds
// the k-th of them fixes the digit; k drops by the samples in the bins below.  Four passes fix the cost word.  If more than one
// sample carries the K-th cost, passes over the index word follow -- only the ceil(log256 N) digits an index below N can have;
// otherwise the one thread that holds the sample writes its index.
// One workgroup of 1 024 threads per instance, shaped like ess_lambda_kernel: thread t keeps the cost words t, t + 1024, ... in
// registers up to N = 65 536 (64 per thread), beyond that every pass re-reads the costs (L2-resident).  Integer counts only: the
// result is a function of the costs alone, whatever order the atomics land in; every thread holds the same prefix and k, so all
// control flow is workgroup-uniform.
#include "covo_common.hpp"
#include "elite_key.hpp"

constexpr int ES_THREADS = 1024;
constexpr int ES_WAVES = ES_THREADS / 64;
constexpr int ES_REG = 64;                         // cost words per thread kept in registers
constexpr int ES_REG_MAX_N = ES_THREADS * ES_REG;  // 65 536
constexpr int ES_BINS = 256;

struct EliteLds {
    uint32_t hist[ES_BINS];
    uint32_t wsum[ES_BINS / 64];  // the scan's wave totals
    uint32_t digit, below, count;  // the chosen bin, the samples in the bins below it, the samples in it
    uint32_t umin[ES_WAVES];
};

// one sample into the histogram.  The costs of a step share their leading digits: the lanes that agree with the wave's first
// candidate are counted with one atomic, the others add themselves
__device__ __forceinline__ void elite_count(bool cand, uint32_t d, uint32_t *hist)
{
    const unsigned long long act = __ballot(cand);
    if (act == 0ull) return;  // (wave-uniform)
    const int first = __ffsll((long long)act) - 1;
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, first);
    const unsigned long long same = __ballot(cand && d == d0);
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
    else if (cand && d != d0) atomicAdd(&hist[d], 1u);
}

// One digit pass.  INDEX = false: the samples' words are their cost words; INDEX = true: their indices, over the samples whose cost
// word is ukth.  Candidates: the samples n < N with (word & mask) == prefix; digit = (word >> shift) & 255.  On return, in every
// thread: the digit of the k-th smallest candidate (returned), k lowered by the candidates with a smaller digit, count = the
// candidates with that digit.  L.hist is all zero on entry and on return.  1 <= k <= candidates.  mask, prefix, shift, ukth and k
// are workgroup-uniform (scalar registers).
template <bool REG, bool INDEX>
__device__ __forceinline__ uint32_t elite_digit_pass(const uint32_t (&u)[ES_REG], const float *__restrict__ cost, int N, uint32_t ukth,
                                                     uint32_t mask, uint32_t prefix, int shift, uint32_t &k, uint32_t &count,
                                                     EliteLds &L)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (REG) {
        // the thread index as a value of THIS pass: left to itself the compiler keeps the 64 sample indices and their n < N masks of
        // the unrolled loop alive across the passes, next to the 64 cost words (168 bytes of scratch per lane)
        int t0 = tid;
        asm volatile("" : "+v"(t0));
        asm volatile("" : "+s"(ukth));  // (likewise the 64 masks u[i] == ukth of the index passes)
#pragma unroll
        for (int i = 0; i < ES_REG; ++i) {
            const int n = t0 + i * ES_THREADS;  // (rows beyond N: no candidate, elite_count returns at its first ballot)
            const uint32_t word = INDEX ? (uint32_t)n : u[i];
            elite_count(n < N && (!INDEX || u[i] == ukth) && (word & mask) == prefix, (word >> shift) & 255u, L.hist);
        }
    } else {
        for (int n0 = 0; n0 < N; n0 += ES_THREADS) {  // (every wave takes every trip: the ballots see whole waves)
            const int n = n0 + tid;
            const uint32_t un = n < N ? elite_cost_word(cost[n]) : 0u;
            const uint32_t word = INDEX ? (uint32_t)n : un;
            elite_count(n < N && (!INDEX || un == ukth) && (word & mask) == prefix, (word >> shift) & 255u, L.hist);
        }
    }
    __syncthreads();
    // inclusive scan of the 256 bins by the first four waves
    uint32_t h = 0, incl = 0;
    if (tid < ES_BINS) {  // (wave-uniform)
        h = L.hist[tid];
        L.hist[tid] = 0;
        incl = h;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) L.wsum[wave] = incl;
    }
    __syncthreads();
    if (tid < ES_BINS) {
        for (int w = 0; w < wave; ++w) incl += L.wsum[w];
        if (incl - h < k && k <= incl) {  // exactly one bin
            L.digit = (uint32_t)tid;
            L.below = incl - h;
            L.count = h;
        }
    }
    __syncthreads();
    k -= (uint32_t)__builtin_amdgcn_readfirstlane((int)L.below);
    count = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.count);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)L.digit);
}

// grid (1, instances); out: [instances][COVO_ELITE_FLOATS] = {bits(threshold cost word), bits(threshold index word), cost_min,
// cost_kth, K, elites that carry cost_kth, 0, 0}.  1 <= K <= N.
template <bool REG>
__global__ __launch_bounds__(ES_THREADS) void elite_select_kernel(const float *__restrict__ cost, int N, int K, float *out)
{
    __shared__ EliteLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        const size_t y = blockIdx.y;
        cost += y * N;
        out += y * COVO_ELITE_FLOATS;
    }
    if (tid < ES_BINS) L.hist[tid] = 0;
    // ---- pass 0: the cost words (into registers) and the smallest of them
    uint32_t u[ES_REG];
    uint32_t umin = 0xFFFFFFFFu;
    if (REG) {
#pragma unroll
        for (int i = 0; i < ES_REG; ++i) {
            const int n = tid + i * ES_THREADS;
            const uint32_t un = elite_cost_word(cost[n < N ? n : N - 1]);  // (a clamped load, not a branch per sample)
            u[i] = n < N ? un : 0xFFFFFFFFu;
            umin = u[i] < umin ? u[i] : umin;
        }
    } else {
        for (int n = tid; n < N; n += ES_THREADS) {
            const uint32_t un = elite_cost_word(cost[n]);
            umin = un < umin ? un : umin;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t t = (uint32_t)__shfl_xor((int)umin, o, 64);
        umin = t < umin ? t : umin;
    }
    if (lane == 0) L.umin[wave] = umin;
    __syncthreads();  // (also: the histogram is zero)
    umin = L.umin[0];
#pragma unroll
    for (int i = 1; i < ES_WAVES; ++i) umin = L.umin[i] < umin ? L.umin[i] : umin;
    // ---- the cost word of the K-th smallest key
    uint32_t mask = 0u, ukth = 0u;
    uint32_t k = (uint32_t)K, count = (uint32_t)N;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        const uint32_t d = elite_digit_pass<REG, false>(u, cost, N, 0u, mask, ukth, shift, k, count, L);
        mask |= 0xFFu << shift;
        ukth |= d << shift;
    }
    const uint32_t ties = k;  // the elites among the `count` samples that carry the K-th cost: the k of lowest index
    uint32_t *out_bits = reinterpret_cast<uint32_t *>(out);
    if (count > 1) {  // (workgroup-uniform) the index word, over the digits an index below N can have
        const int nd = N <= (1 << 8) ? 1 : N <= (1 << 16) ? 2 : N <= (1 << 24) ? 3 : 4;
        uint32_t idx = 0u;
        mask = nd < 4 ? ~0u << (8 * nd) : 0u;  // (the digits above are zero in every index)
#pragma unroll 1
        for (int shift = 8 * (nd - 1); shift >= 0; shift -= 8) {
            const uint32_t d = elite_digit_pass<REG, true>(u, cost, N, ukth, mask, idx, shift, k, count, L);
            mask |= 0xFFu << shift;
            idx |= d << shift;
        }
        if (tid == 0) out_bits[ELITE_ROW_INDEX_WORD] = idx;
    } else {  // one sample carries the K-th cost: its thread names it
        int found = -1;
        if (REG) {
            int t0 = tid;  // (as in elite_digit_pass)
            asm volatile("" : "+v"(t0));
#pragma unroll
            for (int i = 0; i < ES_REG; ++i) {
                const int n = t0 + i * ES_THREADS;
                found = (n < N && u[i] == ukth) ? n : found;
            }
        } else {
            for (int n = tid; n < N; n += ES_THREADS) found = elite_cost_word(cost[n]) == ukth ? n : found;
        }
        if (found >= 0) out_bits[ELITE_ROW_INDEX_WORD] = (uint32_t)found;
    }
    if (tid == 0) {
        out_bits[ELITE_ROW_COST_WORD] = ukth;
        out[ELITE_ROW_COST_MIN] = elite_word_cost(umin);
        out[ELITE_ROW_COST_KTH] = elite_word_cost(ukth);
        out[ELITE_ROW_K] = (float)K;
        out[ELITE_ROW_TIES] = (float)ties;
        out[6] = 0.0f;
        out[7] = 0.0f;
    }
}

int launch_elite_select(const float *cost, int N, int n_inst, int K, float *out, hipStream_t s)
{
    if (N <= ES_REG_MAX_N)
        hipLaunchKernelGGL(elite_select_kernel<true>, dim3(1, n_inst), dim3(ES_THREADS), 0, s, cost, N, K, out);
    else
        hipLaunchKernelGGL(elite_select_kernel<false>, dim3(1, n_inst), dim3(ES_THREADS), 0, s, cost, N, K, out);
    COVO_CHECK_HIP(hipGetLastError());
    return 0;
}
