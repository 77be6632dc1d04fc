// The ordered key of a beam candidate, shared by beam.hip and beam_sample.hip: score descending, then flat index ascending, as one
// unsigned 64-bit word, so that a selection round is one max reduction.
#pragma once
#include "common.h"

// (score, flat index) -> a word whose unsigned order is "score ascending, then index descending": the best candidate is the max
__device__ __forceinline__ unsigned long long beam_key(float s, uint32_t idx) {
    uint32_t u = __float_as_uint(s + 0.0f);                          // (-0 -> +0: equal scores must tie)
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}
__device__ __forceinline__ float beam_key_score(unsigned long long k) {
    const uint32_t u = (uint32_t)(k >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}
__device__ __forceinline__ uint32_t beam_key_index(unsigned long long k) { return 0xFFFFFFFFu - (uint32_t)k; }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)k, o, 64), hi = __shfl_xor((uint32_t)(k >> 32), o, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        k = other > k ? other : k;
    }
    return k;
}

// the max of `best` over a workgroup of T threads, in every thread; sh_part (T / 64 words) may be rewritten after the caller's next barrier
template <int T>
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long best, unsigned long long* sh_part) {
    const int tid = threadIdx.x;
    best = wave_max_u64(best);
    if ((tid & 63) == 0) sh_part[tid >> 6] = best;
    __syncthreads();
    best = sh_part[0];
#pragma unroll
    for (int w = 1; w < T / 64; w++) best = sh_part[w] > best ? sh_part[w] : best;
    return best;
}
