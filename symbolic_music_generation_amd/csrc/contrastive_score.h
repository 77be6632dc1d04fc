// The arithmetic of the contrastive re-ranking, shared by mxl_contrastive_select (decode.hip) and mxl_contrastive_step
// (contrastive.hip): both entries call these functions, so the same inputs give the same bits on either path.
#pragma once
#include "common.h"

// 1 / |r| of one bf16 row of d elements (d % 8 == 0), by one wave: 8 bf16 per lane per pass over d
__device__ __forceinline__ float row_inv_norm_wave(const bf16_t* r, int d, int lane) {
    float s = 0.f;
    for (int c = lane * 8; c < d; c += 512) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(r + c);
#pragma unroll
        for (int k = 0; k < 8; k++) { const float f = bf2f((bf16_t)v[k]); s += f * f; }
    }
    return rsqrtf(wave_sum(s));
}

// (1 - alpha) * p - alpha * max_{s < S} cos(h, ctx[s]) of one candidate row h, by a workgroup of four waves that stride over the
// S context positions; ctx rows of d bf16, ctx_inv their reciprocal norms, wmax four floats of LDS.  The result is valid in thread 0.
__device__ __forceinline__ float contrastive_score_row(const bf16_t* ctx, const float* ctx_inv, int S, const bf16_t* h, int d, float p,
                                                       float alpha, float* wmax) {
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float hn = row_inv_norm_wave(h, d, lane);
    float best = -INFINITY;
    for (int s = wid; s < S; s += 4) {
        const bf16_t* c_ = ctx + (size_t)s * d;
        float dot = 0.f;
        for (int c = lane * 8; c < d; c += 512) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(h + c);
            const bf16x8 v = *reinterpret_cast<const bf16x8*>(c_ + c);
#pragma unroll
            for (int k = 0; k < 8; k++) dot += bf2f((bf16_t)a[k]) * bf2f((bf16_t)v[k]);
        }
        dot = wave_sum(dot) * hn * ctx_inv[s];
        best = fmaxf(best, dot);
    }
    if (lane == 0) wmax[wid] = best;
    __syncthreads();
    const float pen = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    return (1.f - alpha) * p - alpha * pen;
}
