// Contrastive search on the device (HF 4.25.1 GenerationMixin.contrastive_search / _ranking_fast over Transformer-XL mems; the
// host reference is generate.contrastive_search).  One decoder row per (sequence, candidate): rows b*K .. b*K + K-1 belong to
// sequence b.  A captured step is
//     [mxl_rules_mask]  mxl_contrastive_topk  mxl_decode_advance  <the model>  mxl_contrastive_step  [mxl_rules_advance]
//     mxl_ring_slot_broadcast
// with no host read in it.
//
// THE INVARIANT.  The K rows of a sequence start from the same prompt, so after the prompt pass their K/V rings, id histories and
// rule words are identical.  A step writes exactly ONE ring slot per layer -- slot t mod M, the K candidates' K/V -- and then picks
// one candidate.  So at that point the K rows differ in that one slot only (and in column t of ids, the candidate tokens).  "All K
// rows take over the picked candidate's rings" is therefore a copy of one slot per (layer, K or V, head) into the other K-1 rows
// (mxl_ring_slot_broadcast), not of the rings; mxl_contrastive_step writes the picked token to column t of all K rows, after which
// the id histories are equal again, and the rule words, which advance after that write along the same token from the same values,
// stay equal.  No reorder of ids or rule words exists on this path.  Everything here relies on it: the top-k reads only the picked
// row's log-probabilities, the stop rule reads `unfinished` of row b*K for the whole sequence.
#include "common.h"
#include "musicxl_internal.h"
#include "contrastive_score.h"

namespace {
constexpr int CS_KMAX = 32;

// (v2, i2) ranks before (v, i) in (value descending, token id ascending) order; i < 0 = no candidate
__device__ __forceinline__ bool cs_before(float v2, int i2, float v, int i) {
    return i2 >= 0 && (i < 0 || v2 > v || (v2 == v && i2 < i));
}

// One workgroup per sequence.  K rounds over the picked row's V log-probabilities: round k finds the best entry that ranks after
// round k-1's, exact for any V and any ties (-inf entries take part and sort last, by id).  Then the softmax over the K values.
__global__ __launch_bounds__(256) void contrastive_topk_kernel(const float* logp, int ldl, int V, int K, const int* sel, long long* ids,
                                                               int ld_ids, const int* t_dev, float* probs, int* dead,
                                                               const int* unfinished, int pad_id) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ float topv[CS_KMAX];
    __shared__ int topi[CS_KMAX];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int col = *t_dev + 1;
    if (col < 0 || col >= ld_ids) return;
    long long* out = ids + (size_t)b * K * ld_ids + col;
    if (unfinished && unfinished[(size_t)b * K] == 0) {            // a finished sequence: pad in all K rows
        if (tid < K) {
            out[(size_t)tid * ld_ids] = pad_id;
            probs[(size_t)b * K + tid] = 0.f;
            dead[(size_t)b * K + tid] = 0;
        }
        return;
    }
    int s = sel[b];
    if (s < 0 || s >= K) s = 0;
    const float* row = logp + ((size_t)b * K + s) * ldl;
    float pv = INFINITY;
    int pi = -1;
    for (int k = 0; k < K; k++) {
        float bv = 0.f;
        int bi = -1;
        for (int i = tid; i < V; i += 256) {
            const float v = row[i];
            const bool after = v < pv || (v == pv && i > pi);
            if (after && (bi < 0 || v > bv)) { bv = v; bi = i; }   // i ascends: among equals the thread keeps the lowest id
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (cs_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { sv[wid] = bv; si[wid] = bi; }
        __syncthreads();
        bv = sv[0]; bi = si[0];
#pragma unroll
        for (int w = 1; w < 4; w++)
            if (cs_before(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
        if (bi < 0) { bv = -INFINITY; pv = -INFINITY; pi = V; }    // nothing left (fewer than K comparable entries): the rest is dead
        else { pv = bv; pi = bi; }
        if (tid == 0) { topv[k] = bv; topi[k] = bi; }
        __syncthreads();
    }
    if (tid == 0) {
        // a candidate at -inf (a barred token) is dead: probability 0, the flag, and candidate 0's token so that its forward is harmless
        const float m = topv[0];
        const int tok0 = topi[0] >= 0 ? topi[0] : 0;
        float sum = 0.f;
        uint32_t alive = 0u;
        for (int k = 0; k < K; k++) {
            const bool live = topi[k] >= 0 && topv[k] > -INFINITY;
            const float e = live ? expf(topv[k] - m) : 0.f;
            alive |= (uint32_t)live << k;
            topv[k] = e;
            sum += e;
        }
        for (int k = 0; k < K; k++) {
            const bool live = (alive >> k) & 1u;
            probs[(size_t)b * K + k] = live ? topv[k] / sum : 0.f;
            dead[(size_t)b * K + k] = live ? 0 : 1;
            out[(size_t)k * ld_ids] = live ? topi[k] : tok0;
        }
    }
}

// one workgroup per candidate row, the arithmetic of mxl_contrastive_select (contrastive_score_row); S = *t_dev context positions
__global__ __launch_bounds__(256) void contrastive_step_score_kernel(const bf16_t* ctx, long long ctx_bs, const float* ctx_inv, int inv_bs,
                                                                     int Smax, const int* t_dev, const bf16_t* hid, int d,
                                                                     const float* probs, const int* dead, float alpha, int K,
                                                                     float* score) {
    __shared__ float wmax[4];
    const int row = blockIdx.x, b = row / K;
    const int S = min(*t_dev, Smax);
    const float sc = contrastive_score_row(ctx + (size_t)b * ctx_bs, ctx_inv + (size_t)b * inv_bs, S, hid + (size_t)row * d, d,
                                           probs[row], alpha, wmax);
    if (threadIdx.x == 0) score[row] = dead[row] ? -INFINITY : sc;
}

// one workgroup per sequence: first maximum, the stop rule, the picked token to column t of all K rows, the picked hidden row and
// its reciprocal norm to context position t, sel[b]
__global__ __launch_bounds__(256) void contrastive_step_pick_kernel(const float* score, int K, long long* ids, int ld_ids, const int* t_dev,
                                                                    const bf16_t* hid, int d, bf16_t* ctx, long long ctx_bs,
                                                                    float* ctx_inv, int inv_bs, int Smax, int* sel, int* unfinished,
                                                                    int* n_done, int eos_id, int pad_id, int stop_later) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int t = *t_dev;
    if (t < 0 || t >= ld_ids || t >= Smax) return;
    int bi = 0;
    float bv = score[(size_t)b * K];
    for (int k = 1; k < K; k++) {
        const float v = score[(size_t)b * K + k];
        if (v > bv) { bv = v; bi = k; }             // first maximum, as torch.max; a dead candidate (-inf) never beats candidate 0
    }
    const size_t src = (size_t)b * K + bi;
    const int live = unfinished ? unfinished[(size_t)b * K] : 1;
    long long tok = ids[src * ld_ids + t];
    __syncthreads();                                // every thread has read what the K threads below overwrite
    // the stop rule of the host path: a finished sequence emits pad, a picked eos finishes it
    bool hit = false;
    if (!live) tok = pad_id;
    else if (unfinished && tok == eos_id) hit = true;
    if (tid < K) {
        ids[((size_t)b * K + tid) * ld_ids + t] = tok;
        if (hit && !stop_later) unfinished[(size_t)b * K + tid] = 0;
    }
    if (tid == 0) {
        sel[b] = bi;
        if (hit && n_done) atomicAdd(n_done, 1);
    }
    const bf16_t* h = hid + src * d;
    bf16_t* c = ctx + (size_t)b * ctx_bs + (size_t)t * d;
    for (int i = tid * 8; i < d; i += 256 * 8) *reinterpret_cast<u32x4*>(c + i) = *reinterpret_cast<const u32x4*>(h + i);
    if (tid < 64) {
        const float r = row_inv_norm_wave(h, d, tid);
        if (tid == 0) ctx_inv[(size_t)b * inv_bs + t] = r;
    }
}

// one workgroup per (head, sequence, ring): slot t mod M of the picked row into the other K - 1 rows, 16 bytes per thread and copy
__global__ __launch_bounds__(256) void ring_slot_broadcast_kernel(char* const* table, int K, int H, int M, int slot_bytes,
                                                                  const int* t_dev, const int* sel) {
    const int h = blockIdx.x, b = blockIdx.y;
    const int t = *t_dev, s = sel[b];
    if (t < 0 || s < 0 || s >= K) return;
    char* base = table[blockIdx.z];
    const long long head_bytes = (long long)M * slot_bytes, row_bytes = (long long)H * head_bytes;
    const long long off = (long long)h * head_bytes + (long long)(t % M) * slot_bytes;
    const int chunks = slot_bytes >> 4;
    const char* from = base + ((long long)b * K + s) * row_bytes + off;
    for (int i = threadIdx.x; i < chunks * K; i += 256) {
        const int k = i / chunks, c = i - k * chunks;
        if (k == s) continue;
        *reinterpret_cast<u32x4*>(base + ((long long)b * K + k) * row_bytes + off + c * 16) = *reinterpret_cast<const u32x4*>(from + c * 16);
    }
}
}  // namespace

extern "C" int mxl_contrastive_topk(const float* logp, int ldl, int V, int B, int K, const int* sel, void* ids, int ld_ids,
                                    const int* t_dev, float* probs, int* dead, const int* unfinished, int pad_id, void* stream) {
    MXL_CHECK_ARG(logp && sel && ids && t_dev && probs && dead);
    MXL_CHECK_ARG(B > 0 && K >= 2 && K <= CS_KMAX && V >= 1 && ldl >= V && ld_ids > 0);
    hipLaunchKernelGGL(contrastive_topk_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logp, ldl, V, K, sel, (long long*)ids, ld_ids,
                       t_dev, probs, dead, unfinished, pad_id);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_contrastive_step(void* ctx, long long ctx_bs, float* ctx_inv_norm, int inv_bs, int Smax, const int* t_dev,
                                    const void* hid, const float* probs, const int* dead, float alpha, int B, int K, int d, float* score,
                                    int* sel, void* ids, int ld_ids, int* unfinished, int* n_done, int eos_id, int pad_id, int stop_later,
                                    void* stream) {
    MXL_CHECK_ARG(ctx && ctx_inv_norm && t_dev && hid && probs && dead && score && sel && ids);
    MXL_CHECK_ARG(B > 0 && K >= 2 && K <= CS_KMAX && d > 0 && (d % 8) == 0 && (ctx_bs % 8) == 0 && Smax > 0 && ld_ids > 0);
    MXL_CHECK_ARG(ctx_bs >= (long long)Smax * d && inv_bs >= Smax);
    MXL_CHECK_ARG(((uintptr_t)ctx % 16) == 0 && ((uintptr_t)hid % 16) == 0);
    hipLaunchKernelGGL(contrastive_step_score_kernel, dim3(B * K), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)ctx, ctx_bs,
                       (const float*)ctx_inv_norm, inv_bs, Smax, t_dev, (const bf16_t*)hid, d, probs, dead, alpha, K, score);
    hipLaunchKernelGGL(contrastive_step_pick_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const float*)score, K, (long long*)ids,
                       ld_ids, t_dev, (const bf16_t*)hid, d, (bf16_t*)ctx, ctx_bs, ctx_inv_norm, inv_bs, Smax, sel, unfinished, n_done,
                       eos_id, pad_id, stop_later);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_ring_slot_broadcast(const void* table, int n_bufs, int B, int K, int H, int M, int dh, const int* t_dev,
                                       const int* sel, void* stream) {
    MXL_CHECK_ARG(table && t_dev && sel);
    MXL_CHECK_ARG(n_bufs >= 1 && n_bufs <= 65535 && B > 0 && B <= 65535 && K >= 2 && K <= CS_KMAX && H > 0 && M > 0);
    MXL_CHECK_ARG(dh > 0 && (dh % 8) == 0);
    hipLaunchKernelGGL(ring_slot_broadcast_kernel, dim3(H, B, n_bufs), dim3(256), 0, (hipStream_t)stream, (char* const*)table, K, H, M,
                       dh * 2, t_dev, sel);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}
