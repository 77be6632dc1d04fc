// The draw of beam-sample on the device (HF 4.25.1 `beam_sample`, as generate.beam_search(do_sample=True) states it on the host):
// every row's log-probabilities go through the warpers with min_tokens_to_keep = 2 and LogitNormalization, and every item draws
// 2 * nb of its nb * V candidates without replacement with probabilities softmax(w) -- by Gumbel-top-k: the 2 * nb largest of
// z = w - log(-log u), u a hashed uniform per candidate (include/musicxl.h, mxl_beam_sample_draw, defines the word and u).  The
// result is the matrix `drawn`: w at the drawn candidates, -inf elsewhere, which mxl_beam_sample_step walks.
//
// Two launches, no workspace:
//   beam_sample_row_kernel    one workgroup per row.  The row is sorted in LDS (value descending, ties by index), position i of
//       the order belongs to thread i / 8, and every sum over the order is a workgroup scan or reduction of fixed shape (below), so
//       that a host model can restate the rounding.  top-k cuts the order, top-p cuts it where the mass before an entry reaches
//       top_p * (the mass of the kept prefix), typical-p drops the entries with at least typical_p of mass before them in the order
//       |-log p - H| ascending; the first two entries of each warper's order always stay.  w = (key - key[0]) - log(sum).  Then
//       z for the entries that stay, the row's own 2 * nb best by 2 * nb workgroup arg-max rounds over (z, flat index) keys, and
//       their w goes to the row of `drawn`, -inf to the rest of it.  An item's 2 * nb best are among its rows' own 2 * nb best.
//   beam_sample_item_kernel   one workgroup per item.  It gathers the finite entries of the item's rows of `drawn` (at most
//       nb * 2 * nb), forms their z again -- the same function of (w, seed, counter, row, token), bit for bit -- keeps the 2 * nb
//       best and sets the others to -inf.
// The arithmetic that decides anything is written with __f*_rn so that no contraction changes it between the two kernels.
#include "common.h"
#include "beam_key.h"
#include "musicxl_internal.h"

namespace {

constexpr int BS_T = 256;                    // threads of a workgroup
constexpr int BS_N = 2048;                   // the largest vocabulary: the LDS sort
constexpr int BS_E = BS_N / BS_T;            // consecutive positions of the order a thread owns
constexpr int BS_BEAM_MAX = 16;
constexpr int BS_CAND = 2 * BS_BEAM_MAX * BS_BEAM_MAX;

// the 32-bit word of a row (every candidate of the row starts from it) and of one of its candidates; include/musicxl.h states both
__device__ __forceinline__ uint32_t bs_row_word(unsigned long long seed, unsigned long long ctr, uint32_t r) {
    const uint32_t h1 = mxl_hash32((uint32_t)(ctr * 0x9E3779B97F4A7C15ULL >> 32) ^ mxl_hash32(r + 0x85ebca6bU * (uint32_t)seed));
    return mxl_hash32(h1 + (uint32_t)ctr + (uint32_t)(seed >> 32));
}
__device__ __forceinline__ uint32_t bs_cand_word(uint32_t row_word, uint32_t v) {
    return mxl_hash32(row_word ^ (v * 0x9E3779B1U + 0x85EBCA77U));
}
// -log(-log u), u = (j + 0.5) / 2^24, j the top 24 bits of the word.  u below one half and 1 - u above it are exact in f32 (an odd
// integer below 2^24 over 2^25), so neither end of the scale loses its last bits: the term runs from -2.85 (j = 0) to 17.33.
__device__ __forceinline__ float bs_gumbel(uint32_t word) {
    const uint32_t j = word >> 8;
    float nlu;
    if (j < (1u << 23)) nlu = -logf((float)(2u * j + 1u) * (1.0f / 33554432.0f));
    else nlu = -log1pf(-((float)(2u * ((1u << 24) - j) - 1u) * (1.0f / 33554432.0f)));
    return -logf(nlu);
}
__device__ __forceinline__ float bs_z(float w, uint32_t row_word, uint32_t v) { return __fadd_rn(w, bs_gumbel(bs_cand_word(row_word, v))); }

// inclusive scan over the order of the workgroup's BS_N values, c[e] = the value at position tid * BS_E + e: a running sum inside
// the thread, a Hillis-Steele scan of the threads' totals inside the wave, the waves' totals added in wave order
__device__ __forceinline__ void bs_block_scan(float (&c)[BS_E], float* sh_red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int e = 1; e < BS_E; e++) c[e] = __fadd_rn(c[e - 1], c[e]);
    float x = c[BS_E - 1];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float y = __shfl_up(x, o, 64);
        if (lane >= o) x = __fadd_rn(y, x);
    }
    float excl = __shfl_up(x, 1, 64);
    if (lane == 0) excl = 0.f;
    if (lane == 63) sh_red[wave] = x;
    __syncthreads();
    float off = 0.f;
    for (int w = 0; w < wave; w++) off = __fadd_rn(off, sh_red[w]);
    off = __fadd_rn(off, excl);
#pragma unroll
    for (int e = 0; e < BS_E; e++) c[e] = __fadd_rn(off, c[e]);
    __syncthreads();                                                 // sh_red may be rewritten
}

// the sum of `part` over the workgroup, in every thread: a butterfly inside the wave, the four waves in order
__device__ __forceinline__ float bs_block_sum(float part, float* sh_red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part = __fadd_rn(part, __shfl_xor(part, o, 64));
    if ((tid & 63) == 0) sh_red[tid >> 6] = part;
    __syncthreads();
    const float s = __fadd_rn(__fadd_rn(__fadd_rn(sh_red[0], sh_red[1]), sh_red[2]), sh_red[3]);
    __syncthreads();
    return s;
}

__device__ __forceinline__ int bs_block_min(int x, int* sh_int) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64));
    if ((tid & 63) == 0) sh_int[tid >> 6] = x;
    __syncthreads();
    x = min(min(sh_int[0], sh_int[1]), min(sh_int[2], sh_int[3]));
    __syncthreads();
    return x;
}

__global__ __launch_bounds__(BS_T) void beam_sample_row_kernel(const float* logp, int ldl, int V, const float* beam_scores, int nb,
                                                               const unsigned long long* rng_ctr, unsigned long long seed, int top_k,
                                                               float top_p, float temperature, float typical_p, float* drawn,
                                                               float* out_warped) {
    __shared__ float key[BS_N], cum[BS_N], pp[BS_N], dev[BS_N];
    __shared__ int idx[BS_N];
    __shared__ float sh_red[BS_T / 64];
    __shared__ int sh_int[BS_T / 64];
    __shared__ unsigned long long sh_part[BS_T / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* row = logp + (size_t)r * ldl;
    float* drow = drawn + (size_t)r * ldl;
    float* wrow = out_warped ? out_warped + (size_t)r * V : nullptr;
    const bool live = beam_scores[r] != -INFINITY;
    const float invt = 1.f / temperature;
    int N = 2;
    while (N < V) N <<= 1;
    for (int i = tid; i < BS_N; i += BS_T) {
        key[i] = (live && i < V) ? __fmul_rn(row[i], invt) : -INFINITY;
        idx[i] = i;
    }
    for (int v = tid; v < V; v += BS_T) drow[v] = -INFINITY;
    __syncthreads();
    // bitonic sort of the first N entries, descending by key, ties by ascending index (a dead row is -inf throughout: it stays put)
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N; i += BS_T) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool up = ((i & k) == 0);
                    const float a = key[i], c = key[ixj];
                    const int ia = idx[i], ic = idx[ixj];
                    const bool a_first = (a > c) || (a == c && ia < ic);
                    if (up ? !a_first : a_first) {
                        key[i] = c; key[ixj] = a; idx[i] = ic; idx[ixj] = ia;
                    }
                }
            }
            __syncthreads();
        }
    }
    const float m = key[0];
    if (!(m > -INFINITY)) {                                          // a dead row, or one the rules bar whole: no candidate
        if (wrow)
            for (int v = tid; v < V; v += BS_T) wrow[v] = -INFINITY;
        return;
    }
    const int p0 = tid * BS_E;                                       // this thread's positions of the order
    int keep = top_k > 0 ? min(max(top_k, 2), V) : V;

    float c[BS_E];
#pragma unroll
    for (int e = 0; e < BS_E; e++) c[e] = p0 + e < keep ? __expf(__fsub_rn(key[p0 + e], m)) : 0.f;
    bs_block_scan(c, sh_red);
#pragma unroll
    for (int e = 0; e < BS_E; e++) cum[p0 + e] = c[e];
    __syncthreads();
    if (top_p > 0.f && top_p < 1.f) {
        // an entry stays iff the mass ordered before it is below top_p of the whole; the two best always stay
        const float thr = __fmul_rn(top_p, cum[keep - 1]);
        int first = keep;
#pragma unroll
        for (int e = BS_E - 1; e >= 0; e--) {
            const int i = p0 + e;
            if (i >= 2 && i < keep && !(cum[i - 1] < thr)) first = i;
        }
        keep = bs_block_min(first, sh_int);
    }
    float S = cum[keep - 1];

    bool drop[BS_E];
#pragma unroll
    for (int e = 0; e < BS_E; e++) drop[e] = false;
    if (typical_p > 0.f && typical_p < 1.f) {
        // HF TypicalLogitsWarper on what is left: order by |-log p - H| ascending (ties by position), an entry stays iff the mass
        // ordered before it is below typical_p; the first two of that order always stay.  No second sort: every thread
        // accumulates the mass and the count before each of its entries, over the positions in order.
        const float logs = __logf(S);
        float part = 0.f;
#pragma unroll
        for (int e = 0; e < BS_E; e++) {
            const int i = p0 + e;
            if (i < keep) {
                const float nl = __fsub_rn(__fsub_rn(key[i], m), logs);
                const float p = __expf(nl);
                pp[i] = p;
                if (p > 0.f) part = __fsub_rn(part, __fmul_rn(p, nl));
            }
        }
        const float ent = bs_block_sum(part, sh_red);
#pragma unroll
        for (int e = 0; e < BS_E; e++) {
            const int i = p0 + e;
            if (i < keep) dev[i] = fabsf(__fsub_rn(-__fsub_rn(__fsub_rn(key[i], m), logs), ent));
        }
        __syncthreads();
        float di[BS_E], before[BS_E];
        int rank[BS_E];
#pragma unroll
        for (int e = 0; e < BS_E; e++) {
            di[e] = p0 + e < keep ? dev[p0 + e] : 0.f;
            before[e] = 0.f;
            rank[e] = 0;
        }
        for (int j = 0; j < keep; j++) {
            const float dj = dev[j], pj = pp[j];
#pragma unroll
            for (int e = 0; e < BS_E; e++) {
                const bool ahead = dj < di[e] || (dj == di[e] && j < p0 + e);
                before[e] = __fadd_rn(before[e], ahead ? pj : 0.f);
                rank[e] += ahead;
            }
        }
        float kept = 0.f;
#pragma unroll
        for (int e = 0; e < BS_E; e++) {
            const int i = p0 + e;
            if (i < keep) {
                drop[e] = rank[e] >= 2 && !(before[e] < typical_p);
                if (!drop[e]) kept = __fadd_rn(kept, __expf(__fsub_rn(key[i], m)));
            }
        }
        S = bs_block_sum(kept, sh_red);
    }

    // w, the Gumbel keys of the entries that stay, and the full warped row for whoever asks
    const float logS = __logf(S);
    const uint32_t row_word = bs_row_word(seed, *rng_ctr, (uint32_t)r);
    const uint32_t jrow = (uint32_t)(r % nb);
    unsigned long long zk[BS_E];
    float w[BS_E];
#pragma unroll
    for (int e = 0; e < BS_E; e++) {
        const int i = p0 + e;
        const int v = idx[i];
        const bool stay = i < keep && !drop[e] && key[i] > -INFINITY;
        w[e] = stay ? __fsub_rn(__fsub_rn(key[i], m), logS) : -INFINITY;
        zk[e] = stay ? beam_key(bs_z(w[e], row_word, (uint32_t)v), jrow * (uint32_t)V + (uint32_t)v) : 0ull;
        if (wrow && v < V) wrow[v] = w[e];
    }
    unsigned long long prev = ~0ull;
    for (int round = 0; round < 2 * nb; round++) {
        unsigned long long best = 0;
#pragma unroll
        for (int e = 0; e < BS_E; e++)
            if (zk[e] < prev && zk[e] > best) best = zk[e];
        best = block_max_u64<BS_T>(best, sh_part);
        if (best == 0) break;                                        // fewer entries than rounds (the same in every thread)
#pragma unroll
        for (int e = 0; e < BS_E; e++)
            if (zk[e] == best) drow[idx[p0 + e]] = w[e];
        prev = best;
        __syncthreads();                                             // sh_part is rewritten by the next round
    }
}

__global__ __launch_bounds__(BS_T) void beam_sample_item_kernel(int ldl, int V, int nb, const unsigned long long* rng_ctr,
                                                                unsigned long long seed, float* drawn) {
    __shared__ unsigned long long cand[BS_CAND];
    __shared__ unsigned long long sh_part[BS_T / 64];
    __shared__ int sh_n;
    const int b = blockIdx.x, tid = threadIdx.x, row0 = b * nb;
    if (tid == 0) sh_n = 0;
    __syncthreads();
    const unsigned long long ctr = *rng_ctr;
    for (int j = 0; j < nb; j++) {
        const float* drow = drawn + (size_t)(row0 + j) * ldl;
        const uint32_t row_word = bs_row_word(seed, ctr, (uint32_t)(row0 + j));
        for (int v = tid; v < V; v += BS_T) {
            const float w = drow[v];
            if (w > -INFINITY) {
                const int at = atomicAdd(&sh_n, 1);
                if (at < BS_CAND) cand[at] = beam_key(bs_z(w, row_word, (uint32_t)v), (uint32_t)j * (uint32_t)V + (uint32_t)v);
            }
        }
    }
    __syncthreads();
    const int n = min(sh_n, BS_CAND);
    if (n <= 2 * nb) return;                                         // every candidate the rows left is drawn
    unsigned long long mine[BS_CAND / BS_T];
#pragma unroll
    for (int e = 0; e < BS_CAND / BS_T; e++) mine[e] = tid + e * BS_T < n ? cand[tid + e * BS_T] : 0ull;
    unsigned long long prev = ~0ull;
    for (int round = 0; round < 2 * nb; round++) {
        unsigned long long best = 0;
#pragma unroll
        for (int e = 0; e < BS_CAND / BS_T; e++)
            if (mine[e] < prev && mine[e] > best) best = mine[e];
        prev = block_max_u64<BS_T>(best, sh_part);
        __syncthreads();                                             // sh_part is rewritten by the next round
    }
    // what sorts after the last one drawn goes back to -inf
#pragma unroll
    for (int e = 0; e < BS_CAND / BS_T; e++) {
        if (mine[e] != 0ull && mine[e] < prev) {
            const uint32_t flat = beam_key_index(mine[e]);
            const uint32_t j = flat / (uint32_t)V;
            drawn[(size_t)(row0 + j) * ldl + (flat - j * (uint32_t)V)] = -INFINITY;
        }
    }
}

}  // namespace

extern "C" int mxl_beam_sample_draw(const float* logp, int ldl, int V, const float* beam_scores, int Bs, int nb,
                                    const unsigned long long* rng_ctr, unsigned long long seed, int top_k, float top_p,
                                    float temperature, float typical_p, float* drawn, float* out_warped, void* stream) {
    MXL_CHECK_ARG(logp && beam_scores && rng_ctr && drawn && drawn != logp);
    MXL_CHECK_ARG(V >= 2 && V <= BS_N && ldl >= V && nb >= 2 && nb <= BS_BEAM_MAX && Bs > 0);
    MXL_CHECK_ARG((long long)Bs * nb < (1LL << 31));
    MXL_CHECK_ARG(temperature > 0.f && temperature < INFINITY && top_k >= 0 && top_p > 0.f && typical_p > 0.f);
    hipLaunchKernelGGL(beam_sample_row_kernel, dim3(Bs * nb), dim3(BS_T), 0, (hipStream_t)stream, logp, ldl, V, beam_scores, nb, rng_ctr,
                       seed, top_k, top_p, temperature, typical_p, drawn, out_warped);
    MXL_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_sample_item_kernel, dim3(Bs), dim3(BS_T), 0, (hipStream_t)stream, ldl, V, nb, rng_ctr, seed, drawn);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}
