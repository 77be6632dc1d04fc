// Autoregressive decode step for Transformer-XL: everything a step needs lives on the device
// (position counter, RNG counter, token buffer), so the whole step is capture-safe and replays as a hipGraph.
//
// Upstream recomputes K/V of all mem_len memory rows every step (cat(mems, h) through qkv_net).  Because qkv_net has no
// bias, caching the *projected* K/V rows is numerically the same computation done once: a ring of M slots per layer,
// slot = position mod M.  A query at position t sees distances d = 0..M-1 (same_length window); slots never written
// are the zero mems of `init_mems` (k = v = 0): they still take softmax mass through the positional term, exactly as
// upstream, because the cache is zero-initialised and BD is evaluated for all M distances.
#include "common.h"
#include "musicxl_internal.h"
#include "contrastive_score.h"

namespace {

// h0[b] = E[ids[b][t]] * scale          (t read from device memory)
__global__ void decode_embed_kernel(const long long* ids, int ld_ids, const int* t_dev, const bf16_t* E, bf16_t* out, int B,
                                    int d, int V, float scale) {
    const int chunks = d >> 3;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= B * chunks) return;
    const int b = gid / chunks, c = gid % chunks;
    long long id = ids[(size_t)b * ld_ids + *t_dev];
    if (id < 0 || id >= V) id = 0;
    const bf16x8 e = *reinterpret_cast<const bf16x8*>(E + (size_t)id * d + c * 8);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = bf2f((bf16_t)e[j]) * scale;
    u32x4 o = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
    *reinterpret_cast<u32x4*>(out + (size_t)b * d + c * 8) = o;
}

// cache[b][t mod M] = (k, v) of the current token (rows of the (B, 3d) qkv buffer)
// ring layout is head-major (B, H, M, dh): the attention kernel of one (b, h) then streams one contiguous 2*M*dh-byte
// region instead of 128-byte pieces at a d-element stride (DRAM page locality)
// optionally also qr[b][:] = q + r_r_bias (bf16), the operand of the per-step BD product -- one launch instead of two
__global__ void kv_append_kernel(const bf16_t* qkv, bf16_t* kc, bf16_t* vc, const int* t_dev, int B, int M, int d, int dh,
                                 const float* rrb, bf16_t* qr) {
    const int chunks = d >> 3;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= B * chunks) return;
    const int b = gid / chunks, c = gid % chunks;
    if (qr) {
        const bf16x8 qv = *reinterpret_cast<const bf16x8*>(qkv + (size_t)b * 3 * d + c * 8);
        u32x4 w;
        bf16_t* wp = reinterpret_cast<bf16_t*>(&w);
#pragma unroll
        for (int j = 0; j < 8; j++) wp[j] = f2bf(bf2f((bf16_t)qv[j]) + rrb[c * 8 + j]);
        *reinterpret_cast<u32x4*>(qr + (size_t)b * d + c * 8) = w;
    }
    const int slot = (*t_dev) % M;
    const int h = (c * 8) / dh, e = (c * 8) % dh, H = d / dh;
    const u32x4 k = *reinterpret_cast<const u32x4*>(qkv + (size_t)b * 3 * d + d + c * 8);
    const u32x4 v = *reinterpret_cast<const u32x4*>(qkv + (size_t)b * 3 * d + 2 * d + c * 8);
    const size_t o = (((size_t)b * H + h) * M + slot) * dh + e;
    *reinterpret_cast<u32x4*>(kc + o) = k;
    *reinterpret_cast<u32x4*>(vc + o) = v;
}

// bulk fill after the prompt forward: cache slots (p mod M) <- K/V rows of positions p in [max(0, T-M), T)
__global__ void kv_fill_kernel(const bf16_t* qkv, bf16_t* kc, bf16_t* vc, int B, int T, int M, int d, int dh) {
    const int chunks = d >> 3;
    const int keep = min(T, M);
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)B * keep * chunks) return;
    const int c = (int)(gid % chunks);
    const int r = (int)((gid / chunks) % keep);
    const int b = (int)(gid / ((long long)chunks * keep));
    const int pos = T - keep + r;
    const int slot = pos % M;
    const bf16_t* row = qkv + ((size_t)b * T + pos) * 3 * d;
    const int h = (c * 8) / dh, e = (c * 8) % dh, H = d / dh;
    const size_t o = (((size_t)b * H + h) * M + slot) * dh + e;
    *reinterpret_cast<u32x4*>(kc + o) = *reinterpret_cast<const u32x4*>(row + d + c * 8);
    *reinterpret_cast<u32x4*>(vc + o) = *reinterpret_cast<const u32x4*>(row + 2 * d + c * 8);
}

// left-padded prompt pass: k = v = 0 in rows j < n_pad[b] of a (B, T, 3d) qkv buffer, i.e. every pad column becomes one more
// zero-memory slot (qkv_net has no bias, so a zero mem projects to k = v = 0).  Columns [d, 3d) only; queries are left alone.
// grid (ceil(T * 2d/8 / 256), B): one thread per 8 elements, n_pad read on the device (no host sync, capture-safe)
__global__ void kv_zero_pad_kernel(bf16_t* qkv, const int* n_pad, int T, int d) {
    const int chunks = (2 * d) >> 3;
    const int b = blockIdx.y;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)T * chunks) return;
    const int j = (int)(gid / chunks), c = (int)(gid % chunks);
    if (j >= n_pad[b]) return;                          // not a pad row
    *reinterpret_cast<u32x4*>(qkv + ((size_t)b * T + j) * 3 * d + d + c * 8) = u32x4{0u, 0u, 0u, 0u};
}

// BD of one decode step (mxl_decode_bd): workgroup = (256 distances, head), wave = 64 distances x all (<= 64) batch rows x dh = 64:
// 16 fragment loads straight from global memory (qr and the head's Rd columns are L2-resident), 32 MFMAs, 16-byte fp32 stores
// along the distance axis.  The batched 128 x 128-tile GEMM this replaces took 9.7 us per layer for 0.2 GFLOP.
typedef __attribute__((ext_vector_type(8))) __bf16 dec_mfma_bf16x8;
__global__ __launch_bounds__(256) void decode_bd_kernel(const bf16_t* qr, const bf16_t* rd, float* bd, int B, int H, int M,
                                                        int ld_qr, int ld_rd) {
    const int h = blockIdx.y, wid = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int r0 = blockIdx.x * 256 + wid * 64;
    if (r0 >= M) return;
    const int li = l & 15, kq = 8 * (l >> 4);
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    bf16x8 fr[4][2], fq[4][2];
#pragma unroll
    for (int f = 0; f < 4; f++)
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            const int r = r0 + f * 16 + li, b = f * 16 + li;
            fr[f][ks] = r < M ? *reinterpret_cast<const bf16x8*>(rd + (size_t)r * ld_rd + h * 64 + ks * 32 + kq) : z;
            fq[f][ks] = b < B ? *reinterpret_cast<const bf16x8*>(qr + (size_t)b * ld_qr + h * 64 + ks * 32 + kq) : z;
        }
    // acc[mf][nf][j]: b = mf*16 + (l & 15), r = r0 + nf*16 + 4*(l >> 4) + j
#pragma unroll
    for (int mf = 0; mf < 4; mf++) {
        const int b = mf * 16 + li;
#pragma unroll
        for (int nf = 0; nf < 4; nf++) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ks++)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(dec_mfma_bf16x8, fr[nf][ks]),
                                                              __builtin_bit_cast(dec_mfma_bf16x8, fq[mf][ks]), acc, 0, 0, 0);
            const int r = r0 + nf * 16 + 4 * (l >> 4);
            if (b < B && r < M) {
                float* o = bd + ((size_t)b * H + h) * M + r;
                if (r + 3 < M && (M & 3) == 0) *reinterpret_cast<f32x4*>(o) = acc;
                else
#pragma unroll
                    for (int j = 0; j < 4; j++) if (r + j < M) o[j] = acc[j];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// sampler: HF GenerationMixin.sample / greedy_search on log-probs (B, V): repetition penalty (logits processor, over every
// token already in the row) -> temperature -> top-k -> top-p -> typical-p -> renormalise -> multinomial
// (musicnlp/trainer/eval.py:277-333 builds these arguments).  One workgroup per row; bitonic sort of (value, index) in LDS
// (V <= 2048).  greedy = argmax (ties -> lowest index, like torch.argmax).
// ---------------------------------------------------------------------------------------------------------------
constexpr int SORT_N = 2048;

// token v under a row's words (rules_load below): its class under the allow word (c: a rule over classes is on), with the bar budget
// the slots the row still has free (against what the token needs: slots_need), with the key rule the pitch classes of the row's
// key.  `inkey` has bits 12..31 set, and a token
// that is no pitch has pcs 0xFF, which tests bit 31: one byte load and one shift, no branch.  `forced` >= 0 (gd: the guide group is
// on): the row is fed that token from its guide -- it alone is allowed, whatever the other groups say.  `rw` (rg: the register group
// is on): the open part's bounds as register_word packs them; a pitch passes the one unsigned compare reg[v] - lo <= hi - lo, and a
// token that is no pitch has bit 7 of its reg entry set, which is or-ed in: one byte load, no branch.
struct RegWord {
    const unsigned char* reg;
    uint32_t lo, span;
};
// A `slots` entry k (DecodeRules, budget): bits 0..14 are the slots the token takes, bit 15 says that it needs one more free than it
// takes (a sub-word token that ends on an open note start: the pitch it leaves open still needs a duration).  0xFFFF is not such a
// pair but "unknown length", beyond every rem and within BUDGET_NONE alone.  Entries without bit 15 read as they always did.
constexpr int SLOTS_RARE = 0xFFFF;
__device__ __forceinline__ int slots_take(int k) { return k & 0x7FFF; }
__device__ __forceinline__ int slots_need(int k) { return k == SLOTS_RARE ? k : (k & 0x7FFF) + (k >> 15); }
__device__ __forceinline__ bool token_allowed(const unsigned char* cls, uint32_t allow, const unsigned short* slots, int remcap,
                                              const unsigned char* pcs, uint32_t inkey, long long v, bool c, bool bud, bool ink,
                                              bool gd = false, int forced = -1, bool rg = false, RegWord rw = RegWord{nullptr, 0u, 127u}) {
    if (gd && forced >= 0) return v == forced;
    bool ok = (!c || ((allow >> cls[v]) & 1u)) && (!bud || slots_need(slots[v]) <= remcap) && (!ink || ((inkey >> (pcs[v] & 31)) & 1u));
    if (rg) {
        const uint32_t p = rw.reg[v];
        ok = ok && ((uint32_t)(p - rw.lo <= rw.span) | (p >> 7));
    }
    return ok;
}

// the row's next token (returned to every thread of the workgroup).
// G: under class rules -- a token that `gallow` (the row's allow word: its grammar state's mask less what the budget and the count
// bar) does not admit is -inf from the moment the row enters LDS and is never rewritten by the repetition penalty, which is HF's
// processor order "penalty, min_length, grammar, then the warpers": every warper and the renormalisation see allowed tokens only.
// BUD (with G): a token whose `bslots` entry exceeds `remcap` (the slots still free; 0xFFFF in an unconstrained row, which admits
// every entry) is -inf in the same place.
// INK (with or without G): a pitch token whose class `pcs` is not a bit of `inkey` (the row's key; every bit in a row without one)
// is -inf in the same place.
// GD (with G): in a row with `forced` >= 0 every token but that one is -inf in the same place, the other groups and min_length
// have no say, and the sampler -- greedy or not -- is left with a one-token support.
// RG (with or without G): a pitch token whose MIDI number lies outside the bounds `rw` of the row's open part is -inf in the same
// place.
template <bool G = false, bool BUD = false, bool INK = false, bool GD = false, bool RG = false>
__device__ __forceinline__ int sample_row(const float* logp, int ldl, int V, const long long* ids, int ld_ids,
                                          const int* t_dev, const unsigned long long* rng_ctr, unsigned long long seed,
                                          int do_sample, int top_k, float top_p, float temperature,
                                          float repetition_penalty, float typical_p, float* out_probs, int eos_id = -1,
                                          int min_length = 0, const unsigned char* gcls = nullptr, uint32_t gallow = 0u,
                                          const unsigned short* bslots = nullptr, int remcap = 0,
                                          const unsigned char* pcs = nullptr, uint32_t inkey = ~0u, int forced = -1,
                                          RegWord rw = RegWord{nullptr, 0u, 127u}) {
    __shared__ float key[SORT_N];
    __shared__ int idx[SORT_N];
    __shared__ int sh_pick;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = logp + (size_t)b * ldl;
    const float invt = 1.f / temperature;
    for (int i = tid; i < SORT_N; i += 256) {
        if (G || INK || RG) key[i] = (i < V && token_allowed(gcls, gallow, bslots, remcap, pcs, inkey, i, G, BUD, INK, GD, forced, RG, rw)) ? row[i] * invt : -INFINITY;
        else key[i] = i < V ? row[i] * invt : -INFINITY;
        idx[i] = i;
    }
    __syncthreads();
    if (repetition_penalty != 1.f) {
        // HF RepetitionPenaltyLogitsProcessor: every id present in the row so far (prompt + generated, positions 0..t) has its
        // raw score multiplied (score < 0) or divided (score >= 0) by the penalty, once however often it occurs -- the writes
        // below all store the same value, so duplicates are harmless.
        const int tcur = *t_dev;
        const long long* hist = ids + (size_t)b * ld_ids;
        for (int j = tid; j <= tcur; j += 256) {
            const long long tok = hist[j];
            if (tok >= 0 && tok < V && (!(G || INK || RG) || token_allowed(gcls, gallow, bslots, remcap, pcs, inkey, tok, G, BUD, INK, GD, forced, RG, rw))) {
                const float v = row[tok];
                key[tok] = (v < 0.f ? v * repetition_penalty : v / repetition_penalty) * invt;
            }
        }
        __syncthreads();
    }
    if (min_length > 0 && eos_id >= 0 && eos_id < V && !(GD && forced >= 0)) {
        // HF MinLengthLogitsProcessor (after the repetition penalty, before the warpers): eos is barred while the row is
        // shorter than min_length -- the row holds columns 0..t, t + 1 of them
        if (tid == 0 && *t_dev + 1 < min_length) key[eos_id] = -INFINITY;
        __syncthreads();
    }
    // Small supports (greedy, or top-k <= 64) need only the first few entries of the sorted order: take them by repeated
    // workgroup arg-max (same order as the sort: value descending, ties by ascending index) -- 2 barriers per entry instead of
    // the 66 barrier stages of the full sort.
    const int nsel = !do_sample ? 1 : ((top_k > 0 && top_k <= 64 && top_k < V) ? top_k : 0);
    if (nsel > 0) {
        __shared__ float wbest[4];
        __shared__ int warg[4];
        float vals[SORT_N / 256];
#pragma unroll
        for (int e = 0; e < SORT_N / 256; e++) vals[e] = key[tid + 256 * e];
        __syncthreads();                                  // everyone has its copy before key[] is overwritten with the selection
        for (int rnd = 0; rnd < nsel; rnd++) {
            float bv = -INFINITY;
            int bi = 0x7fffffff;
#pragma unroll
            for (int e = 0; e < SORT_N / 256; e++) {
                const int gi = tid + 256 * e;
                if (gi < V && (vals[e] > bv || (vals[e] == bv && gi < bi))) { bv = vals[e]; bi = gi; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if ((tid & 63) == 0) { wbest[tid >> 6] = bv; warg[tid >> 6] = bi; }
            __syncthreads();
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const float ov = wbest[w];
                const int oi = warg[w];
                if (w == 0 || ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if (bi == 0x7fffffff) bi = 0;                 // every remaining value is -inf
            if ((bi & 255) == tid) {
#pragma unroll
                for (int e = 0; e < SORT_N / 256; e++) if (e == (bi >> 8)) vals[e] = -INFINITY;
            }
            if (tid == 0) { key[rnd] = bv; idx[rnd] = bi; }
            __syncthreads();
        }
    } else
    // bitonic sort, descending by key, ties by ascending index
    for (int k = 2; k <= SORT_N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < SORT_N; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool up = ((i & k) == 0);
                    const float a = key[i], c = key[ixj];
                    const int ia = idx[i], ic = idx[ixj];
                    const bool a_first = (a > c) || (a == c && ia < ic);   // a should come before c in descending order
                    if (up ? !a_first : a_first) {
                        key[i] = c; key[ixj] = a; idx[i] = ic; idx[ixj] = ia;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (!do_sample) {
        if (tid == 0) sh_pick = idx[0];
        __syncthreads();
        return sh_pick;
    }
    int keep = (top_k > 0 && top_k < V) ? top_k : V;
    __shared__ int sh_keep;
    __shared__ float sh_sum, sh_max;       // the head of the order can itself be dropped as atypical: keep its value
    // softmax over the kept prefix (max is key[0]); serial prefix over <= V terms by one thread is negligible here
    if (tid == 0) {
        const float m = key[0];
        float s = 0.f;
        for (int i = 0; i < keep; i++) s += __expf(key[i] - m);
        if (top_p > 0.f && top_p < 1.f) {
            // HF TopPLogitsWarper: keep the smallest prefix whose cumulative probability exceeds top_p (>= 1 token)
            float c = 0.f;
            int kk = 0;
            for (int i = 0; i < keep; i++) {
                c += __expf(key[i] - m) / s;
                kk = i + 1;
                if (c >= top_p) break;
            }
            keep = kk;
            s = 0.f;
            for (int i = 0; i < keep; i++) s += __expf(key[i] - m);
        }
        sh_keep = keep;
        sh_sum = s;
        sh_max = m;
    }
    if (typical_p > 0.f && typical_p < 1.f) {
        // HF TypicalLogitsWarper on the surviving support: order the tokens by |-log p - H| ascending and keep the shortest
        // prefix of that order whose mass reaches typical_p, i.e. token i stays iff the mass of the tokens ordered before it
        // is below typical_p.  No second sort: each thread accumulates that "mass before" for its own entries.
        __shared__ float pp[SORT_N], dev[SORT_N];
        __shared__ float red[4];
        __syncthreads();
        keep = sh_keep;
        const float m = sh_max, logs = __logf(sh_sum);
        float part = 0.f;
        for (int i = tid; i < keep; i += 256) {
            const float nl = key[i] - m - logs;
            const float p = __expf(nl);
            pp[i] = p;
            if (p > 0.f) part -= p * nl;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
        if ((tid & 63) == 0) red[tid >> 6] = part;
        __syncthreads();
        const float ent = red[0] + red[1] + red[2] + red[3];
        for (int i = tid; i < keep; i += 256) dev[i] = fabsf(-(key[i] - m - logs) - ent);
        __syncthreads();
        bool drop[SORT_N / 256];
#pragma unroll
        for (int e = 0; e < SORT_N / 256; e++) {
            const int i = tid + 256 * e;
            drop[e] = false;
            if (i < keep) {
                const float di = dev[i];
                float before = 0.f;
                for (int j = 0; j < keep; j++) {
                    const float dj = dev[j];
                    before += (dj < di || (dj == di && j < i)) ? pp[j] : 0.f;
                }
                drop[e] = before >= typical_p;
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < SORT_N / 256; e++)
            if (drop[e]) key[tid + 256 * e] = -INFINITY;
        __syncthreads();
        if (tid == 0) {
            float s = 0.f;
            for (int i = 0; i < keep; i++) s += __expf(key[i] - m);
            sh_sum = s;
        }
    }
    if (tid == 0) {
        keep = sh_keep;
        const float m = sh_max, s = sh_sum;
        // uniform in [0,1) from a counter-based hash (counter advanced by the advance kernel)
        const unsigned long long ctr = *rng_ctr;
        const uint32_t h1 = mxl_hash32((uint32_t)(ctr * 0x9E3779B97F4A7C15ULL >> 32) ^ mxl_hash32((uint32_t)b + 0x85ebca6bU * (uint32_t)seed));
        const uint32_t h2 = mxl_hash32(h1 + (uint32_t)ctr + (uint32_t)(seed >> 32));
        const float u = (float)(h2 >> 8) * (1.0f / 16777216.0f);
        float c = 0.f;
        int pick = -1, last = 0;
        for (int i = 0; i < keep; i++) {
            const float p = __expf(key[i] - m) / s;
            if (p > 0.f) last = i;
            c += p;
            if (u < c && p > 0.f) { pick = i; break; }
        }
        if (pick < 0) pick = last;
        sh_pick = idx[pick];
        if (out_probs) {   // diagnostic / test hook: renormalised probabilities of the kept support, in vocab order
            for (int i = 0; i < V; i++) out_probs[(size_t)b * V + i] = 0.f;
            for (int i = 0; i < keep; i++) out_probs[(size_t)b * V + idx[i]] = __expf(key[i] - m) / s;
        }
    }
    __syncthreads();
    return sh_pick;
}

// ---------------------------------------------------------------------------------------------------------------
// The rules of one generation (include/musicxl.h, "Rules of a generation"), passed to kernels by value.  Eight groups, each off when
// its state pointer (unfinished / gstate / gbar / gleft / gkey / gpos / gpart / gcopy) is NULL; the budget, the count, the guide and
// the repeat read the token classes `cls` of the grammar group and nothing else of it, the key and the register read nothing of it at
// all.
//   stop     HF greedy_search / sample: a finished row emits pad, a live row that emits eos is finished; eos barred below min_length
//   grammar  a token class automaton: cls (V,) token -> class, allow (S,) bit c = class c may follow in state s, next (S, C) successor
//   budget   grammar.BarBudget: per row `bar` (bar length in slots, 0 = unconstrained) and `rem` (slots still free in the open
//            channel).  slots (V,) uint16: duration token -> slots, 0 = no duration, 0xFFFF = unknown length; bars (V,) uint16: time
//            signature token -> bar length, 0xFFFF = no time signature; opens / need_free / need_full: class bit masks.  Any other
//            slots entry is a pair: bits 0..14 = the slots the token takes from rem, bit 15 = it needs one more free than it takes
//            (grammar.subword_grammar: a token over several base tokens that ends on an open note start); read by slots_take /
//            slots_need in token_allowed, budget_move and budget_scan_kernel and nowhere else
//   count    grammar.BarCount: per row `left`, the bars the row may still open (< 0 = no limit, the row is untouched).  A class in
//            `count` (<bar>) is barred at left == 0, a class in `end` (</s>) while left > 0, and a kept token of a `count` class
//            takes 1 from a positive left
//   key      grammar.KeyRule: per row `key`, the ordinal 0..23 of the row's key (< 0 = none, the row is untouched).  keys (V,) uint8:
//            Key_* token -> ordinal, 0xFF = no key token; pcs (V,) uint8: pitch token -> pitch class 0..11, 0xFF = no pitch (rests and
//            the rare pitch included); inkey (24,) uint16: bit pc = pitch class pc belongs to the key.  A pitch outside the row's key is
//            barred, and a kept key token sets the row's key
//   guide    grammar.MelodyGuide: per row `pos`, the next index into the row's guide, and `force`, 1 = the row is fed from its guide.
//            guide (B, ld_guide) int32: the rows' guide tokens; glen (B,) int32: their lengths, 0 = no guide, the row is untouched;
//            enter / leave: class bit masks (<bar> / <bass>).  A row with force == 1 and pos < glen may emit guide[b][pos] alone, and
//            that token is never barred: the group overrides every other one and min_length.  A kept token under force takes pos one
//            on and, if its class is in `leave`, clears force; a kept `enter` token of a free row with pos < glen sets force and
//            takes pos one on (it is the guide's own <bar>)
//   register grammar.RegisterRule: per row `range` (the bounds lo_melody, hi_melody, lo_bass, hi_bass as MIDI numbers, one byte each
//            from the lowest; fixed for the generation), `part` (0 = no open part, 1 = melody, 2 = bass) and `floor` (the lowest melody
//            pitch of the open bar, 128 = none yet).  reg (V,) uint8: pitch token -> MIDI number 0..127, <melody> / <bass> / <bar> ->
//            REG_MELODY / REG_BASS / REG_BAR, 0xFF = anything else (rests and the rare pitch included).  A pitch outside the open
//            part's bounds is barred; in the bass, with gap >= 0 and a floor, the upper bound is min(hi_bass, floor - gap).  A kept part
//            token sets part, <bar> clears part and floor, a melody pitch lowers floor
//   repeat   grammar.BarRepeat: per row `bars` (generated bars opened so far), `copy` (the column of the row's own history the next
//            token is copied from, -1 = the row chooses) and `stop` (the column where the copy ends, exclusive).  plan (B, ld_plan)
//            int32: plan[b][k] = -1, bar k is free, or j < k, bar k repeats generated bar j; nplan (B,) int32: planned bars, 0 = the
//            row is untouched; barcol (B, ld_plan) int32, written here: the column of the `enter` token of generated bar k; renter /
//            rleave: class bit masks (<bar> / <bass>); span: 0 = the whole bar is copied, 1 = up to its first `leave` token; hist
//            (B, ld_hist) int64: the rows' ids.  A row with copy >= 0 may emit hist[b][copy] alone, as under the guide; a kept token
//            under copy takes copy one on and ends the copy at `stop` or, under span 1, at a `leave` token; a kept `enter` token of a
//            free row with bars < nplan records its column and, if the plan names a source, starts the copy behind the source's
//            `enter` token
// The next rule is one more group of mxl_rules, one line in each of rules_load / rules_move and one in make_rules.
// ---------------------------------------------------------------------------------------------------------------
using DecodeRules = mxl_rules;               // the struct of the C ABI is the kernels' argument: no second layout, no copy step

constexpr int BUDGET_NONE = 0xFFFF;          // slots: unknown length (beyond any rem); bars: not a time signature

// classes a row at (bar, rem) bars: the closers while slots are free, the note starters once none is
__device__ __forceinline__ uint32_t budget_deny(int bar, int rem, uint32_t need_free, uint32_t need_full) {
    return bar > 0 ? (rem > 0 ? need_full : need_free) : 0u;
}
// the largest need (slots_need) the row admits
__device__ __forceinline__ int budget_remcap(int bar, int rem) { return bar > 0 ? rem : BUDGET_NONE; }
// (bar, rem) after a token of class c with slots entry k and bars entry sig (BarBudget.move): the token takes slots_take(k)
__device__ __forceinline__ void budget_move(int& bar, int& rem, int c, int k, int sig, uint32_t opens) {
    if (sig != BUDGET_NONE) { bar = sig; rem = 0; }
    if ((opens >> c) & 1u) rem = bar;
    if (bar > 0 && k != BUDGET_NONE) rem = max(rem - slots_take(k), 0);
}
// classes a row with `left` bars to go bars: the end while bars are owed, another bar once none is
__device__ __forceinline__ uint32_t barcount_deny(int left, uint32_t count, uint32_t end) {
    return left > 0 ? end : (left == 0 ? count : 0u);
}
// left after a token of class c (BarCount.move)
__device__ __forceinline__ int barcount_move(int left, int c, uint32_t count) {
    return (left > 0 && ((count >> c) & 1u)) ? left - 1 : left;
}
constexpr int N_KEYS = 24;
constexpr uint32_t KEY_ANY = ~0u;            // the pitch-class word of a row without a key
constexpr int KEY_NONE = 0xFF;               // keys: no key token; pcs: no pitch
// the pitch classes a row in `key` admits, as token_allowed reads them: bits 0..11 from the table, every bit above them set
__device__ __forceinline__ uint32_t key_word(const unsigned short* inkey, int key) {
    return (unsigned)key < (unsigned)N_KEYS ? ((uint32_t)inkey[key] | 0xFFFFF000u) : KEY_ANY;
}
constexpr int REG_MELODY = 0x80, REG_BASS = 0x81, REG_BAR = 0x82;   // reg: the tokens that move the row's part
constexpr int FLOOR_NONE = 128;              // gfloor: no melody pitch in the open bar yet
// the bounds of a row in `part` under `range`, `floor` and `gap`, as token_allowed reads them: lo and hi - lo; bounds that leave no
// pitch (the floor under lo_bass) become lo = 256, which no reg entry reaches -- the rest and the rare pitch stay, see musicxl.h
__device__ __forceinline__ RegWord register_word(const unsigned char* reg, uint32_t range, int part, int floor, int gap) {
    int lo = 0, hi = 127;
    if (part == 1) { lo = range & 0xFF; hi = (range >> 8) & 0xFF; }
    else if (part == 2) {
        lo = (range >> 16) & 0xFF;
        hi = (range >> 24) & 0xFF;
        if (gap >= 0 && floor < FLOOR_NONE) hi = min(hi, floor - gap);
    }
    return hi >= lo ? RegWord{reg, (uint32_t)lo, (uint32_t)(hi - lo)} : RegWord{reg, 256u, 0u};
}
// (part, floor) after a token with reg entry p (RegisterRule.move)
__device__ __forceinline__ void register_move(int& part, int& floor, int p) {
    if (p == REG_MELODY) part = 1;
    else if (p == REG_BASS) part = 2;
    else if (p == REG_BAR) { part = 0; floor = FLOOR_NONE; }
    else if (p < 128 && part == 1) floor = min(floor, p);
}

// The words of row b and what they admit: `allow` has a bit per class the row may emit (every bit without a grammar), `remcap` is
// the largest slots entry, `inkey` a bit per pitch class (key_word), `forced` the token the row is fed at this step, from its guide or
// (rp) from its own history (-1 = none: the row chooses), `rw` the bounds of the open part (register_word).  g / bud / cnt / ink / gd /
// rg / rp: which groups are on -- compile-time constants in the fused kernel, pointer tests in the unfused pair; everything here
// inlines and folds on them.
struct RowWords {
    int gs, bar, rem, left;
    uint32_t allow;
    int remcap;
    uint32_t inkey;
    int pos, force, forced;
    int part, floor;
    RegWord rw;
    int nplan, nbars, copy, cstop;
};
__device__ __forceinline__ RowWords rules_load(const DecodeRules& r, int b, bool g, bool bud, bool cnt, bool ink, bool gd = false,
                                               bool rg = false, bool rp = false) {
    RowWords w{0, 0, 0, -1, ~0u, BUDGET_NONE, KEY_ANY, 0, 0, -1, 0, FLOOR_NONE, RegWord{nullptr, 0u, 127u}, 0, 0, -1, 0};
    if (g) { w.gs = r.gstate[b]; w.allow = r.allow[w.gs]; }
    if (bud) {
        w.bar = r.gbar[b];
        w.rem = r.grem[b];
        w.allow &= ~budget_deny(w.bar, w.rem, r.need_free, r.need_full);
        w.remcap = budget_remcap(w.bar, w.rem);
    }
    if (cnt) { w.left = r.gleft[b]; w.allow &= ~barcount_deny(w.left, r.count, r.end); }
    if (ink) w.inkey = key_word(r.inkey, r.gkey[b]);
    if (gd) {
        w.pos = r.gpos[b];
        w.force = r.gforce[b];
        if (w.force && w.pos >= 0 && w.pos < min(r.glen[b], r.ld_guide)) w.forced = r.guide[(size_t)b * r.ld_guide + w.pos];
    }
    if (rg) {
        w.part = r.gpart[b];
        w.floor = r.gfloor[b];
        w.rw = register_word(r.reg, (uint32_t)r.grange[b], w.part, w.floor, r.gap);
    }
    if (rp) {                                        // the copy reads a column the row wrote in an earlier launch: copy < stop <= t + 1
        w.nplan = min(r.nplan[b], r.ld_plan);
        w.nbars = r.gbars[b];
        w.copy = r.gcopy[b];
        w.cstop = r.gstop[b];
        if (w.nplan > 0 && w.copy >= 0 && w.copy < r.ld_hist) {
            const long long tk = r.hist[(size_t)b * r.ld_hist + w.copy];
            w.forced = (tk >= 0 && tk <= 0x7fffffffLL) ? (int)tk : -1;
        }
    }
    return w;
}
// row b moves along `tok`, a token of the vocabulary that the row chose itself (a row finished before the step emits pad, which is
// not its choice and need not be a token its state allows: such a row keeps its words)
// `col` (rp): the column of the row's history that `tok` is written at
__device__ __forceinline__ void rules_move(const DecodeRules& r, RowWords w, int b, long long tok, bool g, bool bud, bool cnt, bool ink,
                                           bool gd = false, bool rg = false, int col = 0, bool rp = false) {
    const int c = (g || bud || cnt || gd || rp) ? r.cls[tok] : 0;
    if (g) r.gstate[b] = r.next[w.gs * r.C + c];
    if (bud) {
        budget_move(w.bar, w.rem, c, r.slots[tok], r.bars[tok], r.opens);
        r.gbar[b] = w.bar;
        r.grem[b] = w.rem;
    }
    if (cnt) r.gleft[b] = barcount_move(w.left, c, r.count);
    if (ink) {
        const int k = r.keys[tok];
        if (k != KEY_NONE) r.gkey[b] = k;            // KeyRule.move: a key token sets the row's key, nothing else changes it
    }
    if (gd) {                                        // MelodyGuide.move
        if (w.force) {
            r.gpos[b] = w.pos + 1;
            if ((r.leave >> c) & 1u) r.gforce[b] = 0;
        } else if (((r.enter >> c) & 1u) && w.pos < r.glen[b]) {
            r.gpos[b] = w.pos + 1;
            r.gforce[b] = 1;
        }
    }
    if (rg) {                                        // RegisterRule.move
        register_move(w.part, w.floor, r.reg[tok]);
        r.gpart[b] = w.part;
        r.gfloor[b] = w.floor;
    }
    if (rp) {                                        // BarRepeat.move
        if (w.copy >= 0) {
            const int nc = w.copy + 1;
            r.gcopy[b] = (nc >= w.cstop || (r.span == 1 && ((r.rleave >> c) & 1u))) ? -1 : nc;
        } else if (((r.renter >> c) & 1u) && w.nbars >= 0 && w.nbars < w.nplan) {
            const int k = w.nbars;
            int* cols = r.barcol + (size_t)b * r.ld_plan;
            cols[k] = col;
            r.gbars[b] = k + 1;
            const int j = r.plan[(size_t)b * r.ld_plan + k];
            if (j >= 0 && j < k) {
                const int from = cols[j] + 1, stop = (j + 1 == k) ? col : cols[j + 1];
                if (from >= 1 && from < stop && stop <= col) { r.gcopy[b] = from; r.gstop[b] = stop; }
            }
        }
    }
}

__global__ __launch_bounds__(256) void sample_kernel(const float* logp, int ldl, int V, long long* ids, int ld_ids,
                                                     const int* t_dev, unsigned long long* rng_ctr, unsigned long long seed,
                                                     int do_sample, int top_k, float top_p, float temperature,
                                                     float repetition_penalty, float typical_p, float* out_probs) {
    const int tok = sample_row(logp, ldl, V, ids, ld_ids, t_dev, rng_ctr, seed, do_sample, top_k, top_p, temperature,
                               repetition_penalty, typical_p, out_probs);
    if (threadIdx.x == 0) ids[(size_t)blockIdx.x * ld_ids + *t_dev + 1] = tok;
}

// Round 6: the sampler with the two launches that always follow it.  The sampled token's embedding row E[tok] * scale -- the input
// of the NEXT decode step (mxl_decode_embed's arithmetic) -- is written by the row's workgroup, and the workgroup that finishes last
// advances the position and RNG counters (mxl_decode_advance): every other workgroup has read them by then.  `scores` may be the
// head's raw logits instead of log-probabilities when no repetition penalty is in force: every other warper, the argmax and the
// renormalised draw are invariant under the per-row shift log-softmax applies.
//
// G / BUD / CNT / INK / GD / RG / RP: the grammar, budget, count, key, guide, register and repeat groups of `r` as compile-time
// variants (BUD, CNT, GD and RP ride on G, INK and RG stand alone; RP feeds its token through the sampler's GD arm and is never on
// beside GD); the stop group is the runtime test of r.unfinished it has always been.  The row's words
// select the allow word, remcap, the key's pitch classes and the open part's bounds the sampler applies (rules_load), and thread 0 moves them along the token the row keeps (rules_move).  The move sits AFTER the eos rule: a row that
// was finished before this step emits pad and its words stay frozen; the step in which a live row emits eos still moves them, so a
// finished row of the music grammar rests in END.  The words are per-row: row b's workgroup is their only reader and writer within a
// launch, and the next launch on the stream sees them by stream order -- there is no hand-off between workgroups here beyond the
// arrival counter below.
template <bool G, bool BUD, bool CNT, bool INK, bool GD, bool RG, bool RP = false>
__global__ __launch_bounds__(256) void sample_step_kernel(const float* scores, int ldl, int V, long long* ids, int ld_ids,
                                                          int* t_dev, unsigned long long* rng_ctr, unsigned long long seed,
                                                          int do_sample, int top_k, float top_p, float temperature,
                                                          float repetition_penalty, float typical_p, const bf16_t* E, bf16_t* emb_out,
                                                          int d, float scale, int* counter, float* out_probs, DecodeRules r) {
    static_assert(G || !(BUD || CNT || GD || RP), "the bar budget, the bar count, the guide and the repeat ride on the grammar");
    static_assert(!(GD && RP), "a row is fed from its guide or from its own history, not both");
    int* const unfinished = r.unfinished;
    const RowWords w = rules_load(r, blockIdx.x, G, BUD, CNT, INK, GD, RG, RP);
    int tok = sample_row<G, BUD, INK, GD || RP, RG>(scores, ldl, V, ids, ld_ids, t_dev, rng_ctr, seed, do_sample, top_k, top_p, temperature,
                                      repetition_penalty, typical_p, out_probs, unfinished ? r.eos_id : -1,
                                      unfinished ? r.min_length : 0, r.cls, w.allow, r.slots, w.remcap, r.pcs, w.inkey, w.forced, w.rw);
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ int sh_tok, sh_live;
    bool was_live = true;                       // (thread 0) the token is the row's own choice
    if (unfinished) {
        // stop state (HF greedy_search / sample): a finished row emits pad; a live row that emits eos is finished from now on
        if (tid == 0) {
            int live = unfinished[b];
            int tk = tok;
            was_live = live != 0;
            if (!live) tk = r.pad_id;
            else if (tk == r.eos_id) live = 0;
            unfinished[b] = live;
            sh_tok = tk;
            sh_live = live;
        }
        __syncthreads();
        tok = sh_tok;
    }
    if ((G || INK || RG) && tid == 0 && was_live && tok >= 0 && tok < V)
        rules_move(r, w, b, tok, G, BUD, CNT, INK, GD, RG, RP ? *t_dev + 1 : 0, RP);
    if (tid == 0) ids[(size_t)b * ld_ids + *t_dev + 1] = tok;
    const int id = (tok < 0 || tok >= V) ? 0 : tok;
    for (int c = tid; c < (d >> 3); c += 256) {
        const bf16x8 e = *reinterpret_cast<const bf16x8*>(E + (size_t)id * d + c * 8);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = bf2f((bf16_t)e[j]) * scale;
        const u32x4 o = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
        *reinterpret_cast<u32x4*>(emb_out + (size_t)b * d + c * 8) = o;
    }
    __syncthreads();                            // every thread of the workgroup is past its reads of *t_dev / *rng_ctr
    if (tid == 0 && unfinished) {
        // arrival and the row's live bit in one atomic word (arrivals in bits 0-15, live rows from bit 16): the last arrival
        // takes the number of live rows from the value it gets back, no other memory is read across workgroups
        const int old = __hip_atomic_fetch_add(counter, 1 + (sh_live << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((old & 0xffff) == (int)gridDim.x - 1) {
            __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *r.alive = (old >> 16) + sh_live;
            *t_dev += 1;
            *rng_ctr += 1;
        }
    } else if (tid == 0) {
        const int old = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == (int)gridDim.x - 1) {
            __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *t_dev += 1;
            *rng_ctr += 1;
        }
    }
}

__global__ void advance_kernel(int* t_dev, unsigned long long* rng_ctr) {
    *t_dev += 1;
    *rng_ctr += 1;
}

// ---------------------------------------------------------------------------------------------------------------
// The same rules around the samplers that do not carry them (mxl_sample, mxl_sample_large: the unfused, large-vocabulary and
// Reformer paths): one launch before the sampler and one after it and the counter advance.
// ---------------------------------------------------------------------------------------------------------------
// before the sampler: -inf on every token that an enabled group bars, eos below min_length (rows hold columns 0..*t_dev) included;
// one thread per score, every other score untouched.  The sampler's repetition penalty leaves -inf at -inf, so the result is that of
// masking after the penalty.
__global__ __launch_bounds__(256) void rules_mask_kernel(float* scores, int ldl, int B, int V, const int* t_dev, DecodeRules r) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * V) return;
    const int b = (int)(i / V), v = (int)(i - (long long)b * V);
    const bool bud = r.gbar != nullptr, ink = r.gkey != nullptr, gd = r.gpos != nullptr, rg = r.gpart != nullptr;
    const bool rp = r.gcopy != nullptr;
    bool ok = true;
    int forced = -1;
    if (r.cls || ink || rg) {
        const RowWords w = rules_load(r, b, r.gstate != nullptr, bud, r.gleft != nullptr, ink, gd, rg, rp);
        ok = token_allowed(r.cls, w.allow, r.slots, w.remcap, r.pcs, w.inkey, v, r.cls != nullptr, bud, ink, gd || rp, w.forced, rg, w.rw);
        forced = w.forced;
    }
    if (forced < 0 && r.min_length > 0 && v == r.eos_id && *t_dev + 1 < r.min_length) ok = false;
    if (!ok) scores[(size_t)b * ldl + v] = -INFINITY;
}

// after the sampler and the counter advance: the token just written sits at column *t_dev.  One workgroup walks the rows: a row that
// chose its token (live before the step, or no stop group) moves its words along it, then the stop rule is applied to the token --
// `unfinished` still tells which rows were live when they chose it -- and the number of live rows goes to *alive.
__global__ __launch_bounds__(256) void rules_advance_kernel(long long* ids, int ld_ids, const int* t_dev, int B, int V, DecodeRules r) {
    __shared__ int part[4];
    const int tid = threadIdx.x;
    const int t = *t_dev;
    const bool g = r.gstate != nullptr, bud = r.gbar != nullptr, cnt = r.gleft != nullptr, ink = r.gkey != nullptr;
    const bool gd = r.gpos != nullptr, rg = r.gpart != nullptr, rp = r.gcopy != nullptr;
    int n = 0;
    for (int b = tid; b < B; b += 256) {
        long long* p = ids + (size_t)b * ld_ids + t;
        const long long tok = *p;
        int live = r.unfinished ? r.unfinished[b] : 1;
        if (live && (r.cls || ink || rg) && tok >= 0 && tok < V)
            rules_move(r, rules_load(r, b, g, bud, cnt, ink, gd, rg, rp), b, tok, g, bud, cnt, ink, gd, rg, t, rp);
        if (r.unfinished) {
            if (!live) *p = r.pad_id;
            else if (tok == r.eos_id) live = 0;
            r.unfinished[b] = live;
            n += live;
        }
    }
    if (!r.unfinished) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) *r.alive = part[0] + part[1] + part[2] + part[3];
}

// state of every row after its prompt.  One wave per row: the lanes load 64 columns at a time and their classes, then every lane
// walks the 64 classes (the walk is uniform over the wave: table look-ups only, no dependent load of ids).  Columns holding an id
// < 0 are skipped (left pads); first_bad[b] = column of the first token the state bars (or beyond the vocabulary), -1 = none.
__global__ __launch_bounds__(64) void grammar_scan_kernel(const long long* ids, int ld_ids, int Tp, int B, int V,
                                                          const unsigned char* cls, const uint32_t* allow,
                                                          const unsigned char* next, int C, int start, int* gstate,
                                                          int* first_bad) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long* row = ids + (size_t)b * ld_ids;
    int s = start, bad = -1;
    for (int base = 0; base < Tp && bad < 0; base += 64) {
        const int col = base + lane;
        int c = -1;                                              // -1 skip, -2 outside the vocabulary
        if (col < Tp) {
            const long long tok = row[col];
            if (tok >= V) c = -2;
            else if (tok >= 0) c = cls[tok];
        }
        const int n = min(64, Tp - base);
        for (int j = 0; j < n; j++) {
            const int cj = __shfl(c, j, 64);
            if (cj == -1) continue;
            if (cj < 0 || !((allow[s] >> cj) & 1u)) { bad = base + j; break; }
            s = next[s * C + cj];
        }
    }
    if (lane == 0) { gstate[b] = s; first_bad[b] = bad; }
}

// (bar, rem) of every row after its prompt, as grammar_scan_kernel: one wave per row, 64 columns at a time, the walk uniform over
// the wave.  Ids < 0 (left pads) and ids beyond the vocabulary (the grammar scan reports those) are skipped; first_bad[b] = column
// of the first token the budget bars, -1 = none.
__global__ __launch_bounds__(64) void budget_scan_kernel(const long long* ids, int ld_ids, int Tp, int B, int V,
                                                         const unsigned char* cls, const unsigned short* slots,
                                                         const unsigned short* bars, uint32_t opens, uint32_t need_free,
                                                         uint32_t need_full, int* gbar, int* grem, int* first_bad) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long* row = ids + (size_t)b * ld_ids;
    int bar = 0, rem = 0, bad = -1;
    for (int base = 0; base < Tp && bad < 0; base += 64) {
        const int col = base + lane;
        int c = -1, ks = 0;                                      // c = -1: skip; ks = slots entry | bars entry << 16
        if (col < Tp) {
            const long long tok = row[col];
            if (tok >= 0 && tok < V) { c = cls[tok]; ks = (int)slots[tok] | ((int)bars[tok] << 16); }
        }
        const int n = min(64, Tp - base);
        for (int j = 0; j < n; j++) {
            const int cj = __shfl(c, j, 64);
            const int kj = __shfl(ks, j, 64);
            if (cj < 0) continue;
            const int k = kj & 0xFFFF, sig = (kj >> 16) & 0xFFFF;
            if (((budget_deny(bar, rem, need_free, need_full) >> cj) & 1u) || slots_need(k) > budget_remcap(bar, rem)) { bad = base + j; break; }
            budget_move(bar, rem, cj, k, sig, opens);
        }
    }
    if (lane == 0) { gbar[b] = bar; grem[b] = rem; first_bad[b] = bad; }
}

// key of every row after columns 0..Tp-1, from the key gkey[b] holds at the launch (KeyRule.walk), as the two scans above: one wave
// per row, 64 columns at a time.  Ids < 0 (left pads) and ids beyond the vocabulary are skipped.  Columns before `from` only move the
// key (a prompt supplies its key, its pitches are not judged); first_bad[b] = the first column >= from holding a pitch outside the
// row's key, where the walk of that row stops, -1 = none.
__global__ __launch_bounds__(64) void key_scan_kernel(const long long* ids, int ld_ids, int Tp, int from, int B, int V,
                                                      const unsigned char* keys, const unsigned char* pcs,
                                                      const unsigned short* inkey, int* gkey, int* first_bad) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long* row = ids + (size_t)b * ld_ids;
    int key = gkey[b], bad = -1;
    for (int base = 0; base < Tp && bad < 0; base += 64) {
        const int col = base + lane;
        int kp = KEY_NONE | (KEY_NONE << 8);                     // keys entry | pcs entry << 8
        if (col < Tp) {
            const long long tok = row[col];
            if (tok >= 0 && tok < V) kp = (int)keys[tok] | ((int)pcs[tok] << 8);
        }
        const int n = min(64, Tp - base);
        for (int j = 0; j < n; j++) {
            const int kj = __shfl(kp, j, 64);
            const int k = kj & 0xFF, pc = kj >> 8;
            if (base + j >= from && !((key_word(inkey, key) >> (pc & 31)) & 1u)) { bad = base + j; break; }
            if (k != KEY_NONE) key = k;
        }
    }
    if (lane == 0) { gkey[b] = key; first_bad[b] = bad; }
}

// (part, floor) of every row after columns 0..Tp-1, from the words gpart[b] / gfloor[b] hold at the launch (RegisterRule.walk), as the
// scans above: one wave per row, 64 columns at a time, the lanes load the reg entries and every lane walks them.  Ids < 0 (left
// pads) and ids beyond the vocabulary are skipped.  Columns before `from` only move the words (the prompt's pitches are not judged);
// first_bad[b] = the first column >= from holding a pitch outside the bounds of the row's open part, where the walk of that row
// stops, -1 = none.
__global__ __launch_bounds__(64) void register_scan_kernel(const long long* ids, int ld_ids, int Tp, int from, int B, int V,
                                                           const unsigned char* reg, const int* grange, int gap, int* gpart,
                                                           int* gfloor, int* first_bad) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long* row = ids + (size_t)b * ld_ids;
    const uint32_t range = (uint32_t)grange[b];
    int part = gpart[b], floor = gfloor[b], bad = -1;
    for (int base = 0; base < Tp && bad < 0; base += 64) {
        const int col = base + lane;
        int p = 0xFF;
        if (col < Tp) {
            const long long tok = row[col];
            if (tok >= 0 && tok < V) p = reg[tok];
        }
        const int n = min(64, Tp - base);
        for (int j = 0; j < n; j++) {
            const uint32_t pj = (uint32_t)__shfl(p, j, 64);
            const RegWord rw = register_word(reg, range, part, floor, gap);
            if (base + j >= from && !((uint32_t)(pj - rw.lo <= rw.span) | (pj >> 7))) { bad = base + j; break; }
            register_move(part, floor, (int)pj);
        }
    }
    if (lane == 0) { gpart[b] = part; gfloor[b] = floor; first_bad[b] = bad; }
}

}  // namespace

extern "C" int mxl_decode_embed(const void* ids, int ld_ids, const int* t_dev, const void* E, void* out, int B, int d,
                                int V, float scale, void* stream) {
    MXL_CHECK_ARG(ids && t_dev && E && out && B > 0 && (d % 8) == 0);
    const int n = B * (d / 8);
    hipLaunchKernelGGL(decode_embed_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const long long*)ids,
                       ld_ids, t_dev, (const bf16_t*)E, (bf16_t*)out, B, d, V, scale);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_kv_append(const void* qkv, void* kcache, void* vcache, const int* t_dev, int B, int M, int d, int dh,
                             const float* r_r_bias, void* qr_out, void* stream) {
    MXL_CHECK_ARG(qkv && kcache && vcache && t_dev && B > 0 && M > 0 && (d % 8) == 0 && dh > 0 && (dh % 8) == 0 && (d % dh) == 0);
    MXL_CHECK_ARG(!qr_out || r_r_bias);
    const int n = B * (d / 8);
    hipLaunchKernelGGL(kv_append_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv,
                       (bf16_t*)kcache, (bf16_t*)vcache, t_dev, B, M, d, dh, r_r_bias, (bf16_t*)qr_out);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_kv_fill(const void* qkv, void* kcache, void* vcache, int B, int T, int M, int d, int dh, void* stream) {
    MXL_CHECK_ARG(qkv && kcache && vcache && B > 0 && T > 0 && M > 0 && (d % 8) == 0 && dh > 0 && (dh % 8) == 0 && (d % dh) == 0);
    const long long n = (long long)B * (T < M ? T : M) * (d / 8);
    hipLaunchKernelGGL(kv_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)qkv, (bf16_t*)kcache, (bf16_t*)vcache, B, T, M, d, dh);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_kv_zero_pad(void* qkv, const int* n_pad, int B, int T, int d, void* stream) {
    MXL_CHECK_ARG(qkv && n_pad && B > 0 && B <= 65535 && T > 0 && d > 0 && (d % 8) == 0);
    MXL_CHECK_ARG(((uintptr_t)qkv % 16) == 0);
    const long long n = (long long)T * (2 * d / 8);
    hipLaunchKernelGGL(kv_zero_pad_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       (bf16_t*)qkv, n_pad, T, d);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_decode_bd(const void* qr, const void* rd, float* bd, int B, int H, int dh, int M, int ld_qr, int ld_rd,
                             void* stream) {
    MXL_CHECK_ARG(qr && rd && bd && B > 0 && B <= 64 && H > 0 && M > 0);
    if (dh != 64) return MXL_EUNSUPPORTED;
    MXL_CHECK_ARG(ld_qr >= H * 64 && ld_rd >= H * 64 && (ld_qr % 8) == 0 && (ld_rd % 8) == 0);
    MXL_CHECK_ARG(((uintptr_t)qr % 16) == 0 && ((uintptr_t)rd % 16) == 0 && ((uintptr_t)bd % 16) == 0);
    hipLaunchKernelGGL(decode_bd_kernel, dim3((M + 255) / 256, H), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qr,
                       (const bf16_t*)rd, bd, B, H, M, ld_qr, ld_rd);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_sample(const float* logprobs, int ldl, int V, void* ids, int ld_ids, const int* t_dev,
                          unsigned long long* rng_ctr, unsigned long long seed, int B, int do_sample, int top_k, float top_p,
                          float temperature, float repetition_penalty, float typical_p, float* out_probs, void* stream) {
    MXL_CHECK_ARG(logprobs && ids && t_dev && rng_ctr && B > 0 && V > 0 && V <= SORT_N && temperature > 0.f);
    MXL_CHECK_ARG(repetition_penalty > 0.f && typical_p > 0.f);
    hipLaunchKernelGGL(sample_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logprobs, ldl, V, (long long*)ids, ld_ids,
                       t_dev, rng_ctr, seed, do_sample, top_k, top_p, temperature, repetition_penalty, typical_p, out_probs);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" size_t mxl_rules_size(void) { return sizeof(mxl_rules); }

// the one check of the rules (include/musicxl.h, mxl_rules), before any launch, and the struct the kernel gets: within a group all
// pointers or none; budget, count, guide and repeat read `cls`; the repeat needs the count, which ends its rows, its history, and the
// guide off: a row is fed from one place.
// fused: the launch that also samples -- budget, count, guide and repeat ride on the grammar there, and arrivals and live rows share
// one 32-bit word.  moves: the launch moves the words (all but the mask) -- the repeat then needs the stop group, whose finished rows
// keep their words.  ids / ld_ids: the history where the launch has the rows' ids itself (all but the mask, which takes the struct's)
static int make_rules(mxl_rules* out, const mxl_rules* rules, int B, bool fused, bool moves, const void* ids = nullptr, int ld_ids = 0) {
    MXL_CHECK_ARG(rules && ((uintptr_t)rules % alignof(mxl_rules)) == 0);   // (a misaligned pointer is no mxl_rules: refused, not read)
    mxl_rules r = *rules;
    if (moves) { r.hist = (const long long*)ids; r.ld_hist = ld_ids; }
    MXL_CHECK_ARG((r.unfinished == nullptr) == (r.alive == nullptr));
    MXL_CHECK_ARG((r.allow == nullptr) == (r.gstate == nullptr) && (r.next == nullptr) == (r.gstate == nullptr));
    MXL_CHECK_ARG(!r.gstate || (r.cls && r.C >= 1 && r.C <= 32));
    MXL_CHECK_ARG((r.slots == nullptr) == (r.gbar == nullptr) && (r.bars == nullptr) == (r.gbar == nullptr) && (r.grem == nullptr) == (r.gbar == nullptr));
    MXL_CHECK_ARG(!(r.gbar || r.gleft) || r.cls);
    MXL_CHECK_ARG((r.keys == nullptr) == (r.gkey == nullptr) && (r.pcs == nullptr) == (r.gkey == nullptr) && (r.inkey == nullptr) == (r.gkey == nullptr));
    MXL_CHECK_ARG((r.guide == nullptr) == (r.gpos == nullptr) && (r.glen == nullptr) == (r.gpos == nullptr) && (r.gforce == nullptr) == (r.gpos == nullptr));
    MXL_CHECK_ARG(!r.gpos || (r.cls && r.ld_guide >= 1));
    MXL_CHECK_ARG((r.reg == nullptr) == (r.gpart == nullptr) && (r.grange == nullptr) == (r.gpart == nullptr) && (r.gfloor == nullptr) == (r.gpart == nullptr));
    MXL_CHECK_ARG(!r.gpart || (r.gap >= -1 && r.gap <= 127));
    MXL_CHECK_ARG((r.plan == nullptr) == (r.gcopy == nullptr) && (r.nplan == nullptr) == (r.gcopy == nullptr) && (r.barcol == nullptr) == (r.gcopy == nullptr));
    MXL_CHECK_ARG((r.gbars == nullptr) == (r.gcopy == nullptr) && (r.gstop == nullptr) == (r.gcopy == nullptr));
    MXL_CHECK_ARG(!r.gcopy || (r.cls && r.gleft && !r.gpos && r.ld_plan >= 1 && r.hist && r.ld_hist >= 1 && (r.span == 0 || r.span == 1)));
    MXL_CHECK_ARG(!r.gcopy || !moves || r.unfinished);
    if (fused) MXL_CHECK_ARG(!(r.gbar || r.gleft || r.gpos || r.gcopy) || r.gstate);
    if (fused && r.unfinished) MXL_CHECK_ARG(B <= 32767);
    if (!r.unfinished && fused) { r.eos_id = -1; r.pad_id = 0; r.min_length = 0; }
    *out = r;
    return MXL_OK;
}

// f(std::bool_constant<flags>{}...): runtime flags as compile-time ones, one branch per flag
template <class F>
static void with_flags(F&& f) { f(); }
template <class F, class... Rest>
static void with_flags(F&& f, bool first, Rest... rest) {
    if (first) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

extern "C" int mxl_sample_step(const float* scores, int ldl, int V, void* ids, int ld_ids, int* t_dev, unsigned long long* rng_ctr,
                               unsigned long long seed, int B, int do_sample, int top_k, float top_p, float temperature,
                               float repetition_penalty, float typical_p, const void* E, void* emb_out, int d, float scale,
                               int* counter, const mxl_rules* rules, float* out_probs, void* stream) {
    MXL_CHECK_ARG(scores && ids && t_dev && rng_ctr && E && emb_out && counter && B > 0 && V > 0 && V <= SORT_N && temperature > 0.f);
    MXL_CHECK_ARG(repetition_penalty > 0.f && typical_p > 0.f && d > 0 && (d % 8) == 0);
    MXL_CHECK_ARG(((uintptr_t)E % 16) == 0 && ((uintptr_t)emb_out % 16) == 0);
    mxl_rules r;
    if (const int e = make_rules(&r, rules, B, true, true, ids, ld_ids)) return e;
    // one instantiation per set of groups the kernel's static_asserts admit -- the budget, the count, the guide and the repeat ride on
    // the grammar, the repeat on the count as well and never beside the guide (make_rules lets no other set through): 4 without the
    // grammar, 32 with it, 8 with the repeat
    bool launched = false;
    with_flags([&](auto G, auto BUD, auto CNT, auto INK, auto GD, auto RG, auto RP) {
        if constexpr ((G || !(BUD || CNT || GD || RP)) && !(GD && RP) && (!RP || CNT)) {
            hipLaunchKernelGGL((sample_step_kernel<G, BUD, CNT, INK, GD, RG, RP>), dim3(B), dim3(256), 0, (hipStream_t)stream, scores, ldl,
                               V, (long long*)ids, ld_ids, t_dev, rng_ctr, seed, do_sample, top_k, top_p, temperature, repetition_penalty,
                               typical_p, (const bf16_t*)E, (bf16_t*)emb_out, d, scale, counter, out_probs, r);
            launched = true;
        }
    }, r.gstate != nullptr, r.gbar != nullptr, r.gleft != nullptr, r.gkey != nullptr, r.gpos != nullptr, r.gpart != nullptr,
       r.gcopy != nullptr);
    MXL_CHECK_ARG(launched);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_rules_mask(float* scores, int ldl, int B, int V, const int* t_dev, const mxl_rules* rules, void* stream) {
    MXL_CHECK_ARG(rules && ((uintptr_t)rules % alignof(mxl_rules)) == 0);   // (a misaligned pointer is no mxl_rules: refused, not read)
    MXL_CHECK_ARG(scores && B > 0 && V > 0 && ldl >= V && (t_dev || rules->min_length <= 0));
    const long long n = (long long)B * V;
    MXL_CHECK_ARG(n <= (1LL << 38));
    mxl_rules r;
    if (const int e = make_rules(&r, rules, B, false, false)) return e;
    if (!r.cls && !r.gkey && !r.gpart && (r.min_length <= 0 || r.eos_id < 0 || r.eos_id >= V)) return MXL_OK;   // nothing to bar
    hipLaunchKernelGGL(rules_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scores, ldl, B, V, t_dev, r);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_rules_advance(void* ids, int ld_ids, const int* t_dev, int B, int V, const mxl_rules* rules, void* stream) {
    MXL_CHECK_ARG(rules && ((uintptr_t)rules % alignof(mxl_rules)) == 0);   // (a misaligned pointer is no mxl_rules: refused, not read)
    MXL_CHECK_ARG(ids && t_dev && B > 0 && (V > 0 || !(rules->cls || rules->gkey || rules->gpart)));
    mxl_rules r;
    if (const int e = make_rules(&r, rules, B, false, true, ids, ld_ids)) return e;
    if (!r.cls && !r.gkey && !r.gpart && !r.unfinished) return MXL_OK;                           // nothing to move
    hipLaunchKernelGGL(rules_advance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (long long*)ids, ld_ids, t_dev, B, V, r);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_register_scan(const void* ids, int ld_ids, int Tp, int from, int B, int V, const void* reg, const void* grange, int gap,
                                 int* gpart, int* gfloor, int* first_bad, void* stream) {
    MXL_CHECK_ARG(ids && B > 0 && V > 0 && Tp >= 0 && ld_ids >= Tp && from >= 0 && reg && grange && gpart && gfloor && first_bad);
    MXL_CHECK_ARG(gap >= -1 && gap <= 127);
    hipLaunchKernelGGL(register_scan_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const long long*)ids, ld_ids, Tp, from, B, V,
                       (const unsigned char*)reg, (const int*)grange, gap, gpart, gfloor, first_bad);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_key_scan(const void* ids, int ld_ids, int Tp, int from, int B, int V, const void* keys, const void* pcs,
                            const void* inkey, int* gkey, int* first_bad, void* stream) {
    MXL_CHECK_ARG(ids && B > 0 && V > 0 && Tp >= 0 && ld_ids >= Tp && from >= 0 && keys && pcs && inkey && gkey && first_bad);
    hipLaunchKernelGGL(key_scan_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const long long*)ids, ld_ids, Tp, from, B, V,
                       (const unsigned char*)keys, (const unsigned char*)pcs, (const unsigned short*)inkey, gkey, first_bad);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_grammar_scan(const void* ids, int ld_ids, int Tp, int B, int V, const void* cls, const void* allow,
                                const void* next, int C, int start, int* gstate, int* first_bad, void* stream) {
    MXL_CHECK_ARG(ids && B > 0 && V > 0 && Tp >= 0 && ld_ids >= Tp && first_bad && start >= 0 && start < 256);
    MXL_CHECK_ARG(cls && allow && next && gstate && C >= 1 && C <= 32);
    hipLaunchKernelGGL(grammar_scan_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const long long*)ids, ld_ids, Tp, B, V,
                       (const unsigned char*)cls, (const uint32_t*)allow, (const unsigned char*)next, C, start, gstate, first_bad);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_budget_scan(const void* ids, int ld_ids, int Tp, int B, int V, const void* cls, const void* slots, const void* bars,
                               unsigned opens, unsigned need_free, unsigned need_full, int* gbar, int* grem, int* first_bad,
                               void* stream) {
    MXL_CHECK_ARG(ids && B > 0 && V > 0 && Tp >= 0 && ld_ids >= Tp && first_bad);
    MXL_CHECK_ARG(cls && slots && bars && gbar && grem);       // any masks are meaningful: bits beyond the classes never match
    hipLaunchKernelGGL(budget_scan_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const long long*)ids, ld_ids, Tp, B, V,
                       (const unsigned char*)cls, (const unsigned short*)slots, (const unsigned short*)bars, opens, need_free,
                       need_full, gbar, grem, first_bad);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_decode_advance(int* t_dev, unsigned long long* rng_ctr, void* stream) {
    MXL_CHECK_ARG(t_dev && rng_ctr);
    hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, t_dev, rng_ctr);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Contrastive search (HF 4.25.1 GenerationMixin.contrastive_search / _ranking_fast, reached from
// musicnlp/trainer/eval.py:296-302 with the mems patch of musicnlp/models/transformer_xl.py:229-234): candidate k of sequence b
// is scored  (1 - alpha) * p[b][k]  -  alpha * max_s cos(h_cand[b*K + k], h_ctx[b][s]),  s over the S context positions.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void row_inv_norm_kernel(const bf16_t* x, long long ld, int d, float* out, int n) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= n) return;
    const float r = row_inv_norm_wave(x + (size_t)j * ld, d, lane);
    if (lane == 0) out[j] = r;
}

// one workgroup per candidate row: four waves stride over the context positions, 8 bf16 per lane per pass over d
// (contrastive_score_row, shared with mxl_contrastive_step)
__global__ __launch_bounds__(256) void contrastive_score_kernel(const bf16_t* ctx, long long ctx_bs, const float* ctx_inv, int inv_bs,
                                                                int S, const bf16_t* hid, int d, const float* probs, float alpha,
                                                                int K, float* score) {
    __shared__ float wmax[4];
    const int row = blockIdx.x, b = row / K;
    const float sc = contrastive_score_row(ctx + (size_t)b * ctx_bs, ctx_inv + (size_t)b * inv_bs, S, hid + (size_t)row * d, d,
                                           probs[row], alpha, wmax);
    if (threadIdx.x == 0) score[row] = sc;
}

__global__ void contrastive_pick_kernel(const float* score, int K, long long* sel, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int bi = 0;
    float bv = score[(size_t)b * K];
    for (int k = 1; k < K; k++) {
        const float v = score[(size_t)b * K + k];
        if (v > bv) { bv = v; bi = k; }             // first maximum, as torch.max
    }
    sel[b] = bi;
}
}  // namespace

extern "C" int mxl_row_inv_norm_bf16(const void* x, long long ld, int n, int d, float* out, void* stream) {
    MXL_CHECK_ARG(x && out && n > 0 && d > 0 && (d % 8) == 0 && (ld % 8) == 0);
    hipLaunchKernelGGL(row_inv_norm_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ld, d, out, n);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_contrastive_select(const void* ctx, long long ctx_bs, const float* ctx_inv_norm, int inv_bs, int S, const void* hid,
                                      const float* probs, float alpha, int B, int K, int d, float* score, void* sel, void* stream) {
    MXL_CHECK_ARG(ctx && ctx_inv_norm && hid && probs && score && sel && B > 0 && K > 0 && S > 0 && d > 0 && (d % 8) == 0 &&
                  (ctx_bs % 8) == 0);
    hipLaunchKernelGGL(contrastive_score_kernel, dim3(B * K), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)ctx, ctx_bs,
                       ctx_inv_norm, inv_bs, S, (const bf16_t*)hid, d, probs, alpha, K, score);
    hipLaunchKernelGGL(contrastive_pick_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, score, K, (long long*)sel, B);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}
