// Shared rings under contrastive search (generate(contrastive_rings='shared')): one K/V ring per prompt, read by its K candidates.
//
// csrc/contrastive.hip states the invariant: the K rows of a prompt differ in the one ring slot the current step wrote, and only until
// the pick.  So the rings of rows b*K .. b*K + K-1 are one ring (B0, H, M, dh), and the slot of the step -- t mod M -- is the one place
// where a candidate reads its own k / v.  Three launches keep that state:
//   mxl_kv_stash               where mxl_kv_append sat: qr = q + r_r_bias, and the row's k / v into the layer's stash (no ring write)
//   mxl_relattn_decode_shared  the attention of the K queries of every prompt over the prompt's ring; slot t mod M comes from the
//                              row's own qkv row, the ring's slot t mod M is never read
//   mxl_kv_commit_shared       after the pick: the stash of row b*K + sel[b] goes into slot t mod M of ring b, all layers in one launch
//
// The attention kernel is decode_attn_kernel of decode_attn.hip run for G queries at once.  Per query nothing moves: bf16(q + r_w_bias),
// the f32 dot in the same lane order, the same slot-to-lane assignment (a lane's slots are lo + wid*KPW + ksub + m*4*KPW, whatever the
// batch depth), the same pieces and merge order, P rounded to bf16 before P.V -- so every sum adds what it adds there in the order it adds
// it there, and the output of row b*K + k equals, bit for bit, mxl_relattn_decode_split_live's at the same `pieces` on K copies of ring
// b whose slot t mod M holds candidate k's k / v (tests/test_contrastive_shared_ops_gpu.py).  What is shared is the load: a K or V
// fragment fetched from HBM serves the G queries the workgroup holds.
//
// G.  A query costs 8 registers of q and 8 of o per lane and cap * 4 bytes of LDS for its scores; decode_attn_kernel's 250 registers at
// dh = 64 leave room for neither 16 nor 32 queries.  G = 8 with 4-deep double-buffered batches takes 204 registers and no scratch
// (8-deep: spills; the positional terms, which that kernel carries in registers beside a batch, wait in the score buffer here), and
// at M = 2048 in one piece 74 KB of LDS: two workgroups per CU, as there.  K <= 4 runs G = 4 at depth 8 (244 registers, no scratch).
// A prompt's ring is therefore read ceil(K / 8) times per layer and step: once for K = 4, twice for K = 16, four times for K = 32
// (K times before).  The batch depth changes no bit: a lane visits its slots in ascending order whatever it is.
//
// Measured (profiles/contrastive_shared_rings.txt): the launch is bound by its per-query vector and LDS work, not by HBM -- at a full
// ring it reads at 1.2 - 1.3 TB/s where the launch on the copies streams 6.6 -- so a second read of the ring costs little, and the
// next step is fewer instructions per query and slot (the MFMA form, which changes the order of the sums), not a larger G.
#include "decode_attn.h"
#include "musicxl_internal.h"

namespace {

constexpr int SH_KMAX = 32;
inline size_t shared_lds(int G, int dh, int cap) { return group_lds(G, dh, cap, 2 * dh * 2); }      // (the queries' own k / v)

// grid (head, prompt * groups + group, ring piece), 256 threads; dynamic LDS: scores [G][cap] f32, the output scratch [4][G][DH] f32,
// the queries' own k / v [G][2][DH] bf16.  A group past the last candidate (K % G != 0) runs its spare queries on the prompt's last
// row and writes nothing for them.
template <int DH, int G>
__global__ __launch_bounds__(256, 2) void decode_attn_shared_kernel(const bf16_t* qkv, const bf16_t* kc, const bf16_t* vc,
                                                                 const float* bd, const float* rwb, bf16_t* out, const int* t_dev,
                                                                 int K, int ngroups, int H, int M, float scale, float* ws,
                                                                 int* arrived, const int* live, int cap) {
    constexpr int LPK = DH / 8;          // lanes per key row
    constexpr int KPW = 64 / LPK;        // keys per wave per iteration
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sc = reinterpret_cast<float*>(smem);                      // [G][cap] positional terms -> scores -> probabilities
    float* red = sc + (size_t)G * cap;                               // [4][G][DH]
    bf16_t* own = reinterpret_cast<bf16_t*>(red + 4 * G * DH);       // [G][2][DH]: k, v of the step's slot, per query
    __shared__ float wred[2][G][4];
    const int h = blockIdx.x, b = blockIdx.y / ngroups, g0 = (blockIdx.y % ngroups) * G;
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    const int c8 = lane % LPK, ksub = lane / LPK;
    const int d = H * DH;
    const int nact = min(G, K - g0);                                 // queries of this group that are candidates
    const int row0 = b * K + g0;
    auto row_of = [&](int g) { return group_row(b, K, g0, g); };      // (a lambda: called directly, the row changes the schedule)
    // a finished sequence (live[b*K] == 0; its K rows finish together): no ring byte is read, piece 0 leaves zeros
    if (live != nullptr && live[b * K] == 0) {
        if (blockIdx.z == 0)
            for (int i = tid; i < nact * DH; i += 256) out[(size_t)(row0 + i / DH) * d + h * DH + i % DH] = f2bf(0.f);
        return;
    }
    const int t = *t_dev;
    const int tm = t % M;
    const int NS = gridDim.z, zi = blockIdx.z;
    const RingPiece pc = ring_piece(t, M);
    const int lo = pc.lo, hi = pc.hi, plo = pc.plo, phi = pc.phi;
    const int nw = hi - lo;                                          // scores: written slot s at s - lo, never-written sp at nw + sp - plo

    float qw[G][8];
#pragma unroll
    for (int g = 0; g < G; g++) {
        const bf16x8 qv = *reinterpret_cast<const bf16x8*>(qkv + (size_t)row_of(g) * 3 * d + h * DH + c8 * 8);
#pragma unroll
        for (int j = 0; j < 8; j++) qw[g][j] = biased_query((bf16_t)qv[j], rwb[h * DH + c8 * 8 + j]);
    }
    // the step's own k / v of every query, and the positional terms of the written slots (decode_attn_kernel carries them in
    // registers beside the K batch; here they wait where the score will go)
#pragma clang loop vectorize(disable) unroll(disable)
    for (int i = tid; i < G * 2 * LPK; i += 256) {
        const int g = i / (2 * LPK), w = (i / LPK) & 1, c = i % LPK;
        *reinterpret_cast<u32x4*>(own + (g * 2 + w) * DH + c * 8) =
            *reinterpret_cast<const u32x4*>(qkv + (size_t)row_of(g) * 3 * d + (1 + w) * d + h * DH + c * 8);
    }
    // (the side loops run the G queries inside one pass over the slots: G independent chains per thread, each in the order it has there)
    const float* bdh = bd + (size_t)h * M;
    size_t bdoff[G];
#pragma unroll
    for (int g = 0; g < G; g++) bdoff[g] = (size_t)row_of(g) * H * M;
#pragma clang loop vectorize(disable) unroll(disable)
    for (int i = tid; i < nw; i += 256) {
        int dist = tm - (lo + i);
        if (dist < 0) dist += M;
#pragma unroll
        for (int g = 0; g < G; g++) sc[g * cap + i] = bdh[bdoff[g] + dist];
    }
    __syncthreads();
    const bf16_t* kb = kc + ((size_t)b * H + h) * M * DH + c8 * 8;     // head-major ring of the prompt: rows are DH apart
    const bf16_t* vb = vc + ((size_t)b * H + h) * M * DH + c8 * 8;

    // pass 1: scores.  Double-buffered batches of U key groups with non-temporal loads, as decode_attn_kernel; a fragment is used G
    // times.  The step's slot is left out here -- not loaded, not scored: a score depends on its own slot alone, so the lanes that own
    // slot tm score it below from each query's own k, with the same sum.
    constexpr int U = G == 8 ? 4 : 8;      // batch depth: what the registers beside G queries leave (no scratch at either)
    constexpr int ST = 4 * KPW * U;
    const bool own_here = tm >= lo && tm < hi && wid == ((tm - lo) / KPW) % 4 && ksub == (tm - lo) % KPW;   // this lane's slot is tm
    float mx[G];
#pragma unroll
    for (int g = 0; g < G; g++) mx[g] = -1e30f;
    {
        bf16x8 kA[U], kB[U];
        auto load_k = [&](int s0, bf16x8 (&kv)[U]) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int s = s0 + u * 4 * KPW + ksub;
                const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
                kv[u] = (s < hi && s != tm) ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(kb + (size_t)s * DH)) : z;
            }
        };
        auto score = [&](int g, const bf16x8& kk, int s, bool in) {
            float acc = (in && c8 == 0) ? sc[g * cap + s - lo] : 0.f;
#pragma unroll
            for (int j = 0; j < 8; j++) acc += qw[g][j] * bf2f((bf16_t)kk[j]);
#pragma unroll
            for (int o = 1; o < LPK; o <<= 1) acc += __shfl_xor(acc, o, 64);
            acc *= scale;
            if (in) {
                if (c8 == 0) sc[g * cap + s - lo] = acc;
                mx[g] = fmaxf(mx[g], acc);
            }
        };
        auto use_k = [&](int s0, const bf16x8 (&kv)[U]) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int s = s0 + u * 4 * KPW + ksub;
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int g = 0; g < G; g++) score(g, kv[u], s, s < hi && s != tm);
            }
        };
        int s0 = lo + wid * KPW;
        if (s0 < hi) load_k(s0, kA);
        for (; s0 < hi; s0 += 2 * ST) {
            if (s0 + ST < hi) load_k(s0 + ST, kB);
            use_k(s0, kA);
            if (s0 + ST < hi) {
                if (s0 + 2 * ST < hi) load_k(s0 + 2 * ST, kA);
                use_k(s0 + ST, kB);
            }
        }
        if (own_here) {                                  // (the LPK lanes of the slot are here together)
#pragma unroll
            for (int g = 0; g < G; g++) score(g, *reinterpret_cast<const bf16x8*>(own + (g * 2) * DH + c8 * 8), tm, true);
        }
    }
    group_score_unwritten<G>(sc, cap, bdh, bdoff, tm, nw, plo, phi, M, scale, mx);
    // pass 2 walks the written slots in two ranges, [lo, tm) and (tm, hi), with the step's slot between them: a lane adds its
    // slots in ascending order there as here, and the lane that owns slot tm adds that term from the query's own v in its place.
    // What the cut changes is where lanes run `o += 0 * 0` for slots outside the range, which leaves o as it is.
    const int e1 = min(max(tm, lo), hi), a2 = min(max(tm + 1, lo), hi);
    int va = lo, ve = e1, vs0 = lo + wid * KPW;
    // the first V batch is requested before the softmax section, as there
    bf16x8 vA[U], vB[U];
    auto load_v = [&](int s0, bf16x8 (&vv)[U]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int s = s0 + u * 4 * KPW + ksub;
            const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            vv[u] = (s >= va && s < ve) ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(vb + (size_t)s * DH)) : z;
        }
    };
    if (vs0 < ve) load_v(vs0, vA);
#pragma unroll
    for (int g = 0; g < G; g++) {
        const float m = wave_max(mx[g]);
        if (lane == 0) wred[0][g][wid] = m;
    }
    __syncthreads();
    auto max_of = [&](int g) { return fmaxf(fmaxf(wred[0][g][0], wred[0][g][1]), fmaxf(wred[0][g][2], wred[0][g][3])); };
    auto sum_of = [&](int g) { return wred[1][g][0] + wred[1][g][1] + wred[1][g][2] + wred[1][g][3]; };
    {
        float mg[G], sum[G];
#pragma unroll
        for (int g = 0; g < G; g++) { mg[g] = max_of(g); sum[g] = 0.f; }
#pragma clang loop vectorize(disable) unroll(disable)
        for (int i = tid; i < nw; i += 256) {
#pragma unroll
            for (int g = 0; g < G; g++) {
                const float pv = __expf(sc[g * cap + i] - mg[g]);
                sc[g * cap + i] = pv;
                sum[g] += pv;
            }
        }
#pragma clang loop vectorize(disable) unroll(disable)
        for (int i = tid; i < phi - plo; i += 256) {     // (v = 0 there: only the denominator)
#pragma unroll
            for (int g = 0; g < G; g++) sum[g] += __expf(sc[g * cap + nw + i] - mg[g]);
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            const float sg = wave_sum(sum[g]);
            if (lane == 0) wred[1][g][wid] = sg;
        }
    }
    __syncthreads();

    // pass 2: o = sum_s p_s v_s   (P rounded to bf16); same batched loads, a fragment used G times
    float o[G][8];
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
        for (int j = 0; j < 8; j++) o[g][j] = 0.f;
    {
        auto add = [&](int g, const bf16x8& vv, int s, bool in) { group_add(sc, g * cap + s - lo, o[g], vv, in); };
        auto use_v = [&](int s0, const bf16x8 (&vv)[U]) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int s = s0 + u * 4 * KPW + ksub;
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int g = 0; g < G; g++) add(g, vv[u], s, s >= va && s < ve);
            }
        };
#pragma unroll 1
        for (int half = 0; half < 2; half++) {
            for (; vs0 < ve; vs0 += 2 * ST) {          // (the never-written slots hold v = 0: nothing to add)
                if (vs0 + ST < ve) load_v(vs0 + ST, vB);
                use_v(vs0, vA);
                if (vs0 + ST < ve) {
                    if (vs0 + 2 * ST < ve) load_v(vs0 + 2 * ST, vA);
                    use_v(vs0 + ST, vB);
                }
            }
            if (half == 0) {
                if (own_here) {
#pragma unroll
                    for (int g = 0; g < G; g++) add(g, *reinterpret_cast<const bf16x8*>(own + (g * 2 + 1) * DH + c8 * 8), tm, true);
                }
                va = a2; ve = hi;
                vs0 = lo + wid * KPW + ((a2 - lo) / ST) * ST;       // the batch that holds slot a2
                if (vs0 < ve) load_v(vs0, vA);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
#pragma unroll
            for (int off = LPK; off < 64; off <<= 1) o[g][j] += __shfl_xor(o[g][j], off, 64);
        }
        if (ksub == 0) {
#pragma unroll
            for (int j = 0; j < 8; j++) red[(wid * G + g) * DH + c8 * 8 + j] = o[g][j];
        }
    }
    __syncthreads();
    auto red_of = [&](int g, int e) {
        return red[g * DH + e] + red[(G + g) * DH + e] + red[(2 * G + g) * DH + e] + red[(3 * G + g) * DH + e];
    };
    if (NS == 1) {
        for (int i = tid; i < nact * DH; i += 256) {
            const int g = i / DH, e = i % DH;
            const float inv = 1.f / sum_of(g);
            out[(size_t)(row0 + g) * d + h * DH + e] = f2bf(red_of(g, e) * inv);
        }
        return;
    }
    // ---- ring pieces: every query leaves (o unnormalised, max, sum) where decode_attn_kernel leaves its row's, as agent-scope stores;
    // the group shares the arrival counter of its first row, and its last piece merges every query in piece order
    for (int i = tid; i < nact * DH; i += 256) {
        const int g = i / DH, e = i % DH;
        MXL_AGENT_STORE(ws + ((size_t)(row0 + g) * H + h) * NS * (DH + 2) + zi * (DH + 2) + e, red_of(g, e));
    }
    if (tid < nact) {
        float* wsp = ws + ((size_t)(row0 + tid) * H + h) * NS * (DH + 2) + zi * (DH + 2);
        MXL_AGENT_STORE(wsp + DH, max_of(tid));
        MXL_AGENT_STORE(wsp + DH + 1, sum_of(tid));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int s_last;
    if (tid == 0) s_last = (__hip_atomic_fetch_add(arrived + (size_t)row0 * H + h, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == NS - 1) ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    for (int i = tid; i < nact * DH; i += 256) {
        const int g = i / DH, e = i % DH;
        const float* wsp = ws + ((size_t)(row0 + g) * H + h) * NS * (DH + 2);
        float m = -1e30f;
        for (int k = 0; k < NS; k++) m = fmaxf(m, MXL_AGENT_LOAD(wsp + k * (DH + 2) + DH));
        float num = 0.f, den = 0.f;
        for (int k = 0; k < NS; k++) {
            const float a = __expf(MXL_AGENT_LOAD(wsp + k * (DH + 2) + DH) - m);
            num += a * MXL_AGENT_LOAD(wsp + k * (DH + 2) + e);
            den += a * MXL_AGENT_LOAD(wsp + k * (DH + 2) + DH + 1);
        }
        out[(size_t)(row0 + g) * d + h * DH + e] = f2bf(num / den);
    }
    if (tid == 0) MXL_AGENT_STORE(arrived + (size_t)row0 * H + h, 0);
}

// qr[b] = q + r_r_bias as kv_append_kernel writes it, and stash[b] = (k, v) of the (B, 3d) qkv rows: one thread per 8 elements
__global__ void kv_stash_kernel(const bf16_t* qkv, bf16_t* stash, int B, int d, const float* rrb, bf16_t* qr) {
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
    *reinterpret_cast<u32x4*>(stash + (size_t)b * 2 * d + c * 8) = *reinterpret_cast<const u32x4*>(qkv + (size_t)b * 3 * d + d + c * 8);
    *reinterpret_cast<u32x4*>(stash + (size_t)b * 2 * d + d + c * 8) = *reinterpret_cast<const u32x4*>(qkv + (size_t)b * 3 * d + 2 * d + c * 8);
}

// grid (prompt, ring): ring i < L is the K ring of layer i, ring L + i its V ring; slot t mod M of every head of prompt b <- the
// picked row's stash.  A sel outside 0..K-1 (mxl_contrastive_step writes none) is held to the range.
__global__ __launch_bounds__(256) void kv_commit_shared_kernel(bf16_t* const* table, int L, const bf16_t* stash, int K, int rows, int H,
                                                               int M, int dh, const int* t_dev, const int* sel) {
    const int b = blockIdx.x, i = blockIdx.y;
    const int l = i % L, w = i / L;
    const int t = *t_dev;
    if (t < 0) return;
    const int slot = t % M, d = H * dh;
    const int s = min(max(sel[b], 0), K - 1);
    const bf16_t* from = stash + ((size_t)l * rows + (size_t)b * K + s) * 2 * d + (size_t)w * d;
    bf16_t* ring = table[i];
    for (int c = threadIdx.x; c < (d >> 3); c += 256) {
        const int h = (c * 8) / dh, e = (c * 8) % dh;
        *reinterpret_cast<u32x4*>(ring + (((size_t)b * H + h) * M + slot) * dh + e) = *reinterpret_cast<const u32x4*>(from + c * 8);
    }
}

}  // namespace

extern "C" size_t mxl_relattn_decode_shared_lds_bytes(int K, int dh, int M, int pieces) {
    if (K < 2 || K > SH_KMAX || dh <= 0 || M <= 0 || pieces < 1 || pieces > 8) return 0;
    return shared_lds(group_size(K), dh, group_cap(M, pieces));
}

extern "C" int mxl_relattn_decode_shared(const void* qkv, const void* kcache, const void* vcache, const float* bd,
                                         const float* r_w_bias, void* out, const int* t_dev, int B0, int K, int H, int dh, int M,
                                         float scale, int pieces, float* ws, int* arrived, const int* unfinished, void* stream) {
    MXL_CHECK_ARG(qkv && kcache && vcache && bd && r_w_bias && out && t_dev && B0 > 0 && H > 0 && M > 0);
    MXL_CHECK_ARG(K >= 2 && K <= SH_KMAX && pieces >= 1 && pieces <= 8);
    if (pieces > 1) MXL_CHECK_ARG(ws && arrived);
    MXL_CHECK_ARG(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)kcache % 16) == 0 && ((uintptr_t)vcache % 16) == 0);
    if (dh != 16 && dh != 32 && dh != 64) return MXL_EUNSUPPORTED;
    const int G = group_size(K), cap = group_cap(M, pieces);
    const size_t shm = shared_lds(G, dh, cap);
    MXL_CHECK_ARG(shm <= (size_t)GROUP_LDS_MAX && (long long)B0 * ((K + G - 1) / G) <= 65535);
    hipStream_t s = (hipStream_t)stream;
    const int ngroups = (K + G - 1) / G;
#define LAUNCH(DH, GG) return launch_big_lds<&decode_attn_shared_kernel<DH, GG>>(                                                            \
        dim3(H, B0 * ngroups, pieces), shm, s, (const bf16_t*)qkv, (const bf16_t*)kcache, (const bf16_t*)vcache, bd, r_w_bias, (bf16_t*)out, \
        t_dev, K, ngroups, H, M, scale, ws, arrived, unfinished, cap)
    if (G == 4) {
        switch (dh) {
            case 16: LAUNCH(16, 4);
            case 32: LAUNCH(32, 4);
            default: LAUNCH(64, 4);
        }
    }
    switch (dh) {
        case 16: LAUNCH(16, 8);
        case 32: LAUNCH(32, 8);
        default: LAUNCH(64, 8);
    }
#undef LAUNCH
}

extern "C" int mxl_kv_stash(const void* qkv, void* stash, int B, int d, const float* r_r_bias, void* qr_out, void* stream) {
    MXL_CHECK_ARG(qkv && stash && B > 0 && d > 0 && (d % 8) == 0);
    MXL_CHECK_ARG(!qr_out || r_r_bias);
    MXL_CHECK_ARG(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)stash % 16) == 0 && ((uintptr_t)qr_out % 16) == 0);
    const int n = B * (d / 8);
    hipLaunchKernelGGL(kv_stash_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (bf16_t*)stash, B,
                       d, r_r_bias, (bf16_t*)qr_out);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_kv_commit_shared(const void* table, int n_layers, const void* stash, int B0, int K, int H, int M, int dh,
                                    const int* t_dev, const int* sel, void* stream) {
    MXL_CHECK_ARG(table && stash && t_dev && sel);
    MXL_CHECK_ARG(n_layers >= 1 && 2 * n_layers <= 65535 && B0 > 0 && B0 <= 65535 && K >= 2 && K <= SH_KMAX && H > 0 && M > 0);
    MXL_CHECK_ARG(dh > 0 && (dh % 8) == 0 && ((uintptr_t)stash % 16) == 0);
    hipLaunchKernelGGL(kv_commit_shared_kernel, dim3(B0, 2 * n_layers), dim3(256), 0, (hipStream_t)stream, (bf16_t* const*)table,
                       n_layers, (const bf16_t*)stash, K, B0 * K, H, M, dh, t_dev, sel);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}
