// One prompt ring shared by the n sampled variations of a prompt (generate(do_sample=True, num_return_sequences=n,
// prompt_rings='shared')).
//
// The n rows of a prompt hold the same prompt, so what the prompt pass leaves in their rings is n copies of one ring, and a ring slot
// written for a prompt position never changes.  Every position generated after the prompt is private to its row.  So a layer keeps
//   prompt rings  kp, vp (B0, H, M, dh)      slot p mod M <- position p < Tp, written once by the prompt pass of the B0 prompts (mxl_kv_fill)
//   tail rings    kt, vt (rows, H, Mt, dh)   slot (p - Tp) mod Mt <- position p >= Tp of the row, rows = B0 * n (mxl_kv_append_tail)
// and the attention of a step picks the source per slot.  Ring slot s of the copied mode holds, at step t, position
//   p = t - ((t - s) mod M),
// the latest position <= t that maps to s: p < 0 was never written (the positional term alone, as ever), p >= Tp lies in the row's tail
// at slot (p - Tp) mod Mt, anything else in slot s of the prompt's ring.  No table: t, Tp and s say it all.  A window of M positions
// ending at t holds min(M, t - Tp + 1) generated ones, so with Mt >= min(M, last t - Tp + 1) no live tail slot is overwritten; Tp is
// read from the device (t0_dev), so a captured step serves every prompt length.
//
// The attention kernel is decode_attn_shared_kernel of decode_shared.hip -- G queries of one prompt per workgroup, a prompt-ring fragment
// fetched once for all of them -- with the tail slots fetched per query.  Per query nothing moves against decode_attn_kernel: bf16(q +
// r_w_bias), the f32 dot in the same lane order, the same slot-to-lane assignment (a lane's slots are lo + wid*KPW + ksub + m*4*KPW), the
// pieces and their merge order, P rounded to bf16 before P.V, and a lane adds its slots in ascending order.  That last point is why the
// walk is cut where the source changes and not run source by source: the tail slots are the `nt` slots that end at t mod M going round
// the ring, so ascending order meets at most three runs -- prompt, tail, prompt or tail, prompt, tail -- and each run is walked with the
// loads of its kind from the batch that holds its first slot; lanes whose slot lies outside the run add 0 * 0.  The output of row
// b*n + k therefore equals, bit for bit, mxl_relattn_decode_split_live's at the same `pieces` on the ring the row would own in the
// copied mode (tests/test_prefix_rings_ops_gpu.py).
//
// `unfinished` is per row here (the rows of a prompt finish on their own): a finished row reads no tail byte and leaves zeros, a group
// without a live row reads nothing at all.  Inside a live group a finished query still rides along on the prompt fragments the others
// need -- its numbers are dropped at the store.
#include "decode_attn.h"
#include "musicxl_internal.h"

namespace {

// scores [G][cap] f32 and the output scratch [4][G][dh] f32: decode_shared's without its G * 4 * dh bytes of own k / v
inline size_t prefix_lds(int G, int dh, int cap) { return group_lds(G, dh, cap, 0); }

// grid (head, prompt * groups + group, ring piece), 256 threads.  A group past the last row of a prompt (n % G != 0) runs its spare
// queries on the prompt's last row and writes nothing for them.
template <int DH, int G>
__global__ __launch_bounds__(256, 2) void decode_attn_prefix_kernel(const bf16_t* qkv, const bf16_t* kp, const bf16_t* vp,
                                                                 const bf16_t* kt, const bf16_t* vt, const float* bd, const float* rwb,
                                                                 bf16_t* out, const int* t_dev, const int* t0_dev, int n, int ngroups,
                                                                 int H, int M, int Mt, float scale, float* ws, int* arrived,
                                                                 const int* live, int cap) {
    constexpr int LPK = DH / 8;          // lanes per key row
    constexpr int KPW = 64 / LPK;        // keys per wave per iteration
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sc = reinterpret_cast<float*>(smem);                      // [G][cap] positional terms -> scores -> probabilities
    float* red = sc + (size_t)G * cap;                               // [4][G][DH]
    __shared__ float wred[2][G][4];
    const int h = blockIdx.x, b = blockIdx.y / ngroups, g0 = (blockIdx.y % ngroups) * G;
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    const int c8 = lane % LPK, ksub = lane / LPK;
    const int d = H * DH;
    const int nact = min(G, n - g0);                                 // queries of this group that are rows
    const int row0 = b * n + g0;
    // the live rows of the group, one bit per query
    unsigned alive = 0;
#pragma unroll
    for (int g = 0; g < G; g++) alive |= (live == nullptr || live[group_row(b, n, g0, g)] != 0) ? 1u << g : 0u;
    if (alive == 0) {                                                // no live row: no ring byte is read, piece 0 leaves zeros
        if (blockIdx.z == 0)
            for (int i = tid; i < nact * DH; i += 256) out[(size_t)(row0 + i / DH) * d + h * DH + i % DH] = f2bf(0.f);
        return;
    }
    const int t = *t_dev, Tp = *t0_dev;
    const int tm = t % M;
    const RingPiece pc = ring_piece(t, M);
    const int lo = pc.lo, hi = pc.hi, plo = pc.plo, phi = pc.phi;
    const int NS = gridDim.z, zi = blockIdx.z;
    const int nw = hi - lo;                                          // scores: written slot s at s - lo, never-written sp at nw + sp - plo
    // the tail slots: the nt slots that end at tm going round the ring (distance to tm below nt).  In ascending slot order the
    // written slots are three runs [lo, cx) [cx, cy) [cy, hi) of alternating source, the first one from the tail iff `tail_first`
    const int nt = min(max(t - Tp + 1, 0), M);
    const int ta = tm - nt + 1;
    const bool tail_first = ta < 0;
    const int cx = min(max(tail_first ? tm + 1 : ta, lo), hi), cy = min(max(tail_first ? ta + M : tm + 1, lo), hi);
    // tail slot of ring slot s (a tail slot: its position t - dist is Tp or later)
    auto tail_slot = [&](int s) {
        int dist = tm - s;
        if (dist < 0) dist += M;
        return (t - dist - Tp) % Mt;
    };

    float qw[G][8];
#pragma unroll
    for (int g = 0; g < G; g++) {
        const bf16x8 qv = *reinterpret_cast<const bf16x8*>(qkv + (size_t)group_row(b, n, g0, g) * 3 * d + h * DH + c8 * 8);
#pragma unroll
        for (int j = 0; j < 8; j++) qw[g][j] = biased_query((bf16_t)qv[j], rwb[h * DH + c8 * 8 + j]);
    }
    // the positional terms of the written slots wait where the score will go (decode_shared.hip)
    const float* bdh = bd + (size_t)h * M;
    size_t bdoff[G];
#pragma unroll
    for (int g = 0; g < G; g++) bdoff[g] = (size_t)group_row(b, n, g0, g) * H * M;
#pragma clang loop vectorize(disable) unroll(disable)
    for (int i = tid; i < nw; i += 256) {
        int dist = tm - (lo + i);
        if (dist < 0) dist += M;
#pragma unroll
        for (int g = 0; g < G; g++) sc[g * cap + i] = bdh[bdoff[g] + dist];
    }
    __syncthreads();
    const bf16_t* kb = kp + ((size_t)b * H + h) * M * DH + c8 * 8;     // head-major ring of the prompt: rows are DH apart
    const bf16_t* vb = vp + ((size_t)b * H + h) * M * DH + c8 * 8;
    // head h of query g's tail ring: a workgroup-uniform base, to which a load adds a 32-bit lane offset (the scalar-base form)
    auto tail_of = [&](const bf16_t* ring, int g) { return ring + ((size_t)group_row(b, n, g0, g) * H + h) * Mt * DH; };

    // batch depth of the prompt runs: what the registers beside G queries and the G tail fragments leave without scratch (G = 8: 239
    // registers at depth 2, spills at 4; G = 4: 217 at depth 4).  The depth changes no bit: a lane visits its slots in ascending order.
    constexpr int U = G == 8 ? 2 : 4;
    constexpr int ST = 4 * KPW * U;        // slots per prompt batch of the workgroup
    constexpr int S1 = 4 * KPW;            // slots per tail batch: one slot per lane, G fragments
    const bf16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // pass 1: scores.  A score depends on its own slot alone, so the runs could come in any order; they come in pass 2's.
    float mx[G];
#pragma unroll
    for (int g = 0; g < G; g++) mx[g] = -1e30f;
    {
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
#pragma unroll 1
        for (int run = 0; run < 3; run++) {
            const int va = run == 0 ? lo : (run == 1 ? cx : cy), ve = run == 0 ? cx : (run == 1 ? cy : hi);
            if (va >= ve) continue;
            if (tail_first == ((run & 1) == 0)) {
                // a tail run: every query reads its own row.  One batch of G fragments in a rolling buffer: a fragment is used and the
                // same query's fragment of the next batch requested in its place, so G loads stay in flight
                bf16x8 tA[G];
                auto load_t = [&](int s0, int g) {
                    const int s = s0 + ksub;
                    const bool in = s >= va && s < ve && ((alive >> g) & 1);
                    return in ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(tail_of(kt, g) + (unsigned)(tail_slot(s) * DH + c8 * 8))) : z8;
                };
                int s0 = lo + wid * KPW + ((va - lo) / S1) * S1;
#pragma unroll
                for (int g = 0; g < G; g++) tA[g] = load_t(s0, g);
                for (; s0 < ve; s0 += S1) {
                    const int s = s0 + ksub;
#pragma unroll
                    for (int g = 0; g < G; g++) {
                        score(g, tA[g], s, s >= va && s < ve);
                        tA[g] = load_t(s0 + S1, g);             // (past the run: zeros, no load)
                    }
                }
            } else {
                // a prompt run: double-buffered batches of U key groups with non-temporal loads, a fragment used G times
                bf16x8 kA[U], kB[U];
                auto load_k = [&](int s0, bf16x8 (&kv)[U]) {
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const int s = s0 + u * 4 * KPW + ksub;
                        kv[u] = (s >= va && s < ve) ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(kb + (size_t)s * DH)) : z8;
                    }
                };
                auto use_k = [&](int s0, const bf16x8 (&kv)[U]) {
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const int s = s0 + u * 4 * KPW + ksub;
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int g = 0; g < G; g++) score(g, kv[u], s, s >= va && s < ve);
                    }
                };
                int s0 = lo + wid * KPW + ((va - lo) / ST) * ST;
                if (s0 < ve) load_k(s0, kA);
                for (; s0 < ve; s0 += 2 * ST) {
                    if (s0 + ST < ve) load_k(s0 + ST, kB);
                    use_k(s0, kA);
                    if (s0 + ST < ve) {
                        if (s0 + 2 * ST < ve) load_k(s0 + 2 * ST, kA);
                        use_k(s0 + ST, kB);
                    }
                }
            }
        }
    }
    group_score_unwritten<G>(sc, cap, bdh, bdoff, tm, nw, plo, phi, M, scale, mx);
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

    // pass 2: o = sum_s p_s v_s   (P rounded to bf16), the three runs in ascending order
    float o[G][8];
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
        for (int j = 0; j < 8; j++) o[g][j] = 0.f;
    {
        auto add = [&](int g, const bf16x8& vv, int s, bool in) { group_add(sc, g * cap + s - lo, o[g], vv, in); };
#pragma unroll 1
        for (int run = 0; run < 3; run++) {
            const int va = run == 0 ? lo : (run == 1 ? cx : cy), ve = run == 0 ? cx : (run == 1 ? cy : hi);
            if (va >= ve) continue;
            if (tail_first == ((run & 1) == 0)) {
                bf16x8 tA[G];
                auto load_t = [&](int s0, int g) {
                    const int s = s0 + ksub;
                    const bool in = s >= va && s < ve && ((alive >> g) & 1);
                    return in ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(tail_of(vt, g) + (unsigned)(tail_slot(s) * DH + c8 * 8))) : z8;
                };
                int s0 = lo + wid * KPW + ((va - lo) / S1) * S1;
#pragma unroll
                for (int g = 0; g < G; g++) tA[g] = load_t(s0, g);
                for (; s0 < ve; s0 += S1) {
                    const int s = s0 + ksub;
#pragma unroll
                    for (int g = 0; g < G; g++) {
                        add(g, tA[g], s, s >= va && s < ve);
                        tA[g] = load_t(s0 + S1, g);
                    }
                }
            } else {
                bf16x8 vA[U], vB[U];
                auto load_v = [&](int s0, bf16x8 (&vv)[U]) {
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const int s = s0 + u * 4 * KPW + ksub;
                        vv[u] = (s >= va && s < ve) ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(vb + (size_t)s * DH)) : z8;
                    }
                };
                auto use_v = [&](int s0, const bf16x8 (&vv)[U]) {
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const int s = s0 + u * 4 * KPW + ksub;
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int g = 0; g < G; g++) add(g, vv[u], s, s >= va && s < ve);
                    }
                };
                int s0 = lo + wid * KPW + ((va - lo) / ST) * ST;
                if (s0 < ve) load_v(s0, vA);
                for (; s0 < ve; s0 += 2 * ST) {          // (the never-written slots hold v = 0: nothing to add)
                    if (s0 + ST < ve) load_v(s0 + ST, vB);
                    use_v(s0, vA);
                    if (s0 + ST < ve) {
                        if (s0 + 2 * ST < ve) load_v(s0 + 2 * ST, vA);
                        use_v(s0 + ST, vB);
                    }
                }
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
            out[(size_t)(row0 + g) * d + h * DH + e] = ((alive >> g) & 1) ? f2bf(red_of(g, e) * inv) : f2bf(0.f);
        }
        return;
    }
    // ---- ring pieces: every live query leaves (o unnormalised, max, sum) where decode_attn_kernel leaves its row's, as agent-scope
    // stores; the group shares the arrival counter of its first row, and its last piece merges every live query in piece order
    for (int i = tid; i < nact * DH; i += 256) {
        const int g = i / DH, e = i % DH;
        if ((alive >> g) & 1)
            MXL_AGENT_STORE(ws + ((size_t)(row0 + g) * H + h) * NS * (DH + 2) + zi * (DH + 2) + e, red_of(g, e));
    }
    if (tid < nact && ((alive >> tid) & 1)) {
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
        if (!((alive >> g) & 1)) {
            out[(size_t)(row0 + g) * d + h * DH + e] = f2bf(0.f);
            continue;
        }
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

// qr[b] = q + r_r_bias as kv_append_kernel writes it, and tail slot (t - t0) mod Mt of row b <- (k, v) of the (B, 3d) qkv rows: one
// thread per 8 elements.  t < t0 (a prompt position: the prompt pass wrote it) writes no ring.
__global__ void kv_append_tail_kernel(const bf16_t* qkv, bf16_t* kt, bf16_t* vt, const int* t_dev, const int* t0_dev, int B, int Mt,
                                      int d, int dh, const float* rrb, bf16_t* qr) {
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
    const int gen = *t_dev - *t0_dev;
    if (gen < 0) return;
    const int slot = gen % Mt;
    const int h = (c * 8) / dh, e = (c * 8) % dh, H = d / dh;
    const u32x4 k = *reinterpret_cast<const u32x4*>(qkv + (size_t)b * 3 * d + d + c * 8);
    const u32x4 v = *reinterpret_cast<const u32x4*>(qkv + (size_t)b * 3 * d + 2 * d + c * 8);
    const size_t o = (((size_t)b * H + h) * Mt + slot) * dh + e;
    *reinterpret_cast<u32x4*>(kt + o) = k;
    *reinterpret_cast<u32x4*>(vt + o) = v;
}

}  // namespace

extern "C" size_t mxl_relattn_decode_prefix_lds_bytes(int n, int dh, int M, int pieces) {
    if (n < 2 || dh <= 0 || M <= 0 || pieces < 1 || pieces > 8) return 0;
    return prefix_lds(group_size(n), dh, group_cap(M, pieces));
}

extern "C" int mxl_relattn_decode_prefix(const void* qkv, const void* kprompt, const void* vprompt, const void* ktail, const void* vtail,
                                         const float* bd, const float* r_w_bias, void* out, const int* t_dev, const int* t0_dev, int B0,
                                         int n, int H, int dh, int M, int Mt, float scale, int pieces, float* ws, int* arrived,
                                         const int* unfinished, void* stream) {
    MXL_CHECK_ARG(qkv && kprompt && vprompt && ktail && vtail && bd && r_w_bias && out && t_dev && t0_dev && B0 > 0 && H > 0);
    MXL_CHECK_ARG(M >= 16 && (M % 16) == 0 && Mt >= 16 && Mt <= M && (Mt % 16) == 0 && n >= 2 && pieces >= 1 && pieces <= 8);
    if (pieces > 1) MXL_CHECK_ARG(ws && arrived);
    MXL_CHECK_ARG(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)kprompt % 16) == 0 && ((uintptr_t)vprompt % 16) == 0 &&
                  ((uintptr_t)ktail % 16) == 0 && ((uintptr_t)vtail % 16) == 0);
    if (dh != 16 && dh != 32 && dh != 64) return MXL_EUNSUPPORTED;
    const int G = group_size(n), cap = group_cap(M, pieces);
    const size_t shm = prefix_lds(G, dh, cap);
    MXL_CHECK_ARG(shm <= (size_t)GROUP_LDS_MAX && (long long)B0 * ((n + G - 1) / G) <= 65535);
    hipStream_t s = (hipStream_t)stream;
    const int ngroups = (n + G - 1) / G;
#define LAUNCH(DH, GG) return launch_big_lds<&decode_attn_prefix_kernel<DH, GG>>(                                                              \
        dim3(H, B0 * ngroups, pieces), shm, s, (const bf16_t*)qkv, (const bf16_t*)kprompt, (const bf16_t*)vprompt, (const bf16_t*)ktail,      \
        (const bf16_t*)vtail, bd, r_w_bias, (bf16_t*)out, t_dev, t0_dev, n, ngroups, H, M, Mt, scale, ws, arrived, unfinished, cap)
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

extern "C" int mxl_kv_append_tail(const void* qkv, void* ktail, void* vtail, const int* t_dev, const int* t0_dev, int B, int Mt, int d,
                                  int dh, const float* r_r_bias, void* qr_out, void* stream) {
    MXL_CHECK_ARG(qkv && ktail && vtail && t_dev && t0_dev && B > 0 && d > 0 && (d % 8) == 0 && dh > 0 && (dh % 8) == 0 && (d % dh) == 0);
    MXL_CHECK_ARG(Mt >= 16 && (Mt % 16) == 0);
    MXL_CHECK_ARG(!qr_out || r_r_bias);
    MXL_CHECK_ARG(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)ktail % 16) == 0 && ((uintptr_t)vtail % 16) == 0 &&
                  ((uintptr_t)qr_out % 16) == 0);
    const int n = B * (d / 8);
    hipLaunchKernelGGL(kv_append_tail_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (bf16_t*)ktail,
                       (bf16_t*)vtail, t_dev, t0_dev, B, Mt, d, dh, r_r_bias, (bf16_t*)qr_out);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}
