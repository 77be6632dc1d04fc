// Ring attention of one Transformer-XL decode step over bf16 K/V rings (decode.hip says what a ring is and writes it): one query
// per workgroup, its ring read either from the row's own rings or, slot by slot, through an owner table.
//
// OWNED (beam search with beam_rings='indexed'): the K row and the V row of a written slot s of row b are read from the ring of row
// (b / nb) * nb + owner[b][s].  A ring slot written for position p never changes, so a beam points at the slot in its ancestor's ring
// instead of owning a copy; the (rows, M) owner table is kept by mxl_beam_owner_follow (beam.hip), which states the wrap argument.
// The table is a template parameter of the one kernel: everything but the source row of a load is one text -- which thread takes
// which slot and in which order, the pieces and their last-arrival merge, the `live` skip, the never-written slots, P rounded to bf16
// -- so on rings gathered by the table the plain kernel gives the same bits, and the identity table gives its bits on the same rings
// (tests/test_beam_owner_ops_gpu.py).
#include "decode_attn.h"
#include "musicxl_internal.h"

namespace {

// one workgroup per (head, batch row, ring piece); dh = 8 * LPK, LPK lanes share one key row, 64/LPK keys per wave instruction.
// gridDim.z = NS pieces of the ring (round 5).  A CU streams HBM at ~24 GB/s however many workgroups it holds, so a launch of
// B * H workgroups that is not a multiple of the CU count is as slow as its fullest CU: 384 rings (a lane's 32 sequences x 12
// heads) on 256 CUs take the time of two rings (1 MB: 40.6 us) where 768 half-rings take that of 1.5 (profiles/r05_decode_notes.txt).
// The pieces and their merge are decode_attn.h's; NS = 1 is the single-workgroup form, bit for bit as before.
// Dynamic LDS: scores [M] f32, the output scratch [4][64] f32 and, OWNED, the row's M owner bytes (M % 16 == 0 and B % nb == 0 are
// the entry's to check).
template <int DH, bool OWNED>
__global__ __launch_bounds__(256) void decode_attn_kernel(const bf16_t* qkv, const bf16_t* kc, const bf16_t* vc,
                                                          const float* bd, const float* rwb,
                                                          bf16_t* out, const int* t_dev, int B, int H, int M, float scale,
                                                          float* ws, int* arrived, const int* live,
                                                          const unsigned char* owner, int nb) {
    constexpr int LPK = DH / 8;          // lanes per key row
    constexpr int KPW = 64 / LPK;        // keys per wave per iteration
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sc = reinterpret_cast<float*>(smem);          // [M] scores -> probabilities
    float* red = sc + M;                                 // [4][DH] scratch: 4 * 64 floats max
    __shared__ float wred[8];
    const int h = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    const int c8 = lane % LPK, ksub = lane / LPK;
    const int d = H * DH;
    // a finished row (live[b] == 0, mxl_relattn_decode_split_live): no K / V byte and no owner byte is read; piece 0 leaves zeros in
    // the output slice so that the GEMMs after it never see an uninitialised row, and the other pieces leave at once (the arrival
    // counter of the (sequence, head) is not touched: it stays zero)
    if (live != nullptr && live[b] == 0) {
        if (blockIdx.z == 0 && tid < DH) out[(size_t)b * d + h * DH + tid] = f2bf(0.f);
        return;
    }
    const int t = *t_dev;
    const int tm = t % M;
    const int NS = gridDim.z;
    const RingPiece pc = ring_piece(t, M);
    const int lo = pc.lo, hi = pc.hi, plo = pc.plo, phi = pc.phi;

    float qw[8];
    {
        const bf16x8 qv = *reinterpret_cast<const bf16x8*>(qkv + (size_t)b * 3 * d + h * DH + c8 * 8);
#pragma unroll
        for (int j = 0; j < 8; j++) qw[j] = biased_query((bf16_t)qv[j], rwb[h * DH + c8 * 8 + j]);
    }
    // positional term BD[b,h,dist] = (q + r_r_bias) . Rd[dist], precomputed for the whole batch by one batched GEMM per layer
    // (reads the Rd table once per head instead of once per (sequence, head))
    const float* bdrow = bd + ((size_t)b * H + h) * M;
    // kb / vb are head h of the row's own rings (head-major: rows are DH apart) or, OWNED, of row 0's, to which ring_at adds the source row and the slot
    const bf16_t* kb = kc + ((size_t)(OWNED ? 0 : b) * H + h) * M * DH + c8 * 8;
    const bf16_t* vb = vc + ((size_t)(OWNED ? 0 : b) * H + h) * M * DH + c8 * 8;
    // OWNED: the row's M owner bytes, staged once behind `red`: 16 bytes per thread
    const unsigned char* own = reinterpret_cast<const unsigned char*>(red + 4 * 64);
    if constexpr (OWNED) {
        const u32x4* from = reinterpret_cast<const u32x4*>(owner + (size_t)b * M);
        u32x4* to = reinterpret_cast<u32x4*>(red + 4 * 64);
        for (int i = tid; i < (M >> 4); i += 256) to[i] = from[i];
        __syncthreads();
    }
    // OWNED: element offset of slot s from kb / vb.  An owner byte beyond the item (mxl_beam_owner_follow writes none) is held to
    // the item's last row, so no table sends a read outside the rings; no owner byte of a never-written slot is looked at.
    // (The plain side forms its offset in a statement of its own at the two loads: with both sides behind one expression its
    // dh = 32 instantiation got other register numbers than it had.)
    const size_t ring_stride = (size_t)H * M * DH;
    const int item0 = (b / nb) * nb;
    auto ring_at = [&](int s) -> size_t { return (size_t)(item0 + min((int)own[s], nb - 1)) * ring_stride + (size_t)s * DH; };

    // pass 1: scores.  Explicit batches of U key groups: all U loads of a batch are issued before any is consumed, and batch i + 1
    // is requested before batch i is consumed (two register sets), so each wave keeps 16-32 KiB in flight the whole pass (a plain
    // unroll pragma left one load per iteration on the critical path: ~HBM latency per 8 keys; single batches of 16 drained
    // between batches: 1.31 -> 1.24 ms per full-ring step with the second set and the V prefetch below).
    // The ring rows are read once per step and there are 4.8 GB of them: non-temporal loads, so that they do not push the
    // step's weights, bd and activations out of L2 / MALL (measured over the C5 generation: 51.6 -> 56.2 k tok/s; U 8 -> 16
    // another +1 %).  250 registers (OWNED: 254), no scratch: two workgroups per CU; 12 / 16-deep batches held to 168 registers (three
    // per CU) spill and run at half the speed, 20-deep ones spill too.
    constexpr int U = 16;                   // double-buffered batches: batch i + 1 is requested before batch i is consumed
    float mx = -1e30f;
    {
        bf16x8 kA[U], kB[U];
        float bA[U], bB[U];
        auto load_k = [&](int s0, bf16x8 (&kv)[U], float (&bv)[U]) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int s = s0 + u * 4 * KPW + ksub;
                const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
                if constexpr (OWNED) kv[u] = (s < hi) ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(kb + ring_at(s))) : z;
                else kv[u] = (s < hi) ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(kb + (size_t)s * DH)) : z;
                int dist = tm - s;
                if (dist < 0) dist += M;
                bv[u] = (s < M && c8 == 0) ? bdrow[dist] : 0.f;
            }
        };
        auto use_k = [&](int s0, const bf16x8 (&kv)[U], const float (&bv)[U]) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int s = s0 + u * 4 * KPW + ksub;
                float acc = bv[u];
#pragma unroll
                for (int j = 0; j < 8; j++) acc += qw[j] * bf2f((bf16_t)kv[u][j]);
#pragma unroll
                for (int o = 1; o < LPK; o <<= 1) acc += __shfl_xor(acc, o, 64);
                acc *= scale;
                if (s < hi) {
                    if (c8 == 0) sc[s] = acc;
                    mx = fmaxf(mx, acc);
                }
            }
        };
        // Only the batches that hold a written slot: the ring slots [nvalid, M) are zero memories, whose score is the positional term
        // alone -- they take ONE multiply each (below) instead of a zero dot product, its lane reduction and the batch bookkeeping.
        // (Until round 5 both passes walked all M slots whatever the sequence length: at 1153 written slots of 2048 -- the mean over
        // the C5 generation -- the kernel took 35.7 us against 40.3 us with a full ring, i.e. it was bound by that loop, not by HBM.)
        constexpr int ST = 4 * KPW * U;
        int s0 = lo + wid * KPW;
        if (s0 < hi) load_k(s0, kA, bA);
        for (; s0 < hi; s0 += 2 * ST) {
            if (s0 + ST < hi) load_k(s0 + ST, kB, bB);
            use_k(s0, kA, bA);
            if (s0 + ST < hi) {
                if (s0 + 2 * ST < hi) load_k(s0 + 2 * ST, kA, bA);
                use_k(s0 + ST, kB, bB);
            }
        }
    }
    for (int sp = plo + tid; sp < phi; sp += 256) {      // the never-written slots: score = scale * BD[distance]
        int dist = tm - sp;
        if (dist < 0) dist += M;
        const float a = bdrow[dist] * scale;
        sc[sp] = a;
        mx = fmaxf(mx, a);
    }
    // the first V batch is requested before the softmax section: its latency runs under the two barriers and the exponentials
    bf16x8 vA[U], vB[U];
    auto load_v = [&](int s0, bf16x8 (&vv)[U]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int s = s0 + u * 4 * KPW + ksub;
            const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            if constexpr (OWNED) vv[u] = (s < hi) ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(vb + ring_at(s))) : z;
            else vv[u] = (s < hi) ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(vb + (size_t)s * DH)) : z;
        }
    };
    if (lo + wid * KPW < hi) load_v(lo + wid * KPW, vA);
    mx = wave_max(mx);
    if (lane == 0) wred[wid] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
    float sum = 0.f;
    for (int s = lo + tid; s < hi; s += 256) {
        const float pv = __expf(sc[s] - mx);
        sc[s] = pv;
        sum += pv;
    }
    for (int s = plo + tid; s < phi; s += 256) sum += __expf(sc[s] - mx);      // (v = 0 there: only the denominator)
    sum = wave_sum(sum);
    if (lane == 0) wred[4 + wid] = sum;
    __syncthreads();
    const float inv = 1.f / (wred[4] + wred[5] + wred[6] + wred[7]);

    // pass 2: o = sum_s p_s v_s   (P rounded to bf16 like the training kernel's MFMA operand); same batched loads
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] = 0.f;
    {
        auto use_v = [&](int s0, const bf16x8 (&vv)[U]) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int s = s0 + u * 4 * KPW + ksub;
                const float pv = (s < hi) ? bf2f(f2bf(sc[s])) : 0.f;
#pragma unroll
                for (int j = 0; j < 8; j++) o[j] += pv * bf2f((bf16_t)vv[u][j]);
            }
        };
        constexpr int ST = 4 * KPW * U;
        int s0 = lo + wid * KPW;
        for (; s0 < hi; s0 += 2 * ST) {          // (the never-written slots hold v = 0: nothing to add)
            if (s0 + ST < hi) load_v(s0 + ST, vB);
            use_v(s0, vA);
            if (s0 + ST < hi) {
                if (s0 + 2 * ST < hi) load_v(s0 + 2 * ST, vA);
                use_v(s0 + ST, vB);
            }
        }
    }
    reduce_o<LPK>(o, red + wid * DH + c8 * 8, ksub);
    __syncthreads();
    if (NS == 1) {
        if (tid < DH) out[(size_t)b * d + h * DH + tid] = f2bf(red_sum(red, DH, tid) * inv);
        return;
    }
    pieces_tail<DH>(ws, arrived, b, h, H, red, mx, wred + 4, out);
}

template <bool OWNED>
int relattn_decode_launch(const void* qkv, const void* kcache, const void* vcache, const void* owner, int nb, const float* bd,
                          const float* r_w_bias, void* out, const int* t_dev, int B, int H, int dh, int M, float scale, int pieces,
                          float* ws, int* arrived, const int* live, size_t shm, void* stream) {
    MXL_CHECK_ARG(shm <= 64 * 1024);
    dim3 grid(H, B, pieces);
    hipStream_t s = (hipStream_t)stream;
#define LAUNCH(DH) hipLaunchKernelGGL((decode_attn_kernel<DH, OWNED>), grid, dim3(256), shm, s, (const bf16_t*)qkv, (const bf16_t*)kcache, \
                                      (const bf16_t*)vcache, bd, r_w_bias, (bf16_t*)out, t_dev, B, H, M, scale, ws, arrived, live,        \
                                      (const unsigned char*)owner, nb)
    switch (dh) {
        case 16: LAUNCH(16); break;
        case 32: LAUNCH(32); break;
        case 64: LAUNCH(64); break;
        default: return MXL_EUNSUPPORTED;
    }
#undef LAUNCH
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

int relattn_decode_plain(const void* qkv, const void* kcache, const void* vcache, const float* bd, const float* r_w_bias, void* out,
                         const int* t_dev, int B, int H, int dh, int M, float scale, int pieces, float* ws, int* arrived,
                         const int* live, void* stream) {
    MXL_CHECK_ARG(qkv && kcache && vcache && bd && r_w_bias && out && t_dev && B > 0 && H > 0 && M > 0);
    return relattn_decode_launch<false>(qkv, kcache, vcache, nullptr, 1, bd, r_w_bias, out, t_dev, B, H, dh, M, scale, pieces, ws,
                                        arrived, live, (size_t)M * 4 + 4 * 64 * 4, stream);
}

}  // namespace

extern "C" int mxl_relattn_decode(const void* qkv, const void* kcache, const void* vcache, const float* bd,
                                  const float* r_w_bias, void* out, const int* t_dev, int B, int H,
                                  int dh, int M, float scale, void* stream) {
    return relattn_decode_plain(qkv, kcache, vcache, bd, r_w_bias, out, t_dev, B, H, dh, M, scale, 1, nullptr, nullptr, nullptr, stream);
}

extern "C" size_t mxl_relattn_decode_split_ws_bytes(int B, int H, int dh, int pieces) {
    if (B <= 0 || H <= 0 || dh <= 0 || pieces < 1) return 0;
    return (size_t)B * H * pieces * (dh + 2) * sizeof(float);
}

extern "C" int mxl_relattn_decode_split(const void* qkv, const void* kcache, const void* vcache, const float* bd,
                                        const float* r_w_bias, void* out, const int* t_dev, int B, int H, int dh, int M, float scale,
                                        int pieces, float* ws, int* arrived, void* stream) {
    MXL_CHECK_ARG(pieces >= 1 && pieces <= 8);
    if (pieces > 1) MXL_CHECK_ARG(ws && arrived);
    return relattn_decode_plain(qkv, kcache, vcache, bd, r_w_bias, out, t_dev, B, H, dh, M, scale, pieces, ws, arrived, nullptr, stream);
}

extern "C" int mxl_relattn_decode_split_live(const void* qkv, const void* kcache, const void* vcache, const float* bd,
                                             const float* r_w_bias, void* out, const int* t_dev, int B, int H, int dh, int M,
                                             float scale, int pieces, float* ws, int* arrived, const int* unfinished, void* stream) {
    MXL_CHECK_ARG(pieces >= 1 && pieces <= 8);
    if (pieces > 1) MXL_CHECK_ARG(ws && arrived);
    return relattn_decode_plain(qkv, kcache, vcache, bd, r_w_bias, out, t_dev, B, H, dh, M, scale, pieces, ws, arrived, unfinished,
                                stream);
}

extern "C" int mxl_relattn_decode_owned(const void* qkv, const void* kcache, const void* vcache, const void* owner, int nb,
                                        const float* bd, const float* r_w_bias, void* out, const int* t_dev, int B, int H, int dh,
                                        int M, float scale, int pieces, float* ws, int* arrived, const int* unfinished, void* stream) {
    MXL_CHECK_ARG(qkv && kcache && vcache && owner && bd && r_w_bias && out && t_dev && ((uintptr_t)owner % 16) == 0);
    MXL_CHECK_ARG(nb >= 1 && nb <= 16 && B > 0 && B <= 65535 && (B % nb) == 0 && H > 0 && M > 0 && (M % 16) == 0);
    MXL_CHECK_ARG(pieces >= 1 && pieces <= 8);
    if (pieces > 1) MXL_CHECK_ARG(ws && arrived);
    return relattn_decode_launch<true>(qkv, kcache, vcache, owner, nb, bd, r_w_bias, out, t_dev, B, H, dh, M, scale, pieces, ws,
                                       arrived, unfinished, (size_t)M * 4 + 4 * 64 * 4 + (size_t)M, stream);
}
