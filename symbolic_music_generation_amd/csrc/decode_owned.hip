// Ring attention of one decode step over indexed rings (beam search with beam_rings='indexed'): decode_attn_kernel of decode.hip with
// the K row and the V row of a written slot s of row b read from the ring of row (b / nb) * nb + owner[b][s].  A ring slot written
// for position p never changes, so a beam points at the slot in its ancestor's ring instead of owning a copy; the (rows, M) owner
// table is kept by mxl_beam_owner_follow (beam.hip), which states the wrap argument.
//
// This is a copy of that kernel, not a parameter of it, so that its instantiations stay the code they were.  Everything but the source
// row of a load is the same in the same order -- which thread takes which slot and in which order, the pieces and their last-arrival
// merge, the `live` skip, the never-written slots, P rounded to bf16 -- so on rings gathered by the table decode_attn_kernel gives the
// same bits, and the identity table gives its bits on the same rings (tests/test_beam_owner_ops_gpu.py).
#include "common.h"
#include "musicxl_internal.h"

namespace {

// grid (head, row, ring piece), 256 threads, M * 5 + 1024 bytes of dynamic LDS: scores [M] f32, the output scratch [4][64] f32, then
// the row's M owner bytes.  M % 16 == 0 and B % nb == 0 are the entry's to check.
template <int DH>
__global__ __launch_bounds__(256) void decode_attn_owned_kernel(const bf16_t* qkv, const bf16_t* kc, const bf16_t* vc,
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
    // a finished row (live[b] == 0): no K / V byte and no owner byte is read; piece 0 leaves zeros in the output slice
    if (live != nullptr && live[b] == 0) {
        if (blockIdx.z == 0 && tid < DH) out[(size_t)b * d + h * DH + tid] = f2bf(0.f);
        return;
    }
    const int t = *t_dev;
    const int tm = t % M;
    // never-written slots [nvalid, M): the positional term alone, no K / V read and no owner byte looked at
    const int nvalid = t + 1 < M ? t + 1 : M;
    // this piece's written slots [lo, hi) and never-written slots [plo, phi)
    const int NS = gridDim.z, zi = blockIdx.z;
    const int piece = NS > 1 ? ((((nvalid + NS - 1) / NS) + 31) & ~31) : nvalid;
    const int lo = min(zi * piece, nvalid), hi = min(lo + piece, nvalid);
    const int ppiece = (M - nvalid + NS - 1) / NS;
    const int plo = min(nvalid + zi * ppiece, M), phi = min(plo + ppiece, M);

    float qw[8];
    {
        const bf16x8 qv = *reinterpret_cast<const bf16x8*>(qkv + (size_t)b * 3 * d + h * DH + c8 * 8);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float q = bf2f((bf16_t)qv[j]);
            // mirror the training kernels: (q + bias) is rounded to bf16 before the contraction
            qw[j] = bf2f(f2bf(q + rwb[h * DH + c8 * 8 + j]));
        }
    }
    // positional term BD[b,h,dist] = (q + r_r_bias) . Rd[dist], precomputed for the whole batch by one batched GEMM per layer
    // (reads the Rd table once per head instead of once per (sequence, head))
    const float* bdrow = bd + ((size_t)b * H + h) * M;
    // kb / vb are head h of row 0's rings (head-major: rows are DH apart), and ring_at adds the source row of a slot
    const bf16_t* kb = kc + (size_t)h * M * DH + c8 * 8;
    const bf16_t* vb = vc + (size_t)h * M * DH + c8 * 8;
    // the row's M owner bytes, staged once behind `red`: 16 bytes per thread
    const unsigned char* own = reinterpret_cast<const unsigned char*>(red + 4 * 64);
    {
        const u32x4* from = reinterpret_cast<const u32x4*>(owner + (size_t)b * M);
        u32x4* to = reinterpret_cast<u32x4*>(red + 4 * 64);
        for (int i = tid; i < (M >> 4); i += 256) to[i] = from[i];
        __syncthreads();
    }
    // element offset of slot s from kb / vb; an owner byte beyond the item (mxl_beam_owner_follow writes none) is held to the
    // item's last row, so no table sends a read outside the rings
    const size_t ring_stride = (size_t)H * M * DH;
    const int item0 = (b / nb) * nb;
    auto ring_at = [&](int s) -> size_t { return (size_t)(item0 + min((int)own[s], nb - 1)) * ring_stride + (size_t)s * DH; };

    // pass 1: scores, in double-buffered batches of U key groups with non-temporal loads (decode_attn_kernel: why, and what the
    // register budget allows).  254 registers here against its 250 (dh = 64), no scratch: two workgroups per CU as there.
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
                kv[u] = (s < hi) ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(kb + ring_at(s))) : z;
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
        // only the batches that hold a written slot; the never-written slots take one multiply each below
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
            vv[u] = (s < hi) ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(vb + ring_at(s))) : z;
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
#pragma unroll
    for (int j = 0; j < 8; j++) {
#pragma unroll
        for (int off = LPK; off < 64; off <<= 1) o[j] += __shfl_xor(o[j], off, 64);
    }
    if (ksub == 0) {
#pragma unroll
        for (int j = 0; j < 8; j++) red[wid * DH + c8 * 8 + j] = o[j];
    }
    __syncthreads();
    if (NS == 1) {
        if (tid < DH) {
            const float v = (red[tid] + red[DH + tid] + red[2 * DH + tid] + red[3 * DH + tid]) * inv;
            out[(size_t)b * d + h * DH + tid] = f2bf(v);
        }
        return;
    }
    // ---- ring pieces: leave (o unnormalised, max, sum) as agent-scope stores, the last arrival merges in piece order (decode_attn_kernel)
    float* wsp = ws + ((size_t)b * H + h) * NS * (DH + 2);
    if (tid < DH)
        __hip_atomic_store(wsp + zi * (DH + 2) + tid, red[tid] + red[DH + tid] + red[2 * DH + tid] + red[3 * DH + tid], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) {
        __hip_atomic_store(wsp + zi * (DH + 2) + DH, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(wsp + zi * (DH + 2) + DH + 1, wred[4] + wred[5] + wred[6] + wred[7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int s_last;
    if (tid == 0) s_last = (__hip_atomic_fetch_add(arrived + (size_t)b * H + h, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == NS - 1) ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    if (tid < DH) {
        float m = -1e30f;
        for (int k = 0; k < NS; k++) m = fmaxf(m, __hip_atomic_load(wsp + k * (DH + 2) + DH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        float num = 0.f, den = 0.f;
        for (int k = 0; k < NS; k++) {
            const float a = __expf(__hip_atomic_load(wsp + k * (DH + 2) + DH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - m);
            num += a * __hip_atomic_load(wsp + k * (DH + 2) + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            den += a * __hip_atomic_load(wsp + k * (DH + 2) + DH + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        out[(size_t)b * d + h * DH + tid] = f2bf(num / den);
    }
    if (tid == 0) __hip_atomic_store(arrived + (size_t)b * H + h, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

extern "C" int mxl_relattn_decode_owned(const void* qkv, const void* kcache, const void* vcache, const void* owner, int nb,
                                        const float* bd, const float* r_w_bias, void* out, const int* t_dev, int B, int H, int dh,
                                        int M, float scale, int pieces, float* ws, int* arrived, const int* unfinished, void* stream) {
    MXL_CHECK_ARG(qkv && kcache && vcache && owner && bd && r_w_bias && out && t_dev && ((uintptr_t)owner % 16) == 0);
    MXL_CHECK_ARG(nb >= 1 && nb <= 16 && B > 0 && B <= 65535 && (B % nb) == 0 && H > 0 && M > 0 && (M % 16) == 0);
    MXL_CHECK_ARG(pieces >= 1 && pieces <= 8);
    if (pieces > 1) MXL_CHECK_ARG(ws && arrived);
    const size_t shm = (size_t)M * 4 + 4 * 64 * 4 + (size_t)M;
    MXL_CHECK_ARG(shm <= 64 * 1024);
    dim3 grid(H, B, pieces);
    hipStream_t s = (hipStream_t)stream;
#define LAUNCH(DH) hipLaunchKernelGGL((decode_attn_owned_kernel<DH>), grid, dim3(256), shm, s, (const bf16_t*)qkv, (const bf16_t*)kcache, \
                                      (const bf16_t*)vcache, bd, r_w_bias, (bf16_t*)out, t_dev, B, H, M, scale, ws, arrived, unfinished,  \
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
