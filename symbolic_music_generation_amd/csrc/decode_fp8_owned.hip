// Ring attention of one decode step over indexed FP8 rings (beam search with beam_rings='indexed' on a decoder with kv_dtype='fp8'):
// decode_attn_fp8_kernel of decode_fp8.hip with the 16 K bytes, the 16 V bytes and the two exponents of a written slot s of row b
// read from the rings of row (b / nb) * nb + owner[b][s].  That is the relation decode_attn_owned_kernel (decode_owned.hip) has to
// decode_attn_kernel: a ring slot written for position p never changes, so a beam points at the slot in its ancestor's ring, and
// the (rows, M) owner table is kept by mxl_beam_owner_follow (beam.hip).  The writers are the ones of decode_fp8.hip: every row
// appends to its own ring, which is the slot the follow kernel marks as the row's own.
//
// This is a copy of that kernel, not a parameter of it, and decode_fp8.hip / decode_owned.hip are not touched, so their
// instantiations stay the code they were.  Everything but the source row of a load is the same in the same order -- which lane
// takes which slot, 2^ke staged in sc[s], bf16(p) 2^ve as the P V operand, the pieces and their last-arrival merge, the `live`
// skip, the never-written slots -- so on rings gathered by the table decode_attn_fp8_kernel gives the same bits, and the identity
// table gives its bits on the same rings (tests/test_beam_fp8_owned_ops_gpu.py).  The batch depth changes no bit: a lane visits
// its slots in ascending order whatever it is.
#include "common.h"
#include "musicxl_internal.h"

namespace {

// depth of the double-buffered batches.  decode_attn_fp8_kernel runs 12 in 168 registers (dh = 64), three workgroups per CU.  The
// source row of every load in flight costs registers here: 12 takes 182 (two workgroups per CU), 11 takes 168 again, 10 takes 162,
// 8 takes 128; none of them spills.  11 keeps the three workgroups, and measured (a lane at a full ring, identity table, two passes
// per build: profiles/beam_fp8_rings.txt) it is 27.4 / 27.6 us against 28.3 / 28.5 for 12 and 27.8 / 27.6 for 8.
constexpr int FP8_OWNED_U = 11;

typedef float fp8o_f2 __attribute__((ext_vector_type(2)));

// 2^n for n in [-126, 127]
__device__ __forceinline__ float fp8o_pow2(int n) { return __uint_as_float((uint32_t)(n + 127) << 23); }

// 16 e4m3fn bytes -> 16 f32 (v_cvt_pk_f32_fp8: two elements per instruction)
__device__ __forceinline__ void fp8o_unpack16(const u32x4 w, float (&f)[16]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const fp8o_f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
        const fp8o_f2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
        f[4 * i] = lo[0]; f[4 * i + 1] = lo[1]; f[4 * i + 2] = hi[0]; f[4 * i + 3] = hi[1];
    }
}

// grid (head, row, ring piece), 256 threads, M * 5 + 1024 bytes of dynamic LDS: sc [M] f32 (2^ke -> scores -> bf16(p) 2^ve), the
// output scratch [4][64] f32, then the row's M owner bytes.  M % 16 == 0 and B % nb == 0 are the entry's to check.
template <int DH, int U>
__global__ __launch_bounds__(256) void decode_attn_fp8_owned_kernel(const bf16_t* qkv, const unsigned char* kc8, const signed char* ke,
                                                                    const unsigned char* vc8, const signed char* ve, const float* bd,
                                                                    const float* rwb, bf16_t* out, const int* t_dev, int B, int H,
                                                                    int M, float scale, float* ws, int* arrived, const int* live,
                                                                    const unsigned char* owner, int nb) {
    constexpr int LPK = DH / 16;         // lanes per key row
    constexpr int KPW = 64 / LPK;        // keys per wave per iteration
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sc = reinterpret_cast<float*>(smem);          // [M] 2^ke -> scores -> bf16(p) 2^ve
    float* red = sc + M;                                 // [4][DH]: 4 * 64 floats max
    __shared__ float wred[8];
    const int h = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    const int c16 = lane % LPK, ksub = lane / LPK;
    const int d = H * DH;
    // a finished row (live[b] == 0): no ring byte and no owner byte is read; piece 0 leaves zeros, the counter is untouched
    if (live != nullptr && live[b] == 0) {
        if (blockIdx.z == 0 && tid < DH) out[(size_t)b * d + h * DH + tid] = f2bf(0.f);
        return;
    }
    const int t = *t_dev;
    const int tm = t % M;
    // never-written slots [nvalid, M): the positional term alone, no ring byte read and no owner byte looked at
    const int nvalid = t + 1 < M ? t + 1 : M;
    const int NS = gridDim.z, zi = blockIdx.z;
    const int piece = NS > 1 ? ((((nvalid + NS - 1) / NS) + 31) & ~31) : nvalid;
    const int lo = min(zi * piece, nvalid), hi = min(lo + piece, nvalid);
    const int ppiece = (M - nvalid + NS - 1) / NS;
    const int plo = min(nvalid + zi * ppiece, M), phi = min(plo + ppiece, M);

    float qw[16];
    {
        const bf16_t* qp = qkv + (size_t)b * 3 * d + h * DH + c16 * 16;
        const bf16x8 q0 = *reinterpret_cast<const bf16x8*>(qp), q1 = *reinterpret_cast<const bf16x8*>(qp + 8);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            qw[j] = bf2f(f2bf(bf2f((bf16_t)q0[j]) + rwb[h * DH + c16 * 16 + j]));
            qw[8 + j] = bf2f(f2bf(bf2f((bf16_t)q1[j]) + rwb[h * DH + c16 * 16 + 8 + j]));
        }
    }
    const float* bdrow = bd + ((size_t)b * H + h) * M;
    // kb / vb / ker / ver are head h of row 0's rings, and slot_at adds the source row of a slot: in slots for the exponents, times
    // DH in bytes for K and V
    const unsigned char* kb = kc8 + (size_t)h * M * DH + c16 * 16;
    const unsigned char* vb = vc8 + (size_t)h * M * DH + c16 * 16;
    const signed char* ker = ke + (size_t)h * M;
    const signed char* ver = ve + (size_t)h * M;
    // the row's M owner bytes, staged once behind `red`: 16 bytes per thread.  The K loads and the exponent staging need them, so
    // the barrier stands before the first K batch is issued
    const unsigned char* own = reinterpret_cast<const unsigned char*>(red + 4 * 64);
    {
        const u32x4* from = reinterpret_cast<const u32x4*>(owner + (size_t)b * M);
        u32x4* to = reinterpret_cast<u32x4*>(red + 4 * 64);
        for (int i = tid; i < (M >> 4); i += 256) to[i] = from[i];
        __syncthreads();
    }
    // an owner byte beyond the item (mxl_beam_owner_follow writes none) is held to the item's last row, so no table sends a read
    // outside the rings
    const size_t ring_stride = (size_t)H * M;
    const int item0 = (b / nb) * nb;
    auto slot_at = [&](int s) -> size_t { return (size_t)(item0 + min((int)own[s], nb - 1)) * ring_stride + (size_t)s; };

    // pass 1: scores, in double-buffered batches of U key groups as in decode_attn_fp8_kernel (non-temporal 16-byte loads)
    float mx = -1e30f;
    {
        u32x4 kA[U], kB[U];
        float bA[U], bB[U];
        auto load_k = [&](int s0, u32x4 (&kv)[U], float (&bv)[U]) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int s = s0 + u * 4 * KPW + ksub;
                const u32x4 z = {0u, 0u, 0u, 0u};
                kv[u] = (s < hi) ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kb + slot_at(s) * DH)) : z;
                int dist = tm - s;
                if (dist < 0) dist += M;
                bv[u] = (s < hi && c16 == 0) ? bdrow[dist] : 0.f;
            }
        };
        auto use_k = [&](int s0, const u32x4 (&kv)[U], const float (&bv)[U]) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int s = s0 + u * 4 * KPW + ksub;
                float kf[16];
                fp8o_unpack16(kv[u], kf);
                float dot = 0.f;
#pragma unroll
                for (int j = 0; j < 16; j++) dot += qw[j] * kf[j];
                float acc = bv[u] + dot * ((s < hi) ? sc[s] : 0.f);
#pragma unroll
                for (int o = 1; o < LPK; o <<= 1) acc += __shfl_xor(acc, o, 64);
                acc *= scale;
                if (s < hi) {
                    if (c16 == 0) sc[s] = acc;
                    mx = fmaxf(mx, acc);
                }
            }
        };
        constexpr int ST = 4 * KPW * U;
        int s0 = lo + wid * KPW;
        if (s0 < hi) load_k(s0, kA, bA);
        for (int s = lo + tid; s < hi; s += 256) sc[s] = fp8o_pow2((int)ker[slot_at(s)]);     // under the first batch's latency
        __syncthreads();
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
    u32x4 vA[U], vB[U];
    auto load_v = [&](int s0, u32x4 (&vv)[U]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int s = s0 + u * 4 * KPW + ksub;
            const u32x4 z = {0u, 0u, 0u, 0u};
            vv[u] = (s < hi) ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vb + slot_at(s) * DH)) : z;
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
        sc[s] = bf2f(f2bf(pv)) * fp8o_pow2((int)ver[slot_at(s)]);      // the P V operand: P rounded to bf16, times the slot's 2^e
        sum += pv;
    }
    for (int s = plo + tid; s < phi; s += 256) sum += __expf(sc[s] - mx);      // (v = 0 there: only the denominator)
    sum = wave_sum(sum);
    if (lane == 0) wred[4 + wid] = sum;
    __syncthreads();
    const float inv = 1.f / (wred[4] + wred[5] + wred[6] + wred[7]);

    // pass 2: o = sum_s p_s v_s; same batched loads
    float o[16];
#pragma unroll
    for (int j = 0; j < 16; j++) o[j] = 0.f;
    {
        auto use_v = [&](int s0, const u32x4 (&vv)[U]) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int s = s0 + u * 4 * KPW + ksub;
                const float pv = (s < hi) ? sc[s] : 0.f;
                float vf[16];
                fp8o_unpack16(vv[u], vf);
#pragma unroll
                for (int j = 0; j < 16; j++) o[j] += pv * vf[j];
            }
        };
        constexpr int ST = 4 * KPW * U;
        int s0 = lo + wid * KPW;
        for (; s0 < hi; s0 += 2 * ST) {
            if (s0 + ST < hi) load_v(s0 + ST, vB);
            use_v(s0, vA);
            if (s0 + ST < hi) {
                if (s0 + 2 * ST < hi) load_v(s0 + 2 * ST, vA);
                use_v(s0 + ST, vB);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
#pragma unroll
        for (int off = LPK; off < 64; off <<= 1) o[j] += __shfl_xor(o[j], off, 64);
    }
    if (ksub == 0) {
#pragma unroll
        for (int j = 0; j < 16; j++) red[wid * DH + c16 * 16 + j] = o[j];
    }
    __syncthreads();
    if (NS == 1) {
        if (tid < DH) {
            const float v = (red[tid] + red[DH + tid] + red[2 * DH + tid] + red[3 * DH + tid]) * inv;
            out[(size_t)b * d + h * DH + tid] = f2bf(v);
        }
        return;
    }
    // ---- ring pieces: partials as agent-scope stores, the last arrival merges in piece order (decode_attn_kernel)
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

extern "C" int mxl_relattn_decode_fp8_owned(const void* qkv, const void* kc8, const void* ke, const void* vc8, const void* ve,
                                            const void* owner, int nb, const float* bd, const float* r_w_bias, void* out,
                                            const int* t_dev, int B, int H, int dh, int M, float scale, int pieces, float* ws,
                                            int* arrived, const int* unfinished, void* stream) {
    MXL_CHECK_ARG(qkv && kc8 && ke && vc8 && ve && owner && bd && r_w_bias && out && t_dev && ((uintptr_t)owner % 16) == 0);
    MXL_CHECK_ARG(nb >= 1 && nb <= 16 && B > 0 && B <= 65535 && (B % nb) == 0 && H > 0 && M > 0 && (M % 16) == 0);
    MXL_CHECK_ARG(pieces >= 1 && pieces <= 8);
    if (pieces > 1) MXL_CHECK_ARG(ws && arrived);
    const size_t shm = (size_t)M * 4 + 4 * 64 * 4 + (size_t)M;
    MXL_CHECK_ARG(shm <= 64 * 1024);
    if (dh != 16 && dh != 32 && dh != 64) return MXL_EUNSUPPORTED;
    MXL_CHECK_ARG(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)kc8 % 16) == 0 && ((uintptr_t)vc8 % 16) == 0);
    dim3 grid(H, B, pieces);
    hipStream_t s = (hipStream_t)stream;
#define LAUNCH(DH) hipLaunchKernelGGL((decode_attn_fp8_owned_kernel<DH, FP8_OWNED_U>), grid, dim3(256), shm, s, (const bf16_t*)qkv,      \
                                      (const unsigned char*)kc8, (const signed char*)ke, (const unsigned char*)vc8, (const signed char*)ve, \
                                      bd, r_w_bias, (bf16_t*)out, t_dev, B, H, M, scale, ws, arrived, unfinished,                        \
                                      (const unsigned char*)owner, nb)
    switch (dh) {
        case 16: LAUNCH(16); break;
        case 32: LAUNCH(32); break;
        case 64: LAUNCH(64); break;
    }
#undef LAUNCH
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}
