// FP8 K/V rings for the Transformer-XL decode step (opt-in: XLDecoder(kv_dtype='fp8')).
//
// A ring (B, H, M, dh) of bf16 becomes (B, H, M, dh) bytes of OCP e4m3fn and (B, H, M) int8 exponents, one per slot and head; the
// stored value is fp8 * 2^e.  For a row x of dh bf16 elements with amax = max|x| = m 2^k, m in [0.5, 1): e = k - 9 if m <= 0.875,
// else k - 8 (the smallest e with amax 2^-e <= 448), clamped to [-126, 127]; amax = 0 gives e = 0 and zero bytes; byte j =
// e4m3fn(x_j 2^-e), round to nearest even, subnormals kept.  The scale is a power of two: scaling is exact in f32 and every
// dequantised value is a bf16 value, so 2^e may be applied per element or once per partial sum without changing a bit.
// Never-written slots and the K / V of left-pad columns are zero bytes with e = 0.
//
// Writers: kv_append_fp8_kernel / kv_fill_fp8_kernel (kv_append_kernel / kv_fill_kernel of decode.hip with the row quantised on the
// way).  Reader: decode_attn_fp8_kernel, decode_attn_kernel's contract (decode_attn.hip) on half the bytes, on the row's own rings or
// through the owner table of the device beam searches.
#include "decode_attn.h"
#include "musicxl_internal.h"

namespace {

// depth of the attention kernel's double-buffered batches.  16 as in decode_attn_kernel needs 254 registers here (16 more query and
// 16 more output floats per lane, the converted operands) and leaves one workgroup per CU; 12 takes 168 (three per CU, 12 KiB per
// wave and batch in flight), 8 takes 126 (four per CU)
constexpr int FP8_ATTN_U = 12;
// the same under an owner table, where the source row of every load in flight costs registers: 12 takes 182 (two workgroups per CU),
// 11 takes 168 again, 10 takes 162, 8 takes 128; none of them spills.  11 keeps the three workgroups, and measured (a lane at a full
// ring, identity table, two passes per build: profiles/beam_fp8_rings.txt) it is 27.4 / 27.6 us against 28.3 / 28.5 for 12 and 27.8 /
// 27.6 for 8.  The batch depth changes no bit: a lane visits its slots in ascending order whatever it is.
constexpr int FP8_OWNED_U = 11;

typedef float fp8_f2 __attribute__((ext_vector_type(2)));

// exponent e of a row with the given amax (>= 0, finite), from the bits of the f32: a normal amax = 1.f 2^(ex - 127) has
// m = 1.f / 2 and k = ex - 126; m <= 0.875 is f <= 0.75.  A subnormal amax (k <= -126) lands below the clamp.
__device__ __forceinline__ int fp8_row_exponent(float amax) {
    const uint32_t bits = __float_as_uint(amax);
    if (bits == 0u) return 0;
    const int ex = (int)(bits >> 23);
    if (ex == 0) return -126;
    const int e = ex - 126 - ((bits & 0x7FFFFFu) <= 0x600000u ? 9 : 8);
    return max(-126, min(127, e));
}
// 2^n for n in [-126, 127]
__device__ __forceinline__ float fp8_pow2(int n) { return __uint_as_float((uint32_t)(n + 127) << 23); }

// 8 bf16 of one row chunk -> 8 e4m3fn bytes of x 2^-e (byte j = element j)
__device__ __forceinline__ u32x2 fp8_pack8(const bf16x8 x, float inv) {
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; j++) f[j] = bf2f((bf16_t)x[j]) * inv;
    int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
    int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
    return u32x2{(uint32_t)w0, (uint32_t)w1};
}
__device__ __forceinline__ float fp8_amax8(const bf16x8 x) {
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) a = fmaxf(a, fabsf(bf2f((bf16_t)x[j])));
    return a;
}

// one chunk of 8 elements of a k row and of a v row into ring slot `slot` of (b, h): the dh / 8 lanes that share the row (a
// power of two of neighbouring lanes, aligned) reduce its amax, every lane packs its 8 bytes, the lane of chunk 0 stores the exponent
__device__ __forceinline__ void fp8_store_row_chunk(const bf16x8 k, const bf16x8 v, unsigned char* kc8, signed char* ke,
                                                    unsigned char* vc8, signed char* ve, size_t row, int e0, int dh, bool valid) {
    float ak = fp8_amax8(k), av = fp8_amax8(v);
    for (int o = 1; o < (dh >> 3); o <<= 1) {
        ak = fmaxf(ak, __shfl_xor(ak, o, 64));
        av = fmaxf(av, __shfl_xor(av, o, 64));
    }
    if (!valid) return;
    const int ek = fp8_row_exponent(ak), ev = fp8_row_exponent(av);
    *reinterpret_cast<u32x2*>(kc8 + row * dh + e0) = fp8_pack8(k, fp8_pow2(-ek));
    *reinterpret_cast<u32x2*>(vc8 + row * dh + e0) = fp8_pack8(v, fp8_pow2(-ev));
    if (e0 == 0) {
        ke[row] = (signed char)ek;
        ve[row] = (signed char)ev;
    }
}

// kv_append_kernel on fp8 rings: slot *t_dev % M of (kc8, ke, vc8, ve) <- the quantised k / v thirds of the qkv row; qr as there
__global__ __launch_bounds__(256) void kv_append_fp8_kernel(const bf16_t* qkv, unsigned char* kc8, signed char* ke, unsigned char* vc8,
                                                            signed char* ve, const int* t_dev, int B, int M, int d, int dh,
                                                            const float* rrb, bf16_t* qr) {
    const int chunks = d >> 3;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = gid < B * chunks;                  // (B * chunks is a multiple of dh / 8: a row's lanes are all valid or none)
    const int g = valid ? gid : 0;
    const int b = g / chunks, c = g % chunks;
    if (qr && valid) {
        const bf16x8 qv = *reinterpret_cast<const bf16x8*>(qkv + (size_t)b * 3 * d + c * 8);
        u32x4 w;
        bf16_t* wp = reinterpret_cast<bf16_t*>(&w);
#pragma unroll
        for (int j = 0; j < 8; j++) wp[j] = f2bf(bf2f((bf16_t)qv[j]) + rrb[c * 8 + j]);
        *reinterpret_cast<u32x4*>(qr + (size_t)b * d + c * 8) = w;
    }
    const int slot = (*t_dev) % M;
    const int h = (c * 8) / dh, e0 = (c * 8) % dh, H = d / dh;
    const bf16x8 k = *reinterpret_cast<const bf16x8*>(qkv + (size_t)b * 3 * d + d + c * 8);
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(qkv + (size_t)b * 3 * d + 2 * d + c * 8);
    fp8_store_row_chunk(k, v, kc8, ke, vc8, ve, ((size_t)b * H + h) * M + slot, e0, dh, valid);
}

// kv_fill_kernel on fp8 rings: slots (p mod M) <- the quantised K / V rows of positions p in [max(0, T - M), T)
__global__ __launch_bounds__(256) void kv_fill_fp8_kernel(const bf16_t* qkv, unsigned char* kc8, signed char* ke, unsigned char* vc8,
                                                          signed char* ve, int B, int T, int M, int d, int dh) {
    const int chunks = d >> 3;
    const int keep = min(T, M);
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = gid < (long long)B * keep * chunks;
    const long long g = valid ? gid : 0;
    const int c = (int)(g % chunks);
    const int r = (int)((g / chunks) % keep);
    const int b = (int)(g / ((long long)chunks * keep));
    const int pos = T - keep + r;
    const int slot = pos % M;
    const bf16_t* row = qkv + ((size_t)b * T + pos) * 3 * d;
    const int h = (c * 8) / dh, e0 = (c * 8) % dh, H = d / dh;
    const bf16x8 k = *reinterpret_cast<const bf16x8*>(row + d + c * 8);
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(row + 2 * d + c * 8);
    fp8_store_row_chunk(k, v, kc8, ke, vc8, ve, ((size_t)b * H + h) * M + slot, e0, dh, valid);
}

// 16 e4m3fn bytes -> 16 f32 (v_cvt_pk_f32_fp8: two elements per instruction)
__device__ __forceinline__ void fp8_unpack16(const u32x4 w, float (&f)[16]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const fp8_f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
        const fp8_f2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
        f[4 * i] = lo[0]; f[4 * i + 1] = lo[1]; f[4 * i + 2] = hi[0]; f[4 * i + 3] = hi[1];
    }
}

// decode_attn_kernel (decode_attn.hip) on fp8 rings: same grid (head, batch row, ring piece), same pieces, partials, arrival counter and
// merge, same arithmetic contract -- q' = bf16(q + r_w_bias), f32 scores with the bd term, never-written slots as the positional
// term alone and counted in the denominator, P rounded to bf16 before the P V sum.  A lane still loads 16 bytes, now 16 elements:
// dh = 16 * LPK, LPK lanes share a key row, 64 / LPK keys per wave instruction, so a batch of U loads covers twice the slots.
// The exponents never enter the batch registers.  K: the piece's 2^ke[s] are staged in sc[s] (the score array, one coalesced byte
// row per (sequence, head)) while the first K batch is in flight; a lane scales its partial dot product by sc[s] before the lane
// reduction (exact: a power of two) and the score then overwrites sc[s].  V: the softmax pass leaves bf16(p_s) 2^ve[s] in sc[s]
// (exact as well), and the P V loop multiplies that with the bare fp8 values.
// OWNED (beam search with beam_rings='indexed' on a decoder with kv_dtype='fp8') is decode_attn_kernel's: the 16 K bytes, the 16 V
// bytes and the two exponents of a written slot s of row b are read from the rings of row (b / nb) * nb + owner[b][s], the table
// mxl_beam_owner_follow (beam.hip) keeps.  The writers do not change: every row appends to its own ring, which is the slot the follow
// kernel marks as the row's own.  Everything but the source row of a load is one text, so on rings gathered by the table the plain
// kernel gives the same bits, and the identity table gives its bits on the same rings (tests/test_beam_fp8_owned_ops_gpu.py).
// Dynamic LDS: sc [M] f32, the output scratch [4][64] f32 and, OWNED, the row's M owner bytes (M % 16 == 0 and B % nb == 0 are the
// entry's to check).
template <int DH, int U, bool OWNED>
__global__ __launch_bounds__(256) void decode_attn_fp8_kernel(const bf16_t* qkv, const unsigned char* kc8, const signed char* ke,
                                                              const unsigned char* vc8, const signed char* ve, const float* bd,
                                                              const float* rwb, bf16_t* out, const int* t_dev, int B, int H, int M,
                                                              float scale, float* ws, int* arrived, const int* live,
                                                              const unsigned char* owner, int nb) {
    constexpr int LPK = DH / 16;         // lanes per key row
    constexpr int KPW = 64 / LPK;        // keys per wave per iteration
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sc = reinterpret_cast<float*>(smem);          // [M] 2^ke -> scores -> bf16(p) 2^ve
    float* red = sc + M;                                 // [4][DH]
    __shared__ float wred[8];
    const int h = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    const int c16 = lane % LPK, ksub = lane / LPK;
    const int d = H * DH;
    if (live != nullptr && live[b] == 0) {               // a finished row: zeros from piece 0, no ring or owner byte read, counter untouched
        if (blockIdx.z == 0 && tid < DH) out[(size_t)b * d + h * DH + tid] = f2bf(0.f);
        return;
    }
    const int t = *t_dev;
    const int tm = t % M;
    const int NS = gridDim.z;
    const RingPiece pc = ring_piece(t, M);
    const int lo = pc.lo, hi = pc.hi, plo = pc.plo, phi = pc.phi;

    float qw[16];
    {
        const bf16_t* qp = qkv + (size_t)b * 3 * d + h * DH + c16 * 16;
        const bf16x8 q0 = *reinterpret_cast<const bf16x8*>(qp), q1 = *reinterpret_cast<const bf16x8*>(qp + 8);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            qw[j] = biased_query((bf16_t)q0[j], rwb[h * DH + c16 * 16 + j]);
            qw[8 + j] = biased_query((bf16_t)q1[j], rwb[h * DH + c16 * 16 + 8 + j]);
        }
    }
    const float* bdrow = bd + ((size_t)b * H + h) * M;
    // kb / vb / ker / ver are head h of the row's own rings or, OWNED, of row 0's, and slot_at adds the slot: in slots for the
    // exponents, times DH in bytes for K and V
    const size_t ring = ((size_t)(OWNED ? 0 : b) * H + h) * M;
    const unsigned char* kb = kc8 + ring * DH + c16 * 16;
    const unsigned char* vb = vc8 + ring * DH + c16 * 16;
    const signed char* ker = ke + ring;
    const signed char* ver = ve + ring;
    // OWNED: the row's M owner bytes, staged once behind `red`: 16 bytes per thread.  The K loads and the exponent staging need them,
    // so the barrier stands before the first K batch is issued
    const unsigned char* own = reinterpret_cast<const unsigned char*>(red + 4 * 64);
    if constexpr (OWNED) {
        const u32x4* from = reinterpret_cast<const u32x4*>(owner + (size_t)b * M);
        u32x4* to = reinterpret_cast<u32x4*>(red + 4 * 64);
        for (int i = tid; i < (M >> 4); i += 256) to[i] = from[i];
        __syncthreads();
    }
    // OWNED: an owner byte beyond the item (mxl_beam_owner_follow writes none) is held to the item's last row, so no table sends a
    // read outside the rings; no owner byte of a never-written slot is looked at
    const size_t ring_stride = (size_t)H * M;
    const int item0 = (b / nb) * nb;
    auto slot_at = [&](int s) -> size_t {
        if constexpr (OWNED) return (size_t)(item0 + min((int)own[s], nb - 1)) * ring_stride + (size_t)s;
        else return (size_t)s;
    };

    // pass 1: scores, in double-buffered batches of U key groups as in decode_attn_kernel (non-temporal 16-byte loads)
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
                fp8_unpack16(kv[u], kf);
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
        for (int s = lo + tid; s < hi; s += 256) sc[s] = fp8_pow2((int)ker[slot_at(s)]);      // under the first batch's latency
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
        sc[s] = bf2f(f2bf(pv)) * fp8_pow2((int)ver[slot_at(s)]);      // the P V operand: P rounded to bf16, times the slot's 2^e
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
                fp8_unpack16(vv[u], vf);
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
    reduce_o<LPK>(o, red + wid * DH + c16 * 16, ksub);
    __syncthreads();
    if (NS == 1) {
        if (tid < DH) out[(size_t)b * d + h * DH + tid] = f2bf(red_sum(red, DH, tid) * inv);
        return;
    }
    pieces_tail<DH>(ws, arrived, b, h, H, red, mx, wred + 4, out);
}

}  // namespace

extern "C" int mxl_kv_append_fp8(const void* qkv, void* kc8, void* ke, void* vc8, void* ve, const int* t_dev, int B, int M, int d,
                                 int dh, const float* r_r_bias, void* qr_out, void* stream) {
    MXL_CHECK_ARG(qkv && kc8 && ke && vc8 && ve && t_dev && B > 0 && M > 0 && d > 0 && dh > 0 && (d % dh) == 0);
    MXL_CHECK_ARG(!qr_out || r_r_bias);
    if (dh != 16 && dh != 32 && dh != 64) return MXL_EUNSUPPORTED;
    MXL_CHECK_ARG(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)kc8 % 8) == 0 && ((uintptr_t)vc8 % 8) == 0 && ((uintptr_t)qr_out % 16) == 0);
    const int n = B * (d / 8);
    hipLaunchKernelGGL(kv_append_fp8_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv,
                       (unsigned char*)kc8, (signed char*)ke, (unsigned char*)vc8, (signed char*)ve, t_dev, B, M, d, dh, r_r_bias,
                       (bf16_t*)qr_out);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_kv_fill_fp8(const void* qkv, void* kc8, void* ke, void* vc8, void* ve, int B, int T, int M, int d, int dh,
                               void* stream) {
    MXL_CHECK_ARG(qkv && kc8 && ke && vc8 && ve && B > 0 && T > 0 && M > 0 && d > 0 && dh > 0 && (d % dh) == 0);
    if (dh != 16 && dh != 32 && dh != 64) return MXL_EUNSUPPORTED;
    MXL_CHECK_ARG(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)kc8 % 8) == 0 && ((uintptr_t)vc8 % 8) == 0);
    const long long n = (long long)B * (T < M ? T : M) * (d / 8);
    MXL_CHECK_ARG((n + 255) / 256 <= 0x7FFFFFFFLL);
    hipLaunchKernelGGL(kv_fill_fp8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv,
                       (unsigned char*)kc8, (signed char*)ke, (unsigned char*)vc8, (signed char*)ve, B, T, M, d, dh);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

namespace {

template <bool OWNED>
int relattn_decode_fp8_launch(const void* qkv, const void* kc8, const void* ke, const void* vc8, const void* ve, const void* owner, int nb,
                              const float* bd, const float* r_w_bias, void* out, const int* t_dev, int B, int H, int dh, int M, float scale,
                              int pieces, float* ws, int* arrived, const int* live, size_t shm, void* stream) {
    MXL_CHECK_ARG(shm <= 64 * 1024);
    if (dh != 16 && dh != 32 && dh != 64) return MXL_EUNSUPPORTED;
    MXL_CHECK_ARG(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)kc8 % 16) == 0 && ((uintptr_t)vc8 % 16) == 0);
    dim3 grid(H, B, pieces);
    hipStream_t s = (hipStream_t)stream;
#define LAUNCH(DH) hipLaunchKernelGGL((decode_attn_fp8_kernel<DH, OWNED ? FP8_OWNED_U : FP8_ATTN_U, OWNED>), grid, dim3(256), shm, s,        \
                                      (const bf16_t*)qkv, (const unsigned char*)kc8, (const signed char*)ke, (const unsigned char*)vc8,     \
                                      (const signed char*)ve, bd, r_w_bias, (bf16_t*)out, t_dev, B, H, M, scale, ws, arrived, live,         \
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

}  // namespace

extern "C" int mxl_relattn_decode_fp8(const void* qkv, const void* kc8, const void* ke, const void* vc8, const void* ve,
                                      const float* bd, const float* r_w_bias, void* out, const int* t_dev, int B, int H, int dh, int M,
                                      float scale, int pieces, float* ws, int* arrived, const int* unfinished, void* stream) {
    MXL_CHECK_ARG(pieces >= 1 && pieces <= 8);
    if (pieces > 1) MXL_CHECK_ARG(ws && arrived);
    MXL_CHECK_ARG(qkv && kc8 && ke && vc8 && ve && bd && r_w_bias && out && t_dev && B > 0 && B <= 65535 && H > 0 && M > 0);
    return relattn_decode_fp8_launch<false>(qkv, kc8, ke, vc8, ve, nullptr, 1, bd, r_w_bias, out, t_dev, B, H, dh, M, scale, pieces, ws,
                                            arrived, unfinished, (size_t)M * 4 + 4 * 64 * 4, stream);
}

extern "C" int mxl_relattn_decode_fp8_owned(const void* qkv, const void* kc8, const void* ke, const void* vc8, const void* ve,
                                            const void* owner, int nb, const float* bd, const float* r_w_bias, void* out,
                                            const int* t_dev, int B, int H, int dh, int M, float scale, int pieces, float* ws,
                                            int* arrived, const int* unfinished, void* stream) {
    MXL_CHECK_ARG(qkv && kc8 && ke && vc8 && ve && owner && bd && r_w_bias && out && t_dev && ((uintptr_t)owner % 16) == 0);
    MXL_CHECK_ARG(nb >= 1 && nb <= 16 && B > 0 && B <= 65535 && (B % nb) == 0 && H > 0 && M > 0 && (M % 16) == 0);
    MXL_CHECK_ARG(pieces >= 1 && pieces <= 8);
    if (pieces > 1) MXL_CHECK_ARG(ws && arrived);
    return relattn_decode_fp8_launch<true>(qkv, kc8, ke, vc8, ve, owner, nb, bd, r_w_bias, out, t_dev, B, H, dh, M, scale, pieces, ws,
                                           arrived, unfinished, (size_t)M * 4 + 4 * 64 * 4 + (size_t)M, stream);
}
