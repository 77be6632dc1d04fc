// What every decode attention kernel shares (decode_attn.hip, decode_fp8.hip: one query per workgroup; decode_shared.hip,
// decode_prefix.hip: G queries per workgroup).  A kernel is one workgroup of 256 threads per (head, row or group of rows, ring
// piece); the helpers below are inlined into it, so a kernel's code is what it was when it carried its own copy of them.
#pragma once
#include "common.h"

// ---- the piece cut.  Ring slots that have never been written (t < M - 1: the sequence is shorter than the memory) are HF's
// zero-initialised mems: k = v = 0, so their score is the positional term alone and they add nothing to the output -- no K / V bytes
// are read for them.  gridDim.z = NS pieces of the ring: piece blockIdx.z takes the written slots [lo, hi) and the never-written
// slots [plo, phi); the written part is cut at multiples of 32 slots.
struct RingPiece {
    int nvalid, lo, hi, plo, phi;
};
__device__ __forceinline__ RingPiece ring_piece(int t, int M) {
    RingPiece p;
    p.nvalid = t + 1 < M ? t + 1 : M;
    const int NS = gridDim.z, zi = blockIdx.z;
    const int piece = NS > 1 ? ((((p.nvalid + NS - 1) / NS) + 31) & ~31) : p.nvalid;
    p.lo = min(zi * piece, p.nvalid);
    p.hi = min(p.lo + piece, p.nvalid);
    const int ppiece = (M - p.nvalid + NS - 1) / NS;
    p.plo = min(p.nvalid + zi * ppiece, M);
    p.phi = min(p.plo + ppiece, M);
    return p;
}

// ---- the query.  Mirrors the training kernels: (q + r_w_bias) is rounded to bf16 before the contraction.  One element; a lane
// loads its 8 (bf16 rings) or 16 (fp8 rings) of them with this in a loop of its own.
__device__ __forceinline__ float biased_query(bf16_t q, float bias) { return bf2f(f2bf(bf2f(q) + bias)); }

// ---- the workgroup reduction of o.  The LPK lanes of a key row hold N elements each of the head's DH = LPK * N; the 64 / LPK key
// rows of a wave are summed by shuffles, and the lanes of key row 0 leave the wave's DH sums at `dst` (the wave's row of `red`, at
// the lane's elements).  The caller's barrier follows; red_sum adds the four waves.
template <int LPK, int N>
__device__ __forceinline__ void reduce_o(float (&o)[N], float* dst, int ksub) {
#pragma unroll
    for (int j = 0; j < N; j++) {
#pragma unroll
        for (int off = LPK; off < 64; off <<= 1) o[j] += __shfl_xor(o[j], off, 64);
    }
    if (ksub == 0) {
#pragma unroll
        for (int j = 0; j < N; j++) dst[j] = o[j];
    }
}
// element e of the four waves' sums, `stride` floats apart
__device__ __forceinline__ float red_sum(const float* red, int stride, int e) {
    return red[e] + red[stride + e] + red[2 * stride + e] + red[3 * stride + e];
}

// ---- ring pieces.  With NS > 1 every piece runs the whole kernel on its slots with its own softmax reference and leaves (o
// unnormalised, max, sum) in `ws`, DH + 2 floats per (row, head, piece); the piece that arrives last (one counter per (row, head),
// reset by that piece for the next launch) merges them in piece order -- a fixed order, so the result does not depend on who is last.
// The pieces of a ring may sit on different XCDs (one L2 each): the partials travel as agent-scope (sc1) stores and loads and the
// counter as a relaxed agent-scope atomic, the stores waited for (vmcnt) before the workgroup's arrival is counted -- the pattern
// scripts/ubench/grid_barrier.hip measured; the compiler's release / acquire fences (buffer_wbl2 / buffer_inv of the whole L2) made
// a 30 us launch take 90.
#define MXL_AGENT_STORE(p, v) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define MXL_AGENT_LOAD(p) __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// one query per workgroup, row b and head h of H: `red` holds the four waves' sums (DH apart), mx is the piece's softmax reference,
// wsum the four waves' shares of its denominator, and `out` the (rows, H * DH) output
template <int DH>
__device__ __forceinline__ void pieces_tail(float* ws, int* arrived, int b, int h, int H, const float* red, float mx, const float* wsum,
                                            bf16_t* out) {
    const int NS = gridDim.z, zi = blockIdx.z, tid = threadIdx.x;
    float* wsp = ws + ((size_t)b * H + h) * NS * (DH + 2);
    if (tid < DH) MXL_AGENT_STORE(wsp + zi * (DH + 2) + tid, red_sum(red, DH, tid));
    if (tid == 0) {
        MXL_AGENT_STORE(wsp + zi * (DH + 2) + DH, mx);
        MXL_AGENT_STORE(wsp + zi * (DH + 2) + DH + 1, wsum[0] + wsum[1] + wsum[2] + wsum[3]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int s_last;
    if (tid == 0) s_last = (__hip_atomic_fetch_add(arrived + (size_t)b * H + h, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == NS - 1) ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    if (tid < DH) {
        float m = -1e30f;
        for (int k = 0; k < NS; k++) m = fmaxf(m, MXL_AGENT_LOAD(wsp + k * (DH + 2) + DH));
        float den = 0.f, num = 0.f;
        for (int k = 0; k < NS; k++) {
            const float a = __expf(MXL_AGENT_LOAD(wsp + k * (DH + 2) + DH) - m);
            num += a * MXL_AGENT_LOAD(wsp + k * (DH + 2) + tid);
            den += a * MXL_AGENT_LOAD(wsp + k * (DH + 2) + DH + 1);
        }
        out[(size_t)b * (H * DH) + h * DH + tid] = f2bf(num / den);
    }
    if (tid == 0) MXL_AGENT_STORE(arrived + (size_t)b * H + h, 0);
}

// ---- G queries per workgroup (decode_shared.hip, decode_prefix.hip): the G rows g0 .. g0 + G - 1 of the K rows of item b share the
// ring fragments a workgroup loads.  Per query nothing moves against the one-query kernels: the same slot-to-lane assignment, the same
// order of every sum, the same pieces and merge order, so a query's output is theirs bit for bit.  grid (head, item * groups + group,
// ring piece).  The two kernels keep their own text of the score, the softmax section, the output reduction and the pieces tail over
// the group's rows (pieces_tail's protocol, per live query, on the arrival counter of the group's first row): as functions here
// those changed the code the compiler generates around them (profiles/decode_attn_refactor.txt).

// score slots a piece needs at most: its written slots [lo, hi) and its never-written slots [plo, phi).  One piece: all M.  NS pieces:
// hi - lo <= ceil(nvalid / NS) + 31 and phi - plo <= ceil((M - nvalid) / NS), and the two ceilings sum to less than M / NS + 2; never
// more than M.  A multiple of 4, so that what follows the scores in LDS stays 16-byte aligned.
inline int group_cap(int M, int pieces) {
    const int c = pieces > 1 ? (M + pieces - 1) / pieces + 34 : M;
    return ((c < M ? c : M) + 3) & ~3;
}
inline int group_size(int K) { return K <= 4 ? 4 : 8; }
// dynamic LDS: scores [G][cap] f32, the output scratch [4][G][dh] f32, and `extra` bytes per query that are the kernel's own
inline size_t group_lds(int G, int dh, int cap, int extra) { return (size_t)G * ((size_t)cap * 4 + 4 * dh * 4 + extra); }
constexpr int GROUP_LDS_MAX = 160 * 1024;      // LDS of a gfx950 CU

// launch KERNEL with `shm` bytes of dynamic LDS, raising the limit of that kernel first where it has not been raised that far
template <auto KERNEL, class... Args>
int launch_big_lds(dim3 grid, size_t shm, hipStream_t s, Args... args) {
    static size_t attr = 64 * 1024;         // dynamic LDS this kernel may take so far
    if (shm > attr) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        if (e != hipSuccess) return (int)e;
        attr = shm;
    }
    hipLaunchKernelGGL(KERNEL, grid, dim3(256), shm, s, args...);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

// row of query g: a group past the last row of an item (K % G != 0) runs its spare queries on the item's last row and writes nothing
// for them
__device__ __forceinline__ int group_row(int b, int K, int g0, int g) { return b * K + min(g0 + g, K - 1); }

// the never-written slots [plo, phi) of the piece, scored behind its nw written ones at sc[g][nw + sp - plo]: score = scale *
// BD[distance].  bdh is head h of row 0's positional terms and bdoff[g] leads to query g's row.
template <int G>
__device__ __forceinline__ void group_score_unwritten(float* sc, int cap, const float* bdh, const size_t (&bdoff)[G], int tm, int nw, int plo,
                                                      int phi, int M, float scale, float (&mx)[G]) {
#pragma clang loop vectorize(disable) unroll(disable)
    for (int sp = plo + threadIdx.x; sp < phi; sp += 256) {
        int dist = tm - sp;
        if (dist < 0) dist += M;
#pragma unroll
        for (int g = 0; g < G; g++) {
            const float a = bdh[bdoff[g] + dist] * scale;
            sc[g * cap + nw + sp - plo] = a;
            mx[g] = fmaxf(mx[g], a);
        }
    }
}

// o += bf16(p) * v for one query and one slot, p at sc[i] (`in`: the lane's slot is one of the run; else 0 * 0 is added)
__device__ __forceinline__ void group_add(const float* sc, int i, float (&o)[8], const bf16x8& vv, bool in) {
    const float pv = in ? bf2f(f2bf(sc[i])) : 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) o[j] += pv * bf2f((bf16_t)vv[j]);
}
