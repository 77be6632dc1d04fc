/*
 * libmusicxl -- C ABI of the MI355X-native Transformer-XL / Reformer hot path.
 *
 * The reference (StefanHeng/Symbolic-Music-Generation) has no FFI for this path: its boundary is the Python object
 * contract of `get_model_n_tokenizer` (musicnlp/trainer/train.py:31-59) and the arithmetic sits in HuggingFace
 * `transformers==4.25.1` (its transfo_xl and reformer model directories).  Each entry point below names the upstream /
 * reference operation it replaces.  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless said otherwise; tensors are row-major, batch-major (B, T, ...);
 *   - bf16 tensors are raw 16-bit words; "f32" means IEEE float;
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work (no sync, no allocation) and is
 *     therefore safe to capture into a hipGraph;
 *   - return value: 0 ok, negative = argument error (MXL_E*), positive = hipError_t from the launch.
 */
#ifndef MUSICXL_H
#define MUSICXL_H

#ifdef __cplusplus
extern "C" {
#endif

#define MXL_ABI_VERSION 3

int mxl_abi_version(void);
/* human-readable text for a negative libmusicxl code or a positive hipError_t */
const char* mxl_error_string(int code);

/* ------------------------------------------------------------------------------------------------------------
 * GEMM (bf16 in, fp32 accumulate on MFMA).  Replaces F.linear / torch.einsum in upstream qkv_net, r_net, o_net,
 * CoreNet (PositionwiseFF), crit.out_layers (modeling_transfo_xl.py), and their autograd backward.
 *   C[M,N] (+)= alpha * op(A) * op(B);  transA=0: A[M][K]  transA=1: A[K][M];  transB=0: B[N][K]  transB=1: B[K][N]
 *   lda/ldb multiples of 8 elements, base pointers 16-byte aligned, K % 8 == 0 unless both operands are transposed.
 * flags: output type (default bf16) and fused epilogue.
 * ---------------------------------------------------------------------------------------------------------- */
#define MXL_GEMM_OUT_F32        0x01  /* C is f32, plain store                                   */
#define MXL_GEMM_OUT_F32_ATOMIC 0x02  /* C is f32, atomicAdd (required when ksplits > 1)         */
#define MXL_GEMM_BIAS           0x04  /* + bias[n]                                               */
#define MXL_GEMM_RELU           0x08  /* max(.,0)            (CoreNet.1)                         */
#define MXL_GEMM_DROPOUT        0x10  /* inverted dropout.  Alone or with BIAS: the (seed, site, m*N+n) keep-mask of mxl_dropout_bf16
                                         (dropout_keep: a backward pass may regenerate it).  Together with MXL_GEMM_RELU (the FFN's
                                         hidden activations) a DIFFERENT mask: one hash per pair of elements (m, n), (m, n + 1),
                                         n even, a 16-bit decision each, the drop probability quantised to 2^-16.  Nothing may
                                         regenerate that one: the backward takes it from the saved bits (MXL_GEMM_SAVE_RELU_MASK)
                                         or from the zeros of the stored activations */
#define MXL_GEMM_RELU_BWD       0x20  /* C = aux[m][n] > 0 ? acc : 0  (backward through relu+dropout) */
#define MXL_GEMM_ADD_AUX        0x40  /* C = epilogue(acc) + aux[m][n]  (residual add after bias/dropout)  */
/* Compute units to leave free of the persistent GEMM grids (0 .. 128; default 0): they launch one workgroup per remaining CU.  For
 * data-parallel training: RCCL's reduction kernels run beside the backward on another stream, and a grid that occupies every CU for its
 * whole duration leaves them nowhere to start until it ends (symbolic_music_generation_amd/dist.py sets it from MXL_RESERVE_CUS when
 * the process group has more than one rank).  Process-wide, not stream-ordered: set it between steps. */
int mxl_set_reserved_cus(int k);
/* which large-tile kernel the last K-contiguous mxl_gemm_bf16* call went to (0: none, 1 / 2: eight waves with 256- / 192-wide tiles,
 * 3: four waves of 128 x 128): for tests that mean to exercise one of them */
int mxl_gemm_last_nt_kernel(void);

/* The relu (+dropout) mask of C as bits instead of the bf16 activations, for the backward through CoreNet.1 / CoreNet.2:
 *   MXL_GEMM_SAVE_RELU_MASK  (with BIAS | RELU [| DROPOUT]): also writes, through `aux`, one bit per output element (> 0)
 *   MXL_GEMM_RELU_BWD_BITS   C = bit ? alpha * acc : 0, bits read through `aux` (the buffer a SAVE call of the same M, N filled)
 * The bits are in the large-tile kernel's accumulator layout (opaque; mxl_gemm_relu_mask_bytes(M, N) bytes, 0 = these M, N do not
 * take that kernel: use MXL_GEMM_RELU_BWD with the activations).  Calls that cannot honour the flags return MXL_EUNSUPPORTED. */
#define MXL_GEMM_SAVE_RELU_MASK 0x100
#define MXL_GEMM_RELU_BWD_BITS  0x200
size_t mxl_gemm_relu_mask_bytes(int M, int N);
int mxl_gemm_bf16(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                  int transA, int transB, int flags, float alpha, const float* bias,
                  const void* aux, int ldaux, int ksplits,
                  float drop_p, unsigned long long seed, unsigned site, void* stream);

/* mxl_gemm_bf16 (bf16 output, no K-split) and, in the same call, colsum[n] += sum_m C[m][n]: the bias gradient of the layer whose
 * output gradient C is (pos_ff.CoreNet.0.bias: C = the masked dX of CoreNet.3).  With MXL_GEMM_RELU_BWD on the large-tile path (M and
 * N multiples of 256) the sums are formed from the epilogue's fp32 values inside the GEMM; otherwise by mxl_colsum_bf16 afterwards. */
int mxl_gemm_bf16_colsum(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                         int transA, int transB, int flags, float alpha, const float* bias, const void* aux, int ldaux,
                         float drop_p, unsigned long long seed, unsigned site, float* colsum, void* stream);

/* C = A . B^T (bf16, the K-contiguous form, no epilogue flags) and, in the same call,
 *     delta[(b * (N / 64) + h) * T + t] = sum_{e < 64} C[m][64 h + e] * O[m][64 h + e]      m = b * T + t
 * -- the attention backward's delta (rows = tokens, heads of 64: C = d attn_vec out of the o_net input gradient, O = attn_vec;
 * upstream RelPartialLearnableMultiHeadAttn has no such tensor, it is the softmax backward's row term sum_j P dP) formed from the
 * bf16 values the GEMM stores, instead of a pass over both matrices.  Only on the four-wave large-tile kernel (M, N multiples of
 * 256, K of 64, M a multiple of T, 16-byte aligned rows): MXL_EUNSUPPORTED otherwise, with C written and delta untouched -- the
 * caller then lets mxl_relattn_bwd_fused compute delta itself. */
int mxl_gemm_bf16_headdot(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, const void* O, int ldo,
                          int T, float* delta, void* stream);

/* same kernel, grid.y = batch: operand element offsets (by / bdiv) * s?1 + (by % bdiv) * s?2 */
int mxl_gemm_bf16_batched(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                          int transA, int transB, int flags, float alpha, int ksplits, int batch, int bdiv,
                          long long sA1, long long sA2, long long sB1, long long sB2, long long sC1, long long sC2,
                          void* stream);

/* skinny-M (M <= 64) weight-streaming form for the decode step: C[M,N] = A[M,K] . W[N,K]^T (+bias)(relu);
 * flags: MXL_GEMM_OUT_F32 | MXL_GEMM_BIAS | MXL_GEMM_RELU.  Deterministic (fixed-order in-workgroup split-K). */
int mxl_gemm_skinny_bf16(const void* A, const void* W, void* C, int M, int N, int K, int lda, int ldw, int ldc, int flags,
                         const float* bias, void* stream);
/* Narrow-N / long-K decode linears (the FFN output projection: N = d, K = 4d): K is sliced over workgroups as well; slice s
 * writes its fp32 partial product to slabs[s] ((64, N) each, rows < M written) and mxl_ln_residual_fwd_partial finishes the
 * linear: y = LayerNorm(res + bf16(sum_s slabs[s] + bias)) -- reduction, bias and the post-LN residual in one launch.
 * (Two launches with a kernel boundary between them: a single-kernel reduction needs device-scope fences that cost more, on
 * eight L2 domains, than the slicing saves.) */
int mxl_gemm_skinny_partial(const void* A, const void* W, float* slabs, int M, int N, int K, int lda, int ldw, int KS,
                            void* stream);
int mxl_ln_residual_fwd_partial(const float* slabs, int KS, long long slab_stride, const float* bias, const void* res,
                                const float* gamma, const float* beta, void* y, int N, int d, float eps, void* stream);
/* The qkv projection of one decode step with the cache append in its epilogue (one launch instead of mxl_gemm_skinny_bf16 +
 * mxl_kv_append): qkv (B, 3d) = x (B, d) . Wqkv (3d, d)^T; the k / v thirds also go into the head-major rings
 * (B, H, Mring, dh) at slot *t_dev % Mring and q + r_r_bias into qr_out (B, d) -- HF's `cat([mems, h])` + qkv_net on the one
 * new row.  B <= 64. */
int mxl_decode_qkv(const void* x, const void* Wqkv, void* qkv, void* kcache, void* vcache, const int* t_dev,
                   const float* r_r_bias, void* qr_out, int B, int d, int dh, int Mring, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Relative-position banded attention (K4).  Replaces RelPartialLearnableMultiHeadAttn.forward between qkv_net and
 * o_net in upstream modeling_transfo_xl.py (AC/BD einsums, _rel_shift, same_length mask, softmax, P.V), as called
 * through musicnlp/models/transformer_xl.py:163-171.
 *   q   : (B, T, H, dh) bf16, element (b,i,h,e) at q + b*q_bs + i*q_rs + h*dh + e   (strides in elements)
 *   k,v : (B, Kc, H, dh) bf16 with row r = key position p - (T - Kc); T <= Kc <= M + T; positions below are the
 *         zero mems of upstream init_mems (k = v = 0) and are synthesised, not read
 *   rd  : (M, H, dh) bf16, rd[d] = r_net(pos_emb(min(d, clamp_len))), d = query position - key position
 *   r_w_bias, r_r_bias : (H, dh) f32;  out : (B, T, H, dh) bf16;  lse : (B, H, T) f32 (natural log) or NULL
 *   dh in {16, 32, 64};  scale = 1/sqrt(dh)
 * ---------------------------------------------------------------------------------------------------------- */
int mxl_relattn_fwd(const void* q, const void* k, const void* v, const void* rd, const float* r_w_bias,
                    const float* r_r_bias, void* out, float* lse, int B, int T, int H, int dh, int M, int Kc,
                    long long q_bs, int q_rs, long long kv_bs, int kv_rs, int rd_rs, long long o_bs, int o_rs,
                    float scale, void* stream);

/* Backward of mxl_relattn_fwd (autograd of the upstream attention core).  out/dout share the (o_bs, o_rs) layout.
 *   delta : (B,H,T) f32 scratch (written);  dq (B,T,H,dh) / dk, dv (B,Kc,H,dh) bf16 with their own strides (written);
 *   dg    : (B,H,T,M) bf16, un-skewed score gradient dG[b,h,i,d] = dSr[i, i-d] (written; may be NULL).  The caller
 *           contracts it with (q + r_r_bias) to get d rd:  d rd[d,h,:] = sum_{b,i} dg[b,h,i,d] * (q + r_r_bias)[b,i,h,:]
 *   d_r_w_bias, d_r_r_bias : (H,dh) f32, accumulated (+=).   M % 8 == 0. */
int mxl_relattn_bwd(const void* q, const void* k, const void* v, const void* rd, const float* r_w_bias,
                    const float* r_r_bias, const void* out, const void* dout, const float* lse, float* delta,
                    void* dq, void* dk, void* dv, void* dg, float* d_r_w_bias, float* d_r_r_bias /* may be NULL: see mxl_relattn_drd */, int B, int T,
                    int H, int dh, int M, int Kc, long long q_bs, int q_rs, long long kv_bs, int kv_rs, int rd_rs,
                    long long o_bs, int o_rs, long long dq_bs, int dq_rs, long long dkv_bs, int dkv_rs,
                    float scale, void* stream);

/* The contraction the caller owes after mxl_relattn_bwd, as one HBM-streaming kernel (dh = 64, T % 32 == 0, M % 8 == 0;
 * MXL_EUNSUPPORTED otherwise -- use mxl_gemm_bf16_batched):
 *   d_rd[delta, h*dh + e] += sum_{b,i} dg[b,h,i,delta] * qr[b,i,h,e]      qr = (q + r_r_bias) in bf16, strides (qr_bs, qr_rs)
 * Optionally also the r_r_bias gradient (rd / d_r_r_bias non-NULL):
 *   d_r_r_bias[h*dh + e] += sum_delta colsum_{b,i}(dg)[h, delta] * rd[delta, h*dh + e]
 * and, when d_r_w_bias_fix is given, the same amount is subtracted there.  This pairs with mxl_relattn_bwd called with
 * d_r_r_bias == NULL: its query-owner kernel then runs in the faster 8-wave form, which has room for one dq accumulator only and
 * therefore leaves the SUM d(r_w_bias) + d(r_r_bias) in d_r_w_bias; after mxl_relattn_drd both hold their own gradient. */
int mxl_relattn_drd(const void* dg, const void* qr, float* d_rd, int B, int T, int H, int dh, int M, long long qr_bs,
                    int qr_rs, int drd_ld, const void* rd, int rd_rs, float* d_r_r_bias, float* d_r_w_bias_fix, void* stream);

/* The pair that keeps phantom distances out of HBM (dh = 64, M % 256 == 0, T % 32 == 0).  With fresh zero memories -- the
 * reference's training: HF Trainer never carries mems, so TransfoXLModel.init_mems supplies zeros every step -- the key positions
 * before the first stored one have k = v = 0 and their score gradient depends on the distance alone:
 *     dG[b,h,i,d] = -scale * delta[b,h,i] * exp(scale * (q + r_r_bias)[b,i,h,:] . rd[d,h,:] - lse[b,h,i]).
 * mxl_relattn_bwd_sparse_dg = mxl_relattn_bwd with d_r_r_bias = NULL that leaves every (32 queries x 256 distances) block of dg
 * lying entirely on such distances UNWRITTEN; mxl_relattn_drd_recompute = mxl_relattn_drd that rebuilds exactly those blocks on
 * MFMA from qr, rd, lse and delta (the buffers mxl_relattn_bwd read / wrote) instead of streaming them.  Half of dg in mode R. */
int mxl_relattn_bwd_sparse_dg(const void* q, const void* k, const void* v, const void* rd, const float* r_w_bias,
                              const float* r_r_bias, const void* out, const void* dout, const float* lse, float* delta, void* dq,
                              void* dk, void* dv, void* dg, float* d_r_w_bias, int B, int T, int H, int dh, int M, int Kc,
                              long long q_bs, int q_rs, long long kv_bs, int kv_rs, int rd_rs, long long o_bs, int o_rs,
                              long long dq_bs, int dq_rs, long long dkv_bs, int dkv_rs, float scale, void* stream);
/* The same pair with the forward's help: mxl_relattn_fwd_phantom also writes, for the distance blocks whose score gradient
 * mxl_relattn_bwd_sparse_dg does not store,  oph[b,i,h,:] = sum_d 2^(G'[i,d] - mph[b,h,i]) * rd[d,h,:]  (G' = the positional score in
 * log2 units; oph (B,T,H*dh) bf16 with out's strides, mph (B,H,T) f32).  Those blocks' contribution to dq is then the elementwise
 *   -scale * delta_i * 2^(mph_i - lse_i * log2 e) * oph_i
 * and mxl_relattn_bwd_sparse_dg_oph does not walk them (M % 256 == 0, T % 32 == 0).  mxl_relattn_drd_recompute is unchanged. */
int mxl_relattn_fwd_phantom(const void* q, const void* k, const void* v, const void* rd, const float* r_w_bias,
                            const float* r_r_bias, void* out, float* lse, void* oph, float* mph, int B, int T, int H,
                            int dh, int M, int Kc, long long q_bs, int q_rs, long long kv_bs, int kv_rs, int rd_rs,
                            long long o_bs, int o_rs, float scale, void* stream);
int mxl_relattn_bwd_sparse_dg_oph(const void* q, const void* k, const void* v, const void* rd, const float* r_w_bias,
                                  const float* r_r_bias, const void* out, const void* dout, const float* lse,
                                  float* delta, void* dq, void* dk, void* dv, void* dg, float* d_r_w_bias,
                                  const void* oph, const float* mph, int B, int T, int H, int dh, int M, int Kc,
                                  long long q_bs, int q_rs, long long kv_bs, int kv_rs, int rd_rs, long long o_bs, int o_rs,
                                  long long dq_bs, int dq_rs, long long dkv_bs, int dkv_rs, float scale, void* stream);
int mxl_relattn_drd_recompute(const void* dg, const void* qr, float* d_rd, int B, int T, int H, int dh, int M, long long qr_bs,
                              int qr_rs, int drd_ld, const void* rd, int rd_rs, float* d_r_r_bias, float* d_r_w_bias_fix,
                              const float* lse, const float* delta, float scale, int Kc, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Round 4: the attention backward as ONE pass over the score cells (dh = 64, T % 32 == 0, M % 32 == 0 [round 6; M % 256 until then:
 * the reference's `small` preset has mem_len 128], Kc % 32 == 0; MXL_EUNSUPPORTED otherwise -- use mxl_relattn_bwd + mxl_relattn_drd).  Same gradients as that pair, no dg tensor:
 *   a workgroup owns 256 keys of one (sequence, head): dk, dv written once; d_rd accumulated on chip per 32-distance block and
 *   added with float atomics (d_rd (M, drd_ld) f32, +=); the partial dq of every (query tile, key block) pair goes to a
 *   slab in `ws` (mxl_relattn_bwd_fused_ws_bytes bytes, opaque) and a finishing kernel sums a query's slabs in fp32 and rounds dq
 *   to bf16 once.  The slabs are bf16 in the shipped build: each (query, key block) partial is rounded to bf16 before that sum,
 *   at most ceil(M / 256) + 1 roundings per dq element (fp32 slabs: build with -DMXL_SLAB_BF16=0; the 12-layer gradient errors are the
 *   same to four digits either way).
 *   d_r_w_bias, d_r_r_bias (H, 64) f32 are accumulated (+=), each with its own gradient (no fix-up pass).
 * Zero memories (Kc < M + T; musicnlp/models/transformer_xl.py:163-171 calls the model without mems, so upstream init_mems
 * supplies zeros): the key positions below the first stored one have k = v = 0 and exist only as distances.  Their part of dq
 * is  -scale * delta_i * 2^(mph_i - lse_i * log2 e) * oph_i  with oph / mph from mxl_relattn_fwd_phantom2(..., oph_all = 1)
 * (required then), and their part of d_rd is owed by the caller: mxl_relattn_drd_phantom.  With Kc == M + T oph / mph are unused.
 * `delta` (B,H,T) f32 scratch is written -- unless bit 1 of `defer_finish` says the caller has filled it already
 * (delta[b][h][i] = sum_e dout . out: mxl_gemm_bf16_headdot forms it inside the GEMM that produces dout).  dq_rs, dq_bs multiples of 8.
 * defer_finish bit 0: the slab sum is left to the caller (mxl_relattn_dq_finish, same ws / oph / mph / lse / delta / dq / d_r_r_bias
 * arguments: with oph it also adds the phantom cells' part of d_r_r_bias, the column sums of their dq term; d_r_r_bias may be NULL).
 * dq and d_r_r_bias are complete only after it.
 * Owner mode (round 7): instead of one workgroup per 256-key block and the slabs, ONE workgroup per (sequence, head) walks its key
 * blocks in order, carries the partial dq of a query tile in `ws` as fp32 (B T H 64 floats in tile order, no larger than the slabs:
 * mxl_relattn_bwd_fused_ws_bytes stays the maximum of both modes; no zero-fill needed) and finishes dq and the phantom cells' part
 * of d_r_r_bias itself -- no finishing kernel, one bf16 rounding per dq element.  dk, dv are bit-identical between the modes.
 * defer_finish bit 2 forces owner mode, bit 3 per-block mode (both: MXL_EINVAL); bit 0 always means per-block mode.  Without a
 * forcing bit owner mode is chosen when its B H equally long workgroups fill the usable compute units (all minus
 * mxl_set_reserved_cus) without a long tail: B H / (ceil(B H / CUs) CUs) >= 0.9. */
size_t mxl_relattn_bwd_fused_ws_bytes(int B, int T, int H, int dh, int M);
int mxl_relattn_bwd_fused(const void* q, const void* k, const void* v, const void* rd, const float* r_w_bias,
                          const float* r_r_bias, const void* out, const void* dout, const float* lse, float* delta,
                          void* dq, void* dk, void* dv, float* d_rd, int drd_ld, float* d_r_w_bias, float* d_r_r_bias,
                          const void* oph, const float* mph, void* ws, int B, int T, int H, int dh, int M, int Kc,
                          long long q_bs, int q_rs, long long kv_bs, int kv_rs, int rd_rs, long long o_bs, int o_rs,
                          long long dq_bs, int dq_rs, long long dkv_bs, int dkv_rs, float scale, int defer_finish, void* stream);
int mxl_relattn_dq_finish(const void* ws, const void* oph, const float* mph, const float* lse, const float* delta, void* dq,
                          float* d_r_r_bias, int B, int T, int H, int dh, int M, int Kc, long long o_bs, int o_rs, long long dq_bs,
                          int dq_rs, float scale, void* stream);
/* mxl_relattn_fwd_phantom with a choice of which phantom cells enter oph: oph_all = 0 is mxl_relattn_fwd_phantom (the
 * all-phantom 256-distance blocks, for mxl_relattn_bwd_sparse_dg_oph); oph_all = 1 sums over EVERY key position below the first
 * stored key tile (for mxl_relattn_bwd_fused; needs (T - Kc) % 64 == 0).  ph_ws (or NULL; oph_all = 1, dh = 64 only): the forward
 * also fills the per-tile records of mxl_relattn_drd_phantom (mxl_relattn_drd_phantom_ws_bytes bytes), sparing the backward
 * mxl_relattn_drd_phantom_prep. */
int mxl_relattn_fwd_phantom2(const void* q, const void* k, const void* v, const void* rd, const float* r_w_bias,
                             const float* r_r_bias, void* out, float* lse, void* oph, float* mph, int oph_all, void* ph_ws, int B,
                             int T, int H, int dh, int M, int Kc, long long q_bs, int q_rs, long long kv_bs, int kv_rs, int rd_rs,
                             long long o_bs, int o_rs, float scale, void* stream);
/* d_rd[delta, h*64 + e] += sum over the PHANTOM cells (key position i - delta below T - Kc) of dG[b,h,i,delta] * qr[b,i,h,e],
 * qr = q + r_r_bias, with dG[i,delta] = -scale * delta_i * exp(scale * qr_i . rd[delta] - lse_i) rebuilt on MFMA (two products and
 * one exponential per cell, nothing streamed) -- cell by cell, so that together with mxl_relattn_bwd_fused every (query, distance)
 * pair is counted once.  (T - Kc) % 64 == 0, T % 32 == 0, M % 32 == 0, M <= 8192, dh == 64.
 * `ws` (mxl_relattn_drd_phantom_ws_bytes bytes, 16-byte aligned) holds one record per (sequence, head, 32-query tile): the tile's
 * bf16((q + r_r_bias) * scale * log2 e) rows in the kernel's LDS image order and -lse * log2 e of its queries -- written by the
 * forward (mxl_relattn_fwd_phantom2(..., ph_ws)) or by mxl_relattn_drd_phantom_prep; `delta` (B,H,T) f32 is the array
 * mxl_relattn_bwd_fused fills.  Those cells' part of d r_r_bias is added by mxl_relattn_dq_finish. */
size_t mxl_relattn_drd_phantom_ws_bytes(int B, int T, int H);
int mxl_relattn_drd_phantom_prep(const void* q, long long q_bs, int q_rs, const float* r_r_bias, const float* lse, void* ws, int B, int T,
                                 int H, int dh, float scale, void* stream);
int mxl_relattn_drd_phantom(const void* ws, const float* delta, float* d_rd, int B, int T, int H, int dh, int M, int drd_ld,
                            const void* rd, int rd_rs, int Kc, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * HBM-bound layer pieces.
 * ---------------------------------------------------------------------------------------------------------- */
/* upstream PositionalEmbedding + drop(pos_emb): out[dist][0:d/2]=sin, [d/2:d]=cos of min(dist,clamp)*inv_freq; (M,d) bf16 */
int mxl_sinusoid_table(void* out, int M, int d, int clamp_len, float drop_p, unsigned long long seed, unsigned site,
                       void* stream);
/* upstream AdaptiveEmbedding (div_val=1) + drop: out[n] = drop(E[ids[n]] * scale); ids int64, E (V,d) bf16.
 * An id outside [0, V) never indexes out of the table: the forward writes the row of id 0 for it, the backward adds nothing. */
int mxl_embed_fwd(const void* ids, const void* E, void* out, int N, int d, int V, float scale, float drop_p,
                  unsigned long long seed, unsigned site, void* stream);
/* its backward: dE[ids[n]] += keep * scale * (dout[n] + dout2[n])  (f32 atomics; dout2 may be NULL) */
int mxl_embed_bwd(const void* ids, const void* dout, const void* dout2, float* dE, int N, int d, int V, float scale,
                  float drop_p, unsigned long long seed, unsigned site, void* stream);
/* y = keep * x / (1-p): the final drop(core_out) of TransfoXLModel.forward (and its backward with x := dy); n % 8 == 0 */
int mxl_dropout_bf16(const void* x, void* y, long long n, float drop_p, unsigned long long seed, unsigned site,
                     void* stream);
/* y = LayerNorm(res + drop(x)) * gamma + beta  (post-LN of dec_attn / pos_ff); z (pre-norm sum), mean, rstd saved
 * for the backward (any of z/mean/rstd/res may be NULL).  x,res,y,z (N,d) bf16; d % 8 == 0, d <= 2048 */
int mxl_ln_residual_fwd(const void* x, const void* res, const float* gamma, const float* beta, void* y, void* z,
                        float* mean, float* rstd, int N, int d, float eps, float drop_p, unsigned long long seed,
                        unsigned site, void* stream);
/* backward of the above for upstream grad dy (+ dy2 if non-NULL): dres = dz, dx = keep*dz/(1-p), dgamma/dbeta += */
int mxl_ln_residual_bwd(const void* dy, const void* dy2, const void* z, const float* mean, const float* rstd,
                        const float* gamma, void* dres, void* dx, float* dgamma, float* dbeta, int N, int d,
                        float drop_p, unsigned long long seed, unsigned site, void* stream);
/* same, and dxsum[c] += sum_rows dx[row][c] (the stored bf16 values; d <= 1024): x is the output of a biased linear layer
 * (pos_ff.CoreNet.3), so this IS that layer's bias gradient -- one pass over dx less than mxl_colsum_bf16 afterwards */
int mxl_ln_residual_bwd_colsum(const void* dy, const void* dy2, const void* z, const float* mean, const float* rstd,
                               const float* gamma, void* dres, void* dx, float* dgamma, float* dbeta, float* dxsum, int N,
                               int d, float drop_p, unsigned long long seed, unsigned site, void* stream);
/* same, with an extra gradient stream added to the residual output: dres = dz + dadd (Reformer's y1 = x1 + f(x2) chains) */
int mxl_ln_residual_bwd_add(const void* dy, const void* dy2, const void* z, const float* mean, const float* rstd,
                            const float* gamma, const void* dadd, void* dres, float* dgamma, float* dbeta, int N, int d,
                            void* stream);
/* same, and in the same pass dx = dropout(dres) (mask of (seed, site), element index row * d + column: the mask mxl_dropout_bf16
 * applies to a compact (N, d) matrix) and, if dxsum != NULL, dxsum[c] += sum_rows dx[row][c] -- what mxl_dropout_bf16 /
 * mxl_dropout_colsum_bf16 over dres would produce, bit for bit, without the extra pass (the Reformer backward's
 * y = x + dropout(f(.)) chains of HF ReformerLayer / _ReversibleFunction, modeling_reformer.py:1535-1757 as cited in SURVEY.md;
 * here with stored activations instead of the reversible recompute).  dx may alias dy; d <= 1024 */
int mxl_ln_residual_bwd_add_drop(const void* dy, const void* dy2, const void* z, const float* mean, const float* rstd,
                                 const float* gamma, const void* dadd, void* dres, void* dx, float* dxsum, float* dgamma,
                                 float* dbeta, int N, int d, float drop_p, unsigned long long seed, unsigned site, void* stream);
/* out[b][t][:] = bf16(x[b][t][:] + bias[:]) with x strided (x_bs, x_rs elements), out compact (B,T,n) */
int mxl_add_rowbias_bf16(const void* x, long long x_bs, int x_rs, const float* bias, void* out, int B, int T, int n,
                         void* stream);
/* out[n] += sum_m X[m][n]  (bias gradients), X (M,N) bf16 with leading dimension ld */
int mxl_colsum_bf16(const void* X, float* out, int M, int N, int ld, void* stream);
/* Y = dropout(X) with the (seed, site) mask over the flat element index (mxl_dropout_bf16) and out[n] += sum_m Y[m][n] in the same
 * pass (the Reformer's feed_forward.output.dense bias gradient: the regenerated forward mask and the column sums); N % 8 == 0 */
int mxl_dropout_colsum_bf16(const void* X, void* Y, float* out, int M, int N, float drop_p, unsigned long long seed,
                            unsigned site, void* stream);
/* Y[m][n] = X[m][n] - mean_m X[m][n]  (bf16 in / out, fp32 arithmetic; N % 8 == 0).  The positional table enters the r_net
 * weight gradient dW_r = sum_d dRd[d]^T phi[d] centred over the distance axis: sum_d dRd[d] = 0 exactly (every softmax row's
 * score gradients sum to zero and every query sees exactly mem_len distances), so the constant part of phi multiplies nothing
 * but the bf16 rounding noise of the score gradients -- which would otherwise dominate the low-frequency columns. */
int mxl_center_columns_bf16(const void* X, void* Y, int M, int N, void* stream);
/* upstream TransfoXLModel._update_mems: out[b] = cat(mem[b], hid[b])[-M:], all (B, len, d) bf16, out != mem */
int mxl_mem_update(const void* mem, const void* hid, void* out, int B, int M, int T, int d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Projected adaptive log-softmax head (K7) = upstream ProjectedAdaptiveLogSoftmax (div_val=1) as used at
 * musicnlp/models/transformer_xl.py:185,193,198-200.  logits (B*T, ldl) f32 = hidden . [E ; cluster_weight]^T + bias,
 * columns [0,V) tokens, [V, V+ncl) clusters.  cutoffs_host: ncl ints on the HOST (read at enqueue time).
 * ---------------------------------------------------------------------------------------------------------- */
/* transformer_xl.py:176-182 all-ignored guard on label row 0 (in place, device) */
int mxl_label_guard(void* labels_row0, int T, long long eos, void* stream);
/* nll (B, T-1) f32 with the shift inside; lse (B*T, 2) f32 scratch kept for backward;
 * acc2[0] += sum(nll), acc2[1] += count(nll != 0)  (caller zeroes acc2) */
int mxl_adaptive_nll_fwd(const float* logits, int ldl, const void* labels, float* nll, float* lse, float* acc2, int B,
                         int T, int V, int ncl, const int* cutoffs_host, void* stream);
/* dlogits (B*T, ldd) bf16 of loss = sum(nll[nll != 0]) / count, times grad_scale; pad columns zeroed */
int mxl_adaptive_nll_bwd(const float* logits, int ldl, const void* labels, const float* nll, const float* lse,
                         const float* acc2, void* dlogits, int ldd, int B, int T, int V, int ncl,
                         const int* cutoffs_host, float grad_scale, void* stream);
/* the same gradient as a two-term bf16 sum: dlogits_hi = bf16(d), dlogits_lo = bf16(d - dlogits_hi).  The consumers (the head's
 * input-gradient and weight-gradient GEMMs, the bias column sum) run once per term and accumulate: a confident prediction of a
 * token that is not the label has d near 1 / count, where one bf16 term is too coarse for sums over tokens that cancel. */
int mxl_adaptive_nll_bwd_split(const float* logits, int ldl, const void* labels, const float* nll, const float* lse,
                               const float* acc2, void* dlogits_hi, void* dlogits_lo, int ldd, int B, int T, int V, int ncl,
                               const int* cutoffs_host, float grad_scale, void* stream);
/* labels=None branch: out (N, ldo) f32 full log-probabilities over the V tokens */
int mxl_adaptive_logprob(const float* logits, int ldl, float* out, int ldo, int N, int V, int ncl,
                         const int* cutoffs_host, void* stream);

/* ---- the same head for LARGE vocabularies (sub-word tokenizers, musicnlp/trainer/wordpiece_tokenizer.py:349-452: V up to 262144
 * with cutoffs [20000, 40000, 200000], musicnlp/models/transformer_xl.py:53-66), in upstream's own structure
 * (ProjectedAdaptiveLogSoftmax.forward with labels): the head softmax (c1 shortlist columns + one column per tail cluster) for
 * every token, the tail softmax of cluster i only for the tokens whose label lies in it (upstream's `mask_i.nonzero()` /
 * `index_select`), the caller walking tokens in chunks -- a (tokens x V) tensor never exists.  Token row = b*T + t; the label of
 * row (b, t) is labels[b][t+1] (shift inside, as above); rows with t = T-1 or an ignored label belong to no cluster. */
/* perm (ncl+2, B*T) int32: row g lists the token rows of group g in increasing order (g = 0 shortlist, 1..ncl tail clusters,
 * ncl+1 ignored); counts[g] their number; tgt_head[row] = the row's target column in the packed head logits [0,c1) + [c1, c1+ncl)
 * (-1: ignored); tgt_tail[row] = label - cutoff_i for a tail token, else -1. */
int mxl_cluster_bucket(const void* labels, int B, int T, int V, int ncl, const int* cutoffs_host, int* perm, int* counts,
                       int* tgt_head, int* tgt_tail, void* stream);
/* dst[j][:] = src[idx[j]][:] (bf16 rows of d elements, d % 8 == 0) and its adjoint dst[idx[j]][:] += src[j][:] (idx unique) */
int mxl_gather_rows_bf16(const void* src, int ld_src, const int* idx, void* dst, int n, int d, void* stream);
int mxl_scatter_add_rows_bf16(const void* src, const int* idx, void* dst, int ld_dst, int n, int d, void* stream);
/* logits (n_rows, ld) f32, row j belongs to token rows_idx[j] (or row0 + j when rows_idx is NULL):
 * lse_out[token] = logsumexp(logits[j][0:ncols]),  pick_out[token] = logits[j][tgt[token]] (0 when tgt[token] < 0) */
int mxl_rows_lse_pick(const float* logits, long long ld, int ncols, int n_rows, const int* rows_idx, int row0, const int* tgt,
                      float* lse_out, float* pick_out, void* stream);
/* nll[b][t] = nll_tok[b*T+t] = (head_lse - head_pick) + (tail_lse - tail_pick if a tail token), 0 for ignored rows;
 * acc2[0] += sum, acc2[1] += count(nll != 0) (caller zeroes acc2) -- the reduction of transformer_xl.py:198-200 */
int mxl_bucket_nll_finish(const float* head_lse, const float* head_pick, const float* tail_lse, const float* tail_pick,
                          const int* tgt_head, const int* tgt_tail, float* nll, float* nll_tok, float* acc2, int B, int T,
                          void* stream);
/* out (n_rows, ldo) bf16 = (softmax(logits[j][0:ncols]) - onehot(tgt[token])) * grad_scale / max(acc2[1], 1), pad columns and
 * the rows of ignored / zero-loss tokens zeroed; out_lo (optional): the bf16 remainder (see mxl_adaptive_nll_bwd_split) */
int mxl_rows_softmax_grad(const float* logits, long long ld, int ncols, int n_rows, const int* rows_idx, int row0, const int* tgt,
                          const float* lse, const float* nll_tok, const float* acc2, float grad_scale, void* out_hi, void* out_lo,
                          int ldo, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Optimiser (K18): torch.optim.AdamW + clip_grad_norm_ as configured at musicnlp/trainer/train.py:165-190.
 * ---------------------------------------------------------------------------------------------------------- */
int mxl_sumsq_f32(const float* x, long long n, float* out_accum, void* stream);
/* p,g,m,v f32 [n]; w16 bf16 working copy (or NULL).  g_eff = g * grad_scale * min(1, max_norm/(sqrt(*sumsq)*grad_scale+1e-6));
 * decoupled weight decay on elements [0, n_decay) only; step >= 1 */
int mxl_adamw_step(float* p, const float* g, float* m, float* v, void* w16, long long n, long long n_decay, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, const float* sumsq,
                   float max_norm, float grad_scale, void* stream);
int mxl_cast_f32_bf16(const float* x, void* y, long long n, void* stream);
/* y = (float)x.  With mxl_cast_f32_bf16 the two ends of the bf16 gradient exchange: a bucket of the flat fp32 gradient buffer
 * is narrowed into a bf16 staging buffer, all-reduced over RCCL at half the bytes (186 MB instead of 372 MB per step at
 * 12L/768d), and widened back in place. */
int mxl_cast_bf16_f32(const void* x, float* y, long long n, void* stream);
/* dst[b][c][r] = src[b][r][c] (bf16; element strides between batch items).  Keeps [in][out] copies of the Linear weights so
 * that the input gradient dX = dY W (autograd of F.linear) runs in the K-contiguous GEMM form. */
int mxl_transpose_bf16(const void* src, void* dst, int rows, int cols, int ld_src, int ld_dst, int batch,
                       long long src_bstride, long long dst_bstride, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Autoregressive decode (A4/A10): replaces the per-token path of HF GenerationMixin.greedy_search / sample driving
 * MyTransfoXLLMHeadModel.prepare_inputs_for_generation (musicnlp/models/transformer_xl.py:223-241) and the upstream
 * cat(mems, h) -> qkv_net recomputation.  All step state is on the device (t_dev = position of the token being fed,
 * rng_ctr), so a step is capture-safe and replays as a hipGraph.
 *   ids     : (B, ld_ids) int64 token buffer; step reads ids[b][t], sampler writes ids[b][t+1]
 *   k/vcache: head-major (B, H, M, dh) bf16 rings of projected K/V rows, slot = position mod M, zero-initialised
 *             (= upstream zero mems)
 * ---------------------------------------------------------------------------------------------------------- */
int mxl_decode_embed(const void* ids, int ld_ids, const int* t_dev, const void* E, void* out, int B, int d, int V,
                     float scale, void* stream);
/* cache[b][t mod M] <- k, v of the (B, 3d) qkv rows of the current token */
int mxl_kv_append(const void* qkv, void* kcache, void* vcache, const int* t_dev, int B, int M, int d, int dh,
                  const float* r_r_bias, void* qr_out, void* stream);   /* qr_out (B, d) bf16 = q + r_r_bias, or NULL */
/* after the prompt forward: cache slots <- K/V rows of the last min(T, M) positions of a (B, T, 3d) qkv buffer */
int mxl_kv_fill(const void* qkv, void* kcache, void* vcache, int B, int T, int M, int d, int dh, void* stream);
/* left-padded prompts: k = v = 0 (columns [d, 3d)) in rows j < n_pad[b] of a (B, T, 3d) bf16 qkv buffer, so every pad column is
 * one more zero-memory slot of the prompt pass (qkv_net has no bias).  n_pad (B,) int32 on the device, each in [0, T]; q columns
 * and rows j >= n_pad[b] are not touched.  Capture-safe (no host read of n_pad). */
int mxl_kv_zero_pad(void* qkv, const int* n_pad, int B, int T, int d, void* stream);
/* positional term of a decode step for the whole batch: bd[b][h][r] = sum_e qr[b][h*dh + e] * rd[r][h*dh + e], r < M.
 * qr (B <= 64, ld_qr) bf16 = q + r_r_bias (mxl_decode_qkv / mxl_kv_append), rd (M, ld_rd) bf16 = r_net(pos_emb) of the layer
 * (rows = distances), bd (B, H, M) f32.  dh = 64.  Replaces the `BD = einsum("ibnd,jnd->ijbn", rr_head_q, r_head_k)` of
 * RelPartialLearnableMultiHeadAttn.forward (transformers 4.25.1 modeling_transfo_xl.py) for a single query position. */
int mxl_decode_bd(const void* qr, const void* rd, float* bd, int B, int H, int dh, int M, int ld_qr, int ld_rd, void* stream);
/* single-query relative attention over the ring, distances 0..M-1.  bd (B, H, M) f32 = (q + r_r_bias) . rd[dist], the
 * positional term for the whole batch (one mxl_gemm_bf16_batched per layer over heads); out (B, H*dh) bf16 */
int mxl_relattn_decode(const void* qkv, const void* kcache, const void* vcache, const float* bd, const float* r_w_bias,
                       void* out, const int* t_dev, int B, int H, int dh, int M, float scale, void* stream);
/* The same with every (sequence, head) ring cut into `pieces` (1..8) workgroups -- for launches whose B * H workgroups would
 * not fill the CUs evenly (a CU streams HBM at a fixed rate however many workgroups it holds: 384 rings on 256 CUs take the
 * time of two).  Each piece runs the softmax over its slots with its own reference; the piece that finishes last merges the
 * (o, max, sum) partials in piece order, so the result is reproducible.  The probabilities are rounded to bf16 relative to the
 * piece's own maximum: outputs differ from mxl_relattn_decode's in the last bf16 bit at most.  ws: mxl_relattn_decode_split_ws_bytes
 * bytes; arrived: B * H ints, zero before the first call (the kernel leaves them zero).  pieces = 1 is mxl_relattn_decode. */
size_t mxl_relattn_decode_split_ws_bytes(int B, int H, int dh, int pieces);
int mxl_relattn_decode_split(const void* qkv, const void* kcache, const void* vcache, const float* bd, const float* r_w_bias,
                             void* out, const int* t_dev, int B, int H, int dh, int M, float scale, int pieces, float* ws,
                             int* arrived, void* stream);
/* mxl_relattn_decode_split with per-row stop state: unfinished (B,) int32 on the device, 0 = the row is finished (eos emitted).
 * A finished row's workgroups read no K / V and leave zeros in its output slice (B, H*dh); live rows are bit-identical to
 * mxl_relattn_decode_split.  unfinished = NULL: every row is live. */
int mxl_relattn_decode_split_live(const void* qkv, const void* kcache, const void* vcache, const float* bd, const float* r_w_bias,
                                  void* out, const int* t_dev, int B, int H, int dh, int M, float scale, int pieces, float* ws,
                                  int* arrived, const int* unfinished, void* stream);
/* mxl_relattn_decode_split_live over indexed rings (mxl_beam_owner_follow): the K row and the V row of a written slot s of row b are
 * read from the ring of row (b / nb) * nb + owner[b][s]; owner (B, M) uint8, its row staged into shared memory at kernel entry.
 * Never-written slots take the positional term alone, with no K / V read and no owner read.  Same arithmetic in the same order as
 * mxl_relattn_decode / _split / _split_live: the output equals theirs bit for bit on rings gathered by the table, and on the same
 * rings under the identity table.  An owner byte >= nb reads the item's last row.  pieces 1..8 with ws / arrived for pieces > 1
 * (pieces = 1: both may be NULL), unfinished (B,) int32 or NULL.  owner non-null and 16-byte aligned, 1 <= nb <= 16, B % nb == 0,
 * B <= 65535, M % 16 == 0, M * 5 + 1024 bytes of shared memory <= 64 KiB; else MXL_EINVAL.  dh 16 / 32 / 64, else MXL_EUNSUPPORTED. */
int mxl_relattn_decode_owned(const void* qkv, const void* kcache, const void* vcache, const void* owner, int nb, const float* bd,
                             const float* r_w_bias, void* out, const int* t_dev, int B, int H, int dh, int M, float scale,
                             int pieces, float* ws, int* arrived, const int* unfinished, void* stream);
/* FP8 K/V rings (opt-in).  A ring (B, H, M, dh) of bf16 is held as kc8 (B, H, M, dh) uint8 of OCP e4m3fn bytes and ke (B, H, M)
 * int8 exponents, one per slot and head (vc8 / ve alike); the stored value is fp8 * 2^e.  For a row x of dh elements with
 * amax = max|x| = m 2^k, m in [0.5, 1): e = k - 9 if m <= 0.875, else k - 8 (the smallest e with amax 2^-e <= 448), clamped to
 * [-126, 127]; amax = 0 gives e = 0 and zero bytes; byte j = e4m3fn(x_j 2^-e), round to nearest even, subnormals kept.  Every
 * dequantised value is a bf16 value.  Zero bytes with e = 0 are a zero memory (never-written slots, left-pad columns).
 * dh = 16, 32 or 64 (else MXL_EUNSUPPORTED, nothing launched); kc8 / vc8 16-byte aligned.
 *
 * mxl_kv_append_fp8: mxl_kv_append on such rings -- slot *t_dev mod M of all four tensors <- the quantised k / v thirds of the
 * (B, 3d) qkv rows, every other slot untouched; qr_out (B, d) bf16 = q + r_r_bias bit for bit as mxl_kv_append writes it, or NULL.
 * *t_dev is read on the device (capture-safe). */
int mxl_kv_append_fp8(const void* qkv, void* kc8, void* ke, void* vc8, void* ve, const int* t_dev, int B, int M, int d, int dh,
                      const float* r_r_bias, void* qr_out, void* stream);
/* mxl_kv_fill on fp8 rings: slots (p mod M) <- the quantised K / V rows of the last min(T, M) positions p of a (B, T, 3d) qkv buffer */
int mxl_kv_fill_fp8(const void* qkv, void* kc8, void* ke, void* vc8, void* ve, int B, int T, int M, int d, int dh, void* stream);
/* mxl_relattn_decode_split_live on fp8 rings: pieces 1..8 with ws (mxl_relattn_decode_split_ws_bytes) and arrived (B * H ints,
 * zero before the first call, left zero) for pieces > 1, unfinished (B,) int32 or NULL.  Same arithmetic as the bf16 entry on the
 * dequantised rings: q' = bf16(q + r_w_bias), f32 scores with the bd term, never-written slots as the positional term alone and
 * counted in the denominator, P rounded to bf16 before the P V sum, pieces merged in piece order; the summation order within a
 * row differs (16 elements per lane).  M * 4 + 1024 bytes of shared memory <= 64 KiB (else MXL_EINVAL, nothing launched). */
int mxl_relattn_decode_fp8(const void* qkv, const void* kc8, const void* ke, const void* vc8, const void* ve, const float* bd,
                           const float* r_w_bias, void* out, const int* t_dev, int B, int H, int dh, int M, float scale, int pieces,
                           float* ws, int* arrived, const int* unfinished, void* stream);
/* mxl_relattn_decode_fp8 over indexed rings (mxl_beam_owner_follow): the 16-byte K and V loads and the two exponents of a written slot
 * s of row b are read from the rings of row (b / nb) * nb + owner[b][s]; owner (B, M) uint8, its row staged into shared memory
 * before the first ring load.  Never-written slots take the positional term alone, with no ring byte and no owner byte read; a
 * finished row reads neither and gets zeros.  Same arithmetic in the same order as mxl_relattn_decode_fp8: the output equals its
 * output bit for bit on rings (bytes and exponents) gathered by the table, and on the same rings under the identity table.  An owner
 * byte >= nb reads the item's last row.  pieces 1..8 with ws / arrived for pieces > 1 (pieces = 1: both may be NULL), unfinished
 * (B,) int32 or NULL.  owner non-null and 16-byte aligned, 1 <= nb <= 16, B % nb == 0, B <= 65535, M % 16 == 0, M * 5 + 1024 bytes
 * of shared memory <= 64 KiB; else MXL_EINVAL.  dh 16 / 32 / 64, else MXL_EUNSUPPORTED.  Nothing is launched on either. */
int mxl_relattn_decode_fp8_owned(const void* qkv, const void* kc8, const void* ke, const void* vc8, const void* ve, const void* owner,
                                 int nb, const float* bd, const float* r_w_bias, void* out, const int* t_dev, int B, int H, int dh,
                                 int M, float scale, int pieces, float* ws, int* arrived, const int* unfinished, void* stream);
/* next token from log-probs (B, ldl): repetition penalty over the ids already in the row (positions 0..*t_dev; HF's
 * RepetitionPenaltyLogitsProcessor, 1.0 = off), then greedy argmax (do_sample=0) or temperature -> top-k -> top-p ->
 * typical-p (HF's TypicalLogitsWarper, 1.0 = off) -> renormalise -> multinomial (do_sample=1), as HF's logits warpers with
 * renormalize_logits=True -- the `sample` strategy's accepted keys at musicnlp/trainer/eval.py:277-326.
 * V <= 2048.  out_probs (B, V) f32 optional: the renormalised distribution actually sampled from (test hook). */
int mxl_sample(const float* logprobs, int ldl, int V, void* ids, int ld_ids, const int* t_dev,
               unsigned long long* rng_ctr, unsigned long long seed, int B, int do_sample, int top_k, float top_p,
               float temperature, float repetition_penalty, float typical_p, float* out_probs, void* stream);
/* The same recipe for V > 2048 (the sub-word vocabularies of musicnlp/trainer/wordpiece_tokenizer.py:349-452, whose sizes pick
 * the cutoff ladder of musicnlp/models/transformer_xl.py:53-66): no sort -- every warper and the multinomial draw are bisections
 * over a 32-bit order key with integer (fixed-point) conditional sums, so the result is independent of timing.  scratch: B * V * 8
 * bytes.  Any V >= 1 is accepted (mxl_sample is faster below 2049). */
int mxl_sample_large(const float* logprobs, int ldl, int V, void* ids, int ld_ids, const int* t_dev,
                     const unsigned long long* rng_ctr, unsigned long long seed, int B, int do_sample, int top_k, float top_p,
                     float temperature, float repetition_penalty, float typical_p, float* out_probs, float* scratch,
                     void* stream);
/* t_dev += 1; rng_ctr += 1 */
int mxl_decode_advance(int* t_dev, unsigned long long* rng_ctr, void* stream);
/* ------------------------------------------------------------------------------------------------------------
 * Rules of a generation.  Eight optional groups of per-row state on the device, applied around every sampled token.  They cross the
 * ABI as one struct, mxl_rules (below), which three entries take by pointer: mxl_sample_step, mxl_rules_mask, mxl_rules_advance.  The
 * struct is read during the call and handed to the kernel by value: the caller may reuse it at once.  A zero-initialised struct
 * means every group is off.
 * A group is off when its state pointer is NULL: unfinished (with alive), gstate (with allow, next), gbar (with grem, slots, bars),
 * gleft, gkey (with keys, pcs, inkey), gpos (with gforce, guide, glen), gpart (with gfloor, grange, reg), gcopy (with gbars, gstop,
 * plan, nplan, barcol).  Within a group either every pointer is given or none; the budget, the count, the guide and the repeat need
 * `cls`; the repeat also needs the count and, where the words move, the stop group, and is never on beside the guide; anything else,
 * a NULL or misaligned `rules` included, is MXL_EINVAL.
 *
 * stop: eos_id, pad_id, min_length, unfinished, alive -- stopping at eos (HF greedy_search / sample with an eos_token_id).
 *   unfinished (B,) int32 (1 = live; set to 1 before the first sampled token) and alive, one int32 = the number of live rows after
 *   the launch.  Per row: next = live ? token : pad_id, then live &= (next != eos_id).  min_length (HF MinLengthLogitsProcessor,
 *   after the repetition penalty): the score of eos_id is -inf while the row (columns 0..*t_dev) is shorter than min_length; 0 = off.
 * grammar: cls, allow, next, C, gstate -- every row may only emit tokens that a token-class automaton allows in the row's state.
 *   Tables: cls (V,) uint8 token -> class (C <= 32 classes); allow (S,) uint32, bit c set <=> class c may be emitted in state s
 *   (S <= 256); next (S, C) uint8 successor state (entries of barred classes hold s itself).  gstate (B,) int32 is the state of
 *   every row.  A barred token's score is -inf after the repetition penalty and min_length and before temperature / top-k / top-p /
 *   typical-p (HF's logits-processor order), so the warpers and the renormalised draw see allowed tokens only.  The caller
 *   guarantees that no reachable state bars every token.
 * budget: slots, bars, opens, need_free, need_full, gbar, grem -- every channel of a generated bar is exactly as long as the row's
 *   time signature.  Per row two int32 words: gbar (bar length in slots; 0 = the row is unconstrained) and grem (slots still free in
 *   the open channel).  Tables: slots (V,) uint16, duration token -> slots, 0 = not a duration, 0xFFFF = a duration of unknown
 *   length; bars (V,) uint16, time signature token -> bar length in slots (0 = unconstrained), 0xFFFF = not a time signature; class
 *   bit masks opens (rem = bar), need_free (allowed only while rem > 0) and need_full (allowed only at rem == 0), over the classes of
 *   `cls`.  In a row with bar > 0 a token is barred if its slots entry exceeds rem or its class is in need_free at rem == 0 or in
 *   need_full at rem > 0; rows with bar == 0 are untouched.  A token moves the row: a bars entry sets bar (rem = 0), a class in opens
 *   sets rem = bar, a slots entry k takes k from rem.  The rule never reads the grammar state.
 *   Format of a slots entry k other than 0xFFFF: bits 0..14 are the slots the token TAKES from rem, and bit 15 set means it NEEDS one
 *   more free than it takes: the token is barred unless (k & 0x7FFF) + (k >> 15) <= rem, and a kept one leaves rem - (k & 0x7FFF).
 *   That is for a token that stands for several base tokens and ends on an open note start (grammar.subword_grammar: `pitch
 *   duration pitch`), whose open pitch still needs a duration.  Entries below 0x8000 therefore mean what they always meant, and
 *   0xFFFF stays "unknown length": barred in a row with bar > 0, admitted in a row with bar == 0.
 * count: count, end, gleft -- a row opens exactly as many further bars as it was asked for.  Per row one int32 word: gleft, the bars
 *   the row may still open; < 0 = no limit, the row is untouched.  count and end are class bit masks over the classes of `cls` (the
 *   music grammar: <bar> and </s>).  A class in count is barred at gleft == 0, a class in end while gleft > 0, and a kept token of a
 *   count class takes 1 from a positive gleft.  Under a bar budget the end class is thereby the only one left when the last bar is
 *   full; without one the rule cannot force the end, it only bars a further bar and an early end.
 * key: keys, pcs, inkey, gkey -- a row whose key is known emits only pitches of that key.  Per row one int32
 *   word: gkey, -1 = the row has no key and is untouched, 0..23 = the ordinal of its key (the order of the reference's key enum, which
 *   the in-key ratio metric uses).  Tables: keys (V,) uint8, key token -> ordinal, 0xFF = any other token; pcs (V,) uint8, pitch token
 *   -> pitch class 0..11, 0xFF = anything the metric does not count as a pitch (rests and the rare-pitch token included: they are never
 *   barred); inkey (24,) uint16, bit pc of inkey[k] set <=> pitch class pc belongs to key k.  In a row with gkey >= 0 token v is barred
 *   iff pcs[v] != 0xFF and bit pcs[v] of inkey[gkey] is clear; the group reads neither `cls` nor the grammar state, and works with
 *   every other group off.  The token is -inf in the same place as under the grammar, the budget and the count.  A kept token with
 *   keys[tok] != 0xFF sets gkey = keys[tok]; nothing else changes gkey.
 *   No dead end: every key holds 7 of the 12 pitch classes, and every pitch class has tokens in each of the music vocabularies (midi,
 *   step, degree), so wherever the grammar or the budget allows "a pitch" -- they judge the class of a token, never which pitch it is --
 *   a pitch of the row's key remains (besides the rest, which the rule never bars).  The host checks it when the tables are built: every
 *   key keeps at least one pitch token.
 * guide: guide, ld_guide, glen, enter, leave, gpos, gforce -- part of a row's output is given, not chosen:
 *   in the music grammar the <bar> <melody> ... <bass> span of every bar, under which the row writes the bass.  Per row two int32
 *   words: gpos, the next index into the row's guide, and gforce, 1 = the row is being fed from its guide, 0 = it chooses freely.
 *   Tables: guide (B, ld_guide) int32, each row's guide tokens; glen (B,) int32, each row's guide length (<= ld_guide), 0 = the row
 *   has no guide and is untouched; enter and leave, class bit masks over the classes of `cls` (the music grammar: <bar> and <bass>).
 *   In a row with gforce == 1 and gpos < glen every token except guide[b][gpos] is barred and that token is never barred: the group
 *   overrides the grammar, the budget, the count, the key and min_length (the caller guarantees that the guide is legal and holds
 *   token ids below V); the token is -inf in the same place as under the other groups, so greedy and sampled rows both keep it.  A row
 *   with gforce == 0 is masked by the other groups alone.  A kept token moves the row: under gforce == 1, gpos += 1 and a token whose
 *   class is in leave sets gforce = 0; under gforce == 0 a token whose class is in enter, while gpos < glen, sets gforce = 1 and gpos
 *   += 1 -- it is the guide's own <bar>.  The words of every other group move along a forced token as along a chosen one.  The group
 *   does not stop a row: the caller sets gleft to the number of bars in the guide, so the count group bars the end while guided bars
 *   are owed and a further bar once none is.
 * register: reg, grange, gpart, gfloor, gap -- every part stays in its register, and the bass under the
 *   melody.  Per row three int32 words: grange, the row's bounds lo_melody, hi_melody, lo_bass, hi_bass as inclusive MIDI numbers, one
 *   byte each from the lowest (fixed for the generation, never written; 0, 127, 0, 127 = unconstrained); gpart, 0 = no part is open,
 *   1 = the melody, 2 = the bass; gfloor, the lowest melody pitch of the open bar, 128 = none yet.  One scalar for the launch: gap, -1
 *   = the bass is not tied to the melody, g >= 0 = it is.  Table: reg (V,) uint8, pitch token -> MIDI number 0..127; 0x80 / 0x81 /
 *   0x82 = the <melody> / <bass> / <bar> token; 0xFF = any other token, the rest and the rare-pitch token included.  In a row with
 *   gpart = p > 0 token v with reg[v] <= 127 is barred iff reg[v] lies outside [lo_p, hi_p]; in the bass with gap >= 0 and gfloor <
 *   128 the upper bound is min(hi_bass, gfloor - gap) -- gap 0 lets the bass touch the bar's lowest melody note, gap 1 keeps it strictly
 *   below.  A row with gpart == 0 is untouched.  The group reads neither `cls` nor the grammar state and works with every other group
 *   off; the token is -inf in the same place as under the other groups, and a token the guide forces is never barred.  A kept token
 *   moves the row: 0x80 sets gpart = 1, 0x81 sets gpart = 2, 0x82 sets gpart = 0 and gfloor = 128, a pitch under gpart == 1 sets
 *   gfloor = min(gfloor, pitch) -- a forced melody note is not judged but does lower the floor -- and nothing else moves the words.
 *   The bound is per bar, not aligned in time: "under the lowest melody note of the bar" is sufficient to keep the parts from
 *   crossing, not necessary.
 *   No dead end: the rule judges pitches by their MIDI number alone and never bars a token whose reg entry is above 127.  The rest and
 *   the rare-pitch token are such tokens and belong to the grammar's class `pitch`, and the budget judges a pitch by that class alone,
 *   so wherever the grammar or the budget allows "a pitch" one of the two remains even when the bounds leave no pitched token (the
 *   floor under lo_bass, say).  The key rule never bars them either.
 * repeat: plan, ld_plan, nplan, barcol, renter, rleave, span, gbars, gcopy, gstop -- song form: a planned
 *   bar repeats an earlier bar the row generated itself, token for token, out of the row's own id history.  A row's generated bars
 *   are the bars it opens after its prompt, numbered 0, 1, ... in the order of their `enter` tokens; the bar open at the end of the
 *   prompt is finished freely and has no number, as the count group counts.  Tables: plan (B, ld_plan) int32, plan[b][k] = -1:
 *   generated bar k is free, j with 0 <= j < k: bar k repeats generated bar j; nplan (B,) int32, the planned bars of the row (<=
 *   ld_plan), 0 = the row is untouched; barcol (B, ld_plan) int32, WRITTEN by the group: the column of ids that holds the `enter` token
 *   of generated bar k; renter and rleave, class bit masks over the classes of `cls` (the music grammar: <bar> and <bass>); span, one
 *   scalar for the launch: 0 = a repeat copies the whole source bar, melody and bass, 1 = it copies up to and including the first
 *   `leave` token, so the row gets the same melody and writes a new bass under it.  Per row three int32 words: gbars, the bars opened
 *   so far (starts at 0); gcopy, the column of the row's own history the next token is copied from, -1 = the row chooses (starts at
 *   -1); gstop, the column where the copy ends, exclusive.  The history is ids (B, ld_ids) itself in the fused and the advance entry;
 *   the mask entry, which sees no ids, takes it as hist / ld_hist.
 *   In a row with nplan > 0 and gcopy >= 0 every token except ids[b][gcopy] is barred and that token is never barred: the group
 *   overrides the grammar, the budget, the count, the key, the register and min_length exactly as the guide's forced token does, in
 *   the same place (-inf where the row enters LDS, before the warpers), so greedy and sampled rows both keep it, and the RNG counter
 *   advances as always.  A kept token of class c, written at column col, moves the row: with gcopy >= 0, gcopy += 1, and gcopy = -1
 *   once gcopy >= gstop, or under span == 1 when c is in rleave; else, if c is in renter and gbars < nplan: k = gbars, barcol[b][k] =
 *   col, gbars = k + 1, and with j = plan[b][k] >= 0, from = barcol[b][j] + 1 and stop = (j + 1 == k) ? col : barcol[b][j + 1], a
 *   copy starts (gcopy = from, gstop = stop) if from < stop.  Nothing else moves the words; the words of every other group move along
 *   a copied token as along a chosen one (a copied melody note lowers the register's floor).  The group does not stop a row: the
 *   caller sets gleft = nplan, so the row opens exactly the planned bars and, under a bar budget, ends when the last one is full.
 *   No dead end: a source bar is complete when its copy starts -- bar j + 1 has been opened, at the latest by the very `enter` token
 *   that starts the copy -- so the copied span is a whole bar (span 0) or a whole melody channel with its <bass> (span 1) that the
 *   grammar and the budget admitted once.  The source started from the automaton state BAR, which is where every `enter` token
 *   leads, and so does its copy.  Time signature and key tokens occur in the header only (MUSIC_TRANSITIONS), so the bar length and,
 *   for what the row chooses after a span-1 copy, the key are the source's: the copy fills its channels exactly as the source did,
 *   and under span 1 it fills the melody channel, after which the row is in B_OPEN with a full budget, where any bass the budget
 *   admits closes the bar.  A source that is itself a copy is fine: the history holds real tokens.  Sources are generated bars only
 *   (j < k, columns the row wrote itself after its prompt), so a copy never reads a pad or a column not yet written: gcopy < gstop
 *   <= col.
 *
 * The words move along the token a row keeps, after the stop rule: a row that was finished before the step emits pad and keeps its
 * words; the step in which a row emits eos still moves them.  Each row's words are read and written for that row alone.
 * ---------------------------------------------------------------------------------------------------------- */
/* The groups above, in that order, as the kernels take them.  `unsigned` is a 32-bit word.  With gpart NULL `gap` is ignored, with
 * gcopy NULL renter / rleave / span / hist / ld_hist are.  The next rule is one more group at the end and a new MXL_ABI_VERSION. */
typedef struct mxl_rules {
    int eos_id, pad_id, min_length;     /* stop */
    int* unfinished;
    int* alive;
    const unsigned char* cls;           /* grammar; the token classes also serve budget, count, guide and repeat */
    const unsigned* allow;
    const unsigned char* next;
    int C;
    int* gstate;
    const unsigned short* slots;        /* budget */
    const unsigned short* bars;
    unsigned opens, need_free, need_full;
    int* gbar;
    int* grem;
    unsigned count, end;                /* count */
    int* gleft;
    const unsigned char* keys;          /* key */
    const unsigned char* pcs;
    const unsigned short* inkey;
    int* gkey;
    const int* guide;                   /* guide */
    int ld_guide;
    const int* glen;
    unsigned enter, leave;
    int* gpos;
    int* gforce;
    const unsigned char* reg;           /* register */
    const int* grange;
    int* gpart;
    int* gfloor;
    int gap;
    const int* plan;                    /* repeat */
    int ld_plan;
    const int* nplan;
    int* barcol;
    unsigned renter, rleave;
    int span;
    int* gbars;
    int* gcopy;
    int* gstop;
    const long long* hist;              /* the rows' ids (B, ld_hist) int64, read by mxl_rules_mask alone */
    int ld_hist;
} mxl_rules;
/* sizeof(mxl_rules) as the library was built: a binding that lays the struct out itself compares its own size with this */
size_t mxl_rules_size(void);
/* mxl_sample + mxl_decode_embed of the sampled token + mxl_decode_advance + the rules in one launch -- the tail of one decode step
 * and the head of the next.  The row's workgroup writes ids[b][t + 1] and emb_out[b] = E[token] * scale (bf16, (B, d)), the token
 * being the one after the stop rule (pad for a finished row); the workgroup that finishes last advances *t_dev and *rng_ctr and
 * writes *alive (counter: one int, zero before the first call, left zero).  `scores` (B, ldl) may be log-probabilities or, when
 * repetition_penalty == 1, the head's raw logits: argmax, top-k / top-p / typical-p and the renormalised draw do not change under the
 * per-row shift that separates the two.  The masks are applied where the row enters LDS.  V <= 2048; with the stop group B <= 32767;
 * the budget, the count, the guide and the repeat need the grammar group here, the key and the register group stand alone, and the
 * repeat feeds its token through the guide's arm of the sampler.  Without the stop group eos_id / pad_id / min_length are ignored.
 * The history of the repeat group is ids / ld_ids: rules->hist / ld_hist are ignored.  The state words and barcol are written by the
 * row's thread 0.  out_probs (B, V) f32 optional, with do_sample: the renormalised distribution the rows were drawn from, as
 * mxl_sample's (test hook). */
int mxl_sample_step(const float* scores, int ldl, int V, void* ids, int ld_ids, int* t_dev, unsigned long long* rng_ctr,
                    unsigned long long seed, int B, int do_sample, int top_k, float top_p, float temperature,
                    float repetition_penalty, float typical_p, const void* E, void* emb_out, int d, float scale,
                    int* counter, const mxl_rules* rules, float* out_probs, void* stream);
/* The same rules around mxl_sample / mxl_sample_large, one launch on either side.  mxl_rules_mask, before the sampler:
 * scores[b][v] = -inf in place wherever an enabled group bars token v, one thread per score, every other score untouched (the
 * sampler's repetition penalty leaves -inf at -inf, so the result is that of masking after the penalty).  It reads no stop state:
 * eos_id is barred while *t_dev + 1 < min_length whenever min_length > 0.  No launch when nothing can be barred.
 * mxl_rules_advance, after the sampler and mxl_decode_advance (the token just written is ids[b][*t_dev]): every row that chose its
 * token moves its words along it, then the stop rule is applied to the token and *alive written.  No launch when every group is off.
 * The mask, which sees no ids, reads the repeat group's history from rules->hist / ld_hist; the advance takes it from ids / ld_ids
 * and ignores the two fields, and writes the state words and barcol from the row's thread. */
int mxl_rules_mask(float* scores, int ldl, int B, int V, const int* t_dev, const mxl_rules* rules, void* stream);
int mxl_rules_advance(void* ids, int ld_ids, const int* t_dev, int B, int V, const mxl_rules* rules, void* stream);
/* (gpart, gfloor) of every row after columns 0..Tp-1 of ids (B, ld_ids) int64, walked from the words gpart[b] / gfloor[b] hold at the
 * launch under the bounds grange[b] and `gap` (the register group above).  Ids < 0 (left pads) and ids >= V are skipped.  Columns
 * before `from` only move the words -- the prompt's pitches are not judged; first_bad[b] = the first column >= from that holds a pitch
 * outside the bounds of the row's open part, where the walk of that row stops, -1 = none.  from = Tp: the words after the prompt. */
int mxl_register_scan(const void* ids, int ld_ids, int Tp, int from, int B, int V, const void* reg, const void* grange, int gap,
                      int* gpart, int* gfloor, int* first_bad, void* stream);
/* Key of every row after columns 0..Tp-1 of ids (B, ld_ids) int64, walked from the key gkey[b] holds at the launch (-1 = none): a
 * key token sets it.  Ids < 0 (left pads) and ids >= V are skipped.  Columns before `from` only move the key -- a prompt supplies its
 * key, its pitches are not judged; first_bad[b] = the first column >= from that holds a pitch outside the row's key, where the walk
 * of that row stops, -1 = none.  from = Tp: the key after the prompt, nothing judged. */
int mxl_key_scan(const void* ids, int ld_ids, int Tp, int from, int B, int V, const void* keys, const void* pcs, const void* inkey,
                 int* gkey, int* first_bad, void* stream);
/* Grammar state of every row after its prompt: ids (B, ld_ids) int64, columns 0..Tp-1 walked from `start`; a column holding an id < 0
 * is skipped (left pad).  first_bad[b] = column of the first token the state bars (or an id >= V), where the walk of that row stops;
 * -1 = the prompt obeys the grammar. */
int mxl_grammar_scan(const void* ids, int ld_ids, int Tp, int B, int V, const void* cls, const void* allow, const void* next, int C,
                     int start, int* gstate, int* first_bad, void* stream);
/* (gbar, grem) of every row after its prompt, from (0, 0): columns 0..Tp-1, ids < 0 (left pads) and ids >= V (mxl_grammar_scan
 * reports those) skipped.  first_bad[b] = column of the first token the budget bars, where the walk of that row stops; -1 = none. */
int mxl_budget_scan(const void* ids, int ld_ids, int Tp, int B, int V, const void* cls, const void* slots, const void* bars,
                    unsigned opens, unsigned need_free, unsigned need_full, int* gbar, int* grem, int* first_bad, void* stream);
/* ------------------------------------------------------------------------------------------------------------
 * Beam search on the device (HF 4.25.1 beam_search + BeamSearchScorer.process).  An item is the nb <= 16 decoder rows of one prompt,
 * rows b * nb .. b * nb + nb - 1 of rows = Bs * nb; one workgroup per item, one launch per decode step, between mxl_rules_mask and
 * mxl_decode_advance / mxl_rules_advance.  cur_len = *t_dev + 1: the rows hold columns 0..cur_len-1, the chosen token goes to cur_len.
 *
 * select: the 2 * nb best of the nb * V candidates logp[r][v] + beam_scores[r] (logp (rows, ldl) f32, ldl >= V >= 2, already masked
 *   by the rules: -inf = barred), ordered by score descending, then by flat index j * V + v ascending (j = the beam within the item);
 *   that order is part of the contract.  -inf takes part like any number and sorts last.  Exact for any V.
 * walk: the candidates in rank order.  An eos at rank < nb joins the item's hypothesis store with score s / cur_len ** length_penalty:
 *   a free slot takes it, a full store replaces its worst entry (the lowest slot among equals) only if the newcomer beats it; an eos at
 *   rank >= nb is skipped; the first nb other candidates continue: beam_scores[row] = s, beam_idx[row] = the row they continue (int32,
 *   a row of the whole batch), their token -> ids[row][cur_len].  Then done |= (the store is full) && (early_stopping || worst stored
 *   score >= rank-0 score / cur_len ** length_penalty), and *n_done counts the items that became done.  An item done before the launch
 *   is frozen: identity beam_idx, pad_id tokens, scores and store untouched.
 * store: hyp_ids (Bs, nb, ld_ids) int64 with hyp_len (Bs, nb) int32 and hyp_score (Bs, nb) f32, slots 0..hyp_n[b]-1 of item b in use;
 *   hyp_n (Bs,), done (Bs,) and n_done (1,) int32, all zero before the first step.  The added hypotheses ids[src][:cur_len] are copied
 *   before anything in ids moves.
 * reorder: ids (rows, ld_ids) int64 follows beam_idx in place, columns 0..cur_len-1; moved[b] = 0 when item b's beam_idx is the
 *   identity.  words (optional, with n_words <= 256 and word_stride >= rows): packed per-row int32 words, word w of row r at
 *   words[w * word_stride + r] (the rules' state words); every word of every row follows beam_idx the same way.
 * dead rows: a row that continues from a -inf candidate -- a barred token, or the child of a dead row -- gets pad_id and keeps -inf.
 *   With words given its word 0, the stop group's `unfinished`, is cleared, as are those of the rows of a done item: the advance
 *   launch with the stop group on then leaves the row's words alone, the mask launch keeps a valid state, the ring attention skips it.
 * Every pointer of the store group is needed; words == NULL exactly when n_words == 0; nb > 16 and anything else amiss is MXL_EINVAL. */
int mxl_beam_step(const float* logp, int ldl, float* beam_scores, void* ids, int ld_ids, const int* t_dev, int Bs, int nb, int V,
                  int eos_id, int pad_id, float length_penalty, int early_stopping, void* hyp_ids, int* hyp_len, float* hyp_score,
                  int* hyp_n, int* done, int* n_done, int* beam_idx, int* moved, int* words, int n_words, int word_stride,
                  void* stream);
/* Diverse (group) beam search (HF 4.25.1 group_beam_search + HammingDiversityLogitsProcessor; the reference's 'beam' strategy runs
 * num_beams=4, num_beam_groups=2): mxl_beam_step for ng groups of gs = nb / ng beams, rows g * gs .. g * gs + gs - 1 of the item,
 * walked in order inside the item's workgroup.  Everything not said here is mxl_beam_step's: the store (one per item, capacity nb,
 * shared by its groups), the order, dead rows, frozen items, ids and the words.
 * score: (logp[j][v] - diversity_penalty * cnt[v]) + beam_scores[j], product, difference and sum each rounded to f32 on its own;
 *   cnt[v] = how many rows of the EARLIER groups of this item continue with token v in this step (rows that continue at -inf do not
 *   count).  For the first group, and with diversity_penalty == 0, the score is logp + beam_scores bit for bit.
 * select: per group the 2 * gs best of its gs * V candidates, score descending, then flat index (j - g * gs) * V + v ascending.
 * walk: per group as mxl_beam_step's with n = gs: an eos at rank < gs joins the store (a free slot of the nb, else it replaces the
 *   worst entry if it beats it), an eos behind is skipped, the first gs others continue inside the group; done |= (the store holds
 *   nb) && (early_stopping || worst stored score >= this group's rank-0 score / cur_len ** length_penalty).  The groups behind the
 *   one that made the item done are not walked in that step: identity, pad_id, scores untouched.
 * 2 <= nb <= 16, 2 <= ng <= nb, nb % ng == 0 (gs = 1 is legal), 0 <= diversity_penalty < inf; else MXL_EINVAL.  The K/V rings follow
 * with mxl_beam_reorder as after mxl_beam_step. */
int mxl_group_beam_step(const float* logp, int ldl, float* beam_scores, void* ids, int ld_ids, const int* t_dev, int Bs, int nb,
                        int ng, float diversity_penalty, int V, int eos_id, int pad_id, float length_penalty, int early_stopping,
                        void* hyp_ids, int* hyp_len, float* hyp_score, int* hyp_n, int* done, int* n_done, int* beam_idx, int* moved,
                        int* words, int n_words, int word_stride, void* stream);
/* ------------------------------------------------------------------------------------------------------------
 * Beam-sample on the device (HF 4.25.1 beam_sample, the reference's default 'beam' strategy): per step mxl_rules_mask, then
 * mxl_beam_sample_draw, then mxl_beam_sample_step, then what follows mxl_beam_step.  An item is the nb rows of one prompt as above.
 *
 * mxl_beam_sample_draw.  logp (rows = Bs * nb, ldl) f32, ldl >= V, already masked by the rules.  Per row r, unless dead:
 *   warp: score[v] = fp32(logp[r][v] * fp32(1 / temperature)), ordered by score descending, ties by v ascending; HF's warpers in HF's
 *     order with min_tokens_to_keep = 2: top_k > 0 keeps the first max(top_k, 2) of the order; 0 < top_p < 1 keeps an entry iff the
 *     probability ordered before it is below top_p, and the two best in any case; 0 < typical_p < 1 orders what is left by
 *     |-log p - H| ascending (ties by the first order) and keeps an entry iff the probability ordered before it is below typical_p,
 *     and the first two of that order in any case; values >= 1 (top_k: 0) switch a warper off.  Then LogitNormalization:
 *     w[r][v] = the log-probability renormalised over what is left, -inf outside it; logsumexp_v w[r][v] = 0.  The running score
 *     plays no part: renormalised per row it drops out of the draw, and the step below takes w itself as the new running score.
 *   dead row: beam_scores[r] == -inf (f32 (rows,), read only).  It contributes no candidate: w[r][.] = -inf.  So does a live row
 *     whose logp is -inf throughout.  No NaN is written anywhere.
 * Per item: 2 * nb of its nb * V candidates are drawn without replacement with probabilities softmax of the flattened w, as the
 *   2 * nb largest of z = w - log(-log u) (Gumbel-top-k), ties by flat index j * V + v ascending (j = r % nb).  For candidate
 *   (global row r, token v), with hash = mxl_hash32 (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16),
 *   all sums and products modulo 2^32, ctr = *rng_ctr (64 bits) and seed (64 bits):
 *       h1   = hash(hi32(ctr * 0x9E3779B97F4A7C15) ^ hash(r + 0x85ebca6b * lo32(seed)))
 *       h2   = hash(h1 + lo32(ctr) + hi32(seed))                      (the sampler's word of row r)
 *       word = hash(h2 ^ (v * 0x9E3779B1 + 0x85EBCA77))
 *       j24  = word >> 8,   u = (j24 + 0.5) / 2^24                   (never 0 or 1)
 *   The Gumbel term -log(-log u) lies in [-2.85, 17.33]: a candidate more than about 20 nats under its item's best is never drawn.
 *   Candidates with w = -inf have z = -inf and are not drawn; an item with fewer than 2 * nb finite candidates draws them all, and
 *   mxl_beam_sample_step fills its ranks with -inf candidates in flat-index order, as mxl_beam_step's select treats -inf.
 * drawn (rows, ldl) f32, output, not logp: columns 0..V-1 hold w[r][v] bit for bit at the item's drawn candidates and -inf
 *   everywhere else; columns V.. are not touched.  out_warped (rows, V) f32, optional (NULL), a test hook: every row's whole w.
 * *rng_ctr is read on the device and not advanced (mxl_decode_advance does that), so the step replays in a graph; the same
 *   arguments give the same bytes.  2 <= V <= 2048, 2 <= nb <= 16, temperature > 0 and finite, top_k >= 0, top_p > 0,
 *   typical_p > 0; anything else is MXL_EINVAL.  Two launches (one workgroup per row, then one per item), no workspace. */
int mxl_beam_sample_draw(const float* logp, int ldl, int V, const float* beam_scores, int Bs, int nb,
                         const unsigned long long* rng_ctr, unsigned long long seed, int top_k, float top_p, float temperature,
                         float typical_p, float* drawn, float* out_warped, void* stream);
/* mxl_beam_step over the matrix `drawn` of mxl_beam_sample_draw, with one difference: the score of candidate (j, v) is drawn[j][v]
 * itself -- -inf when beam_scores[j] is -inf -- and not a sum with the running score; no arithmetic is done on it, so the new
 * beam_scores are entries of `drawn` bit for bit.  Select (the 2 * nb best, score descending then flat index ascending, -inf
 * taking part), walk, store, reorder, dead rows, frozen items, words and the argument domain are mxl_beam_step's. */
int mxl_beam_sample_step(const float* drawn, int ldl, float* beam_scores, void* ids, int ld_ids, const int* t_dev, int Bs, int nb,
                         int V, int eos_id, int pad_id, float length_penalty, int early_stopping, void* hyp_ids, int* hyp_len,
                         float* hyp_score, int* hyp_n, int* done, int* n_done, int* beam_idx, int* moved, int* words, int n_words,
                         int word_stride, void* stream);
/* Contiguous (rows, row_bytes) buffers follow beam_idx in place, item by item (the K/V rings of a decoder: HF _reorder_cache without
 * the second buffer).  buf: one buffer (n_bufs = 1), or table: a device array of n_bufs buffer addresses, one launch for all of them;
 * exactly one of the two is given.  A thread owns one 16-byte column of an item, reads the sources of the rows that change into
 * registers, then writes them: a swap or a cycle needs no copy.  A workgroup whose item has moved[b] == 0 returns before touching
 * memory, rows with beam_idx[r] == r are not written, an index outside the row's item counts as r.  row_bytes % 16 == 0, buffers
 * 16-byte aligned, nb <= 16, Bs and n_bufs <= 65535; else MXL_EINVAL. */
int mxl_beam_reorder(void* buf, const void* table, int n_bufs, int Bs, int nb, long long row_bytes, const int* beam_idx,
                     const int* moved, void* stream);
/* Indexed rings: the alternative to mxl_beam_reorder over the K/V rings.  A ring slot written for position p never changes, so a
 * beam may point at the slot in its ancestor's ring instead of owning a copy.  owner: (Bs * nb, M) uint8 on the device;
 * owner[r][s] = j, 0 <= j < nb, says that slot s of row r's history is held in the ring of row (r / nb) * nb + j; the identity
 * owner[r][:] = r % nb after the prompt pass.  Launched where mxl_beam_reorder is, after the select and before mxl_decode_advance:
 *   follow  an item with moved[b] != 0: owner[j][:] <- owner_old[beam_idx[j] - row0][:] for its nb rows, in place (a thread owns 16
 *           slots, reads the sources of the rows that change into registers, then writes them; an index outside the item counts as j)
 *   mark    every item, moved or not, dead and done rows too: owner[j][(*t_dev + 1) % M] = j -- the slot the coming forward pass
 *           writes into row j's own ring.  On a wrap every row overwrites the slot in the same step and the position it held is
 *           outside every window, so no other fix-up is needed.
 * owner, beam_idx, moved, t_dev non-null, owner 16-byte aligned, 1 <= nb <= 16, M % 16 == 0, 1 <= Bs <= 65535; else MXL_EINVAL. */
int mxl_beam_owner_follow(void* owner, int Bs, int nb, int M, const int* beam_idx, const int* moved, const int* t_dev,
                          void* stream);
/* Contrastive search (the reference's 'contrastive' strategy, musicnlp/trainer/eval.py:296-302, over the mems patch of
 * musicnlp/models/transformer_xl.py:229-234; HF 4.25.1 GenerationMixin.contrastive_search with `_ranking_fast`):
 *   score[b*K + k] = (1 - alpha) * probs[b*K + k] - alpha * max_{s < S} cos(hid[b*K + k], ctx[b][s]);  sel[b] = argmax_k score
 * ctx (B, ., d) bf16 = last-layer hidden states of the S context positions (batch stride ctx_bs elements), ctx_inv_norm (B, .) f32
 * their reciprocal norms (mxl_row_inv_norm_bf16; batch stride inv_bs), hid (B*K, d) bf16 the candidates' hidden states,
 * probs (B*K) f32 their top-k probabilities; sel int64 (B). */
int mxl_row_inv_norm_bf16(const void* x, long long ld, int n, int d, float* out, void* stream);
int mxl_contrastive_select(const void* ctx, long long ctx_bs, const float* ctx_inv_norm, int inv_bs, int S, const void* hid,
                           const float* probs, float alpha, int B, int K, int d, float* score, void* sel, void* stream);
/* Contrastive search with the step on the device (csrc/contrastive.hip; the invariant that makes it cheap is stated there).  A
 * sequence is the K decoder rows b*K .. b*K + K-1 of one prompt, 2 <= K <= 32, rows = B * K; every position is read from *t_dev.
 *
 * mxl_contrastive_topk, before mxl_decode_advance (the rows hold columns 0..*t_dev): one workgroup per sequence reads the
 *   log-probabilities of its picked row, logp[b*K + sel[b]] (logp (rows, ldl) f32, ldl >= V, already masked by the rules; sel (B) int32,
 *   0 before the first step), takes the K best tokens in (value descending, token id ascending) order -- exact for any V -- and the
 *   softmax over those K values (TopKLogitsWarper, then softmax): token k -> ids[b*K + k][*t_dev + 1], probs[b*K + k].  A candidate at
 *   -inf is dead: probs 0, dead[b*K + k] = 1 (else 0), and it carries candidate 0's token.  unfinished (rows) int32 or NULL: a sequence
 *   with unfinished[b*K] == 0 gets pad_id in all K rows.
 * mxl_contrastive_step, after the model has run the candidates (*t_dev = their column): score[b*K + k] = the formula of
 *   mxl_contrastive_select over the S = *t_dev context positions of ctx / ctx_inv_norm, same arithmetic and summation order (scores
 *   are bit-identical), -inf for a dead candidate; sel[b] = the first maximum; the picked row's token, or pad_id for a sequence with
 *   unfinished[b*K] == 0, goes to column *t_dev of all K rows; a picked eos_id of a live sequence adds 1 to *n_done (optional) and
 *   clears unfinished of its K rows -- unless stop_later != 0: then mxl_rules_advance with the stop group follows and clears it
 *   itself, after moving the words.  hid[b*K + sel[b]] -> ctx[b][*t_dev], its reciprocal norm (mxl_row_inv_norm_bf16's bits) ->
 *   ctx_inv_norm[b][*t_dev].  ctx (B, Smax, d) bf16 with batch stride ctx_bs >= Smax * d, ctx_inv_norm batch stride inv_bs >= Smax;
 *   nothing is written when *t_dev >= Smax or >= ld_ids.  unfinished == NULL: no stop rule.  Two launches.
 * mxl_ring_slot_broadcast: table = device array of n_bufs addresses of (rows, H, M, dh) bf16 rings (the K and V rings of every
 *   layer); slot *t_dev mod M of row b*K + sel[b] is copied into the other K - 1 rows of the sequence, for every ring, head and
 *   sequence, in one launch.  No other slot is touched.  dh % 8 == 0, B and n_bufs <= 65535. */
int mxl_contrastive_topk(const float* logp, int ldl, int V, int B, int K, const int* sel, void* ids, int ld_ids, const int* t_dev,
                         float* probs, int* dead, const int* unfinished, int pad_id, void* stream);
int mxl_contrastive_step(void* ctx, long long ctx_bs, float* ctx_inv_norm, int inv_bs, int Smax, const int* t_dev, const void* hid,
                         const float* probs, const int* dead, float alpha, int B, int K, int d, float* score, int* sel, void* ids,
                         int ld_ids, int* unfinished, int* n_done, int eos_id, int pad_id, int stop_later, void* stream);
int mxl_ring_slot_broadcast(const void* table, int n_bufs, int B, int K, int H, int M, int dh, const int* t_dev, const int* sel,
                            void* stream);
/* Shared rings under contrastive search (csrc/decode_shared.hip): the K rows of a prompt differ in the one ring slot the step wrote,
 * so the B0 prompts keep one ring each, (B0, H, M, dh) bf16 per layer, and three capture-safe launches (no host read, no allocation)
 * take the places of mxl_kv_append, mxl_relattn_decode_split_live and mxl_ring_slot_broadcast.  rows = B0 * K, 2 <= K <= 32.
 *
 * mxl_kv_stash: qr_out (B, d) bf16 = q + r_r_bias bit for bit as mxl_kv_append writes it (or NULL), and the k / v thirds of the
 *   (B, 3d) qkv rows -> stash (B, 2d) bf16, k then v, the layer's slice of a (layers, rows, 2d) buffer that lives until the pick.  No
 *   ring is touched.  d % 8 == 0, 16-byte aligned buffers.
 * mxl_relattn_decode_shared: the ring attention of one step for the K queries of every prompt over the prompt's ring.  For the query
 *   of row b*K + k a slot s != *t_dev mod M is read from ring b, and slot *t_dev mod M (K and V) from the row's own qkv row -- the k / v
 *   that mxl_kv_append would have written there; the ring's slot *t_dev mod M is never read.  qkv (rows, 3d), bd (rows, H, M), out
 *   (rows, H*dh), unfinished (rows) or NULL as in mxl_relattn_decode_split_live; a sequence with unfinished[b*K] == 0 reads no ring
 *   byte and leaves zeros in its K rows.  Never-written slots take the positional term alone.  Same arithmetic per query in the same
 *   order, the same pieces and merge: the output of row b*K + k equals what mxl_relattn_decode_split_live writes at the same `pieces`
 *   on K copies of ring b whose slot *t_dev mod M holds candidate k's k / v.  A workgroup holds G = 8 queries (G = 4 for K <= 4) and a
 *   K or V fragment it fetches serves all of them, so a ring is read ceil(K / G) times per launch.  pieces 1..8 with ws
 *   (mxl_relattn_decode_split_ws_bytes(rows, ...)) and arrived (rows * H ints, zero before the first call) for pieces > 1.
 *   Shared memory: mxl_relattn_decode_shared_lds_bytes = G * (cap * 4 + 20 * dh) bytes with cap = M for one piece, else
 *   min(M, ceil(M / pieces) + 34), rounded up to a multiple of 4; it must not exceed 160 KiB.  K outside 2..32, pieces outside 1..8,
 *   too much shared memory, B0 * ceil(K / G) > 65535 or a buffer that is not 16-byte aligned: MXL_EINVAL; dh other than 16 / 32 / 64:
 *   MXL_EUNSUPPORTED; nothing is launched on either.  mxl_relattn_decode_shared_lds_bytes returns 0 for arguments outside the domain.
 * mxl_kv_commit_shared, after mxl_contrastive_step and the rules advance: table = device array of 2 * n_layers addresses of (B0, H, M,
 *   dh) bf16 rings, the K rings of the layers, then their V rings; stash (n_layers, rows, 2d) as mxl_kv_stash left it.  The stash of
 *   row b*K + sel[b] goes into slot *t_dev mod M of ring b, for every layer, head and prompt, in one launch; *t_dev is read on the
 *   device and no other slot is touched.  dh % 8 == 0, B0 and 2 * n_layers <= 65535. */
size_t mxl_relattn_decode_shared_lds_bytes(int K, int dh, int M, int pieces);
int mxl_kv_stash(const void* qkv, void* stash, int B, int d, const float* r_r_bias, void* qr_out, void* stream);
int mxl_relattn_decode_shared(const void* qkv, const void* kcache, const void* vcache, const float* bd, const float* r_w_bias, void* out,
                              const int* t_dev, int B0, int K, int H, int dh, int M, float scale, int pieces, float* ws, int* arrived,
                              const int* unfinished, void* stream);
int mxl_kv_commit_shared(const void* table, int n_layers, const void* stash, int B0, int K, int H, int M, int dh, const int* t_dev,
                         const int* sel, void* stream);
/* One prompt ring shared by the n sampled variations of a prompt (csrc/decode_prefix.hip): the n rows of a prompt hold the same prompt,
 * so per layer the B0 prompts keep one pair of prompt rings, (B0, H, M, dh) bf16, written once by the prompt pass (mxl_kv_fill: slot =
 * position mod M) and never again, and every row a pair of tail rings, (rows, H, Mt, dh) bf16, rows = B0 * n, for the positions generated
 * after the prompt: position p >= Tp of a row lives in tail slot (p - Tp) mod Mt.  Tp is read from the device (t0_dev, one int), so a
 * captured step does not bake the prompt length in.  Mt a multiple of 16 in 16..M, and at least min(M, generated positions), so that no
 * tail slot a window still holds is overwritten.  Both entries are capture-safe: no host read, no allocation.
 *
 * mxl_kv_append_tail, where mxl_kv_append sat: qr_out (B, d) bf16 = q + r_r_bias bit for bit as mxl_kv_append writes it (or NULL), and
 *   the k / v thirds of row b of the (B, 3d) qkv rows -> slot (*t_dev - *t0_dev) mod Mt of row b's tail rings, no other byte; *t_dev <
 *   *t0_dev writes no ring.  d % 8 == 0, dh % 8 == 0, d % dh == 0, Mt % 16 == 0 and >= 16, 16-byte aligned buffers; else MXL_EINVAL.
 * mxl_relattn_decode_prefix: the ring attention of one step for the n queries of every prompt.  With t = *t_dev and Tp = *t0_dev, ring
 *   slot s (0..M-1, in the slot order and lane assignment of mxl_relattn_decode) stands for position p = t - ((t - s) mod M), the latest
 *   one <= t that maps to s: p < 0 was never written and takes the positional term alone (no K / V read); p >= Tp reads K and V from slot
 *   (p - Tp) mod Mt of the row's own tail rings; any other p reads slot s of the prompt's rings.  qkv (rows, 3d), bd (rows, H, M), out
 *   (rows, H*dh) as in mxl_relattn_decode_split_live.  unfinished (rows) or NULL is per row: a row with unfinished == 0 reads no tail
 *   byte and leaves zeros in its output, a group without a live row reads no ring byte.  Same arithmetic per query in the same order,
 *   the same pieces and merge: the output of row b*n + k equals what mxl_relattn_decode_split_live writes at the same `pieces` on the
 *   ring that row would own had every position been appended to it.  A workgroup holds G = 8 queries of one prompt (G = 4 for n <= 4;
 *   the last group of a prompt may be partial); a prompt-ring fragment it fetches serves all of them, tail fragments are fetched per
 *   query.  pieces 1..8 with ws (mxl_relattn_decode_split_ws_bytes(rows, ...)) and arrived (rows * H ints, zero before the first call)
 *   for pieces > 1.  Shared memory: mxl_relattn_decode_prefix_lds_bytes = G * (cap * 4 + 16 * dh) bytes, cap as for
 *   mxl_relattn_decode_shared -- within that entry's G * (cap * 4 + 20 * dh); it must not exceed 160 KiB (any M up to 4096 fits).
 *   M or Mt not a multiple of 16, Mt outside 16..M, n < 2, pieces outside 1..8, too much shared memory, B0 * ceil(n / G) > 65535 or a
 *   buffer that is not 16-byte aligned: MXL_EINVAL; dh other than 16 / 32 / 64: MXL_EUNSUPPORTED; nothing is launched on either.
 *   mxl_relattn_decode_prefix_lds_bytes returns 0 for arguments outside the domain. */
size_t mxl_relattn_decode_prefix_lds_bytes(int n, int dh, int M, int pieces);
int mxl_kv_append_tail(const void* qkv, void* ktail, void* vtail, const int* t_dev, const int* t0_dev, int B, int Mt, int d, int dh,
                       const float* r_r_bias, void* qr_out, void* stream);
int mxl_relattn_decode_prefix(const void* qkv, const void* kprompt, const void* vprompt, const void* ktail, const void* vtail,
                              const float* bd, const float* r_w_bias, void* out, const int* t_dev, const int* t0_dev, int B0, int n, int H,
                              int dh, int M, int Mt, float scale, int pieces, float* ws, int* arrived, const int* unfinished, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Reformer path (A6-A8): replaces HuggingFace modeling_reformer.py as reached through
 * musicnlp/models/reformer.py:114-127 (AxialPositionEmbeddings, LSHSelfAttention._hash_vectors / _stable_argsort /
 * _attend / ReverseSort / hash-round merge, LocalSelfAttention).  Chunk length 64, one chunk look-back, causal decoder.
 * ---------------------------------------------------------------------------------------------------------- */
/* out[b,t] = drop(E[ids]) + cat(W0[t / A1], W1[t % A1]) with HF's 2-D position dropout; E (V,d) bf16, W0 (A0,d0) f32, W1 (A1,d-d0) f32 */
int mxl_axial_embed_fwd(const void* ids, const void* E, const float* W0, const float* W1, void* out, int B, int T, int d,
                        int V, int A0, int A1, int d0, float drop_p, unsigned long long seed, unsigned site_emb,
                        unsigned site_pos, void* stream);
int mxl_axial_embed_bwd(const void* ids, const void* dout, const void* dout2, float* dE, float* dW0, float* dW1, int B, int T,
                        int d, int V, int A0, int A1, int d0, float drop_p, unsigned long long seed, unsigned site_emb,
                        unsigned site_pos, void* stream);
/* buckets[b,h,r*T+t] = r*NB + combined argmax([xR;-xR]) per factor; qk (B,T,H,dh) bf16 strided (bs, rs);
 * rotations (H, dh, n_h, sum(factors)/2) f32 supplied by the caller; factors_host: nfac ints on the host */
int mxl_lsh_hash(const void* qk, long long bs, int rs, const float* rotations, int* buckets, int B, int T, int H, int dh,
                 int n_h, int nfac, const int* factors_host, void* stream);
/* stable sort of the S = n_h*T slots of each of the BH rows by bucket: sorted_idx (slot -> element), sorted_pos = idx % T */
int mxl_lsh_sort(const int* buckets, int* sorted_idx, int* sorted_pos, int BH, int S, int T, int n_buckets_total, void* stream);
/* chunked attention: local (lsh=0, sorted_pos NULL, n_h=1; separate q/k/v) or LSH (lsh=1; k == q == shared qk).
 * out rows (b, round, pos) x (H*dh) bf16; lse (B, n_h, H, T) f32; probs dropout drop_p.
 * T > 64: T % 64 == 0 (chunks of 64 with one look-back chunk).  T <= 64: the single-chunk case -- HF's plain causal attention
 * over the T tokens (no look-back, sorted_pos ignored, n_h must be 1; for lsh the shared-QK key normalisation and the
 * self mask still apply). */
int mxl_chunk_attn_fwd(const void* q, const void* k, const void* v, const int* sorted_pos, void* out, float* lse, int B, int T,
                       int H, int dh, int n_h, int lsh, long long bs, int rs, float drop_p, unsigned long long seed,
                       unsigned site, void* stream);
/* backward: dq, dk, dv (B, n_h, T, H*dh) f32 -- one (T, H*dh) slab per hash round; every element is written exactly once (plain
 * stores, no pre-zeroing) and the rounds are summed by the consumer (mxl_lsh_keynorm_bwd_rounds).  (Until round 6 the rounds of
 * n_h > 1 met in one (B, T, H*dh) buffer through a float atomic per element: 2.9 ms per call at the reference's logged
 * Reformer-base shape against 0.45 ms now.)  n_h == 1: each of the three may instead go out as bf16 through dq16 / dk16 / dv16 (rows
 * of ld16 elements; NULL = use the f32 destination) -- e.g. straight into the (N, 3d) operand of the projection-gradient GEMMs.
 * For lsh, dk is w.r.t. the normalised key (see keynorm_bwd); dout has out's layout; dlse (B,n_h,H,T) f32 or NULL */
int mxl_chunk_attn_bwd(const void* q, const void* k, const void* v, const int* sorted_pos, const void* out, const float* lse,
                       const void* dout, const float* dlse, float* dq, float* dk, float* dv, void* dq16, void* dk16, void* dv16,
                       int ld16, int B, int T, int H, int dh, int n_h, int lsh, long long bs, int rs, float drop_p,
                       unsigned long long seed, unsigned site, void* stream);
/* dqk (B*T rows of ld_dqk elements, H*dh used) bf16 = dq + chain rule of k = qk * rsqrt(mean(qk^2)+1e-6)/sqrt(dh) applied to
 * dk_eff */
int mxl_lsh_keynorm_bwd(const void* qk, long long bs, int rs, const float* dq, const float* dk_eff, void* dqk, int ld_dqk, int B,
                        int T, int H, int dh, void* stream);
/* the same over per-round slabs: dq, dk_eff (and dv) (B, n_h, T, H*dh) f32 are summed over the rounds, in round order, on the way
 * in; dv's sum (the rounds' value gradients) leaves as bf16 rows of ld_dv elements through dv16 (both NULL: no dv) */
int mxl_lsh_keynorm_bwd_rounds(const void* qk, long long bs, int rs, const float* dq, const float* dk_eff, const float* dv, void* dqk,
                               int ld_dqk, void* dv16, int ld_dv, int B, int T, int H, int dh, int n_h, void* stream);
/* hash-round merge: out = sum_r softmax_r(lse) * out_r, and its backward (dout_r, dlse) */
int mxl_lsh_combine(const void* out_r, const float* lse, void* out, int B, int T, int H, int dh, int n_h, void* stream);
int mxl_lsh_combine_bwd(const void* out_r, const float* lse, const void* out, const void* dout, void* dout_r, float* dlse,
                        int B, int T, int H, int dh, int n_h, void* stream);

/* ---- Reformer incremental (cached) decoding: the single-token step of HF's `use_cache` path, i.e. what
 * `model.generate(...)` at musicnlp/trainer/eval.py:333 runs (ReformerDynamicCache HF515:65-148; LSHSelfAttention.forward with
 * past_buckets_states HF515:466-516, 946-1050; LocalSelfAttention HF515:1136-1169, 1327-1329).  The caches hold, per layer,
 * the PROJECTIONS of every position so far ((B, Tmax, H*dh) bf16: k and v for local layers, shared qk and v for LSH layers --
 * HF caches the LayerNorm'ed hidden states and re-projects what it gathers: the same numbers) and, per LSH layer, the offset
 * bucket ids (B*H, n_h, Tmax) int32. */
/* x[b] = E[ids[b, t]] + cat(W0[t / A1], W1[t % A1]): ReformerEmbeddings in eval with start_idx_pos_encodings = t */
int mxl_rf_decode_embed(const void* ids, int ld_ids, int t, const void* E, const float* W0, const float* W1, void* out, int B,
                        int d, int V, int A1, int d0, void* stream);
/* buckets (rows, n_h*T) as written by mxl_lsh_hash (r*NB + b) -> r*(NB+1) + (t < T_real ? b : NB): the padded prefill of HF's
 * eval mode sends pad positions to ONE extra bucket and widens the per-round offsets (HF515:746-756) */
int mxl_lsh_fix_buckets(int* buckets, int rows, int n_h, int T, int T_real, int NB, void* stream);
/* append the new token's bucket ids: raw (rows, n_h) = r*NB + b from mxl_lsh_hash on the one query; cache (rows, n_h, Tmax);
 * *bkmax = maximum id in the cache.  Offsets widen to NB + 1 when *bkmax > n_h*NB - 1 (HF515:961-970); *bkmax is updated. */
int mxl_rf_query_bucket(const int* raw, int* cache, int* bkmax, int rows, int n_h, int NB, int Tmax, int t, void* stream);
/* one query per (sequence, head, round) at position t over <= 128 cached positions.  sorted == NULL: the contiguous range
 * [start, start + count) -- a local layer (lsh = 0: keys / sqrt(dh), no mask) or an LSH layer before its first hashing (lsh = 1:
 * shared-QK key normalisation, self mask -1e5 on position t).  sorted (B*H*n_h, n = t + 1) = mxl_lsh_sort of (cached ; new)
 * bucket ids per round: the 64-slot chunk holding the new token and the chunk before it, slots modulo n (HF515:1032-1050);
 * rounds merged by softmax of their logsumexp (HF515:636-655).  out (B, H*dh) bf16. */
int mxl_rf_decode_attn(const void* q, int ldq, const void* kcache, const void* vcache, const int* sorted, void* out, int B, int H,
                       int dh, int n_h, int Tmax, int n, int t, int start, int count, int lsh, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Evaluation metrics: replaces `preprocess_logits_for_metrics` + ComputeMetrics / IkrMetric on gathered
 * logits (musicnlp/trainer/train.py:265-284, musicnlp/trainer/metrics.py:45-117).
 * ---------------------------------------------------------------------------------------------------------- */
/* ids[n] = argmax_v logits[n][v] (first maximum); logits (N, ld) f32, ids int64 */
int mxl_argmax_rows(const float* logits, int ld, void* ids_out, int N, int V, void* stream);
/* out14[b] = { pitch-class histogram[12] of predicted pitch tokens at non-ignored positions, #correct next tokens, #non-ignored
 * next-token positions }.  preds int64 (B, T-1 if clm_pred_shifted else T), labels int64 (B, T), id2pc int8[V]: pitch class
 * 0..11 of a pitch token id, -1 for every other id (rests and the rare-pitch token included). */
int mxl_eval_counts(const void* preds, int ld_preds, const void* labels, int ld_labels, const signed char* id2pc, int V,
                    int* out14, int B, int T, int clm_pred_shifted, void* stream);

/* the same over a SUB-WORD vocabulary (musicnlp/trainer/wordpiece_tokenizer.py:349-452, pair_merge_tokenizer.py:200-289), whose ids
 * stand for several base tokens: id2hist uint8 (V, 12) = number of pitches of each class an id expands to (the reference's
 * per-id `_id2pchs_exc` lists, wordpiece_tokenizer.py:372-379, reduced to pitch classes) */
int mxl_eval_counts_multi(const void* preds, int ld_preds, const void* labels, int ld_labels, const unsigned char* id2hist, int V,
                          int* out14, int B, int T, int clm_pred_shifted, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Input pipeline: the pad / truncate / label contract of `tokenizer(toks, padding='max_length',
 * truncation=True)` (musicnlp/preprocess/dataset.py:361) + DataCollatorForLanguageModeling(mlm=False) (train.py:360),
 * applied on the device to one packed run of pre-tokenised ids.
 *   tokens  : elem_bytes = 2 (uint16) or 4 (int32) token ids, the B sequences back to back
 *   offsets : int32[B+1] element offsets into `tokens` (sequence b = [offsets[b], offsets[b+1]); may be empty or longer
 *             than max_length: truncated)
 *   ids_out, labels_out : (B, max_length) int64; labels may be NULL.  labels = ids with every pad_id -> -100.
 *   remap (n_tables, v_src) int32 + row_table int32[B] (or both NULL): token v of row b becomes remap[row_table[b]][v]
 *             (row_table[b] < 0: unchanged) -- the reference's step -> degree PitchShift (musicnlp/preprocess/transform.py:
 *             154-237) is one such table per key.
 * ---------------------------------------------------------------------------------------------------------- */
int mxl_pack_clm_batch(const void* tokens, int elem_bytes, const int* offsets, void* ids_out, void* labels_out, int B,
                       int max_length, long long pad_id, const int* remap, const int* row_table, int v_src, void* stream);

/* Post-decode / prompt id ops: out[b] = position of the last (which < 0) or which-th (0-based) occurrence
 * of `token` in row b of ids (B, T) int64, -1 if absent.  With token = the start-of-bar id this is the cut point of
 * MusicGenerator._truncate_last_bar (musicnlp/trainer/eval.py:178-185, which = -1) and of truncate_first_n_bar
 * (eval.py:187-198, which = n_bar). */
int mxl_find_token(const void* ids, int ld_ids, int B, int T, long long token, int which, int* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Measurement hook (no reference counterpart).  While enabled, the launch functions of the attention path bracket
 * EACH of their kernels with a hipEvent pair on the launch stream, so that bench.py can report per-kernel durations measured
 * live inside its timed region.  Enqueue-time cost: two hipEventRecord per kernel; NOT capture-safe (leave it off while a
 * hipGraph is being captured).  Kernel ids: */
#define MXL_KT_RELATTN_FWD   0   /* relattn_fwd_kernel                                  */
#define MXL_KT_RELATTN_DELTA 1   /* relattn_bwd_delta_kernel                            */
#define MXL_KT_RELATTN_DQ    2   /* relattn_bwd_dq8_kernel / relattn_bwd_dq_kernel      */
#define MXL_KT_RELATTN_DKV   3   /* relattn_bwd_dkv_kernel                              */
#define MXL_KT_RELATTN_DRD   4   /* relattn_drd_kernel                                  */
#define MXL_KT_ROWBIAS       5   /* add_rowbias (the q + r_r_bias operand of the dRd contraction) */
#define MXL_KT_RELATTN_FUSED 6   /* relattn_bwd_fused_kernel (mxl_relattn_bwd_fused)    */
#define MXL_KT_RELATTN_DQFIN 7   /* relattn_dq_finish_kernel (mxl_relattn_bwd_fused)    */
#define MXL_KT_CHUNK_FWD     8   /* chunk_attn_fwd_kernel (mxl_chunk_attn_fwd, T > one chunk window)              */
#define MXL_KT_CHUNK_BWD_Q   9   /* chunk_attn_bwd_q_kernel (mxl_chunk_attn_bwd)                                   */
#define MXL_KT_CHUNK_BWD_KV  10  /* chunk_attn_bwd_kv_kernel (mxl_chunk_attn_bwd)                                  */
#define MXL_KT_COUNT         11
int mxl_ktime_enable(int on);
/* waits for every recorded event, adds each kernel's elapsed milliseconds into ms_sum[id] and its launch count into
 * launches[id] (HOST arrays of n >= MXL_KT_COUNT entries, overwritten), and forgets the recorded events */
int mxl_ktime_collect(float* ms_sum, int* launches, int n);

#ifdef __cplusplus
}
#endif
#endif /* MUSICXL_H */
