// Beam search on the device (HF 4.25.1 `beam_search` + `BeamSearchScorer.process`, as generate.beam_search / _BeamHyps state them on
// the host): one launch per decode step that selects, walks, stores and reorders, and one that makes the K/V rings follow their beams.
//
// An item is the nb decoder rows of one prompt, rows b * nb .. b * nb + nb - 1, in ng groups of gs = nb / ng.  Plain beam search is
// ng = 1; diverse (group) beam search, HF 4.25.1 `group_beam_search` with `HammingDiversityLogitsProcessor` as
// generate.group_beam_search states it on the host, is ng >= 2 with a penalty `pen`.  Both run beam_step_kernel, one workgroup per
// item, group after group:
//   score    (logp[j][v] - pen * cnt[v]) + beam_scores[j], each operation rounded on its own as the host rounds it; cnt[v] = the live
//            rows of the earlier groups that chose v in this step.  cnt = 0 or pen = 0 leaves logp + beam_scores bit for bit, which
//            is every score of plain beam search.
//   select   the 2 * gs best of the group's gs * V candidates, ordered by score descending, then by flat index (j - g0) * V + v
//            ascending.  2 * gs rounds of a workgroup arg-max over the keys that come strictly after the previous round's key: score
//            and index are packed into one 64-bit word whose unsigned order is that order, so a round is one max reduction, exact
//            for any V, with no marking and no sort.  -inf takes part like any number and sorts last.
//   walk     thread 0, over a handful of scalars in LDS, _BeamHyps.walk with n = gs over the item's store of capacity nb: an eos
//            among the first gs ranks joins the store (a free slot, else it replaces the worst entry if it beats it), an eos behind
//            them is skipped, the first gs other candidates continue; then the done test with this group's best score, both
//            early_stopping arms.  A done item is frozen: identity, pad tokens, nothing else moves.
//   copy     the added hypotheses ids[src][:cur_len] -> the store, by the whole workgroup, before anything in ids moves
//   reorder  ids rows in place: a thread owns columns, reads the nb sources of a column into registers, then writes them, so a swap
//            needs no second buffer; the chosen tokens go to column cur_len.  The packed per-row rule words follow the same way.
//   dead     a row that continues from a -inf candidate (a barred token, or the child of a dead row) gets pad and keeps -inf; its
//            `unfinished` word (word 0) is cleared, so the rules' advance launch -- with its stop group on -- leaves its words alone,
//            the mask launch keeps finding a valid state, and the ring attention skips it.  The rows of a done item are cleared too.
// Beam-sample (mxl_beam_sample_step) is a third entry of the same kernel: over the `drawn` matrix of beam_sample.hip, with a
// candidate's score its entry itself; select, walk, copy, reorder and dead rows are the ones above.
// The rings follow either whole (beam_reorder_kernel) or not at all: beam_owner_follow_kernel keeps a table of which row of its item
// holds each slot of a row's history, and the attention reads through it (decode_attn.hip, decode_fp8.hip).
#include "common.h"
#include "beam_key.h"
#include "musicxl_internal.h"

namespace {

constexpr int BEAM_MAX = 16;                 // beams per item: the register rows of the reorder
constexpr int BEAM_T = 256;

// What a step does once thread 0 has walked the candidates of an item (all of this in LDS, a barrier behind it): the added
// hypotheses sh_add[slot] = source beam (or -1) are copied out before ids moves, ids and the packed rule words follow sh_src in
// place when `mv`, the chosen tokens sh_tok go to column cur_len, and word 0 of the dead rows (or of every row when `clear`) is zeroed.
__device__ __forceinline__ void beam_store_and_reorder(long long* ids, int ld_ids, int row0, int nb, int cur_len, long long* hyp_ids,
                                                       const int* sh_add, const int* sh_src, const int* sh_tok, const int* sh_dead,
                                                       int mv, int clear, int* words, int n_words, int word_stride) {
    const int tid = threadIdx.x;
    // the added hypotheses, before ids moves
    for (int slot = 0; slot < nb; slot++) {
        const int src = sh_add[slot];
        if (src < 0) continue;
        const long long* from = ids + (size_t)(row0 + src) * ld_ids;
        long long* to = hyp_ids + (size_t)(row0 + slot) * ld_ids;
        for (int c = tid; c < cur_len; c += BEAM_T) to[c] = from[c];
    }
    __syncthreads();

    if (mv) {
        int src[BEAM_MAX];
#pragma unroll
        for (int j = 0; j < BEAM_MAX; j++) src[j] = j < nb ? sh_src[j] : j;
        for (int c = tid; c < cur_len; c += BEAM_T) {
            long long v[BEAM_MAX];
#pragma unroll
            for (int j = 0; j < BEAM_MAX; j++)
                if (j < nb && src[j] != j) v[j] = ids[(size_t)(row0 + src[j]) * ld_ids + c];
#pragma unroll
            for (int j = 0; j < BEAM_MAX; j++)
                if (j < nb && src[j] != j) ids[(size_t)(row0 + j) * ld_ids + c] = v[j];
        }
        if (words && tid < n_words) {
            int* w = words + (size_t)tid * word_stride + row0;
            int v[BEAM_MAX];
#pragma unroll
            for (int j = 0; j < BEAM_MAX; j++)
                if (j < nb && src[j] != j) v[j] = w[src[j]];
#pragma unroll
            for (int j = 0; j < BEAM_MAX; j++)
                if (j < nb && src[j] != j) w[j] = v[j];
        }
    }
    if (tid < nb) ids[(size_t)(row0 + tid) * ld_ids + cur_len] = sh_tok[tid];
    if (words && tid == 0) {                                         // word 0 = unfinished; thread 0 moved it above
        for (int j = 0; j < nb; j++)
            if (sh_dead[j] || clear) words[row0 + j] = 0;
    }
}

// One beam step of every item, for plain (ng = 1, pen = 0) and diverse beam search alike: the groups of an item are walked in order
// inside its workgroup, since a group's scores depend on the tokens the earlier groups chose in this step (sh_prev) and all groups
// share the item's store.  Once the item is done the groups behind are not walked: identity, pad, their scores stay.
// SAMPLE (beam-sample, ng = 1): logp is the `drawn` matrix of mxl_beam_sample_draw and a candidate's score is its entry itself -- -inf
// in a row whose running score is -inf -- with no arithmetic on it; everything else is the same step.
template <bool SAMPLE>
__global__ __launch_bounds__(BEAM_T) void beam_step_kernel(const float* logp, int ldl, float* beam_scores, long long* ids, int ld_ids,
                                                           const int* t_dev, int nb, int ng, float pen, int V, int eos_id, int pad_id,
                                                           float length_penalty, int early_stopping, long long* hyp_ids, int* hyp_len,
                                                           float* hyp_score, int* hyp_n, int* done, int* n_done, int* beam_idx,
                                                           int* moved, int* words, int n_words, int word_stride) {
    __shared__ unsigned long long sh_part[BEAM_T / 64];
    __shared__ unsigned long long sh_cand[2 * BEAM_MAX];
    __shared__ float sh_score[BEAM_MAX], hs[BEAM_MAX];               // hs: the scores of the item's store (thread 0)
    __shared__ int sh_src[BEAM_MAX], sh_tok[BEAM_MAX], sh_dead[BEAM_MAX], sh_add[BEAM_MAX], sh_prev[BEAM_MAX];
    __shared__ int sh_moved, sh_done, sh_n, sh_nprev;
    const int b = blockIdx.x, tid = threadIdx.x, row0 = b * nb, gs = nb / ng;
    const int cur_len = *t_dev + 1;                                  // columns 0..cur_len-1 hold the rows; the new token goes to cur_len
    if (cur_len < 1 || cur_len >= ld_ids) return;                    // (the host keeps max_length within the buffer)
    const bool frozen = done[b] != 0;

    if (tid < nb) {
        sh_score[tid] = beam_scores[row0 + tid];
        sh_src[tid] = tid; sh_tok[tid] = pad_id; sh_dead[tid] = 0; sh_add[tid] = -1;
        hs[tid] = tid < hyp_n[b] ? hyp_score[row0 + tid] : 0.f;
    }
    if (tid == 0) { sh_moved = 0; sh_done = frozen; sh_n = hyp_n[b]; sh_nprev = 0; }
    __syncthreads();

    for (int g = 0; g < ng; g++) {
        if (sh_done) break;                                          // (written before the barrier that ends the last group)
        const int g0 = g * gs, np = sh_nprev;
        unsigned long long prev = ~0ull;
        for (int round = 0; round < 2 * gs; round++) {
            unsigned long long best = 0;
            for (int v = tid; v < V; v += BEAM_T) {
                int c = 0;                                           // (np = 0, no earlier group chose a token: off = +0, logp stays)
                for (int i = 0; i < np; i++) c += sh_prev[i] == v;
                const float off = __fmul_rn(pen, (float)c);
                for (int j = 0; j < gs; j++) {
                    const float lp = logp[(size_t)(row0 + g0 + j) * ldl + v];
                    const float s = SAMPLE ? (sh_score[g0 + j] == -INFINITY ? -INFINITY : lp)
                                           : __fadd_rn(__fsub_rn(lp, off), sh_score[g0 + j]);
                    const unsigned long long k = beam_key(s, (uint32_t)j * (uint32_t)V + (uint32_t)v);
                    if (k < prev && k > best) best = k;
                }
            }
            best = block_max_u64<BEAM_T>(best, sh_part);
            if (tid == 0) sh_cand[round] = best;
            prev = best;
            __syncthreads();                                         // sh_part is rewritten by the next round
        }
        if (tid == 0) {
            int n = sh_n, cnt = 0, mv = sh_moved, npn = np;
            const float norm = powf((float)cur_len, length_penalty);
            for (int rank = 0; rank < 2 * gs && cnt < gs; rank++) {
                const float s = beam_key_score(sh_cand[rank]);
                const uint32_t idx = beam_key_index(sh_cand[rank]);
                const int j = (int)(idx / (uint32_t)V), v = (int)(idx - (uint32_t)j * (uint32_t)V);
                if (j >= gs) continue;                               // (no candidate was left for this round: not reached for V >= 2)
                if (v == eos_id) {
                    if (rank >= gs) continue;
                    const float sc = s / norm;                       // _BeamHyps.add, into the store all groups share
                    int slot = -1;
                    if (n < nb) slot = n++;
                    else {
                        int worst = 0;
                        for (int i = 1; i < nb; i++) if (hs[i] < hs[worst]) worst = i;
                        if (sc > hs[worst]) slot = worst;
                    }
                    if (slot >= 0) { hs[slot] = sc; sh_add[slot] = g0 + j; }
                } else {
                    const bool dead = s == -INFINITY;
                    const int r = g0 + cnt;
                    sh_src[r] = g0 + j;
                    sh_tok[r] = dead ? pad_id : v;
                    sh_dead[r] = dead;
                    sh_score[r] = s;                                 // (every old score of the group is in the keys by now)
                    mv |= j != cnt;
                    if (!dead) sh_prev[npn++] = v;                   // a dead row does not count in the Hamming term
                    cnt++;
                }
            }
            for (; cnt < gs; cnt++) {                                // (not reached: at most gs of 2 * gs candidates are eos)
                const int r = g0 + cnt;
                sh_src[r] = r; sh_tok[r] = pad_id; sh_dead[r] = 1; sh_score[r] = -INFINITY;
            }
            bool d = false;                                          // _BeamHyps.is_done
            if (n >= nb) {
                if (early_stopping) d = true;
                else {
                    float worst = hs[0];
                    for (int i = 1; i < nb; i++) worst = fminf(worst, hs[i]);
                    d = worst >= beam_key_score(sh_cand[0]) / norm;
                }
            }
            sh_n = n; sh_moved = mv; sh_nprev = npn; sh_done = d;
        }
        __syncthreads();
    }

    if (tid == 0) {
        if (!frozen) {
            for (int j = 0; j < nb; j++) {
                beam_scores[row0 + j] = sh_score[j];
                if (sh_add[j] >= 0) { hyp_score[row0 + j] = hs[j]; hyp_len[row0 + j] = cur_len; }
            }
            hyp_n[b] = sh_n;
            if (sh_done) {
                done[b] = 1;
                atomicAdd(n_done, 1);
            }
        }
        for (int j = 0; j < nb; j++) beam_idx[row0 + j] = row0 + sh_src[j];
        moved[b] = sh_moved;
    }
    __syncthreads();
    beam_store_and_reorder(ids, ld_ids, row0, nb, cur_len, hyp_ids, sh_add, sh_src, sh_tok, sh_dead, sh_moved, sh_done, words, n_words,
                           word_stride);
}

// One (rows, row_bytes) buffer, or each of a table of them, follows beam_idx in place, item by item.  grid (column blocks, items,
// buffers); a thread owns one 16-byte column of its item: it reads the sources of the rows that change into registers, then writes
// them.  An item with moved == 0 returns before touching memory; an index outside its item counts as "stays".
__global__ __launch_bounds__(BEAM_T) void beam_reorder_kernel(char* buf, char* const* table, long long row_bytes, int nb,
                                                              const int* beam_idx, const int* moved) {
    const int b = blockIdx.y, row0 = b * nb;
    if (moved[b] == 0) return;
    const long long c = (long long)blockIdx.x * BEAM_T + threadIdx.x;
    if (c >= (row_bytes >> 4)) return;
    char* base = (table ? table[blockIdx.z] : buf) + c * 16;
    int src[BEAM_MAX];
#pragma unroll
    for (int j = 0; j < BEAM_MAX; j++) {
        src[j] = j;
        if (j < nb) {
            const int s = beam_idx[row0 + j] - row0;
            if (s >= 0 && s < nb) src[j] = s;
        }
    }
    u32x4 v[BEAM_MAX];
#pragma unroll
    for (int j = 0; j < BEAM_MAX; j++)
        if (src[j] != j) v[j] = *reinterpret_cast<const u32x4*>(base + (long long)(row0 + src[j]) * row_bytes);
#pragma unroll
    for (int j = 0; j < BEAM_MAX; j++)
        if (src[j] != j) *reinterpret_cast<u32x4*>(base + (long long)(row0 + j) * row_bytes) = v[j];
}

// Indexed rings (mxl_beam_owner_follow): the rings stay where they are and the (rows, M) owner table follows the beams in their
// place.  owner[r][s] = j: slot s of row r's history is held in the ring of row (r / nb) * nb + j.  grid (column blocks, items); a
// thread owns 16 slots of its item, one 16-byte column: when the item moved it reads the source rows of the rows that change into
// registers, then writes them, as beam_reorder_kernel does.  Then -- moved or not, dead and done rows too -- the thread that owns slot
// (t + 1) mod M gives it to each row itself: the coming forward pass writes that slot into every row's own ring, so whatever owner a
// row inherited for it (a stale one from before the wrap included) is no longer true.
__global__ __launch_bounds__(BEAM_T) void beam_owner_follow_kernel(unsigned char* owner, int nb, int M, const int* beam_idx,
                                                                   const int* moved, const int* t_dev) {
    const int b = blockIdx.y, row0 = b * nb;
    const int c = blockIdx.x * BEAM_T + threadIdx.x;
    if (c >= (M >> 4)) return;
    unsigned char* base = owner + (size_t)row0 * M + c * 16;
    if (moved[b] != 0) {
        int src[BEAM_MAX];
#pragma unroll
        for (int j = 0; j < BEAM_MAX; j++) {
            src[j] = j;
            if (j < nb) {
                const int s = beam_idx[row0 + j] - row0;
                if (s >= 0 && s < nb) src[j] = s;
            }
        }
        u32x4 v[BEAM_MAX];
#pragma unroll
        for (int j = 0; j < BEAM_MAX; j++)
            if (src[j] != j) v[j] = *reinterpret_cast<const u32x4*>(base + (size_t)src[j] * M);
#pragma unroll
        for (int j = 0; j < BEAM_MAX; j++)
            if (src[j] != j) *reinterpret_cast<u32x4*>(base + (size_t)j * M) = v[j];
    }
    int slot = (*t_dev + 1) % M;
    if (slot < 0) slot += M;
    if ((slot >> 4) == c)
        for (int j = 0; j < nb; j++) base[(size_t)j * M + (slot & 15)] = (unsigned char)j;
}

}  // namespace

// the argument checks all entries share, and the launch; nb, ng and pen are in the entry's own domain by now
template <bool SAMPLE>
static int beam_step_launch(const float* logp, int ldl, float* beam_scores, void* ids, int ld_ids, const int* t_dev, int Bs, int nb,
                            int ng, float pen, int V, int eos_id, int pad_id, float length_penalty, int early_stopping, void* hyp_ids,
                            int* hyp_len, float* hyp_score, int* hyp_n, int* done, int* n_done, int* beam_idx, int* moved, int* words,
                            int n_words, int word_stride, void* stream) {
    MXL_CHECK_ARG(logp && beam_scores && ids && t_dev && beam_idx && moved);
    MXL_CHECK_ARG(hyp_ids && hyp_len && hyp_score && hyp_n && done && n_done);
    MXL_CHECK_ARG(Bs > 0 && nb <= BEAM_MAX && V >= 2 && ldl >= V && ld_ids >= 2);
    MXL_CHECK_ARG((long long)nb * V < (1LL << 31) && (long long)Bs * nb < (1LL << 31));
    MXL_CHECK_ARG((words == nullptr) == (n_words == 0));
    MXL_CHECK_ARG(!words || (n_words >= 1 && n_words <= BEAM_T && (long long)word_stride >= (long long)Bs * nb));
    hipLaunchKernelGGL(beam_step_kernel<SAMPLE>, dim3(Bs), dim3(BEAM_T), 0, (hipStream_t)stream, logp, ldl, beam_scores, (long long*)ids, ld_ids,
                       t_dev, nb, ng, pen, V, eos_id, pad_id, length_penalty, early_stopping, (long long*)hyp_ids, hyp_len, hyp_score,
                       hyp_n, done, n_done, beam_idx, moved, words, n_words, word_stride);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_beam_step(const float* logp, int ldl, float* beam_scores, void* ids, int ld_ids, const int* t_dev, int Bs, int nb,
                             int V, int eos_id, int pad_id, float length_penalty, int early_stopping, void* hyp_ids, int* hyp_len,
                             float* hyp_score, int* hyp_n, int* done, int* n_done, int* beam_idx, int* moved, int* words, int n_words,
                             int word_stride, void* stream) {
    MXL_CHECK_ARG(nb >= 1);
    return beam_step_launch<false>(logp, ldl, beam_scores, ids, ld_ids, t_dev, Bs, nb, 1, 0.f, V, eos_id, pad_id, length_penalty,
                            early_stopping, hyp_ids, hyp_len, hyp_score, hyp_n, done, n_done, beam_idx, moved, words, n_words,
                            word_stride, stream);
}

extern "C" int mxl_beam_sample_step(const float* drawn, int ldl, float* beam_scores, void* ids, int ld_ids, const int* t_dev, int Bs,
                                    int nb, int V, int eos_id, int pad_id, float length_penalty, int early_stopping, void* hyp_ids,
                                    int* hyp_len, float* hyp_score, int* hyp_n, int* done, int* n_done, int* beam_idx, int* moved,
                                    int* words, int n_words, int word_stride, void* stream) {
    MXL_CHECK_ARG(nb >= 1);
    return beam_step_launch<true>(drawn, ldl, beam_scores, ids, ld_ids, t_dev, Bs, nb, 1, 0.f, V, eos_id, pad_id, length_penalty,
                                  early_stopping, hyp_ids, hyp_len, hyp_score, hyp_n, done, n_done, beam_idx, moved, words, n_words,
                                  word_stride, stream);
}

extern "C" int mxl_group_beam_step(const float* logp, int ldl, float* beam_scores, void* ids, int ld_ids, const int* t_dev, int Bs,
                                   int nb, int ng, float diversity_penalty, int V, int eos_id, int pad_id, float length_penalty,
                                   int early_stopping, void* hyp_ids, int* hyp_len, float* hyp_score, int* hyp_n, int* done, int* n_done,
                                   int* beam_idx, int* moved, int* words, int n_words, int word_stride, void* stream) {
    MXL_CHECK_ARG(nb >= 2 && ng >= 2 && ng <= nb && nb % ng == 0);
    MXL_CHECK_ARG(diversity_penalty >= 0.f && diversity_penalty < INFINITY);
    return beam_step_launch<false>(logp, ldl, beam_scores, ids, ld_ids, t_dev, Bs, nb, ng, diversity_penalty, V, eos_id, pad_id, length_penalty,
                            early_stopping, hyp_ids, hyp_len, hyp_score, hyp_n, done, n_done, beam_idx, moved, words, n_words,
                            word_stride, stream);
}

extern "C" int mxl_beam_reorder(void* buf, const void* table, int n_bufs, int Bs, int nb, long long row_bytes, const int* beam_idx,
                                const int* moved, void* stream) {
    MXL_CHECK_ARG((buf == nullptr) != (table == nullptr) && beam_idx && moved);
    MXL_CHECK_ARG(n_bufs >= 1 && n_bufs <= 65535 && (table || n_bufs == 1));
    MXL_CHECK_ARG(Bs > 0 && Bs <= 65535 && nb >= 1 && nb <= BEAM_MAX);
    MXL_CHECK_ARG(row_bytes > 0 && (row_bytes % 16) == 0 && ((uintptr_t)buf % 16) == 0);
    const long long blocks = ((row_bytes >> 4) + BEAM_T - 1) / BEAM_T;
    MXL_CHECK_ARG(blocks < (1LL << 31));
    hipLaunchKernelGGL(beam_reorder_kernel, dim3((unsigned)blocks, Bs, n_bufs), dim3(BEAM_T), 0, (hipStream_t)stream, (char*)buf,
                       (char* const*)table, row_bytes, nb, beam_idx, moved);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}

extern "C" int mxl_beam_owner_follow(void* owner, int Bs, int nb, int M, const int* beam_idx, const int* moved, const int* t_dev,
                                     void* stream) {
    MXL_CHECK_ARG(owner && beam_idx && moved && t_dev && ((uintptr_t)owner % 16) == 0);
    MXL_CHECK_ARG(Bs > 0 && Bs <= 65535 && nb >= 1 && nb <= BEAM_MAX && M > 0 && (M % 16) == 0);
    const int blocks = ((M >> 4) + BEAM_T - 1) / BEAM_T;
    hipLaunchKernelGGL(beam_owner_follow_kernel, dim3(blocks, Bs), dim3(BEAM_T), 0, (hipStream_t)stream, (unsigned char*)owner, nb, M,
                       beam_idx, moved, t_dev);
    MXL_LAUNCH_CHECK();
    return MXL_OK;
}
