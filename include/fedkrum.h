/*
 * fedkrum.h — C ABI of Krum / Multi-Krum selection on MI355X (gfx950): every staged upload is scored by its squared
 * distance to its K - f - 2 nearest other uploads, the m best-scored uploads are kept whole and only those are
 * averaged (Blanchard et al., NeurIPS 2017: a distance-based server-side defence against poisoned uploads, beside
 * the norm clip of fedclip.h and the coordinate-wise trimmed mean of fedtrim.h).
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued: a refused
 * call says "nothing was launched").  The entry points of this header are bound by fedscale_amd/_native_krum.py;
 * the header has its own version (fk_abi_version); FA_, FCL_ and FT_ABI_VERSION are not touched by it.
 *
 * The arithmetic of a round that starts from model L (P fp32 columns) with K uploads x_k resident in staging, in
 * arrival order, f assumed bad uploads and m uploads kept: 0 <= f, 2f + 3 <= K <= FK_MAX_K, 1 <= m <= K - f.
 *
 *   d_k[p]   = x_k[p] - L[p]                                   fp32, one op
 *   G[i][j]  = sum_p double(d_i[p]) * double(d_j[p])           fp64; every product is exact (24 + 24 bits)
 *   v        = (G[i][i] + G[j][j]) - 2.0 * G[i][j]             fp64, in this order; j != i
 *   dist2    = isnan(v) ? +inf : (v > 0 ? v : +0.0)
 *   score[i] = +0.0, then + the K-f-2 smallest dist2[i][j] (j != i), added one by one in ascending order, fp64
 *   rank[i]  = #{ j : (score[j], j) < (score[i], i) }           lexicographic; ties go to the earlier arrival
 *   c[i]     = (isfinite(score[i]) && rank[i] < m) ? 1.0f : 0.0f
 *   n_sel    = #{ i : c[i] != 0 }
 *   chain[p] = +0.0f; for k in arrival order with c[k] != 0: chain[p] = chain[p] + c[k] * d_k[p]   (fcl_reduce)
 *   out[p]   = n_sel > 0 ? L[p] + chain[p] / float(n_sel) : L[p]
 *
 * How G is summed (fk_gram).  The columns are cut into nsplit contiguous ranges; part[s][i][j] is accumulated in fp64
 * on the matrix unit (v_mfma_f64_16x16x4_f64), in whatever order the instruction and the tile loop impose;
 * G[i][j] = part[0] + part[1] + ... in split order.  Only the lower triangle of row tiles is computed and both
 * halves of G are read from the same partials, so G is exactly symmetric.  The plan — row tile, columns per step,
 * nsplit, columns per split — is a function of (K, P) and compile-time constants only, never of the CU count: a
 * given (K, P) gives the same bits on every run and on every machine of this kind.
 *
 * So G is NOT defined bit for bit by a restatement.  It is exact whenever every partial sum is representable
 * (small-integer data); otherwise it is within the any-order summation bound
 *     P u / (1 - P u) * sum_p |d_i[p] d_j[p]|,   u = 2^-53,
 * which is derived, not measured: it holds for any order of P - 1 correctly rounded adds of exact products, fused
 * or not.  Everything after G (v, dist2, score, rank, c, n_sel, chain, out) is defined bit for bit given G.
 *
 * Consequences.  A row with an inf or NaN anywhere gets dist2 = +inf to every other row: its G[i][i] is +inf or
 * NaN, so v is NaN, +inf, or (inf - inf) NaN — every case leads there.  Its score is +inf and it is never kept.
 * It sits among the f + 1 largest entries that every other row's score leaves out, so up to f + 1 such rows do not
 * move an honest row's score.  If fewer than m rows have a finite score, only those are kept and the mean divides
 * by their number; if no row has a finite score, the model is left as it was (out = L).
 *
 * Zero padding: rows >= K of a tile are zeros inside the kernel; columns >= P are zeros in BOTH operands inside the
 * kernel, so garbage or NaN in [P, ld) never meets anything.
 *
 * Sizes: as fedclip.h — rows (x, last, chain) are read as float4 columns and hold >= round_up(P, 4) floats; out and
 * mirror are written in columns [0, P) only; row and vector pointers are 16-byte aligned, gram / score / workspace
 * 8-byte, c / n_sel 4-byte; ld is a multiple of 4 and >= P.
 */
#ifndef FEDKRUM_H
#define FEDKRUM_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FK_ABI_VERSION 1
#define FK_MAX_K 4096     /* rows of a round: one row's K - 1 distances are sorted in 32 KiB of LDS */
#define FK_PLAN_FIELDS 6  /* int64 of fk_gram_plan */

int32_t fk_abi_version(void);

/*
 * The plan of fk_gram at (K, P) (host only, no GPU needed): plan_out[0..5] = {row tile (64), lower-triangle tiles
 * T (T + 1) / 2 with T = ceil(K / 64), nsplit, columns per split (a multiple of the step), columns per step (32),
 * steps of the last split}.  nsplit = min(ceil(2048 / tiles), ceil(steps / 4)), at least 1, lowered until the
 * workspace nsplit * K * K * 8 fits 512 MiB (at K = 4096 one split is 128 MiB and the tiles alone fill the GPU);
 * then re-derived from the steps per split, so no split is empty.  Returns 0, or FA_E_ARG (K < 1, K > FK_MAX_K,
 * P < 0, NULL plan_out).
 */
int64_t fk_gram_plan(int32_t K, int64_t P, int64_t* plan_out);

/* Bytes of the workspace fk_gram needs at (K, P): nsplit * K * K * 8, at most 512 MiB.  FA_E_ARG as fk_gram_plan. */
int64_t fk_gram_workspace_bytes(int32_t K, int64_t P);

/*
 * gram_out[i*K + j] = G[i][j] of the K rows x[k*ld + p] against last[p] (above), all K x K entries.  Two launches:
 * the tile partials (row tiles x column splits; each step loads a 64 x 32 slab per operand with 16-byte loads,
 * subtracts the step's slice of last, keeps the fp32 differences in LDS and widens fragments as they are read),
 * then the split sum and mirror.  No atomics.
 *   x, last, gram_out, workspace: device memory; workspace_bytes >= fk_gram_workspace_bytes(K, P).
 * Replaces: nothing (the reference has no server-side Krum).
 */
int fk_gram(const float* x, int64_t ld, int32_t K, int64_t P, const float* last, double* gram_out, void* workspace,
            int64_t workspace_bytes, fa_stream_t stream);

/*
 * score_out[i] for i < K from gram (K x K, row-major) by the lines v, dist2 and score above; 2f + 3 <= K.  One
 * workgroup per row: the K - 1 values of dist2 are sorted ascending in LDS and one lane adds the first K - f - 2.
 */
int fk_scores(const double* gram, int32_t K, int32_t f, double* score_out, fa_stream_t stream);

/* c_out[i] (float, 1.0f or 0.0f) for i < K and *n_sel_out (int32) by the lines rank, c and n_sel; 1 <= m <= K. */
int fk_select(const double* score, int32_t K, int32_t m, float* c_out, int32_t* n_sel_out, fa_stream_t stream);

/*
 * out[p] = *n_sel > 0 ? last[p] + chain[p] / float(*n_sel) : last[p], p < P (IEEE division); mirror[p] = out[p]
 * when given.  n_sel is read on the device: no host synchronisation sits between selection and finish.
 *   mirror  optional second copy of out; may be pinned host memory, as fcl_finish's
 */
int fk_finish(const float* chain, const float* last, const int32_t* n_sel, int64_t P, float* out, float* mirror,
              fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDKRUM_H */
