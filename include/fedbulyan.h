/*
 * fedbulyan.h — C ABI of Bulyan on MI355X (gfx950): Krum run theta times, the winner removed each time, and then,
 * for every parameter, the mean of the beta selected values closest to their median (El Mhamdi, Guerraoui, Rouault,
 * ICML 2018).  Multi-Krum (fedkrum.h) hands its winners over whole — one hidden coordinate with a huge value still
 * moves the model; the trimmed means (fedtrim.h, feddeeptrim.h) are safe per coordinate but blind to collusion.
 * Bulyan composes the two and is the only rule of this family with a per-coordinate guarantee.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued: a refused
 * call says "nothing was launched").  The entry points of this header are bound by fedscale_amd/_native_bulyan.py;
 * the header has its own version (fbl_abi_version); no other header's version is touched by it.
 *
 * K uploads x_k are resident in staging in arrival order; the round starts from model L; f uploads are assumed bad.
 *
 *   theta = K - 2f - 2          rows selected
 *   beta  = theta - 2f          values kept per coordinate = K - 4f - 2
 *   0 <= f,  4f + 3 <= K <= FK_MAX_K
 *
 * The paper selects K - 2f rows, which runs its last two Krum calls on fewer than 2f + 3 rows, below Krum's own
 * precondition (fk_scores: 2f + 3 <= K).  With theta = K - 2f - 2 the last call sees exactly 2f + 3 rows, and
 * beta >= 1 is the paper's K >= 4f + 3.
 *
 * Selection, in K-space.  G is fk_gram's matrix, unchanged; dist2[i][j] follows the lines `v` and `dist2` of fedkrum.h.
 *
 *   R_0 = {0..K-1}
 *   for s = 0 .. theta-1:
 *       n = K - s
 *       score_s[i] = +0.0, then + the n - f - 2 smallest dist2[i][j], j in R_s \ {i},
 *                    added one by one in ascending order, fp64        (i in R_s)
 *       pick_s = the i in R_s with the smallest (score_s[i], i), lexicographic
 *       if score_s[pick_s] is not finite: stop with n_sel = s
 *       R_{s+1} = R_s \ {pick_s}
 *   n_sel = theta if never stopped
 *
 * score_0 is fk_scores(G, K, f) bit for bit and pick_0 is the row fk_select(m = 1) keeps.  Outputs: picks[theta]
 * (int32, in selection order, -1 from n_sel on), sel[theta] (the picks in ascending order, which is arrival order,
 * -1 from n_sel on) and n_sel (int32, on the device).
 *
 * A row with an inf or NaN has dist2 = +inf to every other row (fedkrum.h), an infinite score in every iteration, and
 * is never picked.  With b such rows, iteration s offers a finite row n - 1 - b finite distances and adds n - f - 2
 * of them: with b <= f (and still with b = f + 1, as in fedkrum.h) there are enough in every iteration, and K - b >=
 * theta finite rows exist, so every pick is finite.  With more such rows no score is finite, the picks run out —
 * the number of infinite distances a remaining row sees never grows, so this shows in the first iteration —
 * n_sel < theta, and the round leaves the model as it was (below): the stance of fk_finish at n_sel = 0.
 *
 * Mean around the median, per column p, over the selected rows r = 0..theta-1 with v_r = x[sel[r]][p]; everything
 * fp32, rounded to nearest, never fused:
 *
 *   key(v)   feddeeptrim.h's order key
 *   med      the v_r whose key has ascending rank (theta - 1) / 2   (the lower median: an uploaded value, no rounding)
 *   e_r      |v_r - med|, one subtraction, then the sign bit cleared
 *   ekey_r   isnan(e_r) ? 0xFFFFFFFF : bits(e_r)
 *   cut      the ekey of ascending rank beta - 1
 *   n_cut    beta - #{r : ekey_r < cut}
 *   row r is kept if ekey_r < cut, or ekey_r == cut and fewer than n_cut earlier rows (smaller r) have ekey == cut;
 *            exactly beta rows are kept
 *   chain[p] the first kept v_r itself (a kept -0 stays -0), every later kept v_r added in order of r
 *   out[p]   *n_sel == theta ? chain[p] / float(beta) : L[p]           (IEEE division)
 *   kept[sel[r]] += #{p < P : row r kept}                              (int64, optional table, exact in any order)
 *
 * The result is a pure function of (x, sel, theta, beta, P): the grid, the tile width and the lane split change no
 * bit.  Columns >= P never reach an output or a count.  Rows not in sel are never read; an entry of sel outside
 * [0, K) is never dereferenced (its row reads as +0).  Which NaN a NaN result is, is not part of the contract.
 *
 * Sizes: x rows and L hold >= round_up(P, 4) elements and are read as 4-element columns; out and mirror are written
 * in columns [0, P) only.  x, last, out and mirror are 16-byte aligned, gram / workspace / kept 8-byte, picks / sel /
 * n_sel 4-byte; ld is a multiple of 4 and >= P.
 */
#ifndef FEDBULYAN_H
#define FEDBULYAN_H

#include <stdint.h>

#include "fedagg.h"
#include "fedkrum.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FBL_ABI_VERSION 1
#define FBL_PLAN_FIELDS 7 /* int64 written by fbl_plan */

int32_t fbl_abi_version(void);

/* Bytes of the workspace fbl_select needs at K: every row's K - 1 sorted distances (fp64) and their neighbours (int32),
 * and two score vectors.  FA_E_ARG: K < 1 or K > FK_MAX_K. */
int64_t fbl_select_workspace_bytes(int32_t K);

/*
 * picks, sel (theta = K - 2f - 2 int32 each) and *n_sel from gram (K x K, row-major, fk_gram's) by the selection
 * above; 0 <= f, 4f + 3 <= K <= FK_MAX_K.  theta + 2 launches, none of which waits on another workgroup: one workgroup
 * per row sorts that row's (dist2, j) pairs once (LDS bitonic sort); then one launch per iteration, grid K — the
 * workgroup of a remaining row re-derives the previous pick from the previous iteration's scores (every workgroup
 * computes the same argmin, workgroup 0 records it), builds the removed set in LDS, compacts the first n - f - 2
 * surviving distances of its sorted row with a prefix scan and one lane adds them in order; the scores ping-pong
 * between two buffers; a last launch of one workgroup records the last pick and writes sel and *n_sel.
 *   gram, picks, sel, n_sel, workspace: device memory; workspace_bytes >= fbl_select_workspace_bytes(K).
 */
int fbl_select(const double* gram, int32_t K, int32_t f, int32_t* picks, int32_t* sel, int32_t* n_sel,
               void* workspace, int64_t workspace_bytes, fa_stream_t stream);

/*
 * out[p] (and mirror[p] when given), p < P, by the mean around the median above over the theta rows
 * x[sel[r]*ld + p]; 1 <= beta <= theta <= K <= FK_MAX_K.  *n_sel is read on the device: when it differs from theta
 * the workgroups copy their columns of `last` and do nothing else.  One launch: a workgroup of 256 lanes loads a tile
 * of theta rows x W columns through sel into LDS as order keys; a column then belongs to 16, 32 or 64 lanes of ONE
 * wave (fbl_plan), each holding a contiguous slice of its rows in registers; the median and the distance cut are two
 * 32-step bisections on the key bits whose counts are reduced inside the wave — no workgroup barrier and no LDS
 * atomic inside a selection; ties at the cut take their arrival-order rank from a scan over the column's lanes; the
 * kept values go back to LDS and one lane per column chains them in order of r.
 *   x, sel, n_sel, last, out: device memory
 *   mirror  optional second copy of out; may be pinned host memory
 *   kept    optional int64 [K] device table the per-row counts are ADDED to (gathered per workgroup in LDS, integer
 *           atomics at its end); the float outputs are the same bits with and without it
 *   cus     0: the launch is planned for the device's compute units; > 0: for this many (the result's bits do not
 *           depend on it)
 */
int fbl_reduce(const float* x, int64_t ld, int32_t K, int64_t P, const int32_t* sel, const int32_t* n_sel,
               int32_t theta, int32_t beta, const float* last, float* out, float* mirror, int64_t* kept, int32_t cus,
               fa_stream_t stream);

/*
 * The launch fbl_reduce makes at (theta, P) on a GPU of `cus` compute units (host only, no GPU needed):
 * plan_out[0..6] = {lanes per column: 16 up to theta = 80, 16 up to 272, 32 up to 1056, 64 beyond; rows per lane: 5,
 * 17, 33, 65 (odd, so that the lanes of a wave fall into distinct LDS banks); W: columns of a tile, the widest power
 * of two up to 64 with theta (W + 1) words inside 80 KiB, at least 256 / lanes; passes W lanes / 256 a workgroup
 * makes over a tile; LDS bytes the kernel allocates, statically: 20800 at 5 rows per lane, 70720 at 17, 81920 beyond
 * (theta (W + 1) 4 of them are used); tiles ceil(P / W); grid min(tiles, wgs cus) with wgs = 4, 2, 2, 1 workgroups
 * per CU by rows per lane, what LDS and registers leave room for}.  workgroup b walks tiles b, b + grid, ...  Returns FA_OK or FA_E_ARG (cus <= 0, plan_out NULL, negative P, theta < 1, theta > FK_MAX_K).
 */
int fbl_plan(int32_t cus, int32_t theta, int64_t P, int64_t* plan_out);

#ifdef __cplusplus
}
#endif
#endif /* FEDBULYAN_H */
