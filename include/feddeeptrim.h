/*
 * feddeeptrim.h — C ABI of the deep coordinate-wise trimmed mean on MI355X (gfx950): the trimmed mean of fedtrim.h
 * at ANY trim count t with 1 <= t, 2t < K — the 10-20 % trims of Yin et al. (ICML 2018) at K = 1000, the median at
 * any K, Bulyan's inner trimmed mean — for rounds of up to FDT_MAX_ROWS uploads.  fedtrim.h's selection keeps 2t keys
 * per column in registers and stops at t = 16; this one holds a tile of all K rows in LDS and selects there, so the
 * staged rows are read from HBM once and t costs nothing.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued: a refused
 * call says "nothing was launched").  The entry points of this header are bound by fedscale_amd/_native_deeptrim.py;
 * the header has its own version (fdt_abi_version); no other header's version is touched by it.
 *
 * The arithmetic is fedtrim.h's, restated — K staged uploads x_k (fp32, arrival order k = 0..K-1), P columns, trim
 * count t; everything fp32, rounded to nearest, never fused:
 *
 *   Order key.  key(v) = isnan(v) ? 0xFFFFFFFF : (bits(v) >> 31 ? ~bits(v) : bits(v) | 0x80000000), unsigned.
 *     -inf < ... < -0 < +0 < ... < +inf < every NaN; different bit patterns of non-NaN values never tie.
 *   Selection, per column p:
 *     lo[p] = the t-th smallest key (rank t - 1), hi[p] = the t-th largest (rank K - t);
 *     n_lo[p] = t - #{k : key < lo}  rows whose key EQUALS lo[p] that are dropped, in 1..t;
 *     n_hi[p] = t - #{k : key > hi}  the same for hi[p].
 *   Kept set, walking the rows in arrival order with the two counters, low test first:
 *     row k is dropped low  if key < lo, or key == lo while n_lo > 0 (then n_lo -= 1);
 *     otherwise dropped high if key > hi, or key == hi while n_hi > 0 (then n_hi -= 1);
 *     otherwise kept.  Exactly K - 2t rows are kept per column, also when lo == hi.
 *   Sum and mean:
 *     chain[p] = the first kept x_k[p] itself (a kept -0 stays -0); every later kept x_k[p] is added in arrival
 *     order; out[p] = chain[p] / float(K - 2t), IEEE division.  The library computes the denominator.
 *   Per-row counts: dropped[k][0] += #{p < P : row k dropped low}, dropped[k][1] += #{... dropped high}, int64.
 *     Exact integers, so the order they are gathered in cannot change them.  The caller zeroes the table.
 *
 * The result is a pure function of (x, K, P, t): the grid, the tiles a workgroup walks and the tile width change
 * no bit, and for t <= ft_max_trim() it has the bits of ft_select + ft_reduce.  Which NaN a NaN result is, is not
 * part of the contract.  t = 0 is not taken here: that round is plain FedAvg, served by ft_reduce.
 *
 * Sizes: x rows hold >= round_up(P, 4) elements and are read as 4-element columns; columns >= P never reach an
 * output or a count.  out and mirror are written in columns [0, P) only.  x, out and mirror are 16-byte aligned,
 * `dropped` 8-byte; ld is a multiple of 4 and >= P.
 */
#ifndef FEDDEEPTRIM_H
#define FEDDEEPTRIM_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FDT_ABI_VERSION 1
#define FDT_MAX_ROWS 4096   /* the largest K (fdt_max_rows): a tile of 4 columns and its drop counts fit in LDS */
#define FDT_PLAN_FIELDS 7   /* int64 written by fdt_plan */

int32_t fdt_abi_version(void);

/* The largest K fdt_reduce takes: 4096, the bound of the Krum and geometric-median rounds. */
int32_t fdt_max_rows(void);

/*
 * out[p] (and mirror[p] when given) = the trimmed mean of column p of the K rows x[k*ld + p], p < P, by the rule
 * above.  1 <= t, 2t < K <= fdt_max_rows().  One launch: a workgroup of 256 lanes owns tiles of all K rows x C
 * columns (fdt_plan), loads a tile into LDS as order keys, finds rank t - 1 and rank K - t of every column by an
 * 8-bit most-significant-digit radix select on the LDS-resident keys, marks the dropped rows with their exact
 * arrival-order tie ranks, and chains the kept ones with one lane per column.
 *   x        device memory
 *   mirror   optional second copy of out; may be pinned host memory
 *   dropped  optional int64 [K][2] device table the per-row counts are ADDED to (gathered per workgroup in LDS,
 *            integer atomics at its end); the float outputs are the same bits with and without it
 *   cus      0: the launch is planned for the device's compute units; > 0: for this many (the result's bits do not
 *            depend on it — that is what the argument is for)
 */
int fdt_reduce(const float* x, int64_t ld, int32_t K, int64_t P, int32_t t, float* out, float* mirror,
               int64_t* dropped, int32_t cus, fa_stream_t stream);

/*
 * The launch fdt_reduce makes at (K, P, t) on a GPU of `cus` compute units (host only, no GPU needed):
 * plan_out[0..6] = {C: columns of a tile, a function of K alone; lanes per column 256 / C; rows per lane (odd, so
 * that the lanes of a wave fall into distinct LDS banks); LDS bytes of the workgroup; tiles ceil(P / C); grid;
 * workgroups per CU the LDS leaves room for (2, or 1 above 3280 rows)}.  grid < tiles: workgroup b walks tiles b,
 * b + grid, ...  Returns FA_OK or FA_E_ARG (cus <= 0, plan_out NULL, negative P, t < 1, 2t >= K,
 * K > fdt_max_rows()).
 */
int fdt_plan(int32_t cus, int32_t K, int64_t P, int32_t t, int64_t* plan_out);

#ifdef __cplusplus
}
#endif
#endif /* FEDDEEPTRIM_H */
