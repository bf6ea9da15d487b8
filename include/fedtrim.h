/*
 * fedtrim.h — C ABI of the coordinate-wise trimmed mean (and, as its limit case, the coordinate-wise median) on
 * MI355X (gfx950): for every column the t smallest and the t largest of the K staged uploads are dropped and the
 * rest averaged (Yin et al., ICML 2018: a server-side defence against poisoned uploads that needs no norm bound).
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued: a refused
 * call says "nothing was launched").  The entry points of this header are bound by fedscale_amd/_native_trim.py;
 * the header has its own version (ft_abi_version); FA_, FH_ and FCL_ABI_VERSION are not touched by it.
 *
 * The arithmetic of a round of K staged uploads x_k (fp32, arrival order k = 0..K-1), P columns, trim count t with
 * 0 <= t, 2t < K, t <= FT_MAX_TRIM — everything fp32, rounded to nearest, never fused:
 *
 *   Order key.  key(v) = isnan(v) ? 0xFFFFFFFF : (bits(v) >> 31 ? ~bits(v) : bits(v) | 0x80000000), unsigned.
 *     -inf < ... < -0 < +0 < ... < +inf < every NaN; different bit patterns of non-NaN values never tie; key 0
 *     never occurs (it would need bits(v) = 0xFFFFFFFF, a NaN).
 *   Selection (ft_select), per column p, when t > 0:
 *     lo[p] = the t-th smallest key, hi[p] = the t-th largest;
 *     n_lo[p] = t - #{k : key < lo}  rows whose key EQUALS lo[p] that are dropped, in 1..t;
 *     n_hi[p] = t - #{k : key > hi}  the same for hi[p];   ties[p] = n_lo | n_hi << 16.
 *   Kept set, walking the rows in arrival order with the two counters, low test first:
 *     row k is dropped low  if key < lo, or key == lo while n_lo > 0 (then n_lo -= 1);
 *     otherwise dropped high if key > hi, or key == hi while n_hi > 0 (then n_hi -= 1);
 *     otherwise kept.  Exactly K - 2t rows are kept per column, also when lo == hi.
 *   Sum and mean (ft_reduce):
 *     chain[p] = the first kept x_k[p] itself (not +0 + x: a kept -0 stays -0); every later kept x_k[p] is added
 *     in arrival order; out[p] = chain[p] / float(K - 2t), IEEE division.  The library computes the denominator.
 *   Per-row counts: dropped[k][0] += #{p < P : row k dropped low}, dropped[k][1] += #{... dropped high}, int64.
 *     Exact integers, so the order they are gathered in cannot change them.  The caller zeroes the table.
 *
 * Consequences: with t = 0, out has the bits of the unweighted FedAvg round (chain from client 0, divided by
 * float(K)); with t = (K-1)/2, out has the bits of numpy's median over NaN-free columns (odd K: the middle value
 * over 1.0f; even K: the two middle values, smaller + larger in arrival order — fp32 addition commutes — over
 * 2.0f); a column with at most t NaNs gets a NaN-free result, since NaNs sort last and are trimmed first from the
 * top; a column with more than t NaNs gives NaN.  Which NaN (its sign and payload) a NaN result is, is not part of
 * the contract: it is whatever the GPU's adder propagates.
 *
 * Sizes: buffers that are READ column-wise (x rows, and lo / hi / ties in ft_reduce) hold >= round_up(P, 4)
 * elements and are read as 4-element columns; columns >= P never reach an output or a count.  Buffers that are
 * WRITTEN (lo / hi / ties in ft_select, out, mirror) are written in columns [0, P) only.  Row and vector pointers
 * are 16-byte aligned, `dropped` 8-byte; ld is a multiple of 4 and >= P.
 */
#ifndef FEDTRIM_H
#define FEDTRIM_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FT_ABI_VERSION 1
#define FT_MAX_TRIM 16    /* deepest instantiated selection buffer (ft_max_trim) */
#define FT_PLAN_FIELDS 7  /* int64 per launch of ft_plan */
#define FT_KERNEL_SELECT 0
#define FT_KERNEL_REDUCE 1

int32_t ft_abi_version(void);

/*
 * The largest t ft_select / ft_reduce take: 16.  The selection keeps 2 T sorted keys per column in registers; at
 * T = 16 with one float4 column per lane that is 128 registers, which still leaves 3 waves per SIMD and no scratch
 * (trim_reduce.hip's header has the arithmetic).  T = 32 would be 256 registers for the buffers alone: one wave
 * per SIMD at best, on an ALU-bound kernel — not instantiated.  The register budget forces no value below 16.
 */
int32_t ft_max_trim(void);

/*
 * lo[p], hi[p], ties[p] for p < P over the K rows x[k*ld + p] (above).  One lane owns its columns through all K
 * rows and keeps the T smallest and T largest keys of each sorted in registers (T: the smallest instantiated depth
 * >= t, one of 1, 2, 4, 8, 16); the rows are streamed once, non-temporal.  1 <= t, 2t < K, t <= ft_max_trim().
 *   x, lo, hi, ties: device memory.  Replaces: nothing (the reference has no server-side trimmed mean).
 */
int ft_select(const float* x, int64_t ld, int32_t K, int64_t P, int32_t t, uint32_t* lo, uint32_t* hi,
              uint32_t* ties, fa_stream_t stream);

/*
 * out[p] (and mirror[p] when given) = the trimmed mean of column p by the kept rule above, p < P; K >= 1.
 * With t == 0 the three threshold pointers must be NULL and every row is kept; with t > 0 they are ft_select's
 * output for the same x, K and t (values for other rows are not detected; what is then averaged is whatever the
 * kept rule keeps, divided by K - 2t; a column that keeps no row yields +0.0 / (K - 2t)).
 *   mirror   optional second copy of out; may be pinned host memory, as fcl_finish's
 *   dropped  optional int64 [K][2] device table the per-row counts are ADDED to (integer atomics; gathered per
 *            workgroup in LDS while K <= 4096, straight into the table beyond); the float outputs are the same
 *            bits with and without it; with t == 0 nothing is added
 */
int ft_reduce(const float* x, int64_t ld, int32_t K, int64_t P, int32_t t, const uint32_t* lo, const uint32_t* hi,
              const uint32_t* ties, float* out, float* mirror, int64_t* dropped, fa_stream_t stream);

/*
 * The launches ft_select (none when t == 0) and then ft_reduce make at (K, P, t) on a GPU of `cus` compute units
 * (host only, no GPU needed): plan_out[FT_PLAN_FIELDS*i + {0..6}] = {kernel (FT_KERNEL_*), T (0 for the reduce),
 * V, U, first column, tiles, grid} of launch i, for i < min(cap, returned count).  V: float4 loads per lane per
 * row (a strip is 64 lanes x 4 columns, a tile 4 waves of V strips); U: rows loaded ahead of their use; grid <
 * tiles: every workgroup walks ceil(tiles / grid) tiles.  K and t pick the instantiation, never who owns a column.
 * Returns the number of launches (>= 0) or FA_E_ARG (cus <= 0, negative K / P / t / cap, 2t >= K,
 * t > ft_max_trim()).
 */
int64_t ft_plan(int32_t cus, int32_t K, int64_t P, int32_t t, int64_t* plan_out, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* FEDTRIM_H */
