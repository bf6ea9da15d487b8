/*
 * fedsign.h — C ABI of the 1-bit sign delta-upload path on MI355X (gfx950): client updates e = (x - L) + r compressed
 * on the executor to the scaled sign with error feedback (EF-signSGD, 1-bit SGD) — one bit per parameter plus one fp32
 * scale per block of 256 parameters, 9/64 byte per parameter on the wire and in HBM — dequantised exactly and reduced
 * in fp32 on the device.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued).  The entry
 * points of this header are bound by fedscale_amd/_native_sign.py; the header has its own version
 * (fsg_abi_version), FA_ABI_VERSION is not touched by it.
 *
 * What is replaced (reference): nothing — the reference's executor uploads fp32 (torch_client.py:79-91) and its
 * aggregator chains fp32 (aggregator.py:489-511).  The chain computed here is fcl_reduce's (fedclip.h) over
 * dequantised deltas with every coefficient 1, and the round is closed by fcl_finish: L + chain / K.
 *
 * The contract.  The bucket is the float32 entries concatenated in state_dict order, P columns.  Block b covers
 * columns [256b, 256b + 256).  The last block may be partial, with n_b existing columns.  Blocks do not restart at
 * entry boundaries.
 *
 * Encode (executor, one lossy step):
 *   1. e[p] = (x[p] - L[p]) + r[p] in fp32, two unfused roundings.  r is the residual, and `+ r` is skipped when
 *      there is none.  L is the weights the executor was sent for the round; with base == NULL, e = x (+ r).
 *   2. bit[p] is the fp32 sign bit of e[p], so -0 counts as negative.  It is stored as bit p % 8 of byte p / 8.
 *      Padding bits of the last byte, and of the row up to its stride, are 0.
 *   3. Block scale: with a[p] = |e[p]| as fp64, and missing columns of a partial block counting +0.0:
 *          t[l] = ((a[l] + a[l+64]) + a[l+128]) + a[l+192]        for l < 64
 *      then the xor butterfly of wave_sum (fa_common.h): t[l] += t[l ^ m] for m = 32, 16, 8, 4, 2, 1.
 *          scale_b = (float)(t[0] / (double)n_b)
 *      The order is fixed by the block alone, so host and device give the same bits.
 *   4. A block that holds a NaN or an infinity gets the scale bits 0x7FC00000 and all-zero bits.  Its residual_out
 *      columns are +0.0.
 *   5. residual_out[p] = e[p] - deq[p] in fp32, one rounding, where deq[p] = bit[p] ? -scale_b : +scale_b.
 *
 * Dequantise is exact: it is a sign flip of the scale (deq's bits are the scale's with the sign bit xor bit[p]).  A
 * NaN scale makes exactly its block's columns NaN.
 *
 * Reduce runs in fp32, rounded to nearest and never fused.  One thread owns a column through all rows, so no launch
 * plan changes a bit:
 *     chain[p] = FA_ACCUMULATE ? acc_in[p] : +0.0f;     chain[p] += deq_k[p]   for k in arrival order
 * The round closes with the existing fcl_finish: L + chain / K.
 *
 * Staging rows.  Both arrays are 16-byte aligned.  bits is [capacity, ldb] bytes, with
 * ldb = round_up(ceil(P/8), 16); scales is [capacity, lds] floats, with lds = round_up(ceil(P/256), 4).
 */
#ifndef FEDSIGN_H
#define FEDSIGN_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FSG_ABI_VERSION 1
#define FSG_PLAN_FIELDS 6 /* int64 per launch of fsg_reduce_plan */
#define FSG_BLOCK 256     /* columns that share one fp32 scale */

int32_t fsg_abi_version(void);

/*
 * The chain above over n rows of sign bits (column p of row k is bit p % 8 of bits[k*ldb + p/8]) with scales
 * scales[k*lds + p/256], into out[0, P).
 *   bits    device memory, 16-byte aligned; ldb (bytes) a multiple of 16, >= ceil(P / 8).  Rows are read one dword
 *           (32 columns) per lane, up to 4 * ceil(P / 32) <= ldb bytes of each row; bits of columns >= P are never
 *           counted.
 *   scales  device memory, 16-byte aligned; lds (floats) >= ceil(P / 256).  Scales past ceil(P / 256) are never
 *           read.
 *   acc_in  (FA_ACCUMULATE) >= round_up(P, 4) floats, 16-byte aligned; out may alias it.  n == 0 needs it.
 *   out     >= P floats, 16-byte aligned; written in [0, P) only (float4 stores, the last column masked at P).
 *   flags   0 or FA_ACCUMULATE.
 */
int fsg_reduce(const uint8_t* bits, const float* scales, int64_t ldb, int64_t lds, int32_t n, int64_t P,
               const float* acc_in, float* out, int32_t flags, fa_stream_t stream);

/*
 * The launches fsg_reduce makes at (K, P) on a GPU of `cus` compute units (host only, no GPU needed):
 * plan_out[FSG_PLAN_FIELDS*i + {0..5}] = {V, U, first column, tiles, strips per wave, grid} of launch i, for
 * i < min(cap, returned count), as fh_reduce_plan's (fedhalf.h); a strip is 64 lanes x 32 columns.  Returns the
 * number of launches (>= 0) or FA_E_ARG.
 */
int64_t fsg_reduce_plan(int32_t cus, int32_t K, int64_t P, int64_t* plan_out, int32_t cap);

/*
 * The executor-side handler: one contiguous fp32 device row encoded as above in one launch,
 *     e[p] = (base ? x[p] - base[p] : x[p]) (+ residual[p])          p < P
 * into bits (32 * ceil(P / 256) bytes: whole blocks, the padding bits 0), scales (ceil(P / 256) floats) and, when
 * residual_out is given, residual_out (P floats).  base, residual and residual_out may each be NULL; residual_out may
 * alias residual.  x, base, residual and residual_out are device memory of P floats; bits is 16-byte aligned.
 * Stateless, no atomics, no host synchronisation.  The host-side equivalent is
 * fedscale_amd/cloud/execution/sign_upload.py; both give the same bytes.
 */
int fsg_sign_row(const float* x, const float* base, const float* residual, int64_t P, uint8_t* bits, float* scales,
                 float* residual_out, fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDSIGN_H */
