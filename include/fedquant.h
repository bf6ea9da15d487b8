/*
 * fedquant.h — C ABI of the MXFP8 delta-upload path on MI355X (gfx950): client updates d = x - L quantised on the
 * executor to the OCP Microscaling format MXFP8 (blocks of 32 e4m3fn codes sharing one E8M0 scale byte), staged in
 * HBM at 1 + 1/32 bytes per parameter, dequantised exactly and reduced in fp32 on the device.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued).  The entry
 * points of this header are bound by fedscale_amd/_native_quant.py; the header has its own version
 * (fq_abi_version), FA_ABI_VERSION is not touched by it.
 *
 * What is replaced (reference): nothing — the reference's executor uploads fp32 (torch_client.py:79-91) and its
 * aggregator chains fp32 (aggregator.py:489-511).  The chain computed here is fcl_reduce's (fedclip.h) over
 * dequantised deltas with every coefficient 1, and the round is closed by fcl_finish: L + chain / K.
 *
 * Arithmetic.  The bucket is the fp32 entries concatenated in state_dict order, P columns.  Block b covers columns
 * [32b, 32b + 32); the last block may be partial; blocks do not restart at entry boundaries.
 *
 * Quantise (one rounding per element).  d[p] = x[p] - L[p] in fp32, unfused; amax = the largest |d[p]| over the
 * block's existing columns.  With E and M the biased exponent field and the mantissa field of amax's fp32 bits
 * (integer arithmetic only):
 *     s = clamp(E - 8 + (M > 0x600000), 10, 246)        every d of the block finite
 *     s = 255                                            the block holds a NaN or an infinity (codes unspecified;
 *                                                        this library writes 0)
 * i.e. e = floor(log2 amax) - 8, one more when amax > 448 * 2^e, so that no finite element exceeds e4m3's largest
 * finite value.  code[p] = e4m3fn(clamp(d[p] * 2^(127 - s), -448, 448)): to nearest even, subnormal codes kept,
 * -0 stays -0; the multiply by a power of two is exact wherever the result matters; the clamp acts only at s = 246
 * (amax > 1.75 * 2^127); the low clamp at s = 10 keeps every dequantised value a normal fp32 (deltas below about
 * 2^-127 become 0).  Padding codes of a partial block are 0.
 *
 * Dequantise (exact).  deq[p] = value(code[p]) * 2^(s - 127), the fp32 product rounded to nearest: exact for every s
 * in 0..246, subnormal fp32 results included; it can round to +-inf only for s >= 247, which the quantiser never
 * emits.  s = 255 makes the whole block NaN; the NaN codes 0x7F and 0xFF dequantise to NaN.
 *
 * Reduce.  fp32, rounded to nearest, never fused; one thread owns a column through all rows, so no launch plan
 * changes a bit:
 *     chain[p] = FA_ACCUMULATE ? acc_in[p] : +0.0f;     chain[p] = chain[p] + deq_k[p]   for k in arrival order
 */
#ifndef FEDQUANT_H
#define FEDQUANT_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FQ_ABI_VERSION 1
#define FQ_PLAN_FIELDS 6 /* int64 per launch of fq_reduce_plan */
#define FQ_BLOCK 32      /* columns that share one scale byte */

int32_t fq_abi_version(void);

/*
 * The chain above over n rows of codes q8[k*ld + p] with scale bytes scales[k*lds + p/32], into out[0, P).
 *   q8      device memory, 16-byte aligned; ld a multiple of 64, >= P.  Rows are read 16 bytes (16 columns) per
 *           lane, up to round_up(P, 16) <= ld bytes of each row; codes in [P, ld) are never counted.
 *   scales  device memory, 16-byte aligned; lds >= ceil(P / 32).  Scale bytes past ceil(P / 32) are never read.
 *   acc_in  (FA_ACCUMULATE) >= round_up(P, 4) floats, 16-byte aligned; out may alias it.  n == 0 needs it.
 *   out     >= P floats, 16-byte aligned; written in [0, P) only (float4 stores, the last column masked at P).
 *   flags   0 or FA_ACCUMULATE.
 */
int fq_reduce(const uint8_t* q8, const uint8_t* scales, int64_t ld, int64_t lds, int32_t n, int64_t P,
              const float* acc_in, float* out, int32_t flags, fa_stream_t stream);

/*
 * The launches fq_reduce makes at (K, P) on a GPU of `cus` compute units (host only, no GPU needed):
 * plan_out[FQ_PLAN_FIELDS*i + {0..5}] = {V, U, first column, tiles, strips per wave, grid} of launch i, for
 * i < min(cap, returned count), as fh_reduce_plan's (fedhalf.h); a strip is 64 lanes x 16 columns.  Returns the
 * number of launches (>= 0) or FA_E_ARG.
 */
int64_t fq_reduce_plan(int32_t cus, int32_t K, int64_t P, int64_t* plan_out, int32_t cap);

/*
 * The executor-side handler: one contiguous fp32 device row quantised as above,
 *     d[p] = base ? x[p] - base[p] : x[p]          p < P
 * into q8 (round_up(P, 32) codes, the padding codes 0) and scales (ceil(P / 32) bytes).  x, base and q8 are device
 * memory, 16-byte aligned; x and base hold P floats.  Stateless, no atomics, no host synchronisation.  The host-side
 * equivalent is fedscale_amd/cloud/execution/quant_upload.py; both give the same bytes.
 */
int fq_quantize_row(const float* x, const float* base, int64_t P, uint8_t* q8, uint8_t* scales, fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDQUANT_H */
