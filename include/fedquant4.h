/*
 * fedquant4.h — C ABI of the MXFP4 delta-upload path on MI355X (gfx950): client updates d = x - L quantised on the
 * executor to the OCP Microscaling format MXFP4 (blocks of 32 e2m1 codes sharing one E8M0 scale byte), staged in HBM
 * at 17/32 byte per parameter, dequantised exactly and reduced in fp32 on the device.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued).  The entry
 * points of this header are bound by fedscale_amd/_native_quant4.py; the header has its own version
 * (fq4_abi_version), FA_ABI_VERSION and FQ_ABI_VERSION are not touched by it.
 *
 * What is replaced (reference): nothing — the reference's executor uploads fp32 (torch_client.py:79-91) and its
 * aggregator chains fp32 (aggregator.py:489-511).  The chain computed here is fcl_reduce's (fedclip.h) over
 * dequantised deltas with every coefficient 1, and the round is closed by fcl_finish: L + chain / K.
 *
 * Row layout.  The bucket is the fp32 entries concatenated in state_dict order, P columns.  Block b covers columns
 * [32b, 32b + 32); the last block may be partial; blocks do not restart at entry boundaries.  A staged row holds
 * ld / 2 code bytes and ld / 32 scale bytes: column 2i is the low nibble of byte i and column 2i + 1 its high nibble
 * (the OCP order), so one block is exactly one 16-byte load and one scale byte.  A code is s eem: sign, two exponent
 * bits, one mantissa bit; its magnitudes are 0, 0.5, 1, 1.5, 2, 3, 4, 6 for codes 0..7, negated for codes 8..15
 * (code 8 is -0).
 *
 * Dequantise (exact).  deq[p] = value(code[p]) * 2^(s - 127) for a scale byte s in 2..252: every such product is
 * exact and a normal fp32 or a zero (0.5 * 2^-125 = 2^-126 at the bottom, 6 * 2^125 at the top).  Any other scale
 * byte (0, 1, 253, 254, 255) poisons its block: all 32 columns of the chain become NaN, whatever the codes are.
 * This differs from MXFP8 (fedquant.h), which defines all 256 scale bytes through an fp32 multiply: the device widens
 * MXFP4 with the scaled convert (v_cvt_scalef32_pk_f32_fp4), which is not a multiply, and what it gives outside the
 * normal range is not something this contract is built on.
 *
 * Quantise (one rounding per element).  d[p] = x[p] - L[p] in fp32, unfused (then + residual[p], a second unfused
 * add, with error feedback); am = the largest |d[p]| bit pattern over the block's existing columns.  With E and M
 * the biased exponent field and the mantissa field of am (integer arithmetic only):
 *     s = clamp(E - 2 + (M > 0x400000), 2, 252)         every d of the block finite
 *     s = 255                                            the block holds a NaN or an infinity; its codes are 0
 * i.e. e = floor(log2 am) - 2, one more when am > 1.5 * 2^(e+2), so that am / 2^(s - 127) <= 6 and nothing clips
 * below the upper clamp.  code[p] = e2m1(clamp(d[p] * 2^(127 - s), -6, 6)), rounded to the nearest e2m1 value, ties
 * to the code whose low bit is 0 (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); the sign
 * is kept, so -0 and small negatives give code 8.  Padding columns past P are code 0.
 *
 * Error feedback (optional).  residual_out[p] = d[p] - deq[p], one fp32 subtraction per element, with d including
 * the incoming residual; 0 in poisoned (s = 255) blocks.
 *
 * Reduce.  fp32, rounded to nearest, never fused; one thread owns a column through all rows, so no launch plan
 * changes a bit:
 *     chain[p] = FA_ACCUMULATE ? acc_in[p] : +0.0f;     chain[p] = chain[p] + deq_k[p]   for k in arrival order
 * A NaN in a chain is sticky, so a poisoned block of row k makes its 32 columns NaN from row k on: the result is the
 * one a NaN written at the end gives.
 */
#ifndef FEDQUANT4_H
#define FEDQUANT4_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FQ4_ABI_VERSION 1
#define FQ4_PLAN_FIELDS 6 /* int64 per launch of fq4_reduce_plan */
#define FQ4_BLOCK 32      /* columns that share one scale byte: 16 code bytes */
#define FQ4_SCALE_MIN 2   /* scale bytes outside [FQ4_SCALE_MIN, FQ4_SCALE_MAX] poison their block */
#define FQ4_SCALE_MAX 252

int32_t fq4_abi_version(void);

/*
 * The chain above over n rows of codes q4[k*(ld/2) + p/2] with scale bytes scales[k*lds + p/32], into out[0, P).
 *   q4      device memory, 16-byte aligned; ld (in columns) a multiple of 64, >= P.  Rows are read 16 bytes (32
 *           columns) per lane, up to 16 * ceil(P / 32) <= ld / 2 bytes of each row; codes in [P, ld) are never counted.
 *   scales  device memory, 16-byte aligned; lds >= ceil(P / 32).  Scale bytes past ceil(P / 32) are never read.
 *   acc_in  (FA_ACCUMULATE) >= round_up(P, 4) floats, 16-byte aligned; out may alias it.  n == 0 needs it.
 *   out     >= P floats, 16-byte aligned; written in [0, P) only (float4 stores, the last column masked at P).
 *   flags   0 or FA_ACCUMULATE.
 */
int fq4_reduce(const uint8_t* q4, const uint8_t* scales, int64_t ld, int64_t lds, int32_t n, int64_t P,
               const float* acc_in, float* out, int32_t flags, fa_stream_t stream);

/*
 * The launches fq4_reduce makes at (K, P) on a GPU of `cus` compute units (host only, no GPU needed):
 * plan_out[FQ4_PLAN_FIELDS*i + {0..5}] = {V, U, first column, tiles, strips per wave, grid} of launch i, for
 * i < min(cap, returned count), as fq_reduce_plan's (fedquant.h); a strip is 64 lanes x 32 columns.  Returns the
 * number of launches (>= 0) or FA_E_ARG.
 */
int64_t fq4_reduce_plan(int32_t cus, int32_t K, int64_t P, int64_t* plan_out, int32_t cap);

/*
 * The executor-side handler: one contiguous fp32 device row quantised as above,
 *     d[p] = (base ? x[p] - base[p] : x[p]) (+ residual[p])          p < P
 * into q4 (16 * ceil(P / 32) code bytes, the padding codes 0), scales (ceil(P / 32) bytes) and, when residual_out
 * is given, residual_out[0, P).  x, base, residual, residual_out and q4 are device memory, 16-byte aligned; the fp32
 * rows hold P floats; residual_out may be residual.  Stateless, no atomics, no host synchronisation.  The host-side
 * equivalent is fedscale_amd/cloud/execution/quant4_upload.py; both give the same bytes.
 */
int fq4_quantize_row(const float* x, const float* base, const float* residual, int64_t P, uint8_t* q4,
                     uint8_t* scales, float* residual_out, fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDQUANT4_H */
