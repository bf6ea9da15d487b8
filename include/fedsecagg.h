/*
 * fedsecagg.h — C ABI of the secure-aggregation data path on MI355X (gfx950): client updates d = x - L encoded as
 * fixed-point integers mod 2^32 and hidden under pseudorandom masks (Bonawitz et al., CCS 2017; Bell et al., CCS
 * 2020), staged in HBM at 4 bytes per parameter, summed mod 2^32 and unmasked on the device.  The masks cancel in the
 * sum: the server's arithmetic never sees an individual update.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued).  The entry
 * points of this header are bound by fedscale_amd/_native_secagg.py; the header has its own version
 * (fsa_abi_version), FA_ABI_VERSION is not touched by it.
 *
 * What is replaced (reference): nothing — the reference has no secure aggregation.  Key agreement, secret sharing,
 * dropout recovery and authenticated channels are NOT here: the caller supplies the 256-bit keys and decides which
 * are added and which subtracted ("Secure aggregation").
 *
 * Arithmetic.  The bucket is the fp32 entries concatenated in state_dict order, P columns.  int64 entries (counters)
 * travel and reduce exactly as in a plain round, unmasked.  All integer arithmetic is mod 2^32, so no launch plan
 * and no order of the rows changes a bit.
 *
 * Spec.  f = frac_bits in [0, 30], b = mag_bits in [1, 30], B = 2^b - 1.  A round of K uploads needs
 * K * B <= 2^31 - 1 (the caller checks it).
 *
 * Encode (one rounding per element).  d = x[p] - L[p] in fp32, unfused; t = d * 2^f in fp32 (exact, or +-inf);
 * r = rint(t), ties to even; q[p] = (int32) clamp((double) r, -B, B), as a uint32 word; a NaN encodes as 0.
 * -0 and values that round to 0 encode as 0.  stats[0] counts the elements the clamp changed (|r| > B, +-inf
 * included), stats[1] the NaNs.
 *
 * Mask stream.  PRG(key, nonce, c), the mask word of stream column c, is word (c mod 16) of the ChaCha20 block
 * function of RFC 8439 section 2.3 with key = eight uint32 words, nonce = three uint32 words and the 32-bit block
 * counter c div 16; the word is taken after the final add, as a uint32.  Every call names its first stream column
 * col0, a multiple of 16 with col0 + P <= 2^36; column p of the call is stream column col0 + p.
 *
 * Mask sum.  out[p] = acc_in[p] + sum_{m < n_add} PRG(key_m, nonce, col0 + p)
 *                               - sum_{n_add <= m < n_add + n_sub} PRG(key_m, nonce, col0 + p)     (mod 2^32)
 * A client's upload is y = q + PRG(self key) +- PRG(pair keys); the server's unmask is the same call over the
 * accumulated sum with the signs that cancel what the arrived clients applied.
 *
 * Reduce.  sum[p] = (FA_ACCUMULATE ? acc_in[p] : 0) + sum_k y_k[p]   (mod 2^32).
 *
 * Finish.  s = (int32) sum[p]; m = (float)(((double) s * 2^-f) / (double) n), n the number of arrivals;
 * out[p] = L[p] + m in fp32, unfused.  out_of_range[0] = the number of columns with |s| > n * B: a correct unmask
 * never leaves [-nB, nB], and with a wrong or missing key a column is uniform, so it is out of range with
 * probability 1 - (2nB + 1) / 2^32.
 */
#ifndef FEDSECAGG_H
#define FEDSECAGG_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FSA_ABI_VERSION 1
#define FSA_PLAN_FIELDS 6        /* int64 per launch of fsa_reduce_plan */
#define FSA_MAX_KEYS (1 << 20)   /* n_add + n_sub of one fsa_mask_sum call */
#define FSA_MAX_FRAC_BITS 30
#define FSA_MAX_MAG_BITS 30
#define FSA_MASK_TILE 4096       /* columns one workgroup of fsa_mask_sum covers per sweep: 256 lanes x 16 columns */
#define FSA_MASK_GRID_PER_CU 8   /* its grid is at most this many workgroups per compute unit */

int32_t fsa_abi_version(void);

/*
 * The executor-side encoder: one contiguous fp32 device row into fixed-point words,
 *     d[p] = base ? x[p] - base[p] : x[p]          p < P
 * encoded as above into out_u32[0, P).  x, base and out_u32 are device memory, 16-byte aligned, P elements each.
 * stats: two device int64, 8-byte aligned; the call sets them to (n_clamped, n_nan) — cleared on the stream, then
 * counted with integer vector atomics (any order gives the same value).  Nothing outside [0, P) is written.
 */
int fsa_encode_row(const float* x, const float* base, int64_t P, int32_t frac_bits, int32_t mag_bits,
                   uint32_t* out_u32, int64_t* stats, fa_stream_t stream);

/*
 * The mask sum above.
 *   keys    device memory, uint32[(n_add + n_sub) * 8], 4-byte aligned; the first n_add keys are added, the rest
 *           subtracted.  n_add + n_sub <= FSA_MAX_KEYS; with no key at all the call is a copy and keys may be NULL.
 *   col0    a multiple of 16, col0 + P <= 2^36 (FA_E_ARG otherwise).
 *   acc_in  P uint32, 16-byte aligned; read in [0, P) only.
 *   out     P uint32, 16-byte aligned; may alias acc_in (the SAME pointer; a partial overlap is refused); written in
 *           [0, P) only.
 * One ChaCha20 block (16 columns) per lane and key; a lane keeps its 16 words of the sum in registers across all
 * keys, so acc_in / out traffic is 8 bytes per column per call.  A workgroup covers FSA_MASK_TILE columns per sweep,
 * on a grid of at most FSA_MASK_GRID_PER_CU workgroups per compute unit; the last, partial block is masked.
 */
int fsa_mask_sum(const uint32_t* keys, int32_t n_add, int32_t n_sub, uint32_t nonce0, uint32_t nonce1, uint32_t nonce2,
                 int64_t col0, int64_t P, const uint32_t* acc_in, uint32_t* out, fa_stream_t stream);

/*
 * The modular sum above over n rows y[k*ld + p] into out[0, P).
 *   y       device memory, 16-byte aligned; ld a multiple of 64, >= P.  Rows are read 16 bytes (4 columns) per lane,
 *           up to round_up(P, 4) <= ld words of each row; words in [P, ld) are never counted.
 *   acc_in  (FA_ACCUMULATE) >= round_up(P, 4) uint32, 16-byte aligned; out may alias it.  n == 0 needs it.
 *   out     >= P uint32, 16-byte aligned; written in [0, P) only (16-byte stores, the last one masked at P).
 *   flags   0 or FA_ACCUMULATE.
 */
int fsa_reduce(const uint32_t* y, int64_t ld, int32_t n, int64_t P, const uint32_t* acc_in, uint32_t* out,
               int32_t flags, fa_stream_t stream);

/*
 * The launches fsa_reduce makes at (K, P) on a GPU of `cus` compute units (host only, no GPU needed):
 * plan_out[FSA_PLAN_FIELDS*i + {0..5}] = {V, U, first column, tiles, strips per wave, grid} of launch i, for
 * i < min(cap, returned count), as fcl_reduce_plan's (fedclip.h); a strip is 64 lanes x 4 columns.  Returns the
 * number of launches (>= 0) or FA_E_ARG.
 */
int64_t fsa_reduce_plan(int32_t cus, int32_t K, int64_t P, int64_t* plan_out, int32_t cap);

/*
 * The finish above: out[0, P) from the unmasked sum and the round's starting model `last`.
 *   sum, last  device memory, 16-byte aligned, >= round_up(P, 4) elements.
 *   n          arrivals, >= 1, with n * (2^mag_bits - 1) <= 2^31 - 1.
 *   out        device memory, P floats, 16-byte aligned; written in [0, P) only.
 *   mirror     optional (NULL: none): pinned host memory or device memory, P floats, 16-byte aligned; gets the same
 *              values as out, as fcl_finish's mirror.
 *   out_of_range  one device int64, 8-byte aligned: set to the number of columns with |s| > n * B — cleared on the
 *              stream, then counted with integer vector atomics.
 */
int fsa_finish(const uint32_t* sum, const float* last, int64_t P, int32_t frac_bits, int32_t mag_bits, int32_t n,
               float* out, float* mirror, int64_t* out_of_range, fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDSECAGG_H */
