/*
 * fedrotate.h — C ABI of the randomised block Hadamard rotation around the 1-bit sign delta-upload path on MI355X
 * (gfx950): the executor rotates its update y = H D e / 64 per block of 4096 columns before fsg_sign_row
 * (fedsign.h) encodes it, and the aggregator rotates the round's fp32 chain back once before fcl_finish (fedclip.h)
 * closes the round.  After the rotation every block looks Gaussian to the sign encoder whatever the model produced
 * (Suresh et al., ICML 2017; DRIVE, Vargaftik et al., NeurIPS 2021); the rotation is orthonormal, so the error in
 * rotated space is the error in parameter space, and linear, so the aggregator's chain runs over rotated rows
 * unchanged.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless, no
 * atomics, the call's GPU taken from its stream or its output, every operand checked before anything is queued).
 * The entry points of this header are bound by fedscale_amd/_native_rotate.py; the header has its own version
 * (frt_abi_version), FA_ABI_VERSION and FSG_ABI_VERSION are not touched by it.
 *
 * What is replaced (reference): nothing — the reference's executor uploads fp32 and its aggregator chains fp32.
 *
 * The contract.  The bucket is the float32 entries concatenated in state_dict order, P columns, as in fedsign.h.
 * P' = round_up(P, 4096).  Block b covers columns [4096b, 4096b + 4096).  Columns >= P of the last block are
 * padding.
 *
 * Diagonal.  Given by a 64-bit seed and the column p (splitmix64 over the 64-column word w; all arithmetic mod 2^64):
 *     w = p >> 6
 *     z = seed + (w + 1) * 0x9E3779B97F4A7C15
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z ^= z >> 31
 *     d[p] = (z >> (p & 63)) & 1
 * Seed 0 gives z(0..3) = e220a8397b1dcdaf, 6e789e6aa1b965f4, 06c45d188009454f, f88bb8a8724c81ec.  Applying the
 * diagonal is an xor of d[p] into the fp32 sign bit.  It is applied to every column of the padded block, padding
 * included.
 *
 * Forward transform, y = frt_rotate(x, base, P, seed):
 *   1. e[p] = base ? x[p] - base[p] : x[p] for p < P, one fp32 rounding.
 *   2. Padding is +0.0.
 *   3. The sign-bit xor.
 *   4. Twelve butterfly stages in the order h = 1, 2, 4, ..., 2048.  For every index i of the block with
 *      (i & h) == 0 the pair (a, b) = (v[i], v[i + h]) becomes (a + b, a - b).  Each result is one fp32 add or
 *      subtract, rounded to nearest and never fused.  The difference is lower minus upper, not a negated upper minus
 *      lower: the two differ in the sign of zero, and the sign encoder reads that bit.
 *   5. One multiply by 2^-6.
 *   6. All P' columns are written.
 * The stage order is part of the contract, because another order rounds differently.  Within a stage any schedule
 * gives the same bits.
 *
 * Inverse transform, frt_unrotate(y, P, seed): the same twelve stages over the P' columns, the multiply by 2^-6,
 * the sign-bit xor; columns [0, P) only are written.  out may alias y: a block is read whole before any of it is
 * written.
 *
 * What holds exactly.  For integer-valued inputs with |x| <= 2047 every intermediate sum is an exactly representable
 * integer; the forward result then equals the float64 matrix product H D x / 64 bit for bit, and the round trip
 * returns x bit for bit — but for a zero column, which comes back as +0.0 xor d[p].  For general fp32 input the round trip is exact only to rounding (about 7e-7 on unit
 * Gaussians).  The default denormal modes are kept: subnormal inputs, sums and results survive.
 *
 * Non-finite values.  A NaN or an infinity makes every column of its 4096-column block non-finite after the
 * transform: NaN, or for a lone infinity +-inf (two infinities meet in a difference and give NaN).  All 16 of its
 * sign blocks then get fsg_sign_row's NaN scale.  The inverse makes exactly that block of the new model NaN, and no
 * other: no value crosses a block.
 */
#ifndef FEDROTATE_H
#define FEDROTATE_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FRT_ABI_VERSION 1
#define FRT_BLOCK 4096 /* columns of one Hadamard block */

int32_t frt_abi_version(void);

/* P' = round_up(P, FRT_BLOCK) (host only, no GPU needed); FA_E_ARG for a negative P. */
int64_t frt_padded(int64_t P);

/*
 * The forward transform above.
 *   x     device memory of P floats, 4-byte aligned.
 *   base  NULL, or device memory of P floats, 4-byte aligned.
 *   y     device memory of frt_padded(P) floats, 16-byte aligned; all of it is written.  y must not overlap x or
 *         base.
 * P == 0 queues nothing.  Refused (FA_E_ARG, nothing launched): a negative P, a NULL x or y, misalignment.
 */
int frt_rotate(const float* x, const float* base, int64_t P, uint64_t seed, float* y, fa_stream_t stream);

/*
 * The inverse transform above.
 *   y    device memory of frt_padded(P) floats, 16-byte aligned.
 *   out  device memory of P floats, 16-byte aligned; written in [0, P) only.  out may be y.
 * P == 0 queues nothing.  Refused (FA_E_ARG, nothing launched): a negative P, a NULL y or out, misalignment.
 */
int frt_unrotate(const float* y, int64_t P, uint64_t seed, float* out, fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDROTATE_H */
