/*
 * fedsketch.h — C ABI of the Count-Sketch upload path on MI355X (gfx950): FetchSGD rounds (Rothchild et al., ICML
 * 2020).  A client uploads a Count Sketch of its update e = x - L — R x C floats whatever the model's size — the
 * server sums the sketches like dense rows (fa_reduce, fedagg.h), keeps momentum and error feedback in sketch space,
 * and applies only the heavy columns it recovers from the error sketch.  Clients keep no state between rounds.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued).  The entry
 * points of this header are bound by fedscale_amd/_native_sketch.py; the header has its own version
 * (fcs_abi_version), no other header's version is touched by it.
 *
 * What is replaced (reference): nothing — the reference's executor uploads dense fp32 and its aggregator chains
 * dense fp32.
 *
 * The contract: a BLOCKED Count Sketch.  The bucket is the fp32 entries concatenated in state_dict order, P columns,
 * P <= 2^31 - 1.  R in {1, 3, 5, 7} rows, C = 2^c columns with 10 <= c <= 24, a 64-bit seed, NB = ceil(P / C).
 * Column p has block b = p >> c and offset u = p & (C - 1).  A bucket receives exactly one column of each block and
 * sums them in ascending block order, so a table is a pure function of (x, seed, R, C): no atomics, no launch plan
 * changes a bit.  Two columns collide in a row with probability 1/C, independently across rows; two columns of one
 * block never collide.
 *
 * Hash.  mix(s, w) is the splitmix64 of fedrotate.h; all arithmetic mod 2^64:
 *     z = s + (w + 1) * 0x9E3779B97F4A7C15
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z ^= z >> 31
 * With G = 0xD1B54A32D192ED03:
 *     sign of column p in row j    sigma_j(p) = (mix(seed + (2j + 1) G, p >> 6) >> (p & 63)) & 1, xored into the fp32
 *                                  sign bit: one 64-bit word serves 64 columns
 *     mask of block b in row j     m_jb = mix(seed + (2j + 2) G, b) & (C - 1)
 *     bucket of column p in row j  q = u ^ m_jb
 * Seed 0, row 0: the sign words of w = 0..3 are 2d0f28c7e7e786b2, 75856f745165f252, 8674bbc2735955af,
 * 5c1d49a70d26949a; the mask words of b = 0..3 (before the & (C - 1)) are 3c5b66874b9e8a84, 5a1e518fcfcf0d64,
 * 1a215e1f9abe2521, eb0adee8a2cbe4a4.
 *
 * Sketch, T = fcs_sketch_row(x, base, r_in, P, R, C, seed), T fp32 [R, C]:
 *     e[p] = base ? x[p] - base[p] : x[p], one fp32 rounding; with r_in, + r_in[p] as a second unfused add
 *     T[j][q] = (((+0.0 + t_0) + t_1) + ... + t_{NB-1}),  t_b = e[p] ^ (sigma_j(p) << 31),  p = b C + (q ^ m_jb)
 * A block whose p >= P contributes no term (not an added zero).  fp32 adds, rounded to nearest, never fused.  Every
 * one of the R C buckets is written.  With FCS_SUBTRACT_FROM the table is updated in place instead:
 * T[j][q] = T[j][q] - (the chain above), one unfused subtract per bucket.
 *
 * Estimate, est = fcs_estimate(T, P, R, C, seed), est fp32 [P]:
 *     v_j = T[j][u ^ m_jb] ^ (sigma_j(p) << 31)                                  j < R
 *     key(v) = bits(v) ^ (sign(v) ? 0xFFFFFFFF : 0x80000000), compared as uint32
 * which orders -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN with no special case; est[p] is the value whose key is
 * the median of the R keys (R = 1: the value itself).
 *
 * Server state and the round (FetchSGD Alg. 1 with updates x - L in place of gradients, so the step adds).  State:
 * S_u, S_e, fp32 [R, C], zero at the first round.  Per round, over K uploaded tables in arrival order:
 *     1. S = fa_reduce(tables, a = NULL, denom = K, FA_FINALIZE), rows of R C floats
 *     2. fcs_state_step: S_u = rho S_u + S (a multiply, then an add, unfused)
 *     3.                 S_e = S_e + S_u
 *     4. est = fcs_estimate(S_e)
 *     5. (idx, val) = the top-k selection of fedsparse.h over est (no base, no residual): its selection and tie
 *        rules hold
 *     6. fcs_apply: Delta = the dense vector with Delta[idx] = val and +0.0 elsewhere,
 *     7.            L_new[idx] = L[idx] + val; a column not named keeps L's bits
 *     8. S_e = S_e - fcs_sketch_row(Delta), one unfused subtract per bucket (FCS_SUBTRACT_FROM)
 *
 * Non-finite values.  A NaN or an infinity in an update poisons its R buckets and whatever hashes to them, nothing
 * else.  fcs_state_step counts the non-finite entries of S into a device counter (integer atomics, order-free); a
 * round with a non-zero count is refused by its caller before S_u, S_e or the model change (the step writes its
 * results to buffers of the caller's choice, so the old state is still there).
 */
#ifndef FEDSKETCH_H
#define FEDSKETCH_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FCS_ABI_VERSION 1
#define FCS_PLAN_FIELDS 4     /* int64 of fcs_sketch_plan */
#define FCS_TILE 1024         /* the largest bucket tile of a workgroup: 4 waves x 4 buckets per lane */
#define FCS_U 8               /* blocks whose loads a lane keeps in flight ahead of their dependent adds */
#define FCS_SUBTRACT_FROM 1   /* fcs_sketch_row: table = table - sketch, in place */

int32_t fcs_abi_version(void);

/* R * C, the floats of one table (host only); FA_E_ARG unless R is 1, 3, 5 or 7 and C = 2^c with 10 <= c <= 24. */
int64_t fcs_table_floats(int32_t R, int64_t C);

/*
 * The launch fcs_sketch_row makes at (P, R, C) on a GPU of `cus` compute units (host only, no GPU needed):
 * plan_out[0..3] = {bucket tile of a workgroup, blocks in flight (FCS_U), blocks NB, grid}.  A workgroup owns one
 * row and one aligned tile of buckets and walks all NB blocks: the chain never splits over blocks.  The tile is
 * FCS_TILE, halved down to 256 (one wave x 4 buckets per lane) while R * C / tile workgroups do not fill the card.
 * Returns 1, or FA_E_ARG.
 */
int64_t fcs_sketch_plan(int32_t cus, int64_t P, int32_t R, int64_t C, int64_t* plan_out);

/*
 * The sketch above of one contiguous fp32 device row.
 *   x, base, r_in  device memory of P floats each, 16-byte aligned (base and r_in may be NULL).  No float past P is
 *                  read.
 *   table          device memory of R * C floats, 16-byte aligned; all of it is written.  It must not overlap x,
 *                  base or r_in.
 *   tile           0: the plan's tile; 256, 512 or 1024: that tile (every tile gives the same bits).
 *   flags          0 or FCS_SUBTRACT_FROM.
 * P == 0 writes +0.0 to every bucket (or, with FCS_SUBTRACT_FROM, subtracts it).  Refused (FA_E_ARG, nothing launched):
 * a negative P, P > 2^31 - 1, an R or C outside the contract, a NULL x (P > 0) or table, misalignment, another tile.
 */
int fcs_sketch_row(const float* x, const float* base, const float* r_in, int64_t P, int32_t R, int64_t C,
                   uint64_t seed, float* table, int32_t tile, int32_t flags, fa_stream_t stream);

/*
 * The estimate above.  table: R * C floats, 16-byte aligned; est: P floats, 16-byte aligned, written in [0, P) only
 * (float4 stores, the last one masked at P).  est must not overlap table.  P == 0 queues nothing.
 */
int fcs_estimate(const float* table, int64_t P, int32_t R, int64_t C, uint64_t seed, float* est, fa_stream_t stream);

/*
 * Steps 2 and 3 over n floats (n = R * C, a multiple of 4):
 *     su_out[i] = rho * su_in[i] + s[i]      (multiply, then add)
 *     se_out[i] = se_in[i] + su_out[i]
 *     *nonfinite += the entries of s that are NaN or +-inf   (device uint32; the caller clears it)
 * Everything is device memory, 16-byte aligned (nonfinite: 4-byte).  su_out may be su_in and se_out may be se_in; no
 * other overlap.
 */
int fcs_state_step(const float* s, const float* su_in, const float* se_in, float rho, int64_t n, float* su_out,
                   float* se_out, uint32_t* nonfinite, fa_stream_t stream);

/*
 * Steps 6 and 7 over k pairs (idx uint32, val float, device memory, 4-byte aligned; idx values unique, as the
 * selection of fedsparse.h writes them — a value >= P is skipped, so the kernel is memory-safe whatever it is fed):
 *     dense[0, P) = +0.0, then dense[idx[i]] = val[i]
 *     l_out[0, P) = l_in[0, P) when l_out != l_in, then l_out[idx[i]] = l_in[idx[i]] + val[i]
 * dense, l_in, l_out: P floats, 16-byte aligned; dense overlaps neither model buffer.  No atomics.
 */
int fcs_apply(const uint32_t* idx, const float* val, int64_t k, int64_t P, float* dense, const float* l_in,
              float* l_out, fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDSKETCH_H */
