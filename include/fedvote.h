/*
 * fedvote.h — C ABI of the majority-vote sign path on MI355X (gfx950): signSGD with majority vote (Bernstein, Zhao,
 * Azizzadenesheli, Anandkumar, ICLR 2019).  Every client uploads only the sign of its update, one bit per parameter
 * and nothing else; the server takes, per coordinate, the sign of the sum of signs (or the mean of the signs) and
 * moves the model by a server learning rate.  There are no scales: an upload of NaNs or of 1e30s has exactly one
 * vote per coordinate, like any other upload.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued).  The entry
 * points of this header are bound by fedscale_amd/_native_vote.py; the header has its own version
 * (fvt_abi_version), FA_ABI_VERSION is not touched by it.
 *
 * What is replaced (reference): nothing — the reference's executor uploads fp32 (torch_client.py:79-91) and its
 * aggregator chains fp32 (aggregator.py:489-511).
 *
 * The contract.  L is the fp32 bucket the executors were sent for the round (the float32 entries concatenated in
 * state_dict order, P columns), x_k client k's trained bucket, K the number of clients of the round.
 *
 * Upload.  Bit p is the fp32 sign bit of e = x_k[p] - L[p] (one fp32 subtraction), whatever e is: -0.0 and negative
 * NaNs vote "down".  A NaN that the subtraction propagates keeps its operand's sign everywhere; a NaN that it GENERATES
 * (inf - inf) has the platform's default sign — negative on x86 hosts, positive on gfx950 — so that one vote depends
 * on where the upload was encoded.  It is one vote either way.  Column p is bit p % 8 of byte p / 8 (sign1's order);
 * the row is ceil(P / 8) bytes and its padding bits are 0.  No scales, no residual, no non-finite special case;
 * client-side momentum or error feedback is the executor's business.
 *
 * Tally.  c[p] is the number of staged rows whose bit p is set, as a uint32.  It is exact, so it is independent of row
 * order, chunking and launch plan.  The vote margin is v[p] = K - 2 c[p].
 *
 * Finish.  All fp32, each operation rounded to nearest, never contracted, the division correctly rounded:
 *     FVT_MAJORITY   new[p] = L[p] + s,   s = +eta if v > 0, -eta if v < 0, +0.0f on a tie
 *     FVT_MEAN       new[p] = L[p] + fl(eta * fl(float(v) / float(K)))
 * K <= 2^24, so float(v) is exact.  eta is a positive finite float32.
 *
 * Staging rows.  bits is [capacity, ldb] bytes, 16-byte aligned, ldb = round_up(ceil(P / 8), 16).
 */
#ifndef FEDVOTE_H
#define FEDVOTE_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FVT_ABI_VERSION 1
#define FVT_PLAN_FIELDS 7   /* int64 per launch of fvt_count_plan */
#define FVT_MAX_ROWS 65535  /* rows per fvt_count call */
#define FVT_MAX_CLIENTS (1 << 24)
#define FVT_MAJORITY 0
#define FVT_MEAN 1

int32_t fvt_abi_version(void);

/*
 * cnt[p] <- (FA_ACCUMULATE: cnt[p] +) the number of rows k < n whose bit p is set (bit p % 8 of bits[k*ldb + p/8]),
 * for p < P.
 *   bits   device memory, 16-byte aligned; ldb (bytes) a multiple of 16, >= ceil(P / 8).  Rows are read one dword
 *          (32 columns) per lane, up to 4 * ceil(P / 32) <= ldb bytes of each row; bits of columns >= P are never
 *          counted.
 *   n      0 <= n <= FVT_MAX_ROWS.  n == 0 without FA_ACCUMULATE writes zeros.
 *   cnt    >= P uint32, 16-byte aligned; read (FA_ACCUMULATE) and written in [0, P) only.
 *   flags  0 or FA_ACCUMULATE.
 * When the column tiles do not fill the GPU the rows are split over S workgroups per tile (fvt_count_plan), whose
 * partial counts meet in cnt by integer atomic adds (cnt is zeroed on the stream first when not accumulating):
 * integer sums are exact in any order, so the result is the unsplit one bit for bit.
 */
int fvt_count(const uint8_t* bits, int64_t ldb, int32_t n, int64_t P, uint32_t* cnt, int32_t flags,
              fa_stream_t stream);

/*
 * The launches fvt_count makes at (n, P) on a GPU of `cus` compute units (host only, no GPU needed):
 * plan_out[FVT_PLAN_FIELDS*i + {0..6}] = {V, U, first column, tiles, strips per wave, grid, S} of launch i, for
 * i < min(cap, returned count).  The first six are fsg_reduce_plan's (fedsign.h; a strip is 64 lanes x 32 columns,
 * grid counts column workgroups); S is the number of workgroups that share one tile's rows, the same for every launch
 * of a plan and a function of (cus, n, P) alone.  The launch runs grid * S workgroups.  Returns the number of launches
 * (>= 0) or FA_E_ARG.
 */
int64_t fvt_count_plan(int32_t cus, int32_t n, int64_t P, int64_t* plan_out, int32_t cap);

/*
 * The finish above in one streaming pass, 12 bytes per column: out[p] (and mirror[p], when given: device or pinned
 * host memory) from cnt[p] and L[p], p < P.  cnt, L, out and mirror are 16-byte aligned and hold >= P elements; out
 * may alias L.  1 <= K <= FVT_MAX_CLIENTS; a count above K is the caller's error and is not detected.  mode is
 * FVT_MAJORITY or FVT_MEAN.
 */
int fvt_finish(const uint32_t* cnt, const float* L, int64_t P, int32_t K, float eta, int32_t mode, float* out,
               float* mirror, fa_stream_t stream);

/*
 * The executor-side encoder: bits[0, ceil(P / 8)) <- the sign bits of x[p] - base[p] (base == NULL: of x[p]), the
 * padding bits of the last byte 0.  x and base are device memory of P floats, 4-byte aligned; bits is device memory
 * of ceil(P / 8) bytes, any alignment.  One launch, stateless, no atomics, no host synchronisation.  The host-side
 * equivalent is fedscale_amd/cloud/execution/vote_upload.py; both give the same bytes, except the bit of a NaN that
 * the subtraction generates (inf - inf; see Upload above).
 */
int fvt_sign_row(const float* x, const float* base, int64_t P, uint8_t* bits, fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDVOTE_H */
