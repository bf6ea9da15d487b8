/*
 * fedlowrank.h — C ABI of the low-rank delta-upload path on MI355X (gfx950): client updates sent as two thin factors
 * per weight matrix (PowerSGD, Vogels et al. 2019; the stacked B·A aggregation of federated LoRA), staged as fp32
 * factor rows and multiplied out onto the chain by the fp32 matrix unit (v_mfma_f32_32x32x2_f32).
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued).  The entry
 * points of this header are bound by fedscale_amd/_native_lowrank.py; the header has its own version
 * (flr_abi_version), FA_ABI_VERSION is not touched by it.
 *
 * What is replaced (reference): nothing — the reference's executor uploads dense fp32 and its aggregator chains dense
 * fp32.  The round is closed by fcl_finish (fedclip.h): L + chain / K.
 *
 * Entries.  The bucket is the layout's fp32 entries in state_dict order, P floats, entry offsets packed (no
 * alignment).  The caller describes entry e by dims[2e], dims[2e + 1]:
 *     (O, I) with I >= 1   a FACTORED entry of shape (O, *rest), I = prod(rest), O * I floats of the chain;
 *     (numel, 0)           a DENSE entry of numel floats.
 * Which entries are factored at a rank is the caller's rule (lowrank_upload.factored: len(shape) >= 2,
 * min(O, I) > r, r * (O + I) < O * I); the library takes any (O, I) with O, I >= 1.  1 <= rank <= FLR_MAX_RANK.
 *
 * The staged row.  One fp32 row per client, row stride ldf (a multiple of 64 floats), entries in order, each
 * starting 16-byte aligned (flr_row_layout gives the offsets):
 *     factored   Ut [r2, O4], then V [r2, I4]        r2 = round_up(r, 2), O4 = round_up(O, 4), I4 = round_up(I, 4)
 *     dense      numel floats
 * Ut[j, o] and V[j, i] are the factors of the entry's delta d[o, i] = sum_j Ut[j, o] * V[j, i].  Padding rows and
 * columns hold +0.0f: the staging is zero-filled once and padding is never written.
 *
 * Reduce.  For a factored entry, every output element (o, i) takes
 *     acc = FA_ACCUMULATE ? acc_in[off + o * I + i] : +0.0f
 * and then the staged inner index (k, j), k the arrival order and j < r2, in strictly ascending order, two
 * consecutive inner indices per matrix instruction:  acc = mfma(V[j..j+1, i], Ut[j..j+1, o], acc).  Nothing splits
 * the inner dimension and one wave owns an output element through all n * r2 terms, so the bits of an output element
 * are a function of the data alone: not of the tile shape, the tile table, the CU count or how the round was chunked
 * (a chunk boundary falls on a multiple of r2, which is even).
 * For a dense entry: chain[p] = chain[p] + d_k[p] in arrival order, fp32, unfused, starting from acc_in[p] or +0.0f.
 *
 * What the contract does NOT fix: how the matrix unit rounds inside one instruction (whether the two products are
 * rounded before they are added, and in which order the two are added to the accumulator) and how it treats
 * subnormal operands and results.  DESIGN.md states what was observed on the card; the tests assert exactness on
 * integer data and the any-order error bound elsewhere.
 */
#ifndef FEDLOWRANK_H
#define FEDLOWRANK_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLR_ABI_VERSION 1
#define FLR_MAX_RANK 64
#define FLR_PLAN_FIELDS 4 /* int64 per entry of flr_reduce_plan */
#define FLR_DEPTH 8       /* staged inner rows of one LDS stage: a compile-time constant */
#define FLR_DENSE_COLS 256 /* columns of a dense tile */

/* kinds of a tile (and of an entry's tiles) */
#define FLR_KIND_DENSE 0
#define FLR_KIND_SMALL 1 /* 64 x 64 outputs */
#define FLR_KIND_LARGE 2 /* 128 x 128 outputs */

/*
 * The tile table, as flr_reduce_table writes it and flr_reduce's kernel reads it: a head, one flr_entry_t per
 * entry, one flr_tile_t per workgroup.  Tiles are ordered large, small, dense (the longest first); within a kind by
 * entry, tile row, tile column; an entry's tiles are contiguous from first_tile.
 */
typedef struct {
  int32_t magic, rank, r2, n_entries;
  int64_t n_tiles, ldf, P, row_floats; /* row_floats: the floats of a staged row that are in use (<= ldf) */
  int64_t reserved[2];
} flr_head_t; /* 64 bytes */
typedef struct {
  int64_t chain_off, ut_off, v_off; /* floats; a dense entry's staged offset is ut_off */
  int32_t O, I, O4, I4;             /* a dense entry: O = numel, the rest 0 */
  int32_t kind, tile, ntr, ntc;     /* tile: rows = columns of one tile (dense: FLR_DENSE_COLS columns, ntr = 1) */
  int64_t first_tile;
} flr_entry_t; /* 64 bytes */
typedef struct {
  int32_t entry, tr, tc, kind;
} flr_tile_t; /* 16 bytes */

int32_t flr_abi_version(void);

/*
 * The staged offsets above (host only): off_out[2e] = the entry's first float in a staged row (Ut, or the dense
 * values), off_out[2e + 1] = its V (0 for a dense entry).  Returns ldf, the row stride in floats (a multiple of 64,
 * at least 64), or FA_E_ARG (a rank outside 1..FLR_MAX_RANK, a negative dimension), FA_E_RANGE (P or a row beyond
 * 2^31 - 1 floats).  off_out may be NULL.
 */
int64_t flr_row_layout(int32_t rank, int32_t n_entries, const int64_t* dims, int64_t* off_out);

/*
 * The tile table's summary at `cus` compute units (host only): plan_out[FLR_PLAN_FIELDS * e + {0..3}] = {kind, tile
 * size, tile count, first table row} of entry e.  force_tile: 0 = the plan's own choice (the large tile for every
 * factored entry when together they give at least `cus` large tiles, the small one otherwise); 64 or 128 = that tile
 * for every factored entry (tests and measurements: no bit of the result depends on it).  Returns the number of
 * tiles = workgroups of the one launch, or FA_E_ARG / FA_E_RANGE.  plan_out may be NULL.
 */
int64_t flr_reduce_plan(int32_t cus, int32_t rank, int32_t n_entries, const int64_t* dims, int32_t force_tile,
                        int64_t* plan_out);

/*
 * The whole table into table_out (host memory, cap_bytes available).  Returns its size in bytes (a multiple of 16);
 * nothing is written when table_out is NULL or cap_bytes is smaller.
 */
int64_t flr_reduce_table(int32_t cus, int32_t rank, int32_t n_entries, const int64_t* dims, int32_t force_tile,
                         void* table_out, int64_t cap_bytes);

/*
 * The reduce above over n staged rows, one launch.
 *   staged, ldf    device fp32 [n, ldf], 16-byte aligned; ldf as flr_row_layout returns it.
 *   dims           host, as above.
 *   table_dev      the table on the device (16-byte aligned), a copy of table_host.
 *   table_host     the table flr_reduce_table wrote for (the device's CU count, rank, dims, force_tile); compared
 *                  byte for byte with the table of this call's shapes, FA_E_ARG when they differ.
 *   acc_in         (FA_ACCUMULATE) P floats, 16-byte aligned; out may alias it.  n == 0 needs it.
 *   out            P floats, 16-byte aligned; written in [0, P) only.
 *   flags          0 or FA_ACCUMULATE.
 * No scratch, no atomics, no host synchronisation.
 */
int flr_reduce(const float* staged, int64_t ldf, int32_t n, int32_t rank, int32_t n_entries, const int64_t* dims,
               int32_t force_tile, const void* table_dev, const void* table_host, int64_t table_bytes,
               const float* acc_in, float* out, int32_t flags, fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDLOWRANK_H */
