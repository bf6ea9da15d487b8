/*
 * fedsparse.h — C ABI of the top-k sparse delta-upload path on MI355X (gfx950): client updates e = x - L (plus an
 * optional error-feedback residual) sparsified on the executor to their k largest magnitudes, uploaded and staged as
 * (index, value) rows of 8 bytes per kept entry, and chained in fp32 on the device.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued).  The entry
 * points of this header are bound by fedscale_amd/_native_sparse.py; the header has its own version
 * (fs_abi_version), FA_ABI_VERSION is not touched by it.
 *
 * What is replaced (reference): nothing — the reference's executor uploads dense fp32 (torch_client.py:79-91) and
 * its aggregator chains dense fp32 (aggregator.py:489-511).  The round is closed by fcl_finish (fedclip.h):
 * L + chain / K.
 *
 * The contract.  The bucket is the fp32 entries concatenated in state_dict order, P columns.  A sparse row is nnz
 * pairs (idx[j], val[j]): idx uint32, strictly increasing, every value below P; val float32; the two are separate
 * arrays.  Non-fp32 entries (the int64 side table) travel dense and reduce as in the other rounds.
 *
 * Select (executor side).  e[p] = x[p] - base[p] in fp32, unfused; with a residual, + r_in[p] as a second unfused
 * add.  key[p] = the bits of e[p] with the sign cleared, compared as uint32 — so NaN > inf > finite, and +-0 is
 * lowest.  With k = min(k, P), tau = the k-th largest key: every column whose key exceeds tau is kept, and among the
 * columns with key == tau the lowest-indexed ones, until k columns are kept.  The kept columns are output in
 * increasing index order with val = e[idx], unrounded.  If a residual output is asked for, r_out[p] = e[p] for a
 * dropped column and +0.0f for a kept one: the densified upload and r_out together hold every bit of e.
 *
 * Reduce (aggregator side).  fp32, rounded to nearest, never fused; one owner per column through all rows, so no
 * launch plan changes a bit:
 *     chain[p] = FA_ACCUMULATE ? acc_in[p] : +0.0f
 *     for rows in arrival order, for each pair of the row:  chain[idx] = chain[idx] + val
 *     out[0, P) = chain
 * A column a row does not name is not touched by that row: it does not receive an added zero (a -0 in acc_in stays
 * -0).  A row whose flag is non-zero is skipped whole.
 */
#ifndef FEDSPARSE_H
#define FEDSPARSE_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_ABI_VERSION 1
#define FS_PLAN_FIELDS 6 /* int64 per launch of fs_reduce_plan */
#define FS_TILE 4096     /* columns of one tile: a compile-time constant, never a function of the GPU */

int32_t fs_abi_version(void);

/*
 * Staged rows.  idx (uint32) and val (float) are [rows, ldk] device arrays, 16-byte aligned, ldk a multiple of 4
 * (at most 2^30); nnz is a device int32 array, one count per row.  A count outside [0, ldk] cannot be checked on the
 * host without a synchronisation: every kernel reads min(max(nnz, 0), ldk) pairs of the row at most, and
 * fs_check_rows flags it.  P <= 2^31 - 1 throughout.
 *
 * fs_row_offsets: for each row k < n and each boundary b <= ceil(P / FS_TILE), offsets[b * ldo + k] = the position
 * in the row of the first index >= b * FS_TILE (a binary search, one thread per (row, boundary)); ldo >= n.  The
 * offsets depend on the row alone.  offsets: device int32, (ceil(P / FS_TILE) + 1) * ldo entries.
 */
int fs_row_offsets(const uint32_t* idx, int64_t ldk, const int32_t* nnz, int32_t n, int64_t P, int32_t* offsets,
                   int64_t ldo, fa_stream_t stream);

/*
 * flags[k] (device int32, k < n) = non-zero when row k's indices are not strictly increasing, one of them is >= P,
 * or its count is outside [0, ldk]; 0 otherwise.  Streams idx once.  n <= 65535 rows per call (FA_E_RANGE beyond).
 */
int fs_check_rows(const uint32_t* idx, int64_t ldk, const int32_t* nnz, int32_t n, int64_t P, int32_t* flags,
                  fa_stream_t stream);

/*
 * The chain above over n staged rows into out[0, P).
 *   offsets, ldo   as fs_row_offsets wrote them for these rows.
 *   row_flags      device int32 [n] (fs_check_rows, or the caller's): a row with a non-zero flag is skipped whole.
 *   acc_in         (FA_ACCUMULATE) >= round_up(P, 4) floats, 16-byte aligned; out may alias it.  n == 0 needs it.
 *   out            >= P floats, 16-byte aligned; written in [0, P) only (float4 stores, the last column masked at P).
 *   flags          0 or FA_ACCUMULATE.
 * Independently of row_flags and of the offsets, no index read from a row is used as an address before an unsigned
 * range test against the tile, and no pair is read past min(nnz, ldk): the kernel is memory-safe whatever it is fed.
 */
int fs_reduce(const uint32_t* idx, const float* val, int64_t ldk, const int32_t* nnz, const int32_t* offsets,
              int64_t ldo, const int32_t* row_flags, int32_t n, int64_t P, const float* acc_in, float* out,
              int32_t flags, fa_stream_t stream);

/*
 * The launches fs_reduce makes at (K, P) on a GPU of `cus` compute units (host only, no GPU needed):
 * plan_out[FS_PLAN_FIELDS*i + {0..5}] = {tile columns, rows in flight, first column, tiles, tiles per workgroup,
 * grid} of launch i, for i < min(cap, returned count).  Workgroup b reduces tiles b, b + grid, ...; every tile is
 * reduced by exactly one wave, and a tile's columns depend on P only.  Returns the number of launches (>= 0) or
 * FA_E_ARG.
 */
int64_t fs_reduce_plan(int32_t cus, int32_t K, int64_t P, int64_t* plan_out, int32_t cap);

/* Bytes of fs_topk_row's workspace at P columns (host only); FA_E_ARG for a negative P. */
int64_t fs_topk_workspace(int64_t P);

/*
 * The executor-side handler: the selection rule above over one contiguous fp32 device row,
 *     e[p] = (base ? x[p] - base[p] : x[p]) (+ r_in[p] when r_in)          p < P
 * into idx_out / val_out (min(k, P) pairs each, in increasing index order) and, when r_out is not NULL, the residual
 * r_out[0, P) (r_out may be r_in).  x, base, r_in, r_out hold P floats; workspace is >= fs_topk_workspace(P) bytes of
 * device memory whose contents on entry do not matter; everything is 16-byte aligned.  1 <= k; P <= 2^31 - 1.
 * Stateless, integer atomics only (no order dependence), no host synchronisation.  The host-side equivalent is
 * fedscale_amd/cloud/execution/sparse_upload.py; both give the same bytes.
 */
int fs_topk_row(const float* x, const float* base, const float* r_in, int64_t P, int64_t k, void* workspace,
                uint32_t* idx_out, float* val_out, float* r_out, fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDSPARSE_H */
