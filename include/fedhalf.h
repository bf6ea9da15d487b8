/*
 * fedhalf.h — C ABI of the 16-bit client-upload path on MI355X (gfx950): client rows staged in HBM as float16 or
 * bfloat16, reduced in fp32, and the client-side handler that rounds an fp32 model into one such row.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued).  The entry
 * points of this header are bound by fedscale_amd/_native_half.py; the header has its own version
 * (fh_abi_version), FA_ABI_VERSION is not touched by it.
 *
 * What is replaced (reference): the same lines as fa_reduce — Aggregator.update_weight_aggregation,
 * aggregator.py:489-511, and AsyncAggregator.update_weight_aggregation, async_aggregator.py:115-137 — for uploads
 * whose fp32 entries travel in 16 bits.  NOT what those numpy lines would do when handed float16 arrays (they would
 * chain in float16, aggregator.py:500-507): every element is widened to fp32 first, exactly, and the chain is
 * fa_reduce's.  The reference has no 16-bit upload path and no FFI here.
 */
#ifndef FEDHALF_H
#define FEDHALF_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FH_ABI_VERSION 1
#define FH_PLAN_FIELDS 6 /* int64 per launch of fh_reduce_plan */

/* element type of a 16-bit row */
enum {
  FH_F16 = 0,  /* IEEE binary16; subnormals kept, +-inf and NaN pass through */
  FH_BF16 = 1, /* the upper 16 bits of an fp32 */
};

int32_t fh_abi_version(void);

/*
 * fa_reduce (fa_reduce_mirror when `mirror` is not NULL) over K rows of 16-bit elements, x16[k*ld + p]:
 *   chain_p = FA_ACCUMULATE ? acc_in[p] : w_0*f32(x16[0][p])      (w_k = a[k], or 1 when a == NULL)
 *   chain_p = chain_p + w_k*f32(x16[k][p])                          k = (FA_ACCUMULATE ? 0 : 1) .. K-1
 *   out[p]  = FA_FINALIZE ? chain_p / denom : chain_p
 * f32() widens exactly; every other operation is fp32, rounded to nearest, never fused — the bits of fa_reduce on
 * a widened copy of the rows.  One thread owns a column through all K rows, so no launch plan changes a result.
 *   x16    device memory, 16-byte aligned; ld a multiple of 64 elements, >= P.  Rows are read 16 bytes (8 columns)
 *          per lane, up to round_up(P, 8) <= ld elements of each row; columns [P, ld) are never counted.
 *   a, acc_in, out, denom, flags (FA_ACCUMULATE, FA_FINALIZE): as fa_reduce; out may alias acc_in.  acc_in, out
 *          and mirror hold >= round_up(P, 4) floats and are written as float4 columns, masked at ceil(P/4).
 *   mirror optional (needs FA_FINALIZE): a second copy of the mean; may be pinned host memory, as fa_reduce_mirror's.
 */
int fh_reduce(const void* x16, int32_t row_dtype, int64_t ld, int32_t K, int64_t P, const float* a,
              const float* acc_in, float* out, float* mirror, float denom, int32_t flags, fa_stream_t stream);

/*
 * The launches fh_reduce makes at (K, P) on a GPU of `cus` compute units (host only, no GPU needed):
 * plan_out[FH_PLAN_FIELDS*i + {0..5}] = {V, U, first column, tiles, strips per wave, grid} of launch i, for
 * i < min(cap, returned count).  V: 16-byte loads per lane per row (a strip is 64 lanes x 8 columns, a tile 4 waves
 * of `strips per wave` strips); U: rows loaded ahead of their adds; grid < tiles: every workgroup walks
 * ceil(tiles / grid) tiles.  Returns the number of launches (>= 0) or FA_E_ARG.
 */
int64_t fh_reduce_plan(int32_t cus, int32_t K, int64_t P, int32_t weighted, int64_t* plan_out, int32_t cap);
/* ... their count on the current device (needs a GPU: the plan depends on its CU count). */
int64_t fh_reduce_launches(int32_t K, int64_t P, int32_t weighted);

/*
 * The client-side handler: T separately allocated fp32 device tensors rounded into one 16-bit row,
 *   row16[dst_off[t] + i] = round16(src[t][i])      i < numel[t]
 * in one multi-tensor launch per 64 tensors (the table travels in the kernel arguments).  src, numel, dst_off are
 * HOST tables; src[t] is device memory, 4-byte aligned (16-byte loads where it is 16-byte aligned); row16 is device
 * memory, 2-byte aligned, holding max_t(dst_off[t] + numel[t]) elements (checked against its allocation; wider
 * stores where the destination's alignment allows).  Elements of the row outside every tensor are left untouched.  Rounding is to nearest even; float16 keeps subnormals and
 * overflows to +-inf (numpy's astype(np.float16)); bfloat16 rounds as torch.Tensor.to(torch.bfloat16) does on the
 * CPU; NaN stays NaN (payload unspecified).  Replaces: nothing (the reference's executor uploads fp32,
 * torch_client.py:79-91); the host-side equivalent is fedscale_amd/cloud/execution/half_upload.py.
 */
int fh_pack_row(const float* const* src, const int64_t* numel, const int64_t* dst_off, int32_t T, void* row16,
                int32_t row_dtype, fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDHALF_H */
