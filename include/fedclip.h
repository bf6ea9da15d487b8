/*
 * fedclip.h — C ABI of norm-clipped FedAvg on MI355X (gfx950): every staged client update is clipped to a norm
 * bound against the round's starting model before it enters the mean, and Gaussian noise may be added to the mean
 * (server-side clipping against poisoned uploads; central DP-FedAvg).
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued: a refused
 * call says "nothing was launched").  The entry points of this header are bound by fedscale_amd/_native_clip.py;
 * the header has its own version (fcl_abi_version); FA_ABI_VERSION and FH_ABI_VERSION are not touched by it.
 *
 * The arithmetic of a round that starts from model L (P fp32 columns) with K staged uploads x_k in arrival order —
 * everything fp32, rounded to nearest, never fused, unless marked:
 *   d_k[p]   = x_k[p] - L[p]
 *   sq_k     = sum_p double(d_k[p]) * double(d_k[p])            fp64 (fcl_row_sqnorms)
 *   r_k      = M / (sqrt(sq_k) + 1e-6)                          fp64, IEEE (fcl_clip_coefs)
 *   c_k      = !isfinite(sq_k) ? 0.0f : (r_k < 1 ? float(r_k) : 1.0f)
 *   chain[p] = +0.0f; for k in arrival order with c_k != 0: chain[p] = chain[p] + c_k * d_k[p]     (fcl_reduce)
 *   m[p]     = chain[p] / denom;  m[p] = m[p] + sigma * z[p] when sigma > 0;  out[p] = L[p] + m[p]  (fcl_finish)
 *
 * Sizes: buffers that are READ column-wise (x rows, last, chain, acc_in, z) hold >= round_up(P, 4) floats and are
 * read as float4 columns; columns >= P never enter a sum and are never stored.  Buffers that are WRITTEN (chain out,
 * out, mean_delta_out, mirror) are written in columns [0, P) only.  Row and vector pointers are 16-byte aligned,
 * ld is a multiple of 4 and >= P.
 */
#ifndef FEDCLIP_H
#define FEDCLIP_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FCL_ABI_VERSION 1
#define FCL_PLAN_FIELDS 6 /* int64 per launch of fcl_reduce_plan */

int32_t fcl_abi_version(void);

/*
 * Bytes of the workspace fcl_row_sqnorms needs for n rows of P columns: one double per (row, column tile) —
 * n * (wave tiles of fcl_norm_plan) * 8, at least 8.  Negative n or P: FA_E_ARG.  Replaces: nothing.
 */
int64_t fcl_workspace_bytes(int32_t n, int64_t P);

/*
 * sq[k] = sum_p double(x[k*ld + p] - last[p])^2 for the n rows of a chunk, k < n.
 * The difference is fp32; its square is exact in fp64 (so fused and unfused fp64 adds agree); the fp64 adds run in
 * an order fixed by P and compile-time constants alone — never by k, n, or the GPU's CU count — so a row's bits do
 * not depend on the rows it is batched with or on the machine.  First launch: a wave owns a column tile (2048
 * columns, or 4096 when P >= 4 Mi: fcl_norm_plan), keeps its tile of `last` in registers and walks the rows
 * (streamed once, non-temporal); per (row, tile) the wave's total goes to workspace[k * tiles + tile].  Second launch: one wave
 * per row adds the row's tile partials (lane l takes tiles l, l + 64, ... in order, then a 64-lane butterfly) and
 * then the <= 3 columns past the last whole float4.  No atomics.
 *   x, last, sq, workspace: device memory; workspace 8-byte aligned, >= fcl_workspace_bytes(n, P).
 * Replaces: nothing (the reference clips on the client, examples/.../customized_client.py, clip_grad_norm_);
 * the per-client squared norm is what clip_norm.py:57's total_norm squares to.
 */
int fcl_row_sqnorms(const float* x, int64_t ld, int32_t n, int64_t P, const float* last, double* sq,
                    double* workspace, int64_t workspace_bytes, fa_stream_t stream);

/*
 * The launches fcl_row_sqnorms makes at P columns on a GPU of `cus` compute units (host only, no GPU needed):
 * plan_out[0..3] = {wave tiles, workgroups of the first launch, waves per workgroup, columns per wave tile}; a
 * workgroup's waves stride over the tiles, so grid * waves < tiles means a wave walks more than one.  Returns the
 * number of launches (2, or 1 when P < 4: only the second) or FA_E_ARG.  Replaces: nothing.
 */
int64_t fcl_norm_plan(int32_t cus, int64_t P, int64_t* plan_out);

/*
 * c[k] = clip coefficient of sq[k] against max_norm M (clip_norm.py:57-60: clip_coef = max_norm / (total_norm +
 * 1e-6), applied when < 1), k < n; a non-finite sq[k] gives 0.0f and adds one to *rejected (a device int32 the
 * caller zeroes at the start of a round).  One tiny launch, no host synchronisation.
 */
int fcl_clip_coefs(const double* sq, int32_t n, double max_norm, float* c, int32_t* rejected, fa_stream_t stream);

/*
 * The clipped chain over the n rows of a chunk (stands in for aggregator.py:489-511's running sum, on clipped
 * updates):  chain_p = FA_ACCUMULATE ? acc_in[p] : +0.0f;  for k < n with c[k] != 0:
 * chain_p = chain_p + c[k] * (x[k*ld + p] - last[p]);  out[p] = chain_p.
 * A row with c[k] == 0 is skipped, not multiplied by zero (its inf / NaN never reaches the chain).  One thread owns
 * a column through all rows, so no launch plan changes a bit.  flags: 0 or FA_ACCUMULATE; out may alias acc_in.
 * n == 0 needs FA_ACCUMULATE.
 */
int fcl_reduce(const float* x, int64_t ld, int32_t n, int64_t P, const float* last, const float* c,
               const float* acc_in, float* out, int32_t flags, fa_stream_t stream);

/*
 * The launches fcl_reduce makes at (K, P) on a GPU of `cus` compute units (host only, no GPU needed):
 * plan_out[FCL_PLAN_FIELDS*i + {0..5}] = {V, U, first column, tiles, strips per wave, grid} of launch i, for
 * i < min(cap, returned count).  V: float4 loads per lane per row (a strip is 64 lanes x 4 columns, a tile 4 waves
 * of `strips per wave` strips); U: rows loaded ahead of their adds; grid < tiles: every workgroup walks
 * ceil(tiles / grid) tiles.  Returns the number of launches (>= 0) or FA_E_ARG.  Replaces: nothing.
 */
int64_t fcl_reduce_plan(int32_t cus, int32_t K, int64_t P, int64_t* plan_out, int32_t cap);

/*
 * m[p] = chain[p] / denom (IEEE division);  m[p] = m[p] + sigma * z[p] when sigma > 0;  out[p] = last[p] + m[p];
 * mean_delta_out[p] = m[p] and mirror[p] = out[p] when given.  The mean of aggregator.py:505-507 on clipped
 * updates, re-based on the round's starting model; the noise has no counterpart in the reference's aggregator.
 *   z      device memory, required when sigma > 0 (fa_dp_normals(seed, noise_offset + p)); ignored otherwise
 *   mirror optional second copy of out; may be pinned host memory, as fa_reduce_mirror's
 *   sigma  finite, >= 0;  denom > 0
 */
int fcl_finish(const float* chain, const float* last, const float* z, float sigma, float denom, int64_t P,
               float* out, float* mean_delta_out, float* mirror, fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDCLIP_H */
