/*
 * fedgeomed.h — C ABI of geometric-median aggregation on MI355X (gfx950): the new model is the smoothed Weiszfeld
 * iterate of the K uploads (Pillutla, Kakade, Harchaoui: "Robust Aggregation for Federated Learning", RFA) — every
 * finite upload keeps a say, weighted by the inverse of its distance to the aggregate; no count or bound to tune,
 * breakdown point 1/2.  A server-side defence beside the norm clip of fedclip.h, the trimmed mean of fedtrim.h and
 * Multi-Krum of fedkrum.h.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless,
 * the call's GPU taken from its stream or its output, every operand checked before anything is queued: a refused
 * call says "nothing was launched").  The entry points of this header are bound by fedscale_amd/_native_geomed.py;
 * the header has its own version (fgm_abi_version); FA_, FCL_, FT_ and FK_ABI_VERSION are not touched by it.  No
 * atomics anywhere.  The library is built with -ffp-contract=off: no product below is fused; division and square
 * root are IEEE (correctly rounded), as in fcl_clip_coefs.
 *
 * A round starts from model L (P fp32 columns) with K uploads x_k in arrival order, 1 <= K <= FGM_MAX_K, runs R
 * iterations, 1 <= R <= FGM_MAX_ITERS, with smoothing nu > 0 (fp64, finite).  d_k = x_k - L (fp32, one op).
 *
 * The fixed-order sum S(v) of a length-K fp64 vector: pad with +0.0 to a multiple of 64; lane l adds v[l], v[l+64],
 * ... in ascending order starting from +0.0; then a 64-lane butterfly, t_l = t_l + t_(l xor m) for m = 32, 16, 8, 4,
 * 2, 1.  Every sum over K below is S; entries that are "left out" enter as +0.0.
 *
 * Start (fgm_start): q0_k = |x_k - L|^2 in fp64 — the diagonal of fk_gram's G, or fcl_row_sqnorms' output.
 *   valid_k = isfinite(q0_k);  n = #valid;  med = the (n / 2)-th smallest (0-based) valid q0   (n > 0)
 *   w_k = valid_k ? ((q0_k <= med ? 1.0 : sqrt(med) / sqrt(q0_k)) / double(n)) : +0.0;   c_k = float(w_k)
 * The start is the mean of the updates clipped to the median update norm: with fewer than half of the valid uploads
 * bad, med is at most the largest honest squared norm.  (RFA's own start, the plain mean, sits at 10^14 with one
 * upload scaled by 2^50 and three iterations only bring it to 3 * 10^12; L itself is a data point whenever a lazy
 * client uploads L unchanged, gets weight 1 / nu and pins the iterate.)
 *
 * Weights (fgm_weights): q_k is the squared distance of x_k to the current iterate.
 *   valid_k = isfinite(q_k);  dist_k = valid_k ? sqrt(q_k > 0 ? q_k : +0.0) : +0.0
 *   r_k = valid_k ? 1.0 / (dist_k > nu ? dist_k : nu) : +0.0
 *   B = S(r);  obj = S(dist);  n = #valid;  w_k = n > 0 ? r_k / B : +0.0;  c_k = float(w_k)
 *
 * Distances in Gram space (fgm_gram_dist2): G is fk_gram's K x K fp64 output, exactly symmetric, so entry (j, k) is
 * read as G[k*K + j] with coalesced loads.  The iterate is s = sum_k w_k d_k; the weights need not sum to 1.
 *   a_j = +0.0; for each chunk of FGM_CHUNK consecutive k, in ascending chunk order:
 *           part = +0.0; for k ascending in the chunk with w_k != 0: part = part + G[j][k] * w_k;   a_j = a_j + part
 *         (a row with w_k == 0 is skipped, not multiplied: its NaN never reaches a valid a_j)
 *   b   = S(u),  u_j = w_j != 0 ? w_j * a_j : +0.0
 *   q_j = (G[j][j] - 2.0 * a_j) + b
 * A row with an inf or NaN has a non-finite G[j][j], hence a non-finite q_j and weight 0 in every iteration.  The
 * three terms of q_j cancel: distances below about sqrt(u) * |d| (u = 2^-53) are rounding noise, which the clamp of
 * fgm_weights and nu absorb.
 *
 * Finish (fgm_finish): chain is fcl_reduce's, chain[p] = +0.0f; for k in arrival order with c_k != 0: chain[p] =
 * chain[p] + c_k * d_k[p].
 *   out[p] = n_valid > 0 ? last[p] + chain[p] : last[p]
 * There is no division: the weights are normalised already.  sum_k float(w_k) differs from 1 by at most K * 2^-25
 * (each of the K roundings to fp32 moves a weight <= 1 by at most 2^-25).  A weight that rounds to 0.0f leaves its
 * upload out of the chain, by fcl_reduce's own rule: the fate of an upload scaled by 10^38.
 *
 * The two rounds, both defined by the lines above plus existing entry points, with no host synchronisation between
 * the first launch and the last:
 *   gram:    fk_gram(x, L) -> G;  fgm_start(diag G);  R x { fgm_gram_dist2; fgm_weights };  fcl_reduce(x, L, c);
 *            fgm_finish -> out.  One Gram plus one pass over K x P.  G is within fedkrum.h's derived bound;
 *            everything after G is defined bit for bit given G.
 *   stream:  fcl_row_sqnorms(x, L) -> q0;  fgm_start;  fcl_reduce(x, L, c);  fgm_finish -> z;
 *            R x { fcl_row_sqnorms(x, last = z) -> q;  fgm_weights;  fcl_reduce(x, L, c);  fgm_finish -> z };
 *            the last finish writes out (and mirror).  2 + 2R passes over K x P.  Each q carries fcl_row_sqnorms'
 *            last-bits freedom; everything else is bit for bit given the q's.
 * The two agree to the last bits of the model, not bit for bit.
 *
 * Sizes: rows (chain, last) are read as float4 columns and hold >= round_up(P, 4) floats; out and mirror are written
 * in columns [0, P) only; row pointers are 16-byte aligned, q / w / G / workspace / obj 8-byte, c / n_valid 4-byte.
 */
#ifndef FEDGEOMED_H
#define FEDGEOMED_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FGM_ABI_VERSION 1
#define FGM_MAX_K 4096    /* rows of a round: the one-workgroup kernels keep K doubles in 32 KiB of LDS */
#define FGM_MAX_ITERS 64  /* Weiszfeld iterations of a round */
#define FGM_CHUNK 256     /* consecutive k of one partial of fgm_gram_dist2 (and its j per workgroup) */

int32_t fgm_abi_version(void);

/*
 * w[k], c[k] for k < K and *n_valid by the lines of "Start" above, with q0_k = q0[k * stride] (stride K + 1: the
 * diagonal of a K x K Gram; stride 1: a vector).  One workgroup: the norms in LDS, the median by a rank count (ties
 * by arrival; equal values give one med).  stride >= 1.
 */
int fgm_start(const double* q0, int64_t stride, int32_t K, double* w, float* c, int32_t* n_valid, fa_stream_t stream);

/*
 * w[k], c[k] for k < K, *obj_out and *n_valid by the lines of "Weights" above.  One workgroup; nu finite and > 0.
 */
int fgm_weights(const double* q, int32_t K, double nu, double* w, float* c, double* obj_out, int32_t* n_valid,
                fa_stream_t stream);

/* Bytes of the workspace fgm_gram_dist2 needs at K: ceil(K / FGM_CHUNK) * K * 8.  FA_E_ARG: K < 1, K > FGM_MAX_K. */
int64_t fgm_dist2_workspace_bytes(int32_t K);

/*
 * q_out[j] for j < K by the lines of "Distances in Gram space" above.  Two launches: the chunk partials
 * (ceil(K / 256) blocks of j x ceil(K / 256) chunks of k, part[chunk][j] to the workspace), then one workgroup for
 * a, b and q.  The launches are a function of K and compile-time constants only.
 *   gram, w, q_out, workspace: device memory; workspace_bytes >= fgm_dist2_workspace_bytes(K).
 */
int fgm_gram_dist2(const double* gram, int32_t K, const double* w, double* q_out, void* workspace,
                   int64_t workspace_bytes, fa_stream_t stream);

/*
 * out[p] = *n_valid > 0 ? last[p] + chain[p] : last[p], p < P; mirror[p] = out[p] when given.  n_valid is read on
 * the device: no host synchronisation sits between the last weights and the finish.
 *   mirror  optional second copy of out; may be pinned host memory, as fk_finish's
 */
int fgm_finish(const float* chain, const float* last, const int32_t* n_valid, int64_t P, float* out, float* mirror,
               fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDGEOMED_H */
