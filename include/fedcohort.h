/*
 * fedcohort.h — C ABI of the Auxo cohort-clustering features on MI355X (gfx950): per-client gradient
 * signatures of the staged uploads, their centred / normalised forms and the K x K Gram matrix.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory,
 * stateless).  The entry points of this header are bound by fedscale_amd/_native_cohort.py; the header has
 * its own version (fc_abi_version), FA_ABI_VERSION is not touched by it.
 *
 * What is replaced (reference, examples/auxo):
 *   client_metadata.py:10-17   register_gradient: W_old - W per tensor, concatenate (float64 as soon as one
 *                              int64 buffer is present), keep the last len // 10 elements, cast to float16
 *   client_manager.py:208-210  np.mean over the K signatures, centre, sklearn normalize (L2, rows)
 * A "signature" is a row of D float16; matrices are row-major [K][ldd] float16 (ldd >= D elements).  The
 * 16-byte paths are taken when the matrix base is 16-byte aligned and ldd is a multiple of 8; any other
 * base / stride takes element-wise loads and stores with the same results.
 */
#ifndef FEDCOHORT_H
#define FEDCOHORT_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FC_ABI_VERSION 1
#define FC_GRAM_MAX_K 4096 /* fc_gram: rows of the matrix (clients of one cohort round) */

int32_t fc_abi_version(void);

/*
 * Signatures of n staged uploads (rows of x / xi, the round's staging area; x may be pinned host memory the
 * GPU reads over PCIe, as fa_reduce's x):
 *   fp32 segment s = (src, dst, len) of segs[3*s ..]:   sig[k][dst + i] = half_rne(last[src + i] - x[k][src + i])
 *   int64 element e = (q, dst) of isegs[2*e ..]:        sig[k][dst]     = half_rne((double)(last_i64[q] - xi[k][q]))
 * The subtraction is one fp32 op; the conversion rounds to nearest even, keeps float16 subnormals and gives
 * +-inf beyond the float16 range (numpy's cast).  segs / isegs are HOST arrays (int64), checked against ld, ldq
 * and ldd before anything is launched; fedscale_amd/cohort_signature.py (signature_plan) makes them from a
 * layout.  Segment starts are arbitrary: 16-byte loads of x are used from the first aligned element of each
 * (row, segment), scalar loads before it and after the last whole group.
 */
int fc_signature(const float* x, int64_t ld, int32_t n, const float* last, const int64_t* xi, int32_t ldq,
                 const int64_t* last_i64, const int64_t* segs, int32_t nseg, const int64_t* isegs, int32_t niseg,
                 void* sig_out, int64_t ldd, fa_stream_t stream);

/*
 * Column mean, centring and per-row sums of squares, in numpy's order (client_manager.py:208-209 on a list
 * of float16 rows): per column j
 *   acc32 = sum_k float(sig[k][j])           added sequentially in k, in fp32
 *   avg16[j] = half_rne(acc32 / float(K))    IEEE division
 *   centered[k][j] = half_rne(float(sig[k][j]) - float(avg16[j]))
 * and sumsq[k] = sum_j centered[k][j]^2 in fp64 (per-wave partials in `workspace`, summed in a fixed order:
 * no floating-point atomics, the same bits on every run).  workspace: fc_center_workspace_bytes(K, D) bytes of
 * device memory, 8-byte aligned.  centered_out may not alias sig.
 */
int64_t fc_center_workspace_bytes(int32_t K, int64_t D);
int fc_center(const void* sig, int64_t ldd, int32_t K, int64_t D, void* avg16_out, void* centered_out,
              double* sumsq_out, void* workspace, fa_stream_t stream);

/*
 * sklearn.preprocessing.normalize (L2, axis 1) of the centred matrix with the row norms given in fp64:
 *   normalized[k][j] = half_rne(float(centered[k][j]) / float(norm[k]))     a zero norm is replaced by 1
 * normalized_out may alias centered.
 */
int fc_normalize(const void* centered, int64_t ldd, int32_t K, int64_t D, const double* norm_in,
                 void* normalized_out, fa_stream_t stream);

/*
 * gram[i][j] = sum_d float(c[i][d]) * float(c[j][d]): a K x K fp32 matrix (row-major, stride K) from the
 * float16 matrix, on the f16 matrix unit (v_mfma_f32_32x32x16_f16, fp32 accumulation).  Only the lower triangle
 * of 64 x 64 tiles is computed; D is split over workgroups into [nsplit][K][K] partials in `workspace`, which
 * a second launch sums in split order and mirrors, so the result is exactly symmetric and the same on every
 * run.  K and D are zero-padded to the tile shape inside the kernel.  K <= FC_GRAM_MAX_K.
 * workspace: fc_gram_workspace_bytes(K, D) bytes of device memory, 16-byte aligned.
 */
int64_t fc_gram_workspace_bytes(int32_t K, int64_t D);
int fc_gram(const void* c, int64_t ldd, int32_t K, int64_t D, float* gram_out, void* workspace,
            fa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FEDCOHORT_H */
