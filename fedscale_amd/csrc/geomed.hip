// geomed.hip — MI355X (gfx950) kernels of geometric-median (RFA) aggregation (include/fedgeomed.h): the smoothed
// Weiszfeld iteration run in the K-space of the uploads.
//   * fgm_start:      the start weights — the mean of the updates clipped to the median update norm;
//   * fgm_weights:    squared distances to the iterate -> normalised inverse-distance weights and the objective;
//   * fgm_gram_dist2: the squared distances of every upload to sum_k w_k d_k as a quadratic form in fk_gram's G,
//                     chunk partials over (j blocks x k chunks), then one workgroup for a, b and q;
//   * fgm_finish:     L + chain, or L when no upload was valid, with the count read on the device.
//
// Numerics: sequential fp64 IEEE arithmetic, never fused; every sum over K is the fixed-order sum S of the header
// (lane-strided adds of one wave over the vector in LDS, then the 64-lane butterfly).  The one-workgroup kernels keep
// their K doubles in 32 KiB of static LDS; the launches are a function of K and the constants below alone.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/fedgeomed.h"
#include "fa_device.h"
#include "fa_common.h"

namespace {

constexpr int GW = 1024;                    // threads of the one-workgroup kernels
constexpr int GROWS = FGM_MAX_K / GW;       // rows a thread of them owns, at most
static_assert(FGM_MAX_K % GW == 0 && FGM_MAX_K % 64 == 0 && FGM_CHUNK == 256, "geomed.hip: constants");

__device__ __forceinline__ int pad64(int K) { return (K + 63) & ~63; }

// S(v) of the header over sd[0, Kpad) (entries >= K are +0.0), by the 64 lanes of ONE wave; every lane returns it
__device__ __forceinline__ double fixed_sum(const double* sd, int Kpad, int lane) {
  double t = 0.0;
  for (int i = lane; i < Kpad; i += 64) t = t + sd[i];
  return wave_sum(t);
}

// ------------------------------------------------------------------------------------------------
// fgm_start
// ------------------------------------------------------------------------------------------------
// The norms go to LDS with every non-finite one as +inf; a thread ranks its valid rows against all K by (value,
// arrival) and counts the valid ones on the way: the one row of rank n / 2 publishes med and n.
__global__ __launch_bounds__(GW) void k_geomed_start(const double* __restrict__ q0, int64_t stride, int K,
                                                     double* __restrict__ w, float* __restrict__ c,
                                                     int* __restrict__ n_valid) {
  __shared__ double sd[FGM_MAX_K];
  __shared__ double s_med;
  __shared__ int s_n;
  if (threadIdx.x == 0) {
    s_med = 0.0;
    s_n = 0;
  }
  for (int k = threadIdx.x; k < K; k += GW) {
    const double q = q0[(int64_t)k * stride];
    sd[k] = __builtin_isfinite(q) ? q : (double)INFINITY;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K; i += GW) {
    const double si = sd[i];
    if (si < (double)INFINITY) {
      int rank = 0, n = 0;
      for (int j = 0; j < K; ++j) {
        const double sj = sd[j];
        n += sj < (double)INFINITY ? 1 : 0;
        rank += (sj < si || (sj == si && j < i)) ? 1 : 0;
      }
      if (rank == n / 2) {  // ranks of valid rows are 0 .. n - 1, each once: one writer
        s_med = si;
        s_n = n;
      }
    }
  }
  __syncthreads();
  const int n = s_n;
  const double med = s_med, dn = (double)n;
  for (int k = threadIdx.x; k < K; k += GW) {
    const double q = sd[k];
    double wk = 0.0;
    if (q < (double)INFINITY) wk = (q <= med ? 1.0 : sqrt(med) / sqrt(q)) / dn;
    w[k] = wk;
    c[k] = (float)wk;
  }
  if (threadIdx.x == 0) *n_valid = n;
}

// ------------------------------------------------------------------------------------------------
// fgm_weights
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dist_of(double q) {
  return __builtin_isfinite(q) ? sqrt(q > 0.0 ? q : 0.0) : 0.0;
}
__device__ __forceinline__ double inv_of(double q, double nu) {
  if (!__builtin_isfinite(q)) return 0.0;
  const double d = sqrt(q > 0.0 ? q : 0.0);
  return 1.0 / (d > nu ? d : nu);
}

__global__ __launch_bounds__(GW) void k_geomed_weights(const double* __restrict__ q, int K, double nu,
                                                       double* __restrict__ w, float* __restrict__ c,
                                                       double* __restrict__ obj_out, int* __restrict__ n_valid) {
  __shared__ double sd[FGM_MAX_K];
  __shared__ double s_B;
  __shared__ int s_cnt[GW / 64];  // valid rows per wave: integers, so any order of adding them gives n
  const int Kpad = pad64(K), lane = threadIdx.x & 63;
  int cnt = 0;
  for (int k = threadIdx.x; k < Kpad; k += GW) {
    const double qk = k < K ? q[k] : 0.0;
    cnt += k < K && __builtin_isfinite(qk) ? 1 : 0;
    sd[k] = k < K ? dist_of(qk) : 0.0;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
  if (lane == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x < 64) {
    const double obj = fixed_sum(sd, Kpad, lane);
    if (lane == 0) *obj_out = obj;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < Kpad; k += GW) sd[k] = k < K ? inv_of(q[k], nu) : 0.0;
  __syncthreads();
  if (threadIdx.x < 64) {
    const double B = fixed_sum(sd, Kpad, lane);
    if (lane == 0) s_B = B;
  }
  __syncthreads();
  int n = 0;  // n = #isfinite(q), as the header states it
#pragma unroll
  for (int v = 0; v < GW / 64; ++v) n += s_cnt[v];
  const double B = s_B;
  for (int k = threadIdx.x; k < K; k += GW) {
    const double wk = n > 0 ? sd[k] / B : 0.0;
    w[k] = wk;
    c[k] = (float)wk;
  }
  if (threadIdx.x == 0) *n_valid = n;
}

// ------------------------------------------------------------------------------------------------
// fgm_gram_dist2
// ------------------------------------------------------------------------------------------------
// part[chunk][j] = the chunk's ordered sum of G[j][k] * w_k over its k with w_k != 0.  G is symmetric, so thread j
// reads G[k*K + j]: the 256 threads of a workgroup read 2 KiB of row k at a time.  w_k is the same for every thread
// (one LDS broadcast), so the skip is a uniform branch.
__global__ __launch_bounds__(FGM_CHUNK) void k_geomed_partials(const double* __restrict__ gram, int K,
                                                               const double* __restrict__ w,
                                                               double* __restrict__ part) {
  __shared__ double sw[FGM_CHUNK];
  const int k0 = blockIdx.y * FGM_CHUNK;
  const int kn = K - k0 < FGM_CHUNK ? K - k0 : FGM_CHUNK;
  sw[threadIdx.x] = (int)threadIdx.x < kn ? w[k0 + threadIdx.x] : 0.0;
  __syncthreads();
  const int j = blockIdx.x * FGM_CHUNK + threadIdx.x;
  if (j >= K) return;
  const double* g = gram + (int64_t)k0 * K + j;
  double p = 0.0;
  for (int t = 0; t < kn; ++t) {
    const double wk = sw[t];
    if (wk != 0.0) p = p + g[(int64_t)t * K] * wk;
  }
  part[(int64_t)blockIdx.y * K + j] = p;
}

// a_j from the partials in chunk order, b = S(u), q_j = (G[j][j] - 2 a_j) + b
__global__ __launch_bounds__(GW) void k_geomed_dist2(const double* __restrict__ gram, int K, int nchunk,
                                                     const double* __restrict__ w, const double* __restrict__ part,
                                                     double* __restrict__ q_out) {
  __shared__ double sd[FGM_MAX_K];
  __shared__ double s_b;
  const int Kpad = pad64(K), lane = threadIdx.x & 63;
  double a[GROWS];
#pragma unroll
  for (int s = 0; s < GROWS; ++s) {
    const int j = threadIdx.x + s * GW;
    a[s] = 0.0;
    if (j < Kpad) {
      double u = 0.0;
      if (j < K) {
        double aj = 0.0;
        for (int ch = 0; ch < nchunk; ++ch) aj = aj + part[(int64_t)ch * K + j];
        a[s] = aj;
        const double wj = w[j];
        if (wj != 0.0) u = wj * aj;
      }
      sd[j] = u;
    }
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const double b = fixed_sum(sd, Kpad, lane);
    if (lane == 0) s_b = b;
  }
  __syncthreads();
  const double b = s_b;
#pragma unroll
  for (int s = 0; s < GROWS; ++s) {
    const int j = threadIdx.x + s * GW;
    if (j < K) q_out[j] = (gram[(int64_t)j * K + j] - 2.0 * a[s]) + b;
  }
}

// ------------------------------------------------------------------------------------------------
// fgm_finish
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_geomed_finish(const f4* __restrict__ chain, const f4* __restrict__ last,
                                                       const int* __restrict__ n_valid, int64_t P, float* out,
                                                       float* mirror) {
  const int n = *n_valid;
  const int64_t P4 = (P + 3) / 4;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < P4; c += (int64_t)gridDim.x * 256) {
    const f4 l = last[c];
    f4 o = l;
    if (n > 0) {
      const f4 ch = chain[c];
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = l[i] + ch[i];
    }
    const int64_t p = 4 * c;
    if (p + 4 <= P) {
      *reinterpret_cast<f4*>(out + p) = o;
      if (mirror) *reinterpret_cast<f4*>(mirror + p) = o;
    } else {  // the last, partial float4 column: columns >= P are not written
      for (int i = 0; i < (int)(P - p); ++i) {
        out[p + i] = o[i];
        if (mirror) mirror[p + i] = o[i];
      }
    }
  }
}

int check_k(const char* who, int32_t K) {
  if (K < 1) return refuse(FA_E_ARG, "%s: K=%d must be >= 1", who, K);
  if (K > FGM_MAX_K) return refuse(FA_E_ARG, "%s: K=%d rows, the kernels take at most %d (FGM_MAX_K)", who, K, FGM_MAX_K);
  return 0;
}

int nchunks(int K) { return (K + FGM_CHUNK - 1) / FGM_CHUNK; }
bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedgeomed.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t fgm_abi_version(void) { return FGM_ABI_VERSION; }

extern "C" int fgm_start(const double* q0, int64_t stride, int32_t K, double* w, float* c, int32_t* n_valid,
                         fa_stream_t stream) {
  if (const int e = check_k("fgm_start", K)) return e;
  if (stride < 1) return refuse(FA_E_ARG, "fgm_start: stride=%lld must be >= 1", (long long)stride);
  if (!q0 || !w || !c || !n_valid) return refuse(FA_E_ARG, "fgm_start: q0, w, c or n_valid is NULL");
  if (!aligned8(q0) || !aligned8(w) || !aligned4(c) || !aligned4(n_valid))
    return refuse(FA_E_ARG, "fgm_start: q0 and w must be 8-byte, c and n_valid 4-byte aligned");
  FA_DEVICE_SCOPE("fgm_start", stream, w);
  FA_OPERAND("q0", q0, (uint64_t)((int64_t)(K - 1) * stride + 1) * 8);
  FA_OPERAND("w", w, (uint64_t)K * 8);
  FA_OPERAND("c", c, (uint64_t)K * 4);
  FA_OPERAND("n_valid", n_valid, 4);
  hipLaunchKernelGGL(k_geomed_start, dim3(1), dim3(GW), 0, (hipStream_t)stream, q0, stride, (int)K, w, c,
                     (int*)n_valid);
  return check_launch("fgm_start");
}

extern "C" int fgm_weights(const double* q, int32_t K, double nu, double* w, float* c, double* obj_out,
                           int32_t* n_valid, fa_stream_t stream) {
  if (const int e = check_k("fgm_weights", K)) return e;
  if (!(nu > 0.0) || !__builtin_isfinite(nu)) return refuse(FA_E_ARG, "fgm_weights: nu=%g must be finite and > 0", nu);
  if (!q || !w || !c || !obj_out || !n_valid) return refuse(FA_E_ARG, "fgm_weights: q, w, c, obj_out or n_valid is NULL");
  if (!aligned8(q) || !aligned8(w) || !aligned8(obj_out) || !aligned4(c) || !aligned4(n_valid))
    return refuse(FA_E_ARG, "fgm_weights: q, w and obj_out must be 8-byte, c and n_valid 4-byte aligned");
  FA_DEVICE_SCOPE("fgm_weights", stream, w);
  FA_OPERAND("q", q, (uint64_t)K * 8);
  FA_OPERAND("w", w, (uint64_t)K * 8);
  FA_OPERAND("c", c, (uint64_t)K * 4);
  FA_OPERAND("obj_out", obj_out, 8);
  FA_OPERAND("n_valid", n_valid, 4);
  hipLaunchKernelGGL(k_geomed_weights, dim3(1), dim3(GW), 0, (hipStream_t)stream, q, (int)K, nu, w, c, obj_out,
                     (int*)n_valid);
  return check_launch("fgm_weights");
}

extern "C" int64_t fgm_dist2_workspace_bytes(int32_t K) {
  if (const int e = check_k("fgm_dist2_workspace_bytes", K)) return e;
  return (int64_t)nchunks(K) * K * 8;
}

extern "C" int fgm_gram_dist2(const double* gram, int32_t K, const double* w, double* q_out, void* workspace,
                              int64_t workspace_bytes, fa_stream_t stream) {
  if (const int e = check_k("fgm_gram_dist2", K)) return e;
  if (!gram || !w || !q_out || !workspace) return refuse(FA_E_ARG, "fgm_gram_dist2: gram, w, q_out or workspace is NULL");
  if (!aligned8(gram) || !aligned8(w) || !aligned8(q_out) || !aligned8(workspace))
    return refuse(FA_E_ARG, "fgm_gram_dist2: gram, w, q_out and workspace must be 8-byte aligned");
  const int nc = nchunks(K);
  const int64_t need = (int64_t)nc * K * 8;
  if (workspace_bytes < need)
    return refuse(FA_E_ARG, "fgm_gram_dist2: workspace of %lld bytes, K=%d needs %lld (fgm_dist2_workspace_bytes)",
                  (long long)workspace_bytes, K, (long long)need);
  FA_DEVICE_SCOPE("fgm_gram_dist2", stream, q_out);
  FA_OPERAND("gram", gram, (uint64_t)K * K * 8);
  FA_OPERAND("w", w, (uint64_t)K * 8);
  FA_OPERAND("q_out", q_out, (uint64_t)K * 8);
  FA_OPERAND("workspace", workspace, (uint64_t)need);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_geomed_partials, dim3(nc, nc), dim3(FGM_CHUNK), 0, st, gram, (int)K, w, (double*)workspace);
  if (const int e = check_launch("fgm_gram_dist2 (partials)")) return e;
  hipLaunchKernelGGL(k_geomed_dist2, dim3(1), dim3(GW), 0, st, gram, (int)K, nc, w, (const double*)workspace, q_out);
  return check_launch("fgm_gram_dist2");
}

extern "C" int fgm_finish(const float* chain, const float* last, const int32_t* n_valid, int64_t P, float* out,
                          float* mirror, fa_stream_t stream) {
  if (P < 0) return refuse(FA_E_ARG, "fgm_finish: negative P=%lld", (long long)P);
  if (!chain || !last || !n_valid || !out) return refuse(FA_E_ARG, "fgm_finish: chain, last, n_valid or out is NULL");
  if (!aligned16(chain) || !aligned16(last)) return refuse(FA_E_ARG, "fgm_finish: chain and last must be 16-byte aligned");
  if (!aligned16(out) || !aligned16(mirror)) return refuse(FA_E_ARG, "fgm_finish: out and mirror must be 16-byte aligned");
  if (!aligned4(n_valid)) return refuse(FA_E_ARG, "fgm_finish: n_valid must be 4-byte aligned");
  if (P == 0) return FA_OK;
  const int64_t P4 = (P + 3) / 4;
  FA_DEVICE_SCOPE("fgm_finish", stream, out);
  FA_OPERAND("chain", chain, (uint64_t)P4 * 16);
  FA_OPERAND("last", last, (uint64_t)P4 * 16);
  FA_OPERAND("n_valid", n_valid, 4);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  FA_HOST_OK_OPERAND("mirror", mirror, (uint64_t)P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fgm_finish: no CU count for device %d", fa_scope_device());
  int64_t g = (P4 + 255) / 256;
  if (g > (int64_t)cus * 8) g = (int64_t)cus * 8;
  hipLaunchKernelGGL(k_geomed_finish, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const f4*>(chain), reinterpret_cast<const f4*>(last), (const int*)n_valid, P,
                     out, mirror);
  return check_launch("fgm_finish");
}
