// krum_gram.hip — MI355X (gfx950) kernels of Krum / Multi-Krum selection (include/fedkrum.h):
//   * fk_gram:   the K x K fp64 Gram matrix of the updates d_k = x_k - L on the fp64 matrix unit
//                (v_mfma_f64_16x16x4_f64), lower-triangle row tiles x a column split, then the split sum;
//   * fk_scores: per row, the K - 1 clamped squared distances sorted in LDS and the K - f - 2 smallest added in order;
//   * fk_select: rank by (score, arrival), the 0 / 1 coefficients fcl_reduce takes, and their count;
//   * fk_finish: L + chain / n_sel with the count read on the device.
//
// Numerics: d is one fp32 subtraction; its products are exact in fp64; the fp64 adds of a partial run in the order
// the instruction and the tile loop impose, a function of (K, P) and the constants below alone; everything after
// the Gram is sequential fp64 / fp32 IEEE arithmetic, never fused.
//
// The Gram tile.  A workgroup of 4 waves computes a 64 x 64 tile, each wave 32 x 32 as 2 x 2 accumulators of the
// 16 x 16 x 4 instruction (4 independent accumulators, 32 VGPRs).  Per step of 32 columns it fetches 64 x 32 fp32 of
// each operand (a diagonal tile fetches one): 16 KiB for 64 * 64 * 32 * 2 = 262144 FLOP, 16 FLOP per byte, against
// a machine balance of about 10 (78.6 TF fp64 matrix peak over 8 TB/s) — on the compute side of the ridge without
// the 128 accumulator registers per wave a 128 x 128 tile would take, and K = 100 (two row tiles) computes 3 tiles
// of 64 instead of one of 128: three quarters of the FLOP.  LDS rows are 36 floats apart (144 B): the 16 lanes of a
// 16-byte fragment read start 36 r mod 64 banks apart, all different multiples of 4, so a read has no conflict.
// A lane's 16-byte fragment holds columns 4g .. 4g + 3 of its row (g = lane >> 4); element e of it is the
// instruction's k = g of sub-step e, for A and B alike, so the sum pairs every column with itself.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/fedkrum.h"
#include "fa_device.h"
#include "fa_common.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int KB = 64;   // rows of a tile side
constexpr int KS = 32;   // columns per step
constexpr int KPITCH = 36;  // LDS row pitch in floats
constexpr int64_t K_TARGET_WGS = 2048;
constexpr int64_t K_MIN_STEPS = 4;  // steps per split, at least (when there are that many)
constexpr int64_t K_MAX_WS = (int64_t)512 << 20;

struct KrumPlan {
  int tiles;
  int nsplit;
  int64_t pchunk;  // columns per split (a multiple of KS)
  int64_t last_steps;
};
KrumPlan krum_plan(int K, int64_t P) {
  const int T = (K + KB - 1) / KB;
  KrumPlan p;
  p.tiles = T * (T + 1) / 2;
  const int64_t steps = P > 0 ? (P + KS - 1) / KS : 1;
  int64_t ns = (K_TARGET_WGS + p.tiles - 1) / p.tiles;
  const int64_t most = (steps + K_MIN_STEPS - 1) / K_MIN_STEPS;
  if (ns > most) ns = most;
  const int64_t one = (int64_t)K * K * 8;
  while (ns > 1 && ns * one > K_MAX_WS) --ns;
  const int64_t per = (steps + ns - 1) / ns;
  p.pchunk = per * KS;
  p.nsplit = (int)((steps + per - 1) / per);
  p.last_steps = steps - (int64_t)(p.nsplit - 1) * per;
  return p;
}

// ------------------------------------------------------------------------------------------------
// fk_gram
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ f4 diff4(f4 x, f4 l, int nv) {
  f4 d;
#pragma unroll
  for (int c = 0; c < 4; ++c) d[c] = c < nv ? x[c] - l[c] : 0.0f;
  return d;
}

// part[split][i][j] for the tile (I, J <= I) of blockIdx.x over columns [split * pchunk, + pchunk) of d = x - last
__global__ __launch_bounds__(256) void k_krum_gram(const float* __restrict__ x, int64_t ld, int K, int64_t P,
                                                   const float* __restrict__ last, int64_t pchunk,
                                                   double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float sA[KB * KPITCH];
  __shared__ __attribute__((aligned(16))) float sB[KB * KPITCH];
  const int t = blockIdx.x;
  int I = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  const int J = t - I * (I + 1) / 2;
  const bool diag = I == J;
  const int64_t p0 = (int64_t)blockIdx.y * pchunk;
  const int64_t p1 = p0 + pchunk < P ? p0 + pchunk : P;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wi = wave >> 1, wj = wave & 1;
  // this thread's two float4 pieces of a 64 x 32 step of either operand
  const int r0 = threadIdx.x >> 3, r1 = r0 + 32, kc = (threadIdx.x & 7) * 4;
  const int64_t ia0 = (int64_t)I * KB + r0, ia1 = (int64_t)I * KB + r1;
  const int64_t ib0 = (int64_t)J * KB + r0, ib1 = (int64_t)J * KB + r1;
  const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
  f4 ra0, ra1, rb0, rb1, rl;
  int nv = 0;  // valid columns of the fetched float4 (columns >= P are zeros in both operands)
  auto fetch = [&](int64_t pk) {
    const int64_t p = pk + kc;
    const int64_t left = p1 - p;
    nv = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
    ra0 = ra1 = rb0 = rb1 = rl = zero;
    if (nv > 0) {  // p < P: the float4 lies inside round_up(P, 4) <= ld
      rl = *reinterpret_cast<const f4*>(last + p);
      if (ia0 < K) ra0 = *reinterpret_cast<const f4*>(x + ia0 * ld + p);
      if (ia1 < K) ra1 = *reinterpret_cast<const f4*>(x + ia1 * ld + p);
      if (!diag) {
        if (ib0 < K) rb0 = *reinterpret_cast<const f4*>(x + ib0 * ld + p);
        if (ib1 < K) rb1 = *reinterpret_cast<const f4*>(x + ib1 * ld + p);
      }
    }
  };
  d4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
  if (p0 < p1) fetch(p0);
  const float* sBt = diag ? sA : sB;
  const float* pa = sA + (wi * 32 + (lane & 15)) * KPITCH + (lane >> 4) * 4;
  const float* pb = sBt + (wj * 32 + (lane & 15)) * KPITCH + (lane >> 4) * 4;
  for (int64_t pk = p0; pk < p1; pk += KS) {
    __syncthreads();  // the previous step's fragments have been read
    // rows >= K are zeros: their x was never loaded, and 0 - L must not enter
    *reinterpret_cast<f4*>(sA + r0 * KPITCH + kc) = ia0 < K ? diff4(ra0, rl, nv) : zero;
    *reinterpret_cast<f4*>(sA + r1 * KPITCH + kc) = ia1 < K ? diff4(ra1, rl, nv) : zero;
    if (!diag) {
      *reinterpret_cast<f4*>(sB + r0 * KPITCH + kc) = ib0 < K ? diff4(rb0, rl, nv) : zero;
      *reinterpret_cast<f4*>(sB + r1 * KPITCH + kc) = ib1 < K ? diff4(rb1, rl, nv) : zero;
    }
    __syncthreads();
    if (pk + KS < p1) fetch(pk + KS);  // in flight under the MFMAs
#pragma unroll
    for (int h = 0; h < KS / 16; ++h) {
      const f4 a0 = *reinterpret_cast<const f4*>(pa + h * 16);
      const f4 a1 = *reinterpret_cast<const f4*>(pa + 16 * KPITCH + h * 16);
      const f4 b0 = *reinterpret_cast<const f4*>(pb + h * 16);
      const f4 b1 = *reinterpret_cast<const f4*>(pb + 16 * KPITCH + h * 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double da0 = (double)a0[e], da1 = (double)a1[e], db0 = (double)b0[e], db1 = (double)b1[e];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(da0, db0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(da0, db1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(da1, db0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(da1, db1, acc[1][1], 0, 0, 0);
      }
    }
  }
  // the fp64 accumulator: lane l, register r holds C[row (l >> 4) + 4 r][col l & 15]
  double* out = part + (int64_t)blockIdx.y * K * K;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int64_t gj = (int64_t)J * KB + wj * 32 + b * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gi = (int64_t)I * KB + wi * 32 + a * 16 + (lane >> 4) + 4 * r;
        if (gi < K && gj < K) out[gi * K + gj] = acc[a][b][r];
      }
    }
}

// gram[i][j] = sum over the splits, in split order, of part[s][max(i, j)][min(i, j)]: every element of the lower
// triangle lies in a computed tile, and both halves read the same partials, so the matrix is exactly symmetric
__global__ __launch_bounds__(256) void k_krum_gram_sum(const double* __restrict__ part, int nsplit, int K,
                                                       double* __restrict__ gram) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t kk = (int64_t)K * K;
  if (idx >= kk) return;
  const int64_t i = idx / K, j = idx % K;
  const int64_t a = i > j ? i : j, b = i > j ? j : i;
  const double* p = part + a * K + b;
  double s = p[0];
  for (int sp = 1; sp < nsplit; ++sp) s = s + p[(int64_t)sp * kk];
  gram[idx] = s;
}

// ------------------------------------------------------------------------------------------------
// fk_scores
// ------------------------------------------------------------------------------------------------
// One workgroup per row i.  The K - 1 values of dist2 go to LDS, padded with +inf to n (a power of two); dist2 is
// never NaN and never -0, so an ascending bitonic sort has one result whatever it does with equal values; lane 0
// then adds the first K - f - 2 in order.
__global__ __launch_bounds__(256) void k_krum_scores(const double* __restrict__ gram, int K, int f, int n,
                                                     double* __restrict__ score) {
  extern __shared__ double sd[];  // [n]
  const int i = blockIdx.x;
  const double gii = gram[(int64_t)i * K + i];
  for (int s = threadIdx.x; s < n; s += 256) {
    double d = INFINITY;
    if (s < K - 1) {
      const int j = s < i ? s : s + 1;
      const double v = (gii + gram[(int64_t)j * K + j]) - 2.0 * gram[(int64_t)i * K + j];
      d = v != v ? (double)INFINITY : (v > 0.0 ? v : 0.0);
    }
    sd[s] = d;
  }
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int s = threadIdx.x; s < n; s += 256) {
        const int o = s ^ j;
        if (o > s) {
          const double a = sd[s], b = sd[o];
          const bool up = (s & k) == 0;
          if (up ? a > b : a < b) {
            sd[s] = b;
            sd[o] = a;
          }
        }
      }
      __syncthreads();
    }
  if (threadIdx.x == 0) {
    double sc = 0.0;
    const int cnt = K - f - 2;
    for (int s = 0; s < cnt; ++s) sc = sc + sd[s];
    score[i] = sc;
  }
}

// ------------------------------------------------------------------------------------------------
// fk_select
// ------------------------------------------------------------------------------------------------
// One workgroup: the scores in LDS, every thread ranks its rows against all K.  Scores are sums of non-negative
// non-NaN values, so the comparison is a total order.
__global__ __launch_bounds__(1024) void k_krum_select(const double* __restrict__ score, int K, int m,
                                                      float* __restrict__ c, int* __restrict__ n_sel) {
  extern __shared__ double ss[];  // [K]
  __shared__ int count;
  if (threadIdx.x == 0) count = 0;
  for (int i = threadIdx.x; i < K; i += 1024) ss[i] = score[i];
  __syncthreads();
  for (int i = threadIdx.x; i < K; i += 1024) {
    const double si = ss[i];
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const double sj = ss[j];
      rank += (sj < si || (sj == si && j < i)) ? 1 : 0;
    }
    const bool keep = si < (double)INFINITY && si == si && rank < m;
    c[i] = keep ? 1.0f : 0.0f;
    if (keep) atomicAdd(&count, 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) *n_sel = count;
}

// ------------------------------------------------------------------------------------------------
// fk_finish
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_krum_finish(const f4* __restrict__ chain, const f4* __restrict__ last,
                                                     const int* __restrict__ n_sel, int64_t P, float* out,
                                                     float* mirror) {
  const int n = *n_sel;
  const float denom = (float)n;
  const int64_t P4 = (P + 3) / 4;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < P4; c += (int64_t)gridDim.x * 256) {
    const f4 l = last[c];
    f4 o = l;
    if (n > 0) {
      const f4 ch = chain[c];
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = l[i] + __fdiv_rn(ch[i], denom);
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

int check_kp(const char* who, int32_t K, int64_t P) {
  if (K < 1 || P < 0) return refuse(FA_E_ARG, "%s: K=%d must be >= 1 and P=%lld >= 0", who, K, (long long)P);
  if (K > FK_MAX_K) return refuse(FA_E_ARG, "%s: K=%d rows, the kernels take at most %d (FK_MAX_K)", who, K, FK_MAX_K);
  return 0;
}

bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedkrum.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t fk_abi_version(void) { return FK_ABI_VERSION; }

extern "C" int64_t fk_gram_plan(int32_t K, int64_t P, int64_t* plan_out) {
  if (const int e = check_kp("fk_gram_plan", K, P)) return e;
  if (!plan_out) return refuse(FA_E_ARG, "fk_gram_plan: plan_out is NULL");
  const KrumPlan p = krum_plan(K, P);
  plan_out[0] = KB;
  plan_out[1] = p.tiles;
  plan_out[2] = p.nsplit;
  plan_out[3] = p.pchunk;
  plan_out[4] = KS;
  plan_out[5] = p.last_steps;
  return 0;
}

extern "C" int64_t fk_gram_workspace_bytes(int32_t K, int64_t P) {
  if (const int e = check_kp("fk_gram_workspace_bytes", K, P)) return e;
  return (int64_t)krum_plan(K, P).nsplit * K * K * 8;
}

extern "C" int fk_gram(const float* x, int64_t ld, int32_t K, int64_t P, const float* last, double* gram_out,
                       void* workspace, int64_t workspace_bytes, fa_stream_t stream) {
  if (const int e = check_kp("fk_gram", K, P)) return e;
  if (ld < P) return refuse(FA_E_ARG, "fk_gram: ld=%lld < P=%lld", (long long)ld, (long long)P);
  if (ld % 4 != 0) return refuse(FA_E_ARG, "fk_gram: ld=%lld must be a multiple of 4 elements", (long long)ld);
  if (!x || !last || !gram_out || !workspace) return refuse(FA_E_ARG, "fk_gram: x, last, gram_out or workspace is NULL");
  if (!aligned16(x) || !aligned16(last)) return refuse(FA_E_ARG, "fk_gram: x and last must be 16-byte aligned");
  if (!aligned8(gram_out) || !aligned8(workspace))
    return refuse(FA_E_ARG, "fk_gram: gram_out and workspace must be 8-byte aligned");
  const KrumPlan p = krum_plan(K, P);
  const int64_t need = (int64_t)p.nsplit * K * K * 8;
  if (workspace_bytes < need)
    return refuse(FA_E_ARG, "fk_gram: workspace of %lld bytes, K=%d P=%lld needs %lld (fk_gram_workspace_bytes)",
                  (long long)workspace_bytes, K, (long long)P, (long long)need);
  const int64_t P4 = (P + 3) / 4;
  FA_DEVICE_SCOPE("fk_gram", stream, gram_out);
  if (P > 0) {
    FA_OPERAND("x", x, (uint64_t)((int64_t)(K - 1) * ld + P4 * 4) * 4);
    FA_OPERAND("last", last, (uint64_t)P4 * 16);
  }
  FA_OPERAND("gram_out", gram_out, (uint64_t)K * K * 8);
  FA_OPERAND("workspace", workspace, (uint64_t)need);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_krum_gram, dim3(p.tiles, p.nsplit), dim3(256), 0, st, x, ld, (int)K, P, last, p.pchunk,
                     (double*)workspace);
  if (const int e = check_launch("fk_gram")) return e;
  const int64_t kk = (int64_t)K * K;
  hipLaunchKernelGGL(k_krum_gram_sum, dim3((unsigned)((kk + 255) / 256)), dim3(256), 0, st, (const double*)workspace,
                     p.nsplit, (int)K, gram_out);
  return check_launch("fk_gram (sum)");
}

extern "C" int fk_scores(const double* gram, int32_t K, int32_t f, double* score_out, fa_stream_t stream) {
  if (const int e = check_kp("fk_scores", K, 0)) return e;
  if (f < 0 || 2 * (int64_t)f + 3 > K) return refuse(FA_E_ARG, "fk_scores: f=%d needs 0 <= f and 2f + 3 <= K=%d", f, K);
  if (!gram || !score_out) return refuse(FA_E_ARG, "fk_scores: gram or score_out is NULL");
  if (!aligned8(gram) || !aligned8(score_out)) return refuse(FA_E_ARG, "fk_scores: gram and score_out must be 8-byte aligned");
  FA_DEVICE_SCOPE("fk_scores", stream, score_out);
  FA_OPERAND("gram", gram, (uint64_t)K * K * 8);
  FA_OPERAND("score_out", score_out, (uint64_t)K * 8);
  int n = 2;
  while (n < K - 1) n <<= 1;
  hipLaunchKernelGGL(k_krum_scores, dim3((unsigned)K), dim3(256), (size_t)n * 8, (hipStream_t)stream, gram, (int)K,
                     (int)f, n, score_out);
  return check_launch("fk_scores");
}

extern "C" int fk_select(const double* score, int32_t K, int32_t m, float* c_out, int32_t* n_sel_out,
                         fa_stream_t stream) {
  if (const int e = check_kp("fk_select", K, 0)) return e;
  if (m < 1 || m > K) return refuse(FA_E_ARG, "fk_select: m=%d needs 1 <= m <= K=%d", m, K);
  if (!score || !c_out || !n_sel_out) return refuse(FA_E_ARG, "fk_select: score, c_out or n_sel_out is NULL");
  if (!aligned8(score) || !aligned4(c_out) || !aligned4(n_sel_out))
    return refuse(FA_E_ARG, "fk_select: score must be 8-byte, c_out and n_sel_out 4-byte aligned");
  FA_DEVICE_SCOPE("fk_select", stream, c_out);
  FA_OPERAND("score", score, (uint64_t)K * 8);
  FA_OPERAND("c_out", c_out, (uint64_t)K * 4);
  FA_OPERAND("n_sel_out", n_sel_out, 4);
  hipLaunchKernelGGL(k_krum_select, dim3(1), dim3(1024), (size_t)K * 8, (hipStream_t)stream, score, (int)K, (int)m,
                     c_out, (int*)n_sel_out);
  return check_launch("fk_select");
}

extern "C" int fk_finish(const float* chain, const float* last, const int32_t* n_sel, int64_t P, float* out,
                         float* mirror, fa_stream_t stream) {
  if (P < 0) return refuse(FA_E_ARG, "fk_finish: negative P=%lld", (long long)P);
  if (!chain || !last || !n_sel || !out) return refuse(FA_E_ARG, "fk_finish: chain, last, n_sel or out is NULL");
  if (!aligned16(chain) || !aligned16(last)) return refuse(FA_E_ARG, "fk_finish: chain and last must be 16-byte aligned");
  if (!aligned16(out) || !aligned16(mirror)) return refuse(FA_E_ARG, "fk_finish: out and mirror must be 16-byte aligned");
  if (!aligned4(n_sel)) return refuse(FA_E_ARG, "fk_finish: n_sel must be 4-byte aligned");
  if (P == 0) return FA_OK;
  const int64_t P4 = (P + 3) / 4;
  FA_DEVICE_SCOPE("fk_finish", stream, out);
  FA_OPERAND("chain", chain, (uint64_t)P4 * 16);
  FA_OPERAND("last", last, (uint64_t)P4 * 16);
  FA_OPERAND("n_sel", n_sel, 4);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  FA_HOST_OK_OPERAND("mirror", mirror, (uint64_t)P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fk_finish: no CU count for device %d", fa_scope_device());
  int64_t g = (P4 + 255) / 256;
  if (g > (int64_t)cus * 8) g = (int64_t)cus * 8;
  hipLaunchKernelGGL(k_krum_finish, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const f4*>(chain), reinterpret_cast<const f4*>(last), (const int*)n_sel, P, out,
                     mirror);
  return check_launch("fk_finish");
}
