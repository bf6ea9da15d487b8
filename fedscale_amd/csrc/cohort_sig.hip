// cohort_sig.hip — MI355X (gfx950) kernels for Auxo's cohort-clustering features (include/fedcohort.h):
//   * fc_signature: the per-client gradient signature of examples/auxo/client_metadata.py:10-17
//     (W_old - W, the last len // 10 elements of the concatenation, cast to float16) for every staged upload
//     of a chunk, straight out of the round's staging area;
//   * fc_center / fc_normalize: client_manager.py:208-210 (np.mean over the K signatures, centre, sklearn
//     normalize) in numpy's order of operations;
//   * fc_gram: C * C^T of the float16 matrix on the f16 matrix unit, so that cosines and pairwise distances
//     leave the device as K x K instead of K x D.
//
// Numerics: every fp32 op is rounded as numpy rounds it (no FMA contraction); float -> float16 is the hardware
// conversion (round to nearest even, subnormals kept, overflow to inf); sums of squares are fp64 in a fixed
// order; the Gram accumulates exact f16 x f16 products in fp32, D split over workgroups and summed in split order.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/fedcohort.h"
#include "fa_device.h"
#include "fa_common.h"

namespace {

typedef _Float16 h16;
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));

// up to 8 float16 at p (the first nv are inside the matrix): one 16-byte load when `vec` and all 8 are valid
__device__ __forceinline__ h8 ld8(const h16* p, int nv, bool vec) {
  if (vec && nv == 8) return *(const h8*)p;
  h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (c < nv) v[c] = p[c];
  return v;
}
__device__ __forceinline__ void st8(h16* p, int nv, bool vec, h8 v) {
  if (vec && nv == 8) {
    *(h8*)p = v;
    return;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (c < nv) p[c] = v[c];
}

// ------------------------------------------------------------------------------------------------
// fc_signature
// ------------------------------------------------------------------------------------------------
constexpr int SG_MAX = 64;  // segments per launch (the table travels in the kernel arguments, 1.8 KiB)
constexpr int SG_THREADS = 256;
constexpr int64_t SG_CHUNK = SG_THREADS * 8;  // elements of one segment per workgroup

struct SegList {
  int64_t src[SG_MAX], dst[SG_MAX], len[SG_MAX];
  int32_t blk0[SG_MAX + 1];  // first workgroup of each segment; blk0[S] = grid.x
  int32_t S;
};
struct ISegList {
  int64_t dst[SG_MAX];
  int32_t q[SG_MAX];
  int32_t S;
};

__device__ __forceinline__ h16 sig1(float l, float x) { return (h16)(l - x); }

// grid (segment chunks, rows).  Per (row, segment): scalar elements up to the first 16-byte aligned address of
// x, groups of 8 from there (two 16-byte loads of x, streamed; `last` is re-read by every row and stays
// cacheable), scalar elements after the last whole group.  The float16 destination is misaligned against the
// source in general: 16-byte, 4-byte or 2-byte stores by its actual address.
__global__ __launch_bounds__(SG_THREADS) void k_signature(const float* __restrict__ x, int64_t ld, int n,
                                                          const float* __restrict__ last, SegList L,
                                                          h16* __restrict__ sig, int64_t ldd) {
  int lo = 0, hi = L.S - 1;  // largest s with blk0[s] <= blockIdx.x
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (L.blk0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int s = lo;
  const int b = blockIdx.x - L.blk0[s];
  const int64_t len = L.len[s];
  const float* ls = last + L.src[s];
  for (int row = blockIdx.y; row < n; row += gridDim.y) {
    const float* xs = x + (int64_t)row * ld + L.src[s];
    h16* out = sig + (int64_t)row * ldd + L.dst[s];
    int64_t pre = (4 - (((uintptr_t)xs >> 2) & 3)) & 3;
    if (pre > len) pre = len;
    const int64_t nbody = (len - pre) & ~(int64_t)7;
    const int64_t tail = len - pre - nbody;
    const int64_t i = (int64_t)b * SG_CHUNK + (int64_t)threadIdx.x * 8;
    if (i < nbody) {  // i + 8 <= nbody: both are multiples of 8
      const float* xp = xs + pre + i;
      const float* lp = ls + pre + i;
      const f4 a0 = __builtin_nontemporal_load((const f4*)xp);
      const f4 a1 = __builtin_nontemporal_load((const f4*)(xp + 4));
      f4 l0, l1;
      if (((uintptr_t)lp & 15) == 0) {
        l0 = *(const f4*)lp;
        l1 = *(const f4*)(lp + 4);
      } else {
        l0 = f4{lp[0], lp[1], lp[2], lp[3]};
        l1 = f4{lp[4], lp[5], lp[6], lp[7]};
      }
      const h8 v = {sig1(l0.x, a0.x), sig1(l0.y, a0.y), sig1(l0.z, a0.z), sig1(l0.w, a0.w),
                    sig1(l1.x, a1.x), sig1(l1.y, a1.y), sig1(l1.z, a1.z), sig1(l1.w, a1.w)};
      h16* op = out + pre + i;
      if (((uintptr_t)op & 15) == 0) {
        *(h8*)op = v;
      } else if (((uintptr_t)op & 3) == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) *(h2*)(op + 2 * c) = h2{v[2 * c], v[2 * c + 1]};
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) op[c] = v[c];
      }
    }
    if (b == 0) {  // the (at most 3 + 7) elements outside the aligned groups
      int64_t e = -1;
      if ((int64_t)threadIdx.x < pre) e = threadIdx.x;
      else if (threadIdx.x >= 32 && (int64_t)threadIdx.x - 32 < tail) e = pre + nbody + (threadIdx.x - 32);
      if (e >= 0) out[e] = sig1(ls[e], xs[e]);
    }
  }
}

// int64 entries inside the tail: numpy subtracts in int64 (wrapping), widens to float64 and casts to float16.
// Below 2^24 the difference is exact in fp32, so one rounding remains; at or above it every rounding stays
// beyond the float16 range and the cast gives +-inf either way.
__global__ __launch_bounds__(256) void k_signature_i64(const int64_t* __restrict__ xi, int ldq, int n,
                                                       const int64_t* __restrict__ last_i64, ISegList L,
                                                       h16* __restrict__ sig, int64_t ldd) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)n * L.S) return;
  const int row = (int)(t / L.S), e = (int)(t % L.S);
  const int q = L.q[e];
  const int64_t d = (int64_t)((uint64_t)last_i64[q] - (uint64_t)xi[(int64_t)row * ldq + q]);
  sig[(int64_t)row * ldd + L.dst[e]] = (h16)(float)(double)d;
}

// ------------------------------------------------------------------------------------------------
// fc_center: column mean (numpy's order), centring, per-row sums of squares
// ------------------------------------------------------------------------------------------------
constexpr int CT_THREADS = 256;              // fc_normalize
constexpr int64_t CT_COLS = CT_THREADS * 8;  // columns per workgroup (8 per thread: one 16-byte load per row)
constexpr int CW_COLS = 64 * 8;              // fc_center: one wave per workgroup, 512 columns over all K rows
constexpr int CT_SEG = 32;                   // first-level segments of the partial rows

// part: [gridDim.x][K] fp64, one row per workgroup (= wave): its 512 columns of every client.  A wave walks the K
// rows in order (the mean's chain is sequential in k), twice; the call's time follows K, not D.
__global__ __launch_bounds__(64) void k_center(const h16* __restrict__ sig, int64_t ldd, int K, int64_t D,
                                                       h16* __restrict__ avg, h16* __restrict__ cen,
                                                       double* __restrict__ part, int vec) {
  const int64_t j0 = (int64_t)blockIdx.x * CW_COLS + (int64_t)threadIdx.x * 8;
  const int64_t left = D - j0;
  const int nv = left >= 8 ? 8 : (left > 0 ? (int)left : 0);
  const h16* sp = sig + j0;
  // np.mean(list of float16 rows, axis=0): an fp32 accumulator that starts from the first row and adds the others
  // in order, then / K in fp32, then the cast back to float16
  float acc[8];
  {
    const h8 v = ld8(sp, nv, vec);
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = (float)v[c];
  }
#pragma unroll 8
  for (int k = 1; k < K; ++k) {
    const h8 v = ld8(sp + (int64_t)k * ldd, nv, vec);
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = acc[c] + (float)v[c];
  }
  const float fk = (float)K;
  h8 a16;
  float af[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    a16[c] = (h16)(acc[c] / fk);
    af[c] = (float)a16[c];
  }
  st8(avg + j0, nv, vec, a16);
  const int lane = threadIdx.x;
  double* prow = part + (int64_t)blockIdx.x * K;
  for (int k = 0; k < K; ++k) {
    const h8 v = ld8(sp + (int64_t)k * ldd, nv, vec);
    h8 c16;
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      c16[c] = (h16)((float)v[c] - af[c]);
      const float cf = (float)c16[c];
      if (c < nv) s += (double)(cf * cf);  // an f16 square is exact in fp32
    }
    st8(cen + (int64_t)k * ldd + j0, nv, vec, c16);
    s = wave_sum(s);
    if (lane == 0) prow[k] = s;
  }
}

// seg[y][k] = sum of partial rows [y * per, (y + 1) * per) of client k, in row order
__global__ __launch_bounds__(256) void k_center_seg(const double* __restrict__ part, int64_t nrows, int64_t per, int K,
                                                    double* __restrict__ seg) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  const int64_t r0 = (int64_t)blockIdx.y * per;
  const int64_t r1 = r0 + per < nrows ? r0 + per : nrows;
  double s = 0.0;
  for (int64_t r = r0; r < r1; ++r) s += part[r * K + k];
  seg[(int64_t)blockIdx.y * K + k] = s;
}
__global__ __launch_bounds__(256) void k_center_sum(const double* __restrict__ seg, int K, double* __restrict__ sumsq) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  double s = 0.0;
  for (int y = 0; y < CT_SEG; ++y) s += seg[(int64_t)y * K + k];
  sumsq[k] = s;
}

int64_t center_rows(int64_t D) { return (D + CW_COLS - 1) / CW_COLS; }

// ------------------------------------------------------------------------------------------------
// fc_normalize
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CT_THREADS) void k_normalize(const h16* cen, int64_t ldd, int K, int64_t D,
                                                          const double* __restrict__ norm, h16* out, int vec) {
  const int64_t j0 = (int64_t)blockIdx.x * CT_COLS + (int64_t)threadIdx.x * 8;
  const int64_t left = D - j0;
  if (left <= 0) return;
  const int nv = left >= 8 ? 8 : (int)left;
  for (int k = blockIdx.y; k < K; k += gridDim.y) {
    double nd = norm[k];
    if (nd == 0.0) nd = 1.0;  // sklearn's normalize leaves an all-zero row as it is
    const float nf = (float)nd;
    const h8 v = ld8(cen + (int64_t)k * ldd + j0, nv, vec);
    h8 o;
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = (h16)((float)v[c] / nf);
    st8(out + (int64_t)k * ldd + j0, nv, vec, o);
  }
}

// ------------------------------------------------------------------------------------------------
// fc_gram
// ------------------------------------------------------------------------------------------------
constexpr int GB = 64;   // rows of a tile side (a workgroup computes GB x GB, each of its 4 waves 32 x 32)
constexpr int GK = 64;   // float16 of D per step
constexpr int GP = 72;   // LDS row pitch in float16 (144 B: 16-byte aligned rows, 4 banks apart)
constexpr int64_t G_TARGET_WGS = 2048;
constexpr int64_t G_MAX_WS = (int64_t)512 << 20;

struct GramPlan {
  int tiles;       // lower-triangle tiles
  int nsplit;      // workgroups along D
  int64_t dchunk;  // float16 of D per workgroup (a multiple of GK)
};
GramPlan gram_plan(int K, int64_t D) {
  const int T = (K + GB - 1) / GB;
  GramPlan p;
  p.tiles = T * (T + 1) / 2;
  const int64_t steps = D > 0 ? (D + GK - 1) / GK : 1;
  int64_t ns = (G_TARGET_WGS + p.tiles - 1) / p.tiles;
  if (ns > steps) ns = steps;
  const int64_t one = (int64_t)K * K * 4;
  while (ns > 1 && ns * one > G_MAX_WS) --ns;
  const int64_t per = (steps + ns - 1) / ns;
  p.dchunk = per * GK;
  p.nsplit = (int)((steps + per - 1) / per);
  return p;
}

// part[split][i][j] for the tile (I, J <= I) of blockIdx.x over columns [split * dchunk, + dchunk) of c.
// Lane l of a wave (r = l & 31, h = l >> 5) holds A[row r][k = 8h .. 8h + 7] and B[k = 8h ..][col r] of a
// 32x32x16 step: both are 8 consecutive float16 of a row of c, read from the LDS image of the tile.
__global__ __launch_bounds__(256) void k_gram_partial(const h16* __restrict__ c, int64_t ldd, int K, int64_t D,
                                                      int64_t dchunk, float* __restrict__ part, int vec) {
  __shared__ __attribute__((aligned(16))) h16 sA[GB * GP];
  __shared__ __attribute__((aligned(16))) h16 sB[GB * GP];
  const int t = blockIdx.x;
  int I = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  const int J = t - I * (I + 1) / 2;
  const int64_t d0 = (int64_t)blockIdx.y * dchunk;
  const int64_t d1 = d0 + dchunk < D ? d0 + dchunk : D;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wi = wave >> 1, wj = wave & 1;
  // this thread's two 8-element pieces of a 64 x 64 step of either matrix
  const int r0 = threadIdx.x >> 3, r1 = r0 + 32, kc = (threadIdx.x & 7) * 8;
  const int64_t ia0 = (int64_t)I * GB + r0, ia1 = (int64_t)I * GB + r1;
  const int64_t ib0 = (int64_t)J * GB + r0, ib1 = (int64_t)J * GB + r1;
  h8 ra0, ra1, rb0, rb1;
  auto fetch = [&](int64_t dk) {
    const int64_t d = dk + kc;
    const int64_t left = d1 - d;
    const int nv = left >= 8 ? 8 : (left > 0 ? (int)left : 0);
    ra0 = ld8(c + ia0 * ldd + d, ia0 < K ? nv : 0, vec);
    ra1 = ld8(c + ia1 * ldd + d, ia1 < K ? nv : 0, vec);
    rb0 = ld8(c + ib0 * ldd + d, ib0 < K ? nv : 0, vec);
    rb1 = ld8(c + ib1 * ldd + d, ib1 < K ? nv : 0, vec);
  };
  f16v acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  if (d0 < d1) fetch(d0);
  const h16* pa = sA + (wi * 32 + (lane & 31)) * GP + (lane >> 5) * 8;
  const h16* pb = sB + (wj * 32 + (lane & 31)) * GP + (lane >> 5) * 8;
  for (int64_t dk = d0; dk < d1; dk += GK) {
    __syncthreads();  // the previous step's fragments have been read
    *(h8*)(sA + r0 * GP + kc) = ra0;
    *(h8*)(sA + r1 * GP + kc) = ra1;
    *(h8*)(sB + r0 * GP + kc) = rb0;
    *(h8*)(sB + r1 * GP + kc) = rb1;
    __syncthreads();
    if (dk + GK < d1) fetch(dk + GK);  // in flight under the MFMAs
#pragma unroll
    for (int kk = 0; kk < GK / 16; ++kk) {
      const h8 a = *(const h8*)(pa + kk * 16);
      const h8 b = *(const h8*)(pb + kk * 16);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
    }
  }
  float* out = part + (int64_t)blockIdx.y * K * K;
  const int64_t gj = (int64_t)J * GB + wj * 32 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t gi = (int64_t)I * GB + wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (gi < K && gj < K) out[gi * K + gj] = acc[r];
  }
}

// gram[i][j] = sum over the splits, in split order, of part[s][max(i, j)][min(i, j)]: every element of the lower
// triangle lies in a computed tile, and both halves read the same partials, so the matrix is exactly symmetric
__global__ __launch_bounds__(256) void k_gram_reduce(const float* __restrict__ part, int nsplit, int K,
                                                     float* __restrict__ gram) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t kk = (int64_t)K * K;
  if (idx >= kk) return;
  const int64_t i = idx / K, j = idx % K;
  const int64_t a = i > j ? i : j, b = i > j ? j : i;
  const float* p = part + a * K + b;
  float s = p[0];
  for (int sp = 1; sp < nsplit; ++sp) s = s + p[(int64_t)sp * kk];
  gram[idx] = s;
}

bool vec_ok(const void* p, int64_t ldd) { return ((uintptr_t)p & 15) == 0 && ldd % 8 == 0; }

}  // namespace

extern "C" int32_t fc_abi_version(void) { return FC_ABI_VERSION; }

extern "C" int fc_signature(const float* x, int64_t ld, int32_t n, const float* last, const int64_t* xi, int32_t ldq,
                            const int64_t* last_i64, const int64_t* segs, int32_t nseg, const int64_t* isegs,
                            int32_t niseg, void* sig_out, int64_t ldd, fa_stream_t stream) {
  if (n < 0 || nseg < 0 || niseg < 0 || ld < 1 || ldd < 1 || !sig_out)
    return fail(FA_E_ARG, "fc_signature: bad arguments (n=%d nseg=%d niseg=%d ld=%lld ldd=%lld sig_out=%p)", n, nseg,
                niseg, (long long)ld, (long long)ldd, sig_out);
  if ((nseg > 0 && (!segs || !x || !last)) || (niseg > 0 && (!isegs || !xi || !last_i64 || ldq < 1)))
    return fail(FA_E_ARG, "fc_signature: NULL operand for a non-empty segment table");
  if (((uintptr_t)x & 3) || ((uintptr_t)last & 3) || ((uintptr_t)xi & 7) || ((uintptr_t)last_i64 & 7) ||
      ((uintptr_t)sig_out & 1))
    return fail(FA_E_ARG, "fc_signature: misaligned operand (x / last 4, xi / last_i64 8, sig_out 2 bytes)");
  int64_t max_src = 0, max_dst = 0, max_q = -1;
  for (int s = 0; s < nseg; ++s) {
    const int64_t src = segs[3 * s], dst = segs[3 * s + 1], len = segs[3 * s + 2];
    if (src < 0 || dst < 0 || len < 0 || len > ld || src > ld - len || len > ldd || dst > ldd - len)
      return fail(FA_E_ARG, "fc_signature: segment %d (src %lld, dst %lld, len %lld) outside ld=%lld / ldd=%lld", s,
                  (long long)src, (long long)dst, (long long)len, (long long)ld, (long long)ldd);
    if (len > 0 && src + len > max_src) max_src = src + len;
    if (len > 0 && dst + len > max_dst) max_dst = dst + len;
  }
  for (int e = 0; e < niseg; ++e) {
    const int64_t q = isegs[2 * e], dst = isegs[2 * e + 1];
    if (q < 0 || q >= ldq || dst < 0 || dst >= ldd)
      return fail(FA_E_ARG, "fc_signature: int64 element %d (side index %lld, dst %lld) outside ldq=%d / ldd=%lld", e,
                  (long long)q, (long long)dst, ldq, (long long)ldd);
    if (q > max_q) max_q = q;
    if (dst + 1 > max_dst) max_dst = dst + 1;
  }
  if (n == 0 || max_dst == 0) return FA_OK;
  FA_DEVICE_SCOPE("fc_signature", stream, sig_out);
  if (max_src > 0) {
    FA_HOST_OK_OPERAND("x", x, ((uint64_t)(n - 1) * ld + max_src) * 4);
    FA_OPERAND("last", last, (uint64_t)max_src * 4);
  }
  if (max_q >= 0) {
    FA_HOST_OK_OPERAND("xi", xi, ((uint64_t)(n - 1) * ldq + max_q + 1) * 8);
    FA_OPERAND("last_i64", last_i64, (uint64_t)(max_q + 1) * 8);
  }
  FA_OPERAND("sig_out", sig_out, ((uint64_t)(n - 1) * ldd + max_dst) * 2);
  hipStream_t st = (hipStream_t)stream;
  const int gy = n < 65535 ? n : 65535;
  for (int s0 = 0; s0 < nseg;) {
    SegList L;
    int S = 0;
    int64_t blk = 0;
    for (; s0 < nseg && S < SG_MAX; ++s0) {
      const int64_t len = segs[3 * s0 + 2];
      if (len == 0) continue;
      const int64_t nb = (len + SG_CHUNK - 1) / SG_CHUNK;
      if (blk + nb > 0x7fffff00) break;  // (a further launch takes the rest)
      L.src[S] = segs[3 * s0];
      L.dst[S] = segs[3 * s0 + 1];
      L.len[S] = len;
      L.blk0[S] = (int32_t)blk;
      blk += nb;
      ++S;
    }
    if (S == 0) {
      if (s0 < nseg) return fail(FA_E_ARG, "fc_signature: segment %d is too long for one launch", s0);
      break;
    }
    L.blk0[S] = (int32_t)blk;
    L.S = S;
    hipLaunchKernelGGL(k_signature, dim3((unsigned)blk, gy), dim3(SG_THREADS), 0, st, x, ld, (int)n, last, L,
                       (h16*)sig_out, ldd);
    const int e = check_launch("fc_signature");
    if (e) return e;
  }
  for (int e0 = 0; e0 < niseg; e0 += SG_MAX) {
    ISegList L;
    L.S = niseg - e0 < SG_MAX ? niseg - e0 : SG_MAX;
    for (int e = 0; e < L.S; ++e) {
      L.q[e] = (int32_t)isegs[2 * (e0 + e)];
      L.dst[e] = isegs[2 * (e0 + e) + 1];
    }
    const int64_t total = (int64_t)n * L.S;
    hipLaunchKernelGGL(k_signature_i64, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, xi, (int)ldq, (int)n,
                       last_i64, L, (h16*)sig_out, ldd);
    const int e = check_launch("fc_signature (int64 entries)");
    if (e) return e;
  }
  return FA_OK;
}

extern "C" int64_t fc_center_workspace_bytes(int32_t K, int64_t D) {
  if (K < 1 || D < 0) return 0;
  return (center_rows(D) + CT_SEG) * (int64_t)K * 8;
}

extern "C" int fc_center(const void* sig, int64_t ldd, int32_t K, int64_t D, void* avg16_out, void* centered_out,
                         double* sumsq_out, void* workspace, fa_stream_t stream) {
  if (K < 1 || D < 0 || ldd < D || ldd < 1 || !sig || !avg16_out || !centered_out || !sumsq_out || !workspace)
    return fail(FA_E_ARG, "fc_center: bad arguments (K=%d D=%lld ldd=%lld)", K, (long long)D, (long long)ldd);
  if (((uintptr_t)sig & 1) || ((uintptr_t)avg16_out & 1) || ((uintptr_t)centered_out & 1) ||
      ((uintptr_t)sumsq_out & 7) || ((uintptr_t)workspace & 7))
    return fail(FA_E_ARG, "fc_center: misaligned operand");
  if (sig == centered_out) return fail(FA_E_ARG, "fc_center: centered_out may not alias sig");
  FA_DEVICE_SCOPE("fc_center", stream, centered_out);
  const uint64_t mbytes = ((uint64_t)(K - 1) * ldd + D) * 2;
  FA_OPERAND("sig", sig, mbytes);
  FA_OPERAND("avg16_out", avg16_out, (uint64_t)D * 2);
  FA_OPERAND("centered_out", centered_out, mbytes);
  FA_OPERAND("sumsq_out", sumsq_out, (uint64_t)K * 8);
  FA_OPERAND("workspace", workspace, (uint64_t)fc_center_workspace_bytes(K, D));
  hipStream_t st = (hipStream_t)stream;
  const int64_t nrows = center_rows(D);
  double* part = (double*)workspace;
  double* seg = part + nrows * K;
  if (nrows > 0) {
    const int vec = vec_ok(sig, ldd) && vec_ok(centered_out, ldd) && vec_ok(avg16_out, 8);
    hipLaunchKernelGGL(k_center, dim3((unsigned)nrows), dim3(64), 0, st, (const h16*)sig, ldd,
                       (int)K, D, (h16*)avg16_out, (h16*)centered_out, part, vec);
    const int e = check_launch("fc_center");
    if (e) return e;
  }
  const int64_t per = (nrows + CT_SEG - 1) / CT_SEG;
  hipLaunchKernelGGL(k_center_seg, dim3((K + 255) / 256, CT_SEG), dim3(256), 0, st, (const double*)part, nrows, per,
                     (int)K, seg);
  int e = check_launch("fc_center (partials)");
  if (e) return e;
  hipLaunchKernelGGL(k_center_sum, dim3((K + 255) / 256), dim3(256), 0, st, (const double*)seg, (int)K, sumsq_out);
  return check_launch("fc_center (sum)");
}

extern "C" int fc_normalize(const void* centered, int64_t ldd, int32_t K, int64_t D, const double* norm_in,
                            void* normalized_out, fa_stream_t stream) {
  if (K < 1 || D < 0 || ldd < D || ldd < 1 || !centered || !norm_in || !normalized_out)
    return fail(FA_E_ARG, "fc_normalize: bad arguments (K=%d D=%lld ldd=%lld)", K, (long long)D, (long long)ldd);
  if (((uintptr_t)centered & 1) || ((uintptr_t)normalized_out & 1) || ((uintptr_t)norm_in & 7))
    return fail(FA_E_ARG, "fc_normalize: misaligned operand");
  if (D == 0) return FA_OK;
  FA_DEVICE_SCOPE("fc_normalize", stream, normalized_out);
  const uint64_t mbytes = ((uint64_t)(K - 1) * ldd + D) * 2;
  FA_OPERAND("centered", centered, mbytes);
  FA_OPERAND("norm_in", norm_in, (uint64_t)K * 8);
  FA_OPERAND("normalized_out", normalized_out, mbytes);
  const int vec = vec_ok(centered, ldd) && vec_ok(normalized_out, ldd);
  hipLaunchKernelGGL(k_normalize, dim3((unsigned)((D + CT_COLS - 1) / CT_COLS), K < 65535 ? K : 65535),
                     dim3(CT_THREADS), 0, (hipStream_t)stream, (const h16*)centered, ldd, (int)K, D, norm_in,
                     (h16*)normalized_out, vec);
  return check_launch("fc_normalize");
}

extern "C" int64_t fc_gram_workspace_bytes(int32_t K, int64_t D) {
  if (K < 1 || K > FC_GRAM_MAX_K || D < 0) return 0;
  return (int64_t)gram_plan(K, D).nsplit * K * K * 4;
}

extern "C" int fc_gram(const void* c, int64_t ldd, int32_t K, int64_t D, float* gram_out, void* workspace,
                       fa_stream_t stream) {
  if (K < 1 || D < 0 || ldd < D || ldd < 1 || !c || !gram_out || !workspace)
    return fail(FA_E_ARG, "fc_gram: bad arguments (K=%d D=%lld ldd=%lld)", K, (long long)D, (long long)ldd);
  if (K > FC_GRAM_MAX_K)
    return fail(FA_E_ARG, "fc_gram: K=%d rows, the kernel takes at most %d (FC_GRAM_MAX_K)", K, FC_GRAM_MAX_K);
  if (((uintptr_t)c & 1) || ((uintptr_t)gram_out & 3) || ((uintptr_t)workspace & 15))
    return fail(FA_E_ARG, "fc_gram: misaligned operand");
  FA_DEVICE_SCOPE("fc_gram", stream, gram_out);
  FA_OPERAND("c", c, ((uint64_t)(K - 1) * ldd + D) * 2);
  FA_OPERAND("gram_out", gram_out, (uint64_t)K * K * 4);
  FA_OPERAND("workspace", workspace, (uint64_t)fc_gram_workspace_bytes(K, D));
  const GramPlan p = gram_plan(K, D);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gram_partial, dim3(p.tiles, p.nsplit), dim3(256), 0, st, (const h16*)c, ldd, (int)K, D,
                     p.dchunk, (float*)workspace, (int)vec_ok(c, ldd));
  const int e = check_launch("fc_gram");
  if (e) return e;
  const int64_t kk = (int64_t)K * K;
  hipLaunchKernelGGL(k_gram_reduce, dim3((unsigned)((kk + 255) / 256)), dim3(256), 0, st, (const float*)workspace,
                     p.nsplit, (int)K, gram_out);
  return check_launch("fc_gram (reduce)");
}
