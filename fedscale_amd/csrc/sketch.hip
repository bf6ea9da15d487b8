// sketch.hip — MI355X (gfx950) kernels of the Count-Sketch upload path (include/fedsketch.h), FetchSGD rounds:
//   * fcs_sketch_row: the blocked Count Sketch of one fp32 row (minus a base, plus a residual), or — with
//     FCS_SUBTRACT_FROM — that sketch subtracted from a table in place;
//   * fcs_estimate: the median-of-R estimate of every column read back out of a table;
//   * fcs_state_step: the momentum and error-feedback tables of a round, and the count of non-finite sums;
//   * fcs_apply: the k recovered pairs densified for the closing sketch, and added to the model.
//
// Both hash-driven kernels are gathers whose address algebra keeps every access a whole aligned 16-byte one.  A
// bucket q of row j takes from block b the column b C + (q ^ m), m the block's mask: an xor maps an aligned
// power-of-two run of buckets onto an aligned run of columns, so a workgroup's tile of buckets is, in every block, one
// aligned tile of columns (the one at tile index ^ (m >> log2 tile)); inside it the mask's bits 2.. permute lanes and
// its bits 0-1 permute the four components of a lane's float4 — a register select.  A lane owns four consecutive
// buckets for the whole chain over the blocks: no atomics, no LDS, nothing crosses lanes, and the result does not
// depend on the launch.  The chain is a dependent add per block, so a lane keeps FCS_U blocks' loads in flight ahead
// of their adds and computes those blocks' masks and sign words (two splitmix64 each, the mask's on the scalar unit:
// it depends on the row and the block alone) while the loads fly.  The estimate is the same algebra read backwards:
// a workgroup's 1024 columns lie in one block, its R masks are scalars, and a lane gathers R float4s of a table that
// sits in L2 / Infinity Cache, takes the median of their order-preserving integer keys in registers and stores one
// float4.
//
// Numerics: every fp32 op is rounded to nearest and never contracted into an FMA; the default denormal modes are kept.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fedsketch.h"
#include "fa_device.h"
#include "fa_common.h"

// Tuning knob (tools/sketch_measure.py per library, FEDAGG_LIB).  FCS_SHARE_SIGN: the sign word of a
// block, which the 16 lanes of an aligned group share, is hashed by one of them (lane i takes block i & 7 of the load
// group) and read across lanes, instead of by every lane — one hash and sixteen cross-lane reads per lane and group
// in place of eight hashes.  Level at 25 M columns and faster at 1 M, each library in a run of its own
// (profiles/sketch_measure_share_sign.json): off until the two alternate in one run.
#if defined(FCS_SHARE_SIGN)
#if !defined(FA_TUNING) || !FA_TUNING
#error "FCS_SHARE_SIGN is a tuning knob: build with -DFA_TUNING=1"
#endif
#endif
#ifndef FCS_SHARE_SIGN
#define FCS_SHARE_SIGN 0
#endif

namespace {

constexpr uint64_t FCS_G = 0xD1B54A32D192ED03ull;
constexpr int EST_THREADS = 256;  // k_estimate: 1024 columns per workgroup, which divides every C: one block

// A float's bits and back.  By value, on purpose: __builtin_bit_cast applied directly to a vector's component (v.y)
// reads the vector's first component with this compiler.
__device__ __forceinline__ uint32_t fbits(float f) { return __builtin_bit_cast(uint32_t, f); }
__device__ __forceinline__ float bfloat(uint32_t u) { return __builtin_bit_cast(float, u); }

// splitmix64 over the word w (fedrotate.h's)
__host__ __device__ __forceinline__ uint64_t mix(uint64_t s, uint64_t w) {
  uint64_t z = s + (w + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t sign_seed(uint64_t seed, int j) { return seed + (uint64_t)(2 * j + 1) * FCS_G; }
__device__ __forceinline__ uint64_t mask_seed(uint64_t seed, int j) { return seed + (uint64_t)(2 * j + 2) * FCS_G; }

// the four sign bits of the columns p .. p + 3 (p a multiple of 4: they lie in one 64-column word)
__device__ __forceinline__ uint32_t sign_bits(uint64_t sseed, int64_t p) {
  return (uint32_t)(mix(sseed, (uint64_t)p >> 6) >> (p & 63)) & 15u;
}
// bit i of d xored into component i's sign bit
__device__ __forceinline__ f4 sign_apply(f4 v, uint32_t d) {
  v.x = bfloat(fbits(v.x) ^ ((d & 1u) << 31));
  v.y = bfloat(fbits(v.y) ^ ((d & 2u) << 30));
  v.z = bfloat(fbits(v.z) ^ ((d & 4u) << 29));
  v.w = bfloat(fbits(v.w) ^ ((d & 8u) << 28));
  return v;
}
// out[i] = v[i ^ (m & 3)]: the mask's two low bits permute a float4's components (an involution)
__device__ __forceinline__ f4 comp_xor(f4 v, uint32_t m) {
  if (m & 1u) v = f4{v.y, v.x, v.w, v.z};
  if (m & 2u) v = f4{v.z, v.w, v.x, v.y};
  return v;
}

// ------------------------------------------------------------------------------------------------
// k_sketch
// ------------------------------------------------------------------------------------------------
// (A residual r_in is taken for the executor's signature only — the FetchSGD path has none, so the RIN variants are
// on no hot path and are not tuned: with a base and a residual the compiler holds 122 VGPRs and serialises loads.)
// FCS_U whole blocks b0 .. b0 + FCS_U - 1 (FULL), or those of them below nfull: all their loads are issued, then
// their sign words are hashed, then the chain takes them in block order.
template <bool BASE, bool RIN, bool FULL>
__device__ __forceinline__ void sketch_group(const float* __restrict__ x, const float* __restrict__ base,
                                             const float* __restrict__ rin, int64_t b0, int64_t nfull, int c,
                                             uint32_t q0, uint64_t sseed, uint64_t mseed, f4& acc) {
  const uint32_t cm = (1u << c) - 1u;
  f4 v[FCS_U], l[FCS_U], r[FCS_U];
  uint32_t m[FCS_U], d[FCS_U];
  int64_t p[FCS_U];
#pragma unroll
  for (int u = 0; u < FCS_U; ++u) {
    if (!FULL && b0 + u >= nfull) continue;
    m[u] = (uint32_t)mix(mseed, (uint64_t)(b0 + u)) & cm;
    p[u] = ((b0 + u) << c) + (int64_t)(q0 ^ (m[u] & ~3u));
    v[u] = *reinterpret_cast<const f4*>(x + p[u]);
    if (BASE) l[u] = *reinterpret_cast<const f4*>(base + p[u]);
    if (RIN) r[u] = *reinterpret_cast<const f4*>(rin + p[u]);
  }
#if FCS_SHARE_SIGN
  static_assert(FCS_U == 8, "a group of 16 lanes shares the words of 8 blocks");
  const int lane = threadIdx.x & 63;
  int64_t pm = (FULL || b0 < nfull) ? p[0] : 0;
#pragma unroll
  for (int u = 1; u < FCS_U; ++u)
    if ((FULL || b0 + u < nfull) && (lane & (FCS_U - 1)) == u) pm = p[u];
  const uint64_t word = mix(sseed, (uint64_t)pm >> 6);
#pragma unroll
  for (int u = 0; u < FCS_U; ++u) {
    if (!FULL && b0 + u >= nfull) continue;
    const uint64_t w = __shfl((unsigned long long)word, (lane & 48) | u, 64);
    d[u] = (uint32_t)(w >> (p[u] & 63)) & 15u;
  }
#else
#pragma unroll
  for (int u = 0; u < FCS_U; ++u) {
    if (!FULL && b0 + u >= nfull) continue;
    d[u] = sign_bits(sseed, p[u]);
  }
#endif
#pragma unroll
  for (int u = 0; u < FCS_U; ++u) {
    if (!FULL && b0 + u >= nfull) continue;
    f4 e = v[u];
    if (BASE) e = e - l[u];
    if (RIN) e = e + r[u];
    acc = acc + comp_xor(sign_apply(e, d[u]), m[u]);
  }
}

// Workgroup (blockIdx.x, blockIdx.y) owns the buckets [blockIdx.x * tile, + tile) of row blockIdx.y, tile = 4 *
// blockDim.x; gridDim.x * tile == C.  Whole blocks take whole float4 loads (every column below P); the ragged last
// block loads and adds per component, masked against P.
template <bool BASE, bool RIN>
__global__ __launch_bounds__(FCS_TILE / 4) void k_sketch(const float* __restrict__ x, const float* __restrict__ base,
                                                         const float* __restrict__ rin, int64_t P, int c,
                                                         uint64_t seed, float* table, int subtract) {
  const int j = blockIdx.y;
  const uint32_t q0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4u;
  const uint64_t sseed = sign_seed(seed, j), mseed = mask_seed(seed, j);
  const int64_t nfull = P >> c;
  f4 acc = f4{0.f, 0.f, 0.f, 0.f};
  int64_t b0 = 0;
  for (; b0 + FCS_U <= nfull; b0 += FCS_U)
    sketch_group<BASE, RIN, true>(x, base, rin, b0, nfull, c, q0, sseed, mseed, acc);
  if (b0 < nfull) sketch_group<BASE, RIN, false>(x, base, rin, b0, nfull, c, q0, sseed, mseed, acc);
  const int64_t rag = P - (nfull << c);  // columns of the ragged last block
  if (rag > 0) {
    const uint32_t m = (uint32_t)mix(mseed, (uint64_t)nfull) & ((1u << c) - 1u);
    const uint32_t a = q0 ^ (m & ~3u);
    const int64_t p = (nfull << c) + a;
    float e[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t have = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if ((int64_t)a + i < rag) {
        float t = x[p + i];
        if (BASE) t = t - base[p + i];
        if (RIN) t = t + rin[p + i];
        e[i] = t;
        have |= 1u << i;
      }
    }
    if (have) {  // (whole waves skip the hash when their columns lie past P)
      const f4 t = comp_xor(sign_apply(f4{e[0], e[1], e[2], e[3]}, sign_bits(sseed, p)), m);
      const uint32_t mm = m & 3u;  // bucket i takes component i ^ mm, when that column exists
      if ((have >> (0u ^ mm)) & 1u) acc.x = acc.x + t.x;
      if ((have >> (1u ^ mm)) & 1u) acc.y = acc.y + t.y;
      if ((have >> (2u ^ mm)) & 1u) acc.z = acc.z + t.z;
      if ((have >> (3u ^ mm)) & 1u) acc.w = acc.w + t.w;
    }
  }
  f4* dst = reinterpret_cast<f4*>(table + ((int64_t)j << c) + q0);
  if (subtract) acc = *dst - acc;
  *dst = acc;
}

// ------------------------------------------------------------------------------------------------
// k_estimate
// ------------------------------------------------------------------------------------------------
// order-preserving key of a float's bits, and back
__device__ __forceinline__ uint32_t key_of(float f) {
  const uint32_t b = fbits(f);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float of_key(uint32_t k) { return bfloat(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t med3(uint32_t a, uint32_t b, uint32_t c) {  // v_med3_u32
  return umax(umin(a, b), umin(umax(a, b), c));
}
__device__ __forceinline__ void cswap(uint32_t& a, uint32_t& b) {
  const uint32_t lo = umin(a, b);
  b = umax(a, b);
  a = lo;
}
template <int R>
__device__ __forceinline__ uint32_t median(uint32_t k[R]) {
  if (R == 1) return k[0];
  if (R == 3) return med3(k[0], k[1], k[2]);
  if (R == 5)
    return med3(k[4], umax(umin(k[0], k[1]), umin(k[2], k[3])), umin(umax(k[0], k[1]), umax(k[2], k[3])));
  // R == 7: thirteen compare-exchanges that leave the median in k[3]
  cswap(k[0], k[5]); cswap(k[0], k[3]); cswap(k[1], k[6]); cswap(k[2], k[4]); cswap(k[0], k[1]);
  cswap(k[3], k[5]); cswap(k[2], k[6]); cswap(k[2], k[3]); cswap(k[3], k[6]); cswap(k[4], k[5]);
  cswap(k[1], k[4]); cswap(k[1], k[3]); cswap(k[3], k[4]);
  return k[3];
}

// A lane owns the columns p0 .. p0 + 3; the workgroup's 1024 columns lie in one block, so the masks are scalars.
template <int R>
__global__ __launch_bounds__(EST_THREADS) void k_estimate(const float* __restrict__ table, int64_t P, int c,
                                                          uint64_t seed, float* __restrict__ est) {
  const int64_t w0 = (int64_t)blockIdx.x * (4 * EST_THREADS);
  const int64_t p0 = w0 + 4 * threadIdx.x;
  if (p0 >= P) return;
  const uint64_t b = (uint64_t)(w0 >> c);
  const uint32_t cm = (1u << c) - 1u;
  const uint32_t u0 = (uint32_t)p0 & cm;
  f4 t[R];
  uint32_t m[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    m[j] = (uint32_t)mix(mask_seed(seed, j), b) & cm;
    t[j] = *reinterpret_cast<const f4*>(table + ((int64_t)j << c) + (u0 ^ (m[j] & ~3u)));
  }
  uint32_t kx[R], ky[R], kz[R], kw[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const f4 v = sign_apply(comp_xor(t[j], m[j]), sign_bits(sign_seed(seed, j), p0));
    kx[j] = key_of(v.x);
    ky[j] = key_of(v.y);
    kz[j] = key_of(v.z);
    kw[j] = key_of(v.w);
  }
  const f4 o = f4{of_key(median<R>(kx)), of_key(median<R>(ky)), of_key(median<R>(kz)), of_key(median<R>(kw))};
  if (p0 + 4 <= P) {
    *reinterpret_cast<f4*>(est + p0) = o;
  } else {  // the last, partial float4: columns >= P are not written
    est[p0] = o.x;
    if (p0 + 1 < P) est[p0 + 1] = o.y;
    if (p0 + 2 < P) est[p0 + 2] = o.z;
  }
}

// ------------------------------------------------------------------------------------------------
// k_state_step, k_apply_*
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t nonfinite(float f) { return (fbits(f) & 0x7F800000u) == 0x7F800000u ? 1u : 0u; }

__global__ __launch_bounds__(256) void k_state_step(const float* __restrict__ s, const float* su_in,
                                                    const float* se_in, float rho, int64_t n4, float* su_out,
                                                    float* se_out, uint32_t* bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const f4 sv = reinterpret_cast<const f4*>(s)[i];
  f4 u = reinterpret_cast<const f4*>(su_in)[i] * rho;
  u = u + sv;
  const f4 e = reinterpret_cast<const f4*>(se_in)[i] + u;
  reinterpret_cast<f4*>(su_out)[i] = u;
  reinterpret_cast<f4*>(se_out)[i] = e;
  const uint32_t nb = nonfinite(sv.x) + nonfinite(sv.y) + nonfinite(sv.z) + nonfinite(sv.w);
  if (nb) atomicAdd(bad, nb);  // rare; an integer sum does not depend on its order
}

// dense <- +0.0 and, when COPY, l_out <- l_in, over [0, P)
template <bool COPY>
__global__ __launch_bounds__(256) void k_apply_clear(int64_t P, float* __restrict__ dense,
                                                     const float* __restrict__ l_in, float* __restrict__ l_out) {
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= P) return;
  if (p0 + 4 <= P) {
    *reinterpret_cast<f4*>(dense + p0) = f4{0.f, 0.f, 0.f, 0.f};
    if (COPY) *reinterpret_cast<f4*>(l_out + p0) = *reinterpret_cast<const f4*>(l_in + p0);
  } else {
    for (int64_t p = p0; p < P; ++p) {
      dense[p] = 0.f;
      if (COPY) l_out[p] = l_in[p];
    }
  }
}

// one pair per thread; the indices are unique, so no two threads write one column
__global__ __launch_bounds__(256) void k_apply_scatter(const uint32_t* __restrict__ idx, const float* __restrict__ val,
                                                       int64_t k, int64_t P, float* dense, const float* l_in,
                                                       float* l_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= k) return;
  const uint32_t p = idx[i];
  if ((int64_t)p >= P) return;
  const float v = val[i];
  dense[p] = v;
  l_out[p] = l_in[p] + v;
}

// log2 C when (R, C) is a shape of the contract, -1 otherwise
int shape_log2(int32_t R, int64_t C) {
  if (R != 1 && R != 3 && R != 5 && R != 7) return -1;
  for (int c = 10; c <= 24; ++c)
    if (C == ((int64_t)1 << c)) return c;
  return -1;
}

// the bucket tile of a workgroup on `cus` compute units
int plan_tile(int64_t cus, int32_t R, int64_t C) {
  int tile = FCS_TILE;
  while (tile > 256 && (int64_t)R * C / tile < cus) tile >>= 1;
  return tile;
}

bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && x < y + nb && y < x + na;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedsketch.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t fcs_abi_version(void) { return FCS_ABI_VERSION; }

extern "C" int64_t fcs_table_floats(int32_t R, int64_t C) {
  if (shape_log2(R, C) < 0)
    return refuse(FA_E_ARG, "fcs_table_floats: R=%d, C=%lld: R is 1, 3, 5 or 7 and C = 2^c with 10 <= c <= 24", R,
                  (long long)C);
  return (int64_t)R * C;
}

extern "C" int64_t fcs_sketch_plan(int32_t cus, int64_t P, int32_t R, int64_t C, int64_t* plan_out) {
  const int c = shape_log2(R, C);
  if (c < 0 || cus < 1 || P < 0 || P > 0x7fffffffLL || !plan_out)
    return refuse(FA_E_ARG, "fcs_sketch_plan: cus=%d, P=%lld, R=%d, C=%lld", cus, (long long)P, R, (long long)C);
  const int tile = plan_tile(cus, R, C);
  plan_out[0] = tile;
  plan_out[1] = FCS_U;
  plan_out[2] = (P + C - 1) >> c;
  plan_out[3] = (int64_t)R * (C / tile);
  return 1;
}

extern "C" int fcs_sketch_row(const float* x, const float* base, const float* r_in, int64_t P, int32_t R, int64_t C,
                              uint64_t seed, float* table, int32_t tile, int32_t flags, fa_stream_t stream) {
  const int c = shape_log2(R, C);
  if (c < 0)
    return refuse(FA_E_ARG, "fcs_sketch_row: R=%d, C=%lld: R is 1, 3, 5 or 7 and C = 2^c with 10 <= c <= 24", R,
                  (long long)C);
  if (P < 0 || P > 0x7fffffffLL) return refuse(FA_E_ARG, "fcs_sketch_row: P=%lld outside [0, 2^31 - 1]", (long long)P);
  if (!table || (P > 0 && !x)) return refuse(FA_E_ARG, "fcs_sketch_row: x or table is NULL");
  if (!aligned16(x) || !aligned16(base) || !aligned16(r_in) || !aligned16(table))
    return refuse(FA_E_ARG, "fcs_sketch_row: x, base, r_in and table must be 16-byte aligned");
  if (tile != 0 && tile != 256 && tile != 512 && tile != 1024)
    return refuse(FA_E_ARG, "fcs_sketch_row: tile=%d (0, 256, 512 or 1024)", tile);
  if (flags & ~FCS_SUBTRACT_FROM) return refuse(FA_E_ARG, "fcs_sketch_row: unknown flags 0x%x", flags);
  const uint64_t tb = (uint64_t)R * C * 4, xb = (uint64_t)P * 4;
  if (overlap(table, tb, x, xb) || overlap(table, tb, base, xb) || overlap(table, tb, r_in, xb))
    return refuse(FA_E_ARG, "fcs_sketch_row: table overlaps x, base or r_in");
  FA_DEVICE_SCOPE("fcs_sketch_row", stream, table);
  FA_OPERAND("x", x, xb);
  FA_OPERAND("base", base, xb);
  FA_OPERAND("r_in", r_in, xb);
  FA_OPERAND("table", table, tb);
  if (tile == 0) {
    const int cus = cu_count();
    tile = plan_tile(cus > 0 ? cus : 256, R, C);
  }
  const dim3 grid((unsigned)(C / tile), (unsigned)R), block((unsigned)(tile / 4));
  const int sub = flags & FCS_SUBTRACT_FROM;
  hipStream_t st = (hipStream_t)stream;
  if (base && r_in)
    hipLaunchKernelGGL((k_sketch<true, true>), grid, block, 0, st, x, base, r_in, P, c, seed, table, sub);
  else if (base)
    hipLaunchKernelGGL((k_sketch<true, false>), grid, block, 0, st, x, base, r_in, P, c, seed, table, sub);
  else if (r_in)
    hipLaunchKernelGGL((k_sketch<false, true>), grid, block, 0, st, x, base, r_in, P, c, seed, table, sub);
  else
    hipLaunchKernelGGL((k_sketch<false, false>), grid, block, 0, st, x, base, r_in, P, c, seed, table, sub);
  return check_launch("fcs_sketch_row");
}

extern "C" int fcs_estimate(const float* table, int64_t P, int32_t R, int64_t C, uint64_t seed, float* est,
                            fa_stream_t stream) {
  const int c = shape_log2(R, C);
  if (c < 0)
    return refuse(FA_E_ARG, "fcs_estimate: R=%d, C=%lld: R is 1, 3, 5 or 7 and C = 2^c with 10 <= c <= 24", R,
                  (long long)C);
  if (P < 0 || P > 0x7fffffffLL) return refuse(FA_E_ARG, "fcs_estimate: P=%lld outside [0, 2^31 - 1]", (long long)P);
  if (P == 0) return FA_OK;
  if (!table || !est) return refuse(FA_E_ARG, "fcs_estimate: table or est is NULL");
  if (!aligned16(table) || !aligned16(est)) return refuse(FA_E_ARG, "fcs_estimate: table and est must be 16-byte aligned");
  if (overlap(table, (uint64_t)R * C * 4, est, (uint64_t)P * 4))
    return refuse(FA_E_ARG, "fcs_estimate: est overlaps table");
  FA_DEVICE_SCOPE("fcs_estimate", stream, est);
  FA_OPERAND("table", table, (uint64_t)R * C * 4);
  FA_OPERAND("est", est, (uint64_t)P * 4);
  const dim3 grid((unsigned)((P + 4 * EST_THREADS - 1) / (4 * EST_THREADS))), block(EST_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (R == 1) hipLaunchKernelGGL((k_estimate<1>), grid, block, 0, st, table, P, c, seed, est);
  else if (R == 3) hipLaunchKernelGGL((k_estimate<3>), grid, block, 0, st, table, P, c, seed, est);
  else if (R == 5) hipLaunchKernelGGL((k_estimate<5>), grid, block, 0, st, table, P, c, seed, est);
  else hipLaunchKernelGGL((k_estimate<7>), grid, block, 0, st, table, P, c, seed, est);
  return check_launch("fcs_estimate");
}

extern "C" int fcs_state_step(const float* s, const float* su_in, const float* se_in, float rho, int64_t n,
                              float* su_out, float* se_out, uint32_t* nonfinite, fa_stream_t stream) {
  if (n < 0 || n % 4 || n > 7 * ((int64_t)1 << 24))
    return refuse(FA_E_ARG, "fcs_state_step: n=%lld (a multiple of 4, at most 7 * 2^24)", (long long)n);
  if (n == 0) return FA_OK;
  if (!s || !su_in || !se_in || !su_out || !se_out || !nonfinite)
    return refuse(FA_E_ARG, "fcs_state_step: an operand is NULL");
  if (!aligned16(s) || !aligned16(su_in) || !aligned16(se_in) || !aligned16(su_out) || !aligned16(se_out) ||
      ((uintptr_t)nonfinite & 3u))
    return refuse(FA_E_ARG, "fcs_state_step: the tables must be 16-byte aligned, the counter 4-byte");
  const uint64_t nb = (uint64_t)n * 4;
  if (overlap(su_out, nb, se_out, nb) || overlap(su_out, nb, s, nb) || overlap(se_out, nb, s, nb) ||
      overlap(su_out, nb, se_in, nb) || overlap(se_out, nb, su_in, nb) ||
      (su_out != su_in && overlap(su_out, nb, su_in, nb)) || (se_out != se_in && overlap(se_out, nb, se_in, nb)))
    return refuse(FA_E_ARG, "fcs_state_step: su_out may be su_in and se_out may be se_in; no other overlap");
  FA_DEVICE_SCOPE("fcs_state_step", stream, su_out);
  FA_OPERAND("s", s, nb);
  FA_OPERAND("su_in", su_in, nb);
  FA_OPERAND("se_in", se_in, nb);
  FA_OPERAND("su_out", su_out, nb);
  FA_OPERAND("se_out", se_out, nb);
  FA_OPERAND("nonfinite", nonfinite, 4);
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(k_state_step, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s, su_in,
                     se_in, rho, n4, su_out, se_out, nonfinite);
  return check_launch("fcs_state_step");
}

extern "C" int fcs_apply(const uint32_t* idx, const float* val, int64_t k, int64_t P, float* dense,
                         const float* l_in, float* l_out, fa_stream_t stream) {
  if (P < 0 || P > 0x7fffffffLL || k < 0 || k > P)
    return refuse(FA_E_ARG, "fcs_apply: k=%lld pairs of P=%lld columns", (long long)k, (long long)P);
  if (P == 0) return FA_OK;
  if (!dense || !l_in || !l_out || (k > 0 && (!idx || !val))) return refuse(FA_E_ARG, "fcs_apply: an operand is NULL");
  if (!aligned16(dense) || !aligned16(l_in) || !aligned16(l_out) || (((uintptr_t)idx | (uintptr_t)val) & 3u))
    return refuse(FA_E_ARG, "fcs_apply: dense, l_in and l_out must be 16-byte aligned, idx and val 4-byte");
  const uint64_t pb = (uint64_t)P * 4;
  if (overlap(dense, pb, l_in, pb) || overlap(dense, pb, l_out, pb) || (l_out != l_in && overlap(l_out, pb, l_in, pb)))
    return refuse(FA_E_ARG, "fcs_apply: dense overlaps a model buffer, or l_out overlaps l_in without being it");
  FA_DEVICE_SCOPE("fcs_apply", stream, l_out);
  FA_OPERAND("idx", idx, (uint64_t)k * 4);
  FA_OPERAND("val", val, (uint64_t)k * 4);
  FA_OPERAND("dense", dense, pb);
  FA_OPERAND("l_in", l_in, pb);
  FA_OPERAND("l_out", l_out, pb);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(((P + 3) / 4 + 255) / 256)), block(256);
  if (l_out != l_in)
    hipLaunchKernelGGL((k_apply_clear<true>), grid, block, 0, st, P, dense, l_in, l_out);
  else
    hipLaunchKernelGGL((k_apply_clear<false>), grid, block, 0, st, P, dense, l_in, l_out);
  if (k > 0)
    hipLaunchKernelGGL(k_apply_scatter, dim3((unsigned)((k + 255) / 256)), block, 0, st, idx, val, k, P, dense,
                       l_in, l_out);
  return check_launch("fcs_apply");
}
