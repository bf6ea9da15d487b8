// quant4_reduce.hip — MI355X (gfx950) kernels of the MXFP4 delta-upload path (include/fedquant4.h):
//   * fq4_reduce: the in-order fp32 column chain over client deltas staged as OCP e2m1 codes, two to a byte, with one
//     E8M0 scale byte per block of 32 columns — 17/32 byte per parameter per staged row and per reduction pass.  A
//     lane's 16-byte load is one whole block: its 16 code bytes are widened, two columns at a time, by the scaled
//     convert (v_cvt_scalef32_pk_f32_fp4, the block's 2^(s - 127) as its scale operand) and added to the lane's 32
//     accumulators (v_pk_add_f32) in arrival order: one vector operation per column, no LDS, no cross-lane traffic;
//   * fq4_reduce_plan: the launches it makes, as a host-only function of the CU count;
//   * fq4_quantize_row: the executor-side handler, one fp32 row (minus the round's base model, plus the executor's
//     error-feedback residual) into codes, scale bytes and the new residual.
//
// Numerics: every fp32 op is rounded to nearest and never contracted into an FMA; the default denormal modes are
// kept.  Scale bytes outside 2..252 poison their block (the contract's NaN) by a flag per lane and strip, not by the
// arithmetic: what the scaled convert gives for such a scale operand is never stored.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fedquant4.h"
#include "fa_device.h"
#include "fa_common.h"

// Tuning knobs (tools/quant4_reduce_measure.py per library, FEDAGG_LIB).  FQ4_L0_V / FQ4_L0_U: level
// 0's variant.  FQ4_WIDEN: 0 widens a code pair by the scaled convert with the block's scale, 1 by the convert at a
// scale of 1.0 and an fp32 multiply (the same bits for every scale byte of the contract; three operations per pair
// instead of two).  FQ4_ROUND: 0 rounds to e2m1 by v_cvt_scalef32_pk_fp4_f32 at a scale of 1.0, 1 by seven compares.
#if defined(FQ4_L0_V) || defined(FQ4_L0_U) || defined(FQ4_WIDEN) || defined(FQ4_ROUND)
#if !defined(FA_TUNING) || !FA_TUNING
#error "FQ4_L0_V / FQ4_L0_U / FQ4_WIDEN / FQ4_ROUND are tuning knobs: build with -DFA_TUNING=1"
#endif
#endif
#ifndef FQ4_L0_V
#define FQ4_L0_V 4
#endif
#ifndef FQ4_L0_U
#define FQ4_L0_U 4
#endif
#ifndef FQ4_WIDEN
#define FQ4_WIDEN 0
#endif
#ifndef FQ4_ROUND
#define FQ4_ROUND 0
#endif

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

// 2^(s - 127) as an fp32 for a scale byte of the contract (2..252): s << 23, a normal number.  For the five poison
// bytes this is 0, 2^-126, two large powers of two or an infinity; the caller never stores what comes of those.
__device__ __forceinline__ float scale_of(uint32_t s) { return __builtin_bit_cast(float, s << 23); }

// whether a scale byte poisons its block: (s - 2) > 250 as unsigned, true for 0, 1, 253, 254, 255
__device__ __forceinline__ uint32_t poisons(uint32_t s) { return (s - (uint32_t)FQ4_SCALE_MIN) > 250u ? 1u : 0u; }

// byte B of w (columns 2B, 2B + 1 of the dword's eight: low nibble first) widened and scaled
template <int B>
__device__ __forceinline__ f2 widen(uint32_t w, float sc) {
#if FQ4_WIDEN == 0
  return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, B);
#else
  const f2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, B);
  return f2{a.x * sc, a.y * sc};
#endif
}

// the 32 columns of one block (one 16-byte load) dequantised: columns 4h .. 4h+3 in o[h]
__device__ __forceinline__ void dequant(u4 v, float sc, f4 o[8]) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const f2 a = widen<0>(v[w], sc), b = widen<1>(v[w], sc), c = widen<2>(v[w], sc), d = widen<3>(v[w], sc);
    o[2 * w] = f4{a.x, a.y, b.x, b.y};
    o[2 * w + 1] = f4{c.x, c.y, d.x, d.y};
  }
}

// ------------------------------------------------------------------------------------------------
// fq4_reduce
// ------------------------------------------------------------------------------------------------
constexpr int FQ4_WAVES = 4;  // waves per workgroup, each owning V strips of a tile

struct Quant4Args {
  const u4* q;        // the rows, in 16-byte units (one block of 32 columns each)
  const uint8_t* sc;  // the scale bytes, one per block
  int64_t ld16;       // row stride in 16-byte units
  int64_t lds;        // scale row stride in bytes
  int64_t NB;         // blocks to read, ceil(P / 32)
  int64_t P;          // columns to write
  int64_t b0;         // first block of this launch
  int64_t ntiles;     // tiles of this launch; workgroup b takes tiles b, b + grid, ...
  int n;
  int flags;
  const float* acc_in;
  float* out;
};

// One tile: each of the workgroup's waves owns V strips (64 lanes x one 16-byte load: 2048 contiguous columns and 64
// contiguous scale bytes of a row each) and walks all n rows, U rows' loads issued ahead of their adds.  A lane holds
// 32V accumulators, 4UV load registers and UV scale bytes, and owns its blocks alone: block b of a row is lane
// b % 64's load and lane b % 64's scale byte.  Blocks past ceil(P / 32) are masked: their loads are replaced by zero
// codes under the scale byte 127 (+0 x 1 = +0), nothing of them is stored.  bad[j] collects, over all rows, whether a
// scale byte of the lane's block j poisoned it; the block's 32 sums are then replaced by NaN at the store — a NaN
// in a chain is sticky, so that equals the NaN entering at the row that held the byte.
template <int V, int U>
__device__ __forceinline__ void quant4_tile(const Quant4Args& r, int64_t tile, int lane, int wave) {
  const int64_t b0 = r.b0 + (tile * FQ4_WAVES + wave) * (64LL * V) + lane;
  const u4* qu = r.q + b0;
  const uint8_t* su = r.sc + b0;
  bool ok[V];
#pragma unroll
  for (int j = 0; j < V; ++j) ok[j] = (b0 + 64 * j) < r.NB;

  const f4 z4 = f4{0.f, 0.f, 0.f, 0.f};
  const u4 zu = u4{0u, 0u, 0u, 0u};
  f4 s[V][8];
  uint32_t bad[V];
#pragma unroll
  for (int j = 0; j < V; ++j) bad[j] = 0u;
  if (r.flags & FA_ACCUMULATE) {
    const f4* ain = reinterpret_cast<const f4*>(r.acc_in);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t c = 8 * (b0 + 64 * j);
#pragma unroll
      for (int h = 0; h < 8; ++h) s[j][h] = (ok[j] && 4 * (c + h) < r.P) ? ain[c + h] : z4;
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
      for (int h = 0; h < 8; ++h) s[j][h] = z4;
  }

  const u4* row = qu;
  const uint8_t* srow = su;
  int k = 0;
  for (; k + U <= r.n; k += U) {
    u4 t[U][V];
    uint32_t e[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) {
        t[u][j] = ok[j] ? __builtin_nontemporal_load(row + u * r.ld16 + 64 * j) : zu;
        e[u][j] = ok[j] ? (uint32_t)__builtin_nontemporal_load(srow + u * r.lds + 64 * j) : 127u;
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) {
        f4 d[8];
        bad[j] |= poisons(e[u][j]);
        dequant(t[u][j], scale_of(e[u][j]), d);
#pragma unroll
        for (int h = 0; h < 8; ++h) s[j][h] = s[j][h] + d[h];
      }
    row += U * r.ld16;
    srow += U * r.lds;
  }
  for (; k < r.n; ++k) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const u4 t = ok[j] ? __builtin_nontemporal_load(row + 64 * j) : zu;
      const uint32_t e = ok[j] ? (uint32_t)__builtin_nontemporal_load(srow + 64 * j) : 127u;
      f4 d[8];
      bad[j] |= poisons(e);
      dequant(t, scale_of(e), d);
#pragma unroll
      for (int h = 0; h < 8; ++h) s[j][h] = s[j][h] + d[h];
    }
    row += r.ld16;
    srow += r.lds;
  }

  const float qnan = __builtin_bit_cast(float, 0x7fc00000u);
  const f4 n4 = f4{qnan, qnan, qnan, qnan};
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (!ok[j]) continue;
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const f4 v = bad[j] ? n4 : s[j][h];
      const int64_t p = 32 * (b0 + 64 * j) + 4 * h;
      if (p + 4 <= r.P) {
        *reinterpret_cast<f4*>(r.out + p) = v;
      } else if (p < r.P) {  // the last, partial float4 column: columns >= P are not written
        r.out[p] = v.x;
        if (p + 1 < r.P) r.out[p + 1] = v.y;
        if (p + 2 < r.P) r.out[p + 2] = v.z;
      }
    }
  }
}

// LOOP = false: workgroup b reduces tile b.  LOOP = true: a capped grid, workgroup b reduces tiles b, b + grid, ...
template <int V, int U, bool LOOP>
__global__ __launch_bounds__(64 * FQ4_WAVES) void k_reduce_quant4(Quant4Args r) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (LOOP) {
    for (int64_t tile = blockIdx.x; tile < r.ntiles; tile += gridDim.x) quant4_tile<V, U>(r, tile, lane, wave);
  } else {
    quant4_tile<V, U>(r, blockIdx.x, lane, wave);
  }
}

// Launch plan: strip_plan (fa_common.h) over strips of 2048 columns.  Its three variants, sized by registers: one
// 16-byte load becomes 32 fp32 accumulators, so a lane holds 32V + 4UV + UV registers of data, and V x U KiB of loads
// are in flight per wave (the register counts the compiler reports: DESIGN.md §4; no variant uses scratch):
//   level 0  V = 4, U = 4   128 + 64 + 16 of data; the compiler reports 256 VGPRs + 4 AGPRs (8 on the capped grid),
//                           one wave per SIMD: an 8 KiB contiguous run per row and wave, 16 KiB of loads in flight
//                           (U = 8 parks 130 registers in AGPRs; its run: profiles/quant4_reduce_measure_u8.json)
//   level 1  V = 2, U = 4    64 + 32 +  8 of data; 143 VGPRs, three waves per SIMD
//   level 2  V = 1, U = 8    32 + 32 +  8 of data; 108 VGPRs, four waves per SIMD: short rows need the parallelism
// K does not enter the plan today; it is a parameter because fa_reduce's plan depends on it.
constexpr StripGeo FQ4_GEO{FQ4_WAVES, {FQ4_L0_V, 2, 1}, {FQ4_L0_U, 4, 8}, 75, 64 * FQ4_BLOCK};
static_assert(FQ4_PLAN_FIELDS == STRIP_PLAN_FIELDS, "fq4_reduce_plan's row is strip_plan_export's");

int64_t quant4_strips(int64_t P) { return ((P + FQ4_BLOCK - 1) / FQ4_BLOCK + 63) / 64; }

template <int V, int U>
void launch_one(Quant4Args r, const StripLaunch& l, hipStream_t st) {
  r.b0 = l.strip0 * 64;
  r.ntiles = l.tiles;
  const dim3 grid((unsigned)l.grid), blk(64 * FQ4_WAVES);
  if constexpr (V == FQ4_GEO.V[0]) {  // only level 0 runs on a capped grid
    if (l.grid < l.tiles) {
      hipLaunchKernelGGL((k_reduce_quant4<V, U, true>), grid, blk, 0, st, r);
      return;
    }
  }
  hipLaunchKernelGGL((k_reduce_quant4<V, U, false>), grid, blk, 0, st, r);
}

void launch_level(const Quant4Args& r, const StripLaunch& l, hipStream_t st) {
  if (l.level == 0)
    launch_one<FQ4_GEO.V[0], FQ4_GEO.U[0]>(r, l, st);
  else if (l.level == 1)
    launch_one<FQ4_GEO.V[1], FQ4_GEO.U[1]>(r, l, st);
  else
    launch_one<FQ4_GEO.V[2], FQ4_GEO.U[2]>(r, l, st);
}

// ------------------------------------------------------------------------------------------------
// fq4_quantize_row
// ------------------------------------------------------------------------------------------------
constexpr int QZ4_THREADS = 256;  // 8 columns per thread: four neighbouring lanes quantise one block of 32

// two values, already scaled into [-6, 6], rounded to e2m1 (ties to the code whose low bit is 0, the sign kept)
// into byte B of w
template <int B>
__device__ __forceinline__ uint32_t round_pair(uint32_t w, float a, float b) {
#if FQ4_ROUND == 0
  return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, a, b, 1.0f, B);
#else
  uint32_t c[2];
  const float v[2] = {a, b};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float m = __builtin_fabsf(v[i]);
    c[i] = (m > 0.25f) + (m >= 0.75f) + (m > 1.25f) + (m >= 1.75f) + (m > 2.5f) + (m >= 3.5f) + (m > 5.0f);
    c[i] |= (__builtin_bit_cast(uint32_t, v[i]) >> 31) << 3;
  }
  return (w & ~(0xffu << (8 * B))) | ((c[0] | (c[1] << 4)) << (8 * B));
#endif
}

__global__ __launch_bounds__(QZ4_THREADS) void k_quantize_row4(const float* __restrict__ x,
                                                               const float* __restrict__ base,
                                                               const float* residual, int64_t P,
                                                               uint32_t* __restrict__ q4,
                                                               uint8_t* __restrict__ scales, float* residual_out) {
  const int64_t t = (int64_t)blockIdx.x * QZ4_THREADS + threadIdx.x;
  const int64_t p = 8 * t;
  if (p >= (P + 31) / 32 * 32) return;  // whole groups of four lanes leave together
  const bool whole = p + 8 <= P;
  float d[8];
  if (whole) {
    const f4 a0 = *(const f4*)(x + p), a1 = *(const f4*)(x + p + 4);
    d[0] = a0.x; d[1] = a0.y; d[2] = a0.z; d[3] = a0.w;
    d[4] = a1.x; d[5] = a1.y; d[6] = a1.z; d[7] = a1.w;
    if (base) {
      const f4 b0 = *(const f4*)(base + p), b1 = *(const f4*)(base + p + 4);
      d[0] = d[0] - b0.x; d[1] = d[1] - b0.y; d[2] = d[2] - b0.z; d[3] = d[3] - b0.w;
      d[4] = d[4] - b1.x; d[5] = d[5] - b1.y; d[6] = d[6] - b1.z; d[7] = d[7] - b1.w;
    }
    if (residual) {
      const f4 r0 = *(const f4*)(residual + p), r1 = *(const f4*)(residual + p + 4);
      d[0] = d[0] + r0.x; d[1] = d[1] + r0.y; d[2] = d[2] + r0.z; d[3] = d[3] + r0.w;
      d[4] = d[4] + r1.x; d[5] = d[5] + r1.y; d[6] = d[6] + r1.z; d[7] = d[7] + r1.w;
    }
  } else {  // the row's last columns; columns >= P are padding: +0, code 0
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      d[c] = 0.f;
      if (p + c < P) {
        d[c] = base ? x[p + c] - base[p + c] : x[p + c];
        if (residual) d[c] = d[c] + residual[p + c];
      }
    }
  }
  // amax of the block on the bits: as unsigned integers |d| orders as its values do, and an inf or a NaN is on top
  uint32_t am = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const uint32_t b = __builtin_bit_cast(uint32_t, d[c]) & 0x7fffffffu;
    am = b > am ? b : am;
  }
  uint32_t o = (uint32_t)__shfl_xor((int)am, 1, 64);
  am = o > am ? o : am;
  o = (uint32_t)__shfl_xor((int)am, 2, 64);
  am = o > am ? o : am;
  const bool poison = am >= 0x7f800000u;
  int s = (int)(am >> 23) - 2 + ((am & 0x7fffffu) > 0x400000u ? 1 : 0);
  s = s < FQ4_SCALE_MIN ? FQ4_SCALE_MIN : (s > FQ4_SCALE_MAX ? FQ4_SCALE_MAX : s);
  // 2^(127 - s) and 2^(s - 127): normal fp32 numbers for every s in 2..252
  const float mul = __builtin_bit_cast(float, (uint32_t)(254 - s) << 23);
  const float sc = scale_of((uint32_t)s);
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = fminf(fmaxf(d[c] * mul, -6.f), 6.f);
  uint32_t w = 0;
  w = round_pair<0>(w, v[0], v[1]);
  w = round_pair<1>(w, v[2], v[3]);
  w = round_pair<2>(w, v[4], v[5]);
  w = round_pair<3>(w, v[6], v[7]);
  if (poison) w = 0;  // (a padding column is d = +0 and so code 0 already)
  q4[t] = w;
  if ((t & 3) == 0) scales[t >> 2] = poison ? (uint8_t)255 : (uint8_t)s;
  if (residual_out) {
    const f2 q0 = widen<0>(w, sc), q1 = widen<1>(w, sc), q2 = widen<2>(w, sc), q3 = widen<3>(w, sc);
    const float deq[8] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, q3.x, q3.y};
    float ro[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) ro[c] = poison ? 0.f : d[c] - deq[c];
    if (whole) {
      *(f4*)(residual_out + p) = f4{ro[0], ro[1], ro[2], ro[3]};
      *(f4*)(residual_out + p + 4) = f4{ro[4], ro[5], ro[6], ro[7]};
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (p + c < P) residual_out[p + c] = ro[c];
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedquant4.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t fq4_abi_version(void) { return FQ4_ABI_VERSION; }

extern "C" int64_t fq4_reduce_plan(int32_t cus, int32_t K, int64_t P, int64_t* plan_out, int32_t cap) {
  if (cus <= 0 || K < 0 || P < 0 || cap < 0 || (cap > 0 && !plan_out))
    return refuse(FA_E_ARG, "fq4_reduce_plan: bad arguments (cus=%d K=%d P=%lld cap=%d)", cus, K, (long long)P, cap);
  return strip_plan_export(cus, quant4_strips(P), FQ4_GEO, plan_out, cap);
}

extern "C" int fq4_reduce(const uint8_t* q4, const uint8_t* scales, int64_t ld, int64_t lds, int32_t n, int64_t P,
                          const float* acc_in, float* out, int32_t flags, fa_stream_t stream) {
  if (flags & ~FA_ACCUMULATE) return refuse(FA_E_ARG, "fq4_reduce: unknown flags %d (0 or FA_ACCUMULATE)", flags);
  if (n < 0 || P < 0 || ld < P)
    return refuse(FA_E_ARG, "fq4_reduce: ld=%lld < P=%lld, or negative n=%d / P", (long long)ld, (long long)P, n);
  if (ld % 64 != 0) return refuse(FA_E_ARG, "fq4_reduce: ld=%lld must be a multiple of 64 columns", (long long)ld);
  const int64_t NB = (P + FQ4_BLOCK - 1) / FQ4_BLOCK;
  if (lds < NB)
    return refuse(FA_E_ARG, "fq4_reduce: lds=%lld < ceil(P / 32)=%lld scale bytes per row", (long long)lds,
                  (long long)NB);
  if ((flags & FA_ACCUMULATE) && !acc_in) return refuse(FA_E_ARG, "fq4_reduce: FA_ACCUMULATE without acc_in");
  if (n == 0 && !(flags & FA_ACCUMULATE)) return refuse(FA_E_ARG, "fq4_reduce: n=0 rows with nothing to accumulate");
  if (n > 0 && (!q4 || !scales)) return refuse(FA_E_ARG, "fq4_reduce: q4 or scales is NULL");
  if (!out) return refuse(FA_E_ARG, "fq4_reduce: out is NULL");
  if (!aligned16(q4) || !aligned16(scales))
    return refuse(FA_E_ARG, "fq4_reduce: q4 and scales must be 16-byte aligned");
  if (!aligned16(out) || !aligned16(acc_in))
    return refuse(FA_E_ARG, "fq4_reduce: out and acc_in must be 16-byte aligned");
  if (P == 0) return FA_OK;
  const int64_t P4 = (P + 3) / 4;
  if (NB / (64 * FQ4_WAVES) > 0x7fffffffLL) return refuse(FA_E_RANGE, "fq4_reduce: P too large");
  FA_DEVICE_SCOPE("fq4_reduce", stream, out);
  FA_OPERAND("q4", q4, n > 0 ? (uint64_t)((int64_t)(n - 1) * (ld / 2) + NB * 16) : 0);
  FA_OPERAND("scales", scales, n > 0 ? (uint64_t)((int64_t)(n - 1) * lds + NB) : 0);
  FA_OPERAND("acc_in", (flags & FA_ACCUMULATE) ? acc_in : nullptr, (uint64_t)P4 * 16);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fq4_reduce launch plan: no CU count for device %d", fa_scope_device());
  Quant4Args r{};
  r.q = reinterpret_cast<const u4*>(q4); r.sc = scales; r.ld16 = ld / 32; r.lds = lds; r.NB = NB; r.P = P;
  r.n = n; r.flags = flags; r.acc_in = acc_in; r.out = out;
  StripLaunch l[3];
  const int nl = strip_plan(cus, quant4_strips(P), FQ4_GEO, l);
  for (int i = 0; i < nl; ++i) {
    launch_level(r, l[i], (hipStream_t)stream);
    const int e = check_launch("fq4_reduce");
    if (e) return e;
  }
  return FA_OK;
}

extern "C" int fq4_quantize_row(const float* x, const float* base, const float* residual, int64_t P, uint8_t* q4,
                                uint8_t* scales, float* residual_out, fa_stream_t stream) {
  if (P < 0) return refuse(FA_E_ARG, "fq4_quantize_row: negative P=%lld", (long long)P);
  if (P == 0) return FA_OK;
  if (!x || !q4 || !scales) return refuse(FA_E_ARG, "fq4_quantize_row: x, q4 or scales is NULL");
  if (!aligned16(x) || !aligned16(base) || !aligned16(residual) || !aligned16(residual_out) || !aligned16(q4))
    return refuse(FA_E_ARG, "fq4_quantize_row: x, base, residual, residual_out and q4 must be 16-byte aligned");
  const int64_t NB = (P + FQ4_BLOCK - 1) / FQ4_BLOCK;
  const int64_t grid = (NB * 4 + QZ4_THREADS - 1) / QZ4_THREADS;
  if (grid > 0x7fffffffLL) return refuse(FA_E_RANGE, "fq4_quantize_row: P too large");
  FA_DEVICE_SCOPE("fq4_quantize_row", stream, q4);
  FA_OPERAND("x", x, (uint64_t)P * 4);
  FA_OPERAND("base", base, (uint64_t)P * 4);
  FA_OPERAND("residual", residual, (uint64_t)P * 4);
  FA_OPERAND("q4", q4, (uint64_t)NB * (FQ4_BLOCK / 2));
  FA_OPERAND("scales", scales, (uint64_t)NB);
  FA_OPERAND("residual_out", residual_out, (uint64_t)P * 4);
  hipLaunchKernelGGL(k_quantize_row4, dim3((unsigned)grid), dim3(QZ4_THREADS), 0, (hipStream_t)stream, x, base,
                     residual, P, reinterpret_cast<uint32_t*>(q4), scales, residual_out);
  return check_launch("fq4_quantize_row");
}
