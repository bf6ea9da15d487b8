// quant_reduce.hip — MI355X (gfx950) kernels of the MXFP8 delta-upload path (include/fedquant.h):
//   * fq_reduce: the in-order fp32 column chain over client deltas staged as OCP e4m3fn codes with one E8M0 scale
//     byte per block of 32 columns — 1 + 1/32 bytes per parameter per staged row and per reduction pass.  Each code
//     is widened exactly to fp32 (v_cvt_pk_f32_fp8), multiplied by its block's power of two (an fp32 multiply, which
//     the compiler pairs into v_pk_mul_f32; exact for every scale byte the quantiser emits) and added to the chain
//     (v_pk_add_f32), in arrival order;
//   * fq_reduce_plan: the launches it makes, as a host-only function of the CU count;
//   * fq_quantize_row: the executor-side handler, one fp32 row (minus the round's base model) into codes and scales.
//
// Numerics: every fp32 op is rounded to nearest and never contracted into an FMA; the default denormal modes are
// kept, so the subnormal fp32 products of small scale bytes survive.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fedquant.h"
#include "fa_device.h"
#include "fa_common.h"

// Tuning knobs (tools/quant_reduce_measure.py per library, FEDAGG_LIB).  FQ_L0_V / FQ_L0_U: level 0's
// variant.  FQ_PROBE: timing probes whose results are NOT the contract's — 1 takes the scale byte from a kernel
// argument instead of loading it, 2 adds the widened codes without the multiply by the scale.
#if defined(FQ_L0_V) || defined(FQ_L0_U) || defined(FQ_PROBE)
#if !defined(FA_TUNING) || !FA_TUNING
#error "FQ_L0_V / FQ_L0_U / FQ_PROBE are tuning knobs: build with -DFA_TUNING=1"
#endif
#endif
#ifndef FQ_L0_V
#define FQ_L0_V 8
#endif
#ifndef FQ_L0_U
#define FQ_L0_U 4
#endif
#ifndef FQ_PROBE
#define FQ_PROBE 0
#endif

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------
// fq_reduce
// ------------------------------------------------------------------------------------------------
constexpr int FQ_WAVES = 4;  // waves per workgroup, each owning V strips of a tile

// 2^(s - 127) as an fp32: s << 23 for 1..254, the subnormal 2^-127 for 0, and a NaN for 255 (an E8M0 NaN: the whole
// block is NaN — an infinity would leave the block's zero codes as NaN but its others as inf)
__device__ __forceinline__ float scale_of(uint32_t s) {
  uint32_t b = s << 23;
  b = s == 0u ? 0x00400000u : b;
  b = s == 255u ? 0x7fc00000u : b;
  return __builtin_bit_cast(float, b);
}

// 16 columns of a row (one 16-byte load) dequantised: columns 4h .. 4h+3 in o[h]
__device__ __forceinline__ void dequant(u4 v, float sc, f4 o[4]) {
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const f2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[h], false);  // bytes 0, 1
    const f2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[h], true);   // bytes 2, 3
#if FQ_PROBE == 2
    (void)sc;
    o[h] = f4{a.x, a.y, b.x, b.y};
#else
    o[h] = f4{a.x * sc, a.y * sc, b.x * sc, b.y * sc};
#endif
  }
}

struct QuantArgs {
  const u4* q;        // the rows, in 16-byte units (16 columns)
  const uint8_t* sc;  // the scale bytes, one per 32 columns
  int64_t ld16;       // row stride in 16-byte units
  int64_t lds;        // scale row stride in bytes
  int64_t P16;        // 16-byte columns to read, ceil(P / 16)
  int64_t P;          // columns to write
  int64_t c0;         // first 16-byte column of this launch
  int64_t ntiles;     // tiles of this launch; workgroup b takes tiles b, b + grid, ...
  int n;
  int flags;
  const float* acc_in;
  float* out;
};

// One tile, as fh_reduce's: each of the workgroup's waves owns V strips (64 lanes x one 16-byte load: 1024 contiguous
// columns of a row each) and walks all n rows, U rows' loads issued ahead of their adds.  A lane holds 16V
// accumulators, 4UV load registers and UV scale bytes (two neighbouring lanes share a block's byte).  Strips past
// ceil(P / 16) are masked: their loads are replaced by zero codes and a zero scale byte (0 x 2^-127 = 0), nothing of
// them is stored.
template <int V, int U>
__device__ __forceinline__ void quant_tile(const QuantArgs& r, int64_t tile, int lane, int wave) {
  const int64_t c0 = r.c0 + (tile * FQ_WAVES + wave) * (64LL * V) + lane;
  const u4* qu = r.q + c0;
  const uint8_t* su = r.sc + (c0 >> 1);  // (c0 + 64 j) / 2 = c0 / 2 + 32 j, c0 and c0 + 64 j having one parity
  bool ok[V];
#pragma unroll
  for (int j = 0; j < V; ++j) ok[j] = (c0 + 64 * j) < r.P16;

  const f4 z4 = f4{0.f, 0.f, 0.f, 0.f};
  const u4 zu = u4{0u, 0u, 0u, 0u};
  f4 s[V][4];
  if (r.flags & FA_ACCUMULATE) {
    const f4* ain = reinterpret_cast<const f4*>(r.acc_in);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t c = 4 * (c0 + 64 * j);
#pragma unroll
      for (int h = 0; h < 4; ++h) s[j][h] = (ok[j] && 4 * (c + h) < r.P) ? ain[c + h] : z4;
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
      for (int h = 0; h < 4; ++h) s[j][h] = z4;
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
#if FQ_PROBE == 1
        e[u][j] = (uint32_t)r.n & 0xffu;
#else
        e[u][j] = ok[j] ? (uint32_t)__builtin_nontemporal_load(srow + u * r.lds + 32 * j) : 0u;
#endif
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) {
        f4 d[4];
        dequant(t[u][j], scale_of(e[u][j]), d);
#pragma unroll
        for (int h = 0; h < 4; ++h) s[j][h] = s[j][h] + d[h];
      }
    row += U * r.ld16;
    srow += U * r.lds;
  }
  for (; k < r.n; ++k) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const u4 t = ok[j] ? __builtin_nontemporal_load(row + 64 * j) : zu;
      const uint32_t e = ok[j] ? (uint32_t)__builtin_nontemporal_load(srow + 32 * j) : 0u;
      f4 d[4];
      dequant(t, scale_of(e), d);
#pragma unroll
      for (int h = 0; h < 4; ++h) s[j][h] = s[j][h] + d[h];
    }
    row += r.ld16;
    srow += r.lds;
  }

#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (!ok[j]) continue;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int64_t p = 16 * (c0 + 64 * j) + 4 * h;
      if (p + 4 <= r.P) {
        *reinterpret_cast<f4*>(r.out + p) = s[j][h];
      } else if (p < r.P) {  // the last, partial float4 column: columns >= P are not written
        r.out[p] = s[j][h].x;
        if (p + 1 < r.P) r.out[p + 1] = s[j][h].y;
        if (p + 2 < r.P) r.out[p + 2] = s[j][h].z;
      }
    }
  }
}

// LOOP = false: workgroup b reduces tile b.  LOOP = true: a capped grid, workgroup b reduces tiles b, b + grid, ...
template <int V, int U, bool LOOP>
__global__ __launch_bounds__(64 * FQ_WAVES) void k_reduce_quant(QuantArgs r) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (LOOP) {
    for (int64_t tile = blockIdx.x; tile < r.ntiles; tile += gridDim.x) quant_tile<V, U>(r, tile, lane, wave);
  } else {
    quant_tile<V, U>(r, blockIdx.x, lane, wave);
  }
}

// Launch plan: strip_plan (fa_common.h) over strips of 1024 columns.  Its three variants, sized by registers: one
// 16-byte load becomes 16 fp32 accumulators, so a lane holds 16V + 4UV + UV registers of data, and V x U KiB of loads
// are in flight per wave (measured register counts: DESIGN.md §4; no variant uses scratch):
//   level 0  V = 8, U = 4   128 + 128 + 32 registers, one wave per SIMD (the loads in flight park in AGPRs): the
//                           widest contiguous run per row (8 KiB) and 32 KiB of loads in flight per wave
//   level 1  V = 4, U = 4    64 +  64 + 16 registers, two waves per SIMD
//   level 2  V = 1, U = 8    16 +  32 +  8 registers, six waves per SIMD: short rows need the parallelism
// K does not enter the plan today; it is a parameter because fa_reduce's plan depends on it.
constexpr StripGeo FQ_GEO{FQ_WAVES, {FQ_L0_V, 4, 1}, {FQ_L0_U, 4, 8}, 75, 1024};
static_assert(FQ_PLAN_FIELDS == STRIP_PLAN_FIELDS, "fq_reduce_plan's row is strip_plan_export's");

int64_t quant_strips(int64_t P) { return ((P + 15) / 16 + 63) / 64; }

template <int V, int U>
void launch_one(QuantArgs r, const StripLaunch& l, hipStream_t st) {
  r.c0 = l.strip0 * 64;
  r.ntiles = l.tiles;
  const dim3 grid((unsigned)l.grid), blk(64 * FQ_WAVES);
  if constexpr (V == FQ_GEO.V[0]) {  // only level 0 runs on a capped grid
    if (l.grid < l.tiles) {
      hipLaunchKernelGGL((k_reduce_quant<V, U, true>), grid, blk, 0, st, r);
      return;
    }
  }
  hipLaunchKernelGGL((k_reduce_quant<V, U, false>), grid, blk, 0, st, r);
}

void launch_level(const QuantArgs& r, const StripLaunch& l, hipStream_t st) {
  if (l.level == 0)
    launch_one<FQ_GEO.V[0], FQ_GEO.U[0]>(r, l, st);
  else if (l.level == 1)
    launch_one<FQ_GEO.V[1], FQ_GEO.U[1]>(r, l, st);
  else
    launch_one<FQ_GEO.V[2], FQ_GEO.U[2]>(r, l, st);
}

// ------------------------------------------------------------------------------------------------
// fq_quantize_row
// ------------------------------------------------------------------------------------------------
constexpr int QZ_THREADS = 256;  // 8 columns per thread: four neighbouring lanes quantise one block of 32

__global__ __launch_bounds__(QZ_THREADS) void k_quantize_row(const float* __restrict__ x,
                                                             const float* __restrict__ base, int64_t P,
                                                             uint8_t* __restrict__ q8, uint8_t* __restrict__ scales) {
  const int64_t t = (int64_t)blockIdx.x * QZ_THREADS + threadIdx.x;
  const int64_t p = 8 * t;
  if (p >= (P + 31) / 32 * 32) return;  // whole groups of four lanes leave together
  float d[8];
  if (p + 8 <= P) {
    const f4 a0 = *(const f4*)(x + p), a1 = *(const f4*)(x + p + 4);
    d[0] = a0.x; d[1] = a0.y; d[2] = a0.z; d[3] = a0.w;
    d[4] = a1.x; d[5] = a1.y; d[6] = a1.z; d[7] = a1.w;
    if (base) {
      const f4 b0 = *(const f4*)(base + p), b1 = *(const f4*)(base + p + 4);
      d[0] = d[0] - b0.x; d[1] = d[1] - b0.y; d[2] = d[2] - b0.z; d[3] = d[3] - b0.w;
      d[4] = d[4] - b1.x; d[5] = d[5] - b1.y; d[6] = d[6] - b1.z; d[7] = d[7] - b1.w;
    }
  } else {  // the row's last columns; columns >= P are padding: +0, code 0
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      d[c] = 0.f;
      if (p + c < P) d[c] = base ? x[p + c] - base[p + c] : x[p + c];
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
  int s;
  if (am >= 0x7f800000u) {
    s = 255;
  } else {
    s = (int)(am >> 23) - 8 + ((am & 0x7fffffu) > 0x600000u ? 1 : 0);
    s = s < 10 ? 10 : (s > 246 ? 246 : s);
  }
  // 2^(127 - s): a normal fp32 for every s in 10..246 (s = 255: the codes are unspecified; 0 is written, as the
  // host path does)
  const float mul = __builtin_bit_cast(float, (uint32_t)(254 - (s == 255 ? 246 : s)) << 23);
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = fminf(fmaxf(d[c] * mul, -448.f), 448.f);
  int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], w0, true);
  int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], 0, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], w1, true);
  if (s == 255) w0 = w1 = 0;
  *reinterpret_cast<u2*>(q8 + p) = u2{(uint32_t)w0, (uint32_t)w1};
  if ((t & 3) == 0) scales[t >> 2] = (uint8_t)s;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedquant.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t fq_abi_version(void) { return FQ_ABI_VERSION; }

extern "C" int64_t fq_reduce_plan(int32_t cus, int32_t K, int64_t P, int64_t* plan_out, int32_t cap) {
  if (cus <= 0 || K < 0 || P < 0 || cap < 0 || (cap > 0 && !plan_out))
    return refuse(FA_E_ARG, "fq_reduce_plan: bad arguments (cus=%d K=%d P=%lld cap=%d)", cus, K, (long long)P, cap);
  return strip_plan_export(cus, quant_strips(P), FQ_GEO, plan_out, cap);
}

extern "C" int fq_reduce(const uint8_t* q8, const uint8_t* scales, int64_t ld, int64_t lds, int32_t n, int64_t P,
                         const float* acc_in, float* out, int32_t flags, fa_stream_t stream) {
  if (flags & ~FA_ACCUMULATE) return refuse(FA_E_ARG, "fq_reduce: unknown flags %d (0 or FA_ACCUMULATE)", flags);
  if (n < 0 || P < 0 || ld < P)
    return refuse(FA_E_ARG, "fq_reduce: ld=%lld < P=%lld, or negative n=%d / P", (long long)ld, (long long)P, n);
  if (ld % 64 != 0) return refuse(FA_E_ARG, "fq_reduce: ld=%lld must be a multiple of 64 codes", (long long)ld);
  const int64_t NB = (P + FQ_BLOCK - 1) / FQ_BLOCK;
  if (lds < NB)
    return refuse(FA_E_ARG, "fq_reduce: lds=%lld < ceil(P / 32)=%lld scale bytes per row", (long long)lds, (long long)NB);
  if ((flags & FA_ACCUMULATE) && !acc_in) return refuse(FA_E_ARG, "fq_reduce: FA_ACCUMULATE without acc_in");
  if (n == 0 && !(flags & FA_ACCUMULATE)) return refuse(FA_E_ARG, "fq_reduce: n=0 rows with nothing to accumulate");
  if (n > 0 && (!q8 || !scales)) return refuse(FA_E_ARG, "fq_reduce: q8 or scales is NULL");
  if (!out) return refuse(FA_E_ARG, "fq_reduce: out is NULL");
  if (!aligned16(q8) || !aligned16(scales)) return refuse(FA_E_ARG, "fq_reduce: q8 and scales must be 16-byte aligned");
  if (!aligned16(out) || !aligned16(acc_in)) return refuse(FA_E_ARG, "fq_reduce: out and acc_in must be 16-byte aligned");
  if (P == 0) return FA_OK;
  const int64_t P16 = (P + 15) / 16, P4 = (P + 3) / 4;
  if (P16 / (64 * FQ_WAVES) > 0x7fffffffLL) return refuse(FA_E_RANGE, "fq_reduce: P too large");
  FA_DEVICE_SCOPE("fq_reduce", stream, out);
  FA_OPERAND("q8", q8, n > 0 ? (uint64_t)((int64_t)(n - 1) * ld + P16 * 16) : 0);
  FA_OPERAND("scales", scales, n > 0 ? (uint64_t)((int64_t)(n - 1) * lds + NB) : 0);
  FA_OPERAND("acc_in", (flags & FA_ACCUMULATE) ? acc_in : nullptr, (uint64_t)P4 * 16);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fq_reduce launch plan: no CU count for device %d", fa_scope_device());
  QuantArgs r{};
  r.q = reinterpret_cast<const u4*>(q8); r.sc = scales; r.ld16 = ld / 16; r.lds = lds; r.P16 = P16; r.P = P;
  r.n = n; r.flags = flags; r.acc_in = acc_in; r.out = out;
  StripLaunch l[3];
  const int nl = strip_plan(cus, quant_strips(P), FQ_GEO, l);
  for (int i = 0; i < nl; ++i) {
    launch_level(r, l[i], (hipStream_t)stream);
    const int e = check_launch("fq_reduce");
    if (e) return e;
  }
  return FA_OK;
}

extern "C" int fq_quantize_row(const float* x, const float* base, int64_t P, uint8_t* q8, uint8_t* scales,
                               fa_stream_t stream) {
  if (P < 0) return refuse(FA_E_ARG, "fq_quantize_row: negative P=%lld", (long long)P);
  if (P == 0) return FA_OK;
  if (!x || !q8 || !scales) return refuse(FA_E_ARG, "fq_quantize_row: x, q8 or scales is NULL");
  if (!aligned16(x) || !aligned16(base) || !aligned16(q8))
    return refuse(FA_E_ARG, "fq_quantize_row: x, base and q8 must be 16-byte aligned");
  const int64_t NB = (P + FQ_BLOCK - 1) / FQ_BLOCK;
  const int64_t grid = (NB * 4 + QZ_THREADS - 1) / QZ_THREADS;
  if (grid > 0x7fffffffLL) return refuse(FA_E_RANGE, "fq_quantize_row: P too large");
  FA_DEVICE_SCOPE("fq_quantize_row", stream, q8);
  FA_OPERAND("x", x, (uint64_t)P * 4);
  FA_OPERAND("base", base, (uint64_t)P * 4);
  FA_OPERAND("q8", q8, (uint64_t)NB * FQ_BLOCK);
  FA_OPERAND("scales", scales, (uint64_t)NB);
  hipLaunchKernelGGL(k_quantize_row, dim3((unsigned)grid), dim3(QZ_THREADS), 0, (hipStream_t)stream, x, base, P, q8,
                     scales);
  return check_launch("fq_quantize_row");
}
