// reduce_half.hip — MI355X (gfx950) kernels of the 16-bit client-upload path (include/fedhalf.h):
//   * fh_reduce: fa_reduce's in-order fp32 column chain over client rows staged as float16 or bfloat16 — half the
//     HBM bytes per staged row and per reduction pass.  Each element is widened exactly to fp32 (v_cvt_f32_f16, or
//     a 16-bit shift for bfloat16) and then takes the same adds, in the same order, as k_reduce (fedagg.hip);
//   * fh_reduce_plan: the launches it makes, as a host-only function of the CU count;
//   * fh_pack_row: the client-side handler, a model's fp32 tensors rounded into one 16-bit row.
//
// Numerics: every fp32 op is rounded to nearest and never contracted into an FMA; the default denormal modes are
// kept, so float16 and fp32 subnormals survive; the division of FA_FINALIZE is the true fp32 division.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fedhalf.h"
#include "fa_device.h"
#include "fa_common.h"

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------------------------
// fh_reduce
// ------------------------------------------------------------------------------------------------
constexpr int FH_WAVES = 4;  // waves per workgroup, each owning V strips of a tile

// 8 columns of a row (one 16-byte load) widened to fp32: columns 0..3 in lo, 4..7 in hi
template <bool BF>
__device__ __forceinline__ void widen(u4 v, f4& lo, f4& hi) {
  float o[8];
  if (BF) {  // a bfloat16 is the upper half of an fp32
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t w = v[i];
      o[2 * i] = __builtin_bit_cast(float, w << 16);
      o[2 * i + 1] = __builtin_bit_cast(float, w & 0xffff0000u);
    }
  } else {  // v_cvt_f32_f16: exact, subnormals included (the whole vector is cast: a bit_cast of ONE element of an
            // ext_vector reads element 0 whatever the index with this compiler)
    const h8 h = __builtin_bit_cast(h8, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (float)h[i];
  }
  lo = f4{o[0], o[1], o[2], o[3]};
  hi = f4{o[4], o[5], o[6], o[7]};
}

struct HalfArgs {
  const u4* x;     // the rows, in 16-byte units (8 columns)
  int64_t ld8;     // row stride in 16-byte units
  int64_t P8;      // 16-byte columns to read, ceil(P / 8)
  int64_t P4;      // float4 columns to write, ceil(P / 4)
  int64_t c0;      // first 16-byte column of this launch
  int64_t ntiles;  // tiles of this launch; workgroup b takes tiles b, b + grid, ...
  int K;
  int flags;
  const float* a;
  const float* acc_in;
  float* out;
  float* mirror;  // FA_FINALIZE: optional second copy of the mean (may be pinned host memory)
  float denom;
};

// One tile, as k_reduce's (fedagg.hip): each of the workgroup's waves owns V strips (64 lanes x one 16-byte load:
// 512 contiguous columns of a row each) and walks all K rows, U rows' loads issued ahead of their adds.  A lane
// holds 8V accumulators and 4UV load registers.  Strips past ceil(P / 8) are masked; the tile is V strips wide at
// compile time.
template <int V, int U, bool BF, bool W>
__device__ __forceinline__ void half_tile(const HalfArgs& r, int64_t tile, int lane, int wave) {
  const int64_t c0 = r.c0 + (tile * FH_WAVES + wave) * (64LL * V) + lane;
  const u4* xu = r.x + c0;
  bool ok[V];
#pragma unroll
  for (int j = 0; j < V; ++j) ok[j] = (c0 + 64 * j) < r.P8;

  const f4 z4 = f4{0.f, 0.f, 0.f, 0.f};
  const u4 zu = u4{0u, 0u, 0u, 0u};
  f4 s[V][2];
  int k = 0;
  if (r.flags & FA_ACCUMULATE) {
    const f4* ain = reinterpret_cast<const f4*>(r.acc_in);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t c = 2 * (c0 + 64 * j);
      s[j][0] = ok[j] ? ain[c] : z4;  // c < P4 whenever the strip is inside P8
      s[j][1] = (ok[j] && c + 1 < r.P4) ? ain[c + 1] : z4;
    }
  } else {
    const float w0 = W ? r.a[0] : 1.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      f4 lo, hi;
      widen<BF>(ok[j] ? __builtin_nontemporal_load(xu + 64 * j) : zu, lo, hi);
      s[j][0] = W ? lo * w0 : lo;
      s[j][1] = W ? hi * w0 : hi;
    }
    k = 1;
  }

  const u4* row = xu + (int64_t)k * r.ld8;
  for (; k + U <= r.K; k += U) {
    u4 t[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) t[u][j] = ok[j] ? __builtin_nontemporal_load(row + u * r.ld8 + 64 * j) : zu;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float w = W ? r.a[k + u] : 1.f;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        f4 lo, hi;
        widen<BF>(t[u][j], lo, hi);
        s[j][0] = W ? s[j][0] + w * lo : s[j][0] + lo;
        s[j][1] = W ? s[j][1] + w * hi : s[j][1] + hi;
      }
    }
    row += U * r.ld8;
  }
  for (; k < r.K; ++k) {
    const float w = W ? r.a[k] : 1.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      f4 lo, hi;
      widen<BF>(ok[j] ? __builtin_nontemporal_load(row + 64 * j) : zu, lo, hi);
      s[j][0] = W ? s[j][0] + w * lo : s[j][0] + lo;
      s[j][1] = W ? s[j][1] + w * hi : s[j][1] + hi;
    }
    row += r.ld8;
  }

  const bool fin = (r.flags & FA_FINALIZE) != 0;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (!ok[j]) continue;
    const int64_t c = 2 * (c0 + 64 * j);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (c + h >= r.P4) continue;  // stores are float4 columns, masked at ceil(P / 4)
      f4 o = s[j][h];
      if (fin) {
        o.x = __fdiv_rn(o.x, r.denom);
        o.y = __fdiv_rn(o.y, r.denom);
        o.z = __fdiv_rn(o.z, r.denom);
        o.w = __fdiv_rn(o.w, r.denom);
      }
      reinterpret_cast<f4*>(r.out)[c + h] = o;
      if (fin && r.mirror) reinterpret_cast<f4*>(r.mirror)[c + h] = o;
    }
  }
}

// LOOP = false: workgroup b reduces tile b.  LOOP = true: a capped grid, workgroup b reduces tiles b, b + grid, ...
template <int V, int U, bool BF, bool W, bool LOOP>
__global__ __launch_bounds__(64 * FH_WAVES) void k_reduce_half(HalfArgs r) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (LOOP) {
    for (int64_t tile = blockIdx.x; tile < r.ntiles; tile += gridDim.x) half_tile<V, U, BF, W>(r, tile, lane, wave);
  } else {
    half_tile<V, U, BF, W>(r, blockIdx.x, lane, wave);
  }
}

// Launch plan: strip_plan (fa_common.h) over strips of 512 columns.  Its three variants, sized by registers: one
// 16-byte load becomes 8 fp32 accumulators, so a lane holds 8V + 4UV registers of data, and V x U KiB of loads are
// in flight per wave (k_reduce's 32 KiB at the wide end):
//   level 0  V = 16, U = 2   128 + 128 registers, one wave per SIMD: the widest contiguous run per row (16 KiB)
//   level 1  V =  8, U = 4    64 + 128 registers, two waves per SIMD
//   level 2  V =  2, U = 8    16 +  64 registers, five waves per SIMD: short rows need the parallelism
// K and `weighted` do not enter the plan today; they are parameters because fa_reduce's plan depends on them.
#ifndef FH_L2_V  // tuning knobs (tools/half_reduce_measure.py per library, FEDAGG_LIB): level 2's variant
#define FH_L2_V 2
#define FH_L2_U 8
#elif !defined(FA_TUNING) || !FA_TUNING
#error "FH_L2_V / FH_L2_U are tuning knobs: build with -DFA_TUNING=1"
#endif
constexpr StripGeo FH_GEO{FH_WAVES, {16, 8, FH_L2_V}, {2, 4, FH_L2_U}, 75, 512};
static_assert(FH_PLAN_FIELDS == STRIP_PLAN_FIELDS, "fh_reduce_plan's row is strip_plan_export's");

int64_t half_strips(int64_t P) { return ((P + 7) / 8 + 63) / 64; }

template <int V, int U, bool BF, bool W>
void launch_one(HalfArgs r, const StripLaunch& l, hipStream_t st) {
  r.c0 = l.strip0 * 64;
  r.ntiles = l.tiles;
  const dim3 grid((unsigned)l.grid), blk(64 * FH_WAVES);
  if constexpr (V == FH_GEO.V[0]) {  // only level 0 runs on a capped grid
    if (l.grid < l.tiles) {
      hipLaunchKernelGGL((k_reduce_half<V, U, BF, W, true>), grid, blk, 0, st, r);
      return;
    }
  }
  hipLaunchKernelGGL((k_reduce_half<V, U, BF, W, false>), grid, blk, 0, st, r);
}

template <bool BF, bool W>
void launch_level(const HalfArgs& r, const StripLaunch& l, hipStream_t st) {
  if (l.level == 0)
    launch_one<FH_GEO.V[0], FH_GEO.U[0], BF, W>(r, l, st);
  else if (l.level == 1)
    launch_one<FH_GEO.V[1], FH_GEO.U[1], BF, W>(r, l, st);
  else
    launch_one<FH_GEO.V[2], FH_GEO.U[2], BF, W>(r, l, st);
}

// ------------------------------------------------------------------------------------------------
// fh_pack_row
// ------------------------------------------------------------------------------------------------
constexpr int PK_MAX = 64;  // tensors per launch (the table travels in the kernel arguments, 1.8 KiB)
constexpr int PK_THREADS = 256;
constexpr int64_t PK_CHUNK = PK_THREADS * 8;  // elements of one tensor per workgroup

struct PackList {
  const float* src[PK_MAX];
  int64_t n[PK_MAX], dst[PK_MAX];
  int32_t blk0[PK_MAX + 1];  // first workgroup of each tensor; blk0[T] = grid size
  int32_t T;
};

// fp32 -> 16 bits, round to nearest even.  float16: the hardware conversion (subnormals kept, overflow to inf,
// NaN stays NaN).  bfloat16: torch's round_to_nearest_even (c10/util/BFloat16.h): NaN -> 0x7fc0, else add
// 0x7fff + the kept part's lowest bit and truncate (a carry out of the mantissa rounds up to the next exponent,
// the largest finite values to inf).
template <bool BF>
__device__ __forceinline__ uint32_t round16(float x) {
  if (BF) {
    const uint32_t b = __builtin_bit_cast(uint32_t, x);
    if (x != x) return 0x7fc0u;
    return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
  }
  return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x);
}

template <bool BF>
__global__ __launch_bounds__(PK_THREADS) void k_pack_row(PackList L, uint16_t* __restrict__ row) {
  int lo = 0, hi = L.T - 1;  // largest t with blk0[t] <= blockIdx.x
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (L.blk0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int t = lo;
  const int64_t n = L.n[t];
  const int64_t i = (int64_t)(blockIdx.x - L.blk0[t]) * PK_CHUNK + (int64_t)threadIdx.x * 8;
  if (i >= n) return;
  const int cnt = n - i < 8 ? (int)(n - i) : 8;
  const float* sp = L.src[t] + i;
  float v[8];
  if (cnt == 8 && ((uintptr_t)sp & 15) == 0) {
    const f4 a0 = *(const f4*)sp, a1 = *(const f4*)(sp + 4);
    v[0] = a0.x; v[1] = a0.y; v[2] = a0.z; v[3] = a0.w;
    v[4] = a1.x; v[5] = a1.y; v[6] = a1.z; v[7] = a1.w;
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = c < cnt ? sp[c] : 0.f;
  }
  uint32_t h[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) h[c] = round16<BF>(v[c]);
  uint16_t* op = row + L.dst[t] + i;
  if (cnt == 8 && ((uintptr_t)op & 15) == 0) {
    *(u4*)op = u4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
  } else if (cnt == 8 && ((uintptr_t)op & 3) == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) ((uint32_t*)op)[c] = h[2 * c] | (h[2 * c + 1] << 16);
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < cnt) op[c] = (uint16_t)h[c];
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedhalf.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t fh_abi_version(void) { return FH_ABI_VERSION; }

extern "C" int64_t fh_reduce_plan(int32_t cus, int32_t K, int64_t P, int32_t weighted, int64_t* plan_out,
                                  int32_t cap) {
  (void)weighted;
  if (cus <= 0 || K < 0 || P < 0 || cap < 0 || (cap > 0 && !plan_out))
    return fail(FA_E_ARG, "fh_reduce_plan: bad arguments (cus=%d K=%d P=%lld cap=%d)", cus, K, (long long)P, cap);
  return strip_plan_export(cus, half_strips(P), FH_GEO, plan_out, cap);
}

extern "C" int64_t fh_reduce_launches(int32_t K, int64_t P, int32_t weighted) {
  (void)weighted;
  if (K < 0 || P <= 0) return 0;
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fh_reduce_launches: no CU count for device %d", fa_scope_device());
  StripLaunch l[3];
  return strip_plan(cus, half_strips(P), FH_GEO, l);
}

extern "C" int fh_reduce(const void* x16, int32_t row_dtype, int64_t ld, int32_t K, int64_t P, const float* a,
                         const float* acc_in, float* out, float* mirror, float denom, int32_t flags,
                         fa_stream_t stream) {
  if (row_dtype != FH_F16 && row_dtype != FH_BF16)
    return fail(FA_E_ARG, "fh_reduce: row_dtype=%d is neither FH_F16 (0) nor FH_BF16 (1)", row_dtype);
  if (K < 0 || P < 0 || ld < P) return fail(FA_E_ARG, "fh_reduce: bad sizes (ld < P or negative)");
  if (ld % 64 != 0) return fail(FA_E_ARG, "fh_reduce: ld=%lld must be a multiple of 64 elements", (long long)ld);
  if (flags & ~(FA_ACCUMULATE | FA_FINALIZE)) return fail(FA_E_ARG, "fh_reduce: unknown flags %d", flags);
  if ((flags & FA_ACCUMULATE) && !acc_in) return fail(FA_E_ARG, "fh_reduce: FA_ACCUMULATE without acc_in");
  if (K == 0 && !(flags & FA_ACCUMULATE)) return fail(FA_E_ARG, "fh_reduce: K == 0 with nothing to accumulate");
  if (K > 0 && !x16) return fail(FA_E_ARG, "fh_reduce: x16 is NULL");
  if (!out) return fail(FA_E_ARG, "fh_reduce: out is NULL");
  if (!aligned16(x16)) return fail(FA_E_ARG, "fh_reduce: x16 must be 16-byte aligned");
  if (!aligned16(out) || !aligned16(acc_in) || !aligned16(mirror))
    return fail(FA_E_ARG, "fh_reduce: out, acc_in and mirror must be 16-byte aligned");
  if (mirror && !(flags & FA_FINALIZE)) return fail(FA_E_ARG, "fh_reduce: mirror needs FA_FINALIZE");
  if (P == 0) return FA_OK;
  const int64_t P8 = (P + 7) / 8, P4 = (P + 3) / 4;
  if (P8 / (64 * FH_WAVES) > 0x7fffffffLL) return fail(FA_E_RANGE, "fh_reduce: P too large");
  FA_DEVICE_SCOPE("fh_reduce", stream, out);
  FA_OPERAND("x16", x16, K > 0 ? (uint64_t)((K - 1) * ld + P8 * 8) * 2 : 0);
  FA_OPERAND("a", a, (uint64_t)K * 4);
  FA_OPERAND("acc_in", (flags & FA_ACCUMULATE) ? acc_in : nullptr, (uint64_t)P4 * 16);
  FA_OPERAND("out", out, (uint64_t)P4 * 16);
  FA_HOST_OK_OPERAND("mirror", mirror, (uint64_t)P4 * 16);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fh_reduce launch plan: no CU count for device %d", fa_scope_device());
  HalfArgs r{};
  r.x = reinterpret_cast<const u4*>(x16); r.ld8 = ld / 8; r.P8 = P8; r.P4 = P4; r.K = K; r.flags = flags;
  r.a = a; r.acc_in = acc_in; r.out = out; r.mirror = mirror; r.denom = denom;
  StripLaunch l[3];
  const int n = strip_plan(cus, half_strips(P), FH_GEO, l);
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < n; ++i) {
    if (row_dtype == FH_BF16) {
      if (a) launch_level<true, true>(r, l[i], st); else launch_level<true, false>(r, l[i], st);
    } else {
      if (a) launch_level<false, true>(r, l[i], st); else launch_level<false, false>(r, l[i], st);
    }
    const int e = check_launch("fh_reduce");
    if (e) return e;
  }
  return FA_OK;
}

extern "C" int fh_pack_row(const float* const* src, const int64_t* numel, const int64_t* dst_off, int32_t T,
                           void* row16, int32_t row_dtype, fa_stream_t stream) {
  if (row_dtype != FH_F16 && row_dtype != FH_BF16)
    return fail(FA_E_ARG, "fh_pack_row: row_dtype=%d is neither FH_F16 (0) nor FH_BF16 (1)", row_dtype);
  if (T < 0) return fail(FA_E_ARG, "fh_pack_row: negative T");
  if (T > 0 && (!src || !numel || !dst_off)) return fail(FA_E_ARG, "fh_pack_row: NULL table");
  if (!row16 || ((uintptr_t)row16 & 1u)) return fail(FA_E_ARG, "fh_pack_row: row16 NULL or not 2-byte aligned");
  int64_t end = 0;
  for (int i = 0; i < T; ++i) {
    if (numel[i] < 0 || dst_off[i] < 0) return fail(FA_E_ARG, "fh_pack_row: tensor %d: negative size or offset", i);
    if (numel[i] == 0) continue;
    if (!src[i] || ((uintptr_t)src[i] & 3u))
      return fail(FA_E_ARG, "fh_pack_row: tensor %d: src NULL or not 4-byte aligned", i);
    if (numel[i] > PK_CHUNK * (int64_t)(1 << 28) || dst_off[i] > INT64_MAX / 4 - numel[i])
      return fail(FA_E_RANGE, "fh_pack_row: tensor %d too large", i);
    if (dst_off[i] + numel[i] > end) end = dst_off[i] + numel[i];
  }
  if (end == 0) return FA_OK;
  FA_DEVICE_SCOPE("fh_pack_row", stream, row16);
  FA_TABLE("src", src, numel, T, 4);
  FA_OPERAND("row16", row16, (uint64_t)end * 2);
  int t = 0;
  while (t < T) {
    PackList L;
    L.T = 0;
    int64_t blk = 0;
    for (; t < T && L.T < PK_MAX; ++t) {
      if (numel[t] == 0) continue;
      const int64_t nb = (numel[t] + PK_CHUNK - 1) / PK_CHUNK;
      if (L.T > 0 && blk + nb > (1 << 30)) break;  // the next launch takes it
      L.src[L.T] = src[t];
      L.n[L.T] = numel[t];
      L.dst[L.T] = dst_off[t];
      L.blk0[L.T] = (int32_t)blk;
      blk += nb;
      ++L.T;
    }
    if (L.T == 0) continue;
    L.blk0[L.T] = (int32_t)blk;
    if (row_dtype == FH_BF16)
      hipLaunchKernelGGL(k_pack_row<true>, dim3((unsigned)blk), dim3(PK_THREADS), 0, (hipStream_t)stream, L,
                         (uint16_t*)row16);
    else
      hipLaunchKernelGGL(k_pack_row<false>, dim3((unsigned)blk), dim3(PK_THREADS), 0, (hipStream_t)stream, L,
                         (uint16_t*)row16);
    const int e = check_launch("fh_pack_row");
    if (e) return e;
  }
  return FA_OK;
}
