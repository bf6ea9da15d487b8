// sign_reduce.hip — MI355X (gfx950) kernels of the 1-bit sign delta-upload path (include/fedsign.h):
//   * fsg_reduce: the in-order fp32 column chain over client deltas staged as one sign bit per column and one fp32
//     scale per block of 256 columns — 9/64 byte per parameter per staged row and per reduction pass.  A lane reads
//     one dword of a row (32 columns) and its block's scale once, shifts each column's bit into bit 31, merges it
//     into the scale's bits (one v_bfi_b32) and adds the result to the chain, in arrival order.  The reduce
//     is bounded by these vector operations, not by its bytes;
//   * fsg_reduce_plan: the launches it makes, as a host-only function of the CU count;
//   * fsg_sign_row: the executor-side handler, one fp32 row (minus the round's base model, plus the residual) into
//     bits, scales and the new residual in one launch.
//
// Numerics: every fp32 and fp64 op is rounded to nearest and never contracted into an FMA; the default denormal
// modes are kept, so subnormal scales survive.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fedsign.h"
#include "fa_device.h"
#include "fa_common.h"

// Tuning knobs (tools/sign_reduce_measure.py per library, FEDAGG_LIB).  FSG_L0_V / FSG_L0_U: the
// strips per wave and the rows in flight of levels 0 and 1.  FSG_L0_CAP: level 0's grid cap, workgroups per 100 CUs.
#if defined(FSG_L0_V) || defined(FSG_L0_U) || defined(FSG_L0_CAP)
#if !defined(FA_TUNING) || !FA_TUNING
#error "FSG_L0_V / FSG_L0_U / FSG_L0_CAP are tuning knobs: build with -DFA_TUNING=1"
#endif
#endif
#ifndef FSG_L0_V
#define FSG_L0_V 1
#endif
#ifndef FSG_L0_U
#define FSG_L0_U 8
#endif
#ifndef FSG_L0_CAP
#define FSG_L0_CAP 600
#endif

namespace {

typedef uint32_t u2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------
// fsg_reduce
// ------------------------------------------------------------------------------------------------
constexpr int FSG_WAVES = 4;  // waves per workgroup, each owning V strips of a tile

struct SignArgs {
  const uint32_t* w;  // the bit rows, in dwords (32 columns)
  const uint32_t* sc; // the scales' bits, one per 256 columns
  int64_t ldw;        // bit row stride in dwords
  int64_t lds;        // scale row stride in floats
  int64_t Pw;         // dwords to read, ceil(P / 32)
  int64_t P;          // columns to write
  int64_t c0;         // first dword column of this launch
  int64_t ntiles;     // tiles of this launch; workgroup b takes tiles b, b + grid, ...
  int n;
  int flags;
  const float* acc_in;
  float* out;
};

// 32 columns of a row (one dword) and their block's scale onto the lane's chain.  deq's bits are the scale's with
// the sign bit xor the column's bit: a scale whose own sign bit is set flips every bit of the word once, and column
// i is then the scale's magnitude bits under (bit i moved to bit 31) — a shift and a bit-merge per column, then the
// add.  The merge is written as copysign, a pure bit operation (NaN scales keep their payload), which is one
// v_bfi_b32; the same merge spelled with masks compiles to an and and an or.
__device__ __forceinline__ void sign_add(uint32_t w, uint32_t sb, float s[32]) {
  w ^= (uint32_t)((int32_t)sb >> 31);
  const float sc = __builtin_bit_cast(float, sb);
#pragma unroll
  for (int i = 0; i < 32; ++i) s[i] = s[i] + __builtin_copysignf(sc, __builtin_bit_cast(float, w << (31 - i)));
}

// a streamed dword at a uniform base plus the lane's 32-bit byte offset
__device__ __forceinline__ uint32_t ld32(const char* base, uint32_t off) {
  return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(base + off));
}

// One tile: each of the workgroup's waves owns V strips (64 lanes x one dword: 2048 contiguous columns of a row
// each) and walks all n rows, U rows' loads issued ahead of their adds.  A lane holds 32V accumulators and 2UV load
// registers (the dword and the scale: the eight lanes of a block load the same scale address, once per row).  A strip
// past ceil(P / 32) is masked without a branch in the row loop: its lanes read the row's first dword and scale
// instead (always inside the row), and nothing of what they add is stored.
template <int V, int U>
__device__ __forceinline__ void sign_tile(const SignArgs& r, int64_t tile, int lane, int wave) {
  const int64_t c0 = r.c0 + (tile * FSG_WAVES + wave) * (64LL * V) + lane;
  bool ok[V];
  uint32_t ow[V], os[V];  // the lane's dword and scale of a row ((c0 + 64 j) / 8 = c0 / 8 + 8 j), as 32-bit BYTE
                          // offsets from the row's uniform base: a load is then scalar base + one vector register,
                          // where 64-bit lane addresses cost two registers per load in flight (4UV in all)
#pragma unroll
  for (int j = 0; j < V; ++j) {
    ok[j] = (c0 + 64 * j) < r.Pw;
    ow[j] = ok[j] ? 4u * (uint32_t)(c0 + 64 * j) : 0u;
    os[j] = ok[j] ? 4u * (uint32_t)((c0 >> 3) + 8 * j) : 0u;
  }

  float s[V][32];
  if (r.flags & FA_ACCUMULATE) {
    const f4* ain = reinterpret_cast<const f4*>(r.acc_in);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t c = 8 * (c0 + 64 * j);
#pragma unroll
      for (int h = 0; h < 8; ++h) {
        const f4 a = (ok[j] && 4 * (c + h) < r.P) ? ain[c + h] : f4{0.f, 0.f, 0.f, 0.f};
        s[j][4 * h] = a.x; s[j][4 * h + 1] = a.y; s[j][4 * h + 2] = a.z; s[j][4 * h + 3] = a.w;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
      for (int i = 0; i < 32; ++i) s[j][i] = 0.f;
  }

  const char* row = reinterpret_cast<const char*>(r.w);
  const char* srow = reinterpret_cast<const char*>(r.sc);
  const int64_t ldw = 4 * r.ldw, lds = 4 * r.lds;  // row strides in bytes
  int k = 0;
  for (; k + U <= r.n; k += U) {
    uint32_t t[U][V], e[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) {
        t[u][j] = ld32(row + u * ldw, ow[j]);
        e[u][j] = ld32(srow + u * lds, os[j]);
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) {
        sign_add(t[u][j], e[u][j], s[j]);
        // one dword's 32 columns at a time: left alone, the scheduler interleaves all UV dwords' shifts and merges
        // and keeps them live
        __builtin_amdgcn_sched_barrier(0);
      }
    row += U * ldw;
    srow += U * lds;
  }
  for (; k < r.n; ++k) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      sign_add(ld32(row, ow[j]), ld32(srow, os[j]), s[j]);
      __builtin_amdgcn_sched_barrier(0);
    }
    row += ldw;
    srow += lds;
  }

#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (!ok[j]) continue;
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const int64_t p = 32 * (c0 + 64 * j) + 4 * h;
      if (p + 4 <= r.P) {
        *reinterpret_cast<f4*>(r.out + p) = f4{s[j][4 * h], s[j][4 * h + 1], s[j][4 * h + 2], s[j][4 * h + 3]};
      } else if (p < r.P) {  // the last, partial float4 column: columns >= P are not written
        r.out[p] = s[j][4 * h];
        if (p + 1 < r.P) r.out[p + 1] = s[j][4 * h + 1];
        if (p + 2 < r.P) r.out[p + 2] = s[j][4 * h + 2];
      }
    }
  }
}

// LOOP = false: workgroup b reduces tile b.  LOOP = true: a capped grid, workgroup b reduces tiles b, b + grid, ...
template <int V, int U, bool LOOP>
__global__ __launch_bounds__(64 * FSG_WAVES) void k_reduce_sign(SignArgs r) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (LOOP) {
    for (int64_t tile = blockIdx.x; tile < r.ntiles; tile += gridDim.x) sign_tile<V, U>(r, tile, lane, wave);
  } else {
    sign_tile<V, U>(r, blockIdx.x, lane, wave);
  }
}

// Launch plan: strip_plan (fa_common.h) over strips of 2048 columns (64 lanes x one dword).  The reduce is bounded by
// its vector operations, and one wave alone on a SIMD issues them at half the rate of two or more, so — unlike the
// byte-bound reduces, whose level 0 runs on fewer workgroups than CUs — level 0's grid is capped at six workgroups
// per CU: the six waves per SIMD the kernel's registers allow, all resident at once.  A lane holds 32V accumulators
// and 2UV load registers; V = 1, U = 8 compiles to 76 / 78 registers, V = 2 to 254 (the compiler then keeps a second
// copy of the accumulators around the float4 loads and stores: one wave per SIMD, not used).  So all three levels
// run the V = 1 tile and differ in their grids only (measured register counts: DESIGN.md §4; no kernel uses scratch):
//   level 0  V = 1, U = 8   a capped grid, every workgroup walking the same number of tiles
//   level 1  V = 1, U = 8   one whole tile per workgroup: a bucket too short for level 0's grid
//   level 2  V = 1, U = 8   the ragged rest
// K does not enter the plan today; it is a parameter because fa_reduce's plan depends on it.
constexpr StripGeo FSG_GEO{FSG_WAVES, {FSG_L0_V, FSG_L0_V, 1}, {FSG_L0_U, FSG_L0_U, 8}, FSG_L0_CAP, 2048};
static_assert(FSG_PLAN_FIELDS == STRIP_PLAN_FIELDS, "fsg_reduce_plan's row is strip_plan_export's");

int64_t sign_strips(int64_t P) { return ((P + 31) / 32 + 63) / 64; }

template <int V, int U>
void launch_one(SignArgs r, const StripLaunch& l, hipStream_t st) {
  r.c0 = l.strip0 * 64;
  r.ntiles = l.tiles;
  const dim3 grid((unsigned)l.grid), blk(64 * FSG_WAVES);
  if (l.grid < l.tiles)  // only level 0 runs on a capped grid
    hipLaunchKernelGGL((k_reduce_sign<V, U, true>), grid, blk, 0, st, r);
  else
    hipLaunchKernelGGL((k_reduce_sign<V, U, false>), grid, blk, 0, st, r);
}

void launch_level(const SignArgs& r, const StripLaunch& l, hipStream_t st) {
  if (l.level < 2)
    launch_one<FSG_GEO.V[0], FSG_GEO.U[0]>(r, l, st);
  else
    launch_one<FSG_GEO.V[2], FSG_GEO.U[2]>(r, l, st);
}

// ------------------------------------------------------------------------------------------------
// fsg_sign_row
// ------------------------------------------------------------------------------------------------
constexpr int SR_WAVES = 4;  // blocks per workgroup: one wave encodes one block of 256 columns

// One wave per block; lane l holds the block's columns l, l + 64, l + 128 and l + 192 — the four terms of the
// contract's t[l] — so a quarter's 64 sign bits are one __ballot mask, the scale is one wave_sum, and nothing crosses
// waves (no LDS, no barrier).  Each of the four loads of a row is one contiguous 256-byte run per wave.
__global__ __launch_bounds__(64 * SR_WAVES) void k_sign_row(const float* x, const float* base, const float* res,
                                                            int64_t P, int64_t NB, uint8_t* bits, float* scales,
                                                            float* res_out) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * SR_WAVES + (threadIdx.x >> 6);
  if (b >= NB) return;  // whole waves leave together
  const int64_t p0 = b * FSG_BLOCK + lane;
  const int64_t nb = P - b * FSG_BLOCK < FSG_BLOCK ? P - b * FSG_BLOCK : FSG_BLOCK;
  float e[4];
  bool bad = false;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t p = p0 + 64 * q;
    e[q] = 0.f;  // a missing column of a partial block: +0.0, bit 0
    if (p < P) {
      float v = x[p];
      if (base) v = v - base[p];
      if (res) v = v + res[p];
      e[q] = v;
    }
    bad |= (__builtin_bit_cast(uint32_t, e[q]) & 0x7fffffffu) >= 0x7f800000u;
  }
  const bool nan_block = __ballot(bad) != 0ull;
  double t = (((double)fabsf(e[0]) + (double)fabsf(e[1])) + (double)fabsf(e[2])) + (double)fabsf(e[3]);
  t = wave_sum(t);
  const float scale = nan_block ? __builtin_bit_cast(float, 0x7fc00000u) : (float)(t / (double)nb);
  uint64_t mine = 0;  // lane q < 4 keeps quarter q's mask and stores its 8 bytes
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint64_t m = __ballot((__builtin_bit_cast(uint32_t, e[q]) >> 31) != 0u);
    if (lane == q) mine = nan_block ? 0ull : m;
  }
  if (lane < 4)
    *reinterpret_cast<u2*>(bits + b * (FSG_BLOCK / 8) + 8 * lane) = u2{(uint32_t)mine, (uint32_t)(mine >> 32)};
  if (lane == 0) scales[b] = scale;
  if (res_out) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t p = p0 + 64 * q;
      if (p < P) {
        const float deq = (__builtin_bit_cast(uint32_t, e[q]) >> 31) ? -scale : scale;
        res_out[p] = nan_block ? 0.f : e[q] - deq;
      }
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedsign.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t fsg_abi_version(void) { return FSG_ABI_VERSION; }

extern "C" int64_t fsg_reduce_plan(int32_t cus, int32_t K, int64_t P, int64_t* plan_out, int32_t cap) {
  if (cus <= 0 || K < 0 || P < 0 || cap < 0 || (cap > 0 && !plan_out))
    return refuse(FA_E_ARG, "fsg_reduce_plan: bad arguments (cus=%d K=%d P=%lld cap=%d)", cus, K, (long long)P, cap);
  return strip_plan_export(cus, sign_strips(P), FSG_GEO, plan_out, cap);
}

extern "C" int fsg_reduce(const uint8_t* bits, const float* scales, int64_t ldb, int64_t lds, int32_t n, int64_t P,
                          const float* acc_in, float* out, int32_t flags, fa_stream_t stream) {
  if (flags & ~FA_ACCUMULATE) return refuse(FA_E_ARG, "fsg_reduce: unknown flags %d (0 or FA_ACCUMULATE)", flags);
  if (n < 0 || P < 0) return refuse(FA_E_ARG, "fsg_reduce: negative n=%d or P=%lld", n, (long long)P);
  const int64_t PB = (P + 7) / 8, NB = (P + FSG_BLOCK - 1) / FSG_BLOCK, Pw = (P + 31) / 32;
  if (ldb < PB)
    return refuse(FA_E_ARG, "fsg_reduce: ldb=%lld < ceil(P / 8)=%lld bytes per row", (long long)ldb, (long long)PB);
  if (ldb % 16 != 0) return refuse(FA_E_ARG, "fsg_reduce: ldb=%lld must be a multiple of 16 bytes", (long long)ldb);
  if (lds < NB)
    return refuse(FA_E_ARG, "fsg_reduce: lds=%lld < ceil(P / 256)=%lld scales per row", (long long)lds, (long long)NB);
  if ((flags & FA_ACCUMULATE) && !acc_in) return refuse(FA_E_ARG, "fsg_reduce: FA_ACCUMULATE without acc_in");
  if (n == 0 && !(flags & FA_ACCUMULATE)) return refuse(FA_E_ARG, "fsg_reduce: n=0 rows with nothing to accumulate");
  if (n > 0 && (!bits || !scales)) return refuse(FA_E_ARG, "fsg_reduce: bits or scales is NULL");
  if (!out) return refuse(FA_E_ARG, "fsg_reduce: out is NULL");
  if (!aligned16(bits) || !aligned16(scales))
    return refuse(FA_E_ARG, "fsg_reduce: bits and scales must be 16-byte aligned");
  if (!aligned16(out) || !aligned16(acc_in)) return refuse(FA_E_ARG, "fsg_reduce: out and acc_in must be 16-byte aligned");
  if (P == 0) return FA_OK;
  const int64_t P4 = (P + 3) / 4;
  if (Pw * 4 > 0xffffffffLL) return refuse(FA_E_RANGE, "fsg_reduce: P too large (row offsets are 32-bit)");
  FA_DEVICE_SCOPE("fsg_reduce", stream, out);
  FA_OPERAND("bits", bits, n > 0 ? (uint64_t)((int64_t)(n - 1) * ldb + Pw * 4) : 0);
  FA_OPERAND("scales", scales, n > 0 ? (uint64_t)((int64_t)(n - 1) * lds + NB) * 4 : 0);
  FA_OPERAND("acc_in", (flags & FA_ACCUMULATE) ? acc_in : nullptr, (uint64_t)P4 * 16);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fsg_reduce launch plan: no CU count for device %d", fa_scope_device());
  SignArgs r{};
  r.w = reinterpret_cast<const uint32_t*>(bits); r.sc = reinterpret_cast<const uint32_t*>(scales);
  r.ldw = ldb / 4; r.lds = lds; r.Pw = Pw; r.P = P;
  r.n = n; r.flags = flags; r.acc_in = acc_in; r.out = out;
  StripLaunch l[3];
  const int nl = strip_plan(cus, sign_strips(P), FSG_GEO, l);
  for (int i = 0; i < nl; ++i) {
    launch_level(r, l[i], (hipStream_t)stream);
    const int e = check_launch("fsg_reduce");
    if (e) return e;
  }
  return FA_OK;
}

extern "C" int fsg_sign_row(const float* x, const float* base, const float* residual, int64_t P, uint8_t* bits,
                            float* scales, float* residual_out, fa_stream_t stream) {
  if (P < 0) return refuse(FA_E_ARG, "fsg_sign_row: negative P=%lld", (long long)P);
  if (P == 0) return FA_OK;
  if (!x || !bits || !scales) return refuse(FA_E_ARG, "fsg_sign_row: x, bits or scales is NULL");
  if (!aligned16(bits)) return refuse(FA_E_ARG, "fsg_sign_row: bits must be 16-byte aligned");
  if (((uintptr_t)x | (uintptr_t)base | (uintptr_t)residual | (uintptr_t)residual_out | (uintptr_t)scales) & 3u)
    return refuse(FA_E_ARG, "fsg_sign_row: x, base, residual, residual_out and scales must be 4-byte aligned");
  const int64_t NB = (P + FSG_BLOCK - 1) / FSG_BLOCK;
  const int64_t grid = (NB + SR_WAVES - 1) / SR_WAVES;
  if (grid > 0x7fffffffLL) return refuse(FA_E_RANGE, "fsg_sign_row: P too large");
  FA_DEVICE_SCOPE("fsg_sign_row", stream, bits);
  FA_OPERAND("x", x, (uint64_t)P * 4);
  FA_OPERAND("base", base, (uint64_t)P * 4);
  FA_OPERAND("residual", residual, (uint64_t)P * 4);
  FA_OPERAND("bits", bits, (uint64_t)NB * (FSG_BLOCK / 8));
  FA_OPERAND("scales", scales, (uint64_t)NB * 4);
  FA_OPERAND("residual_out", residual_out, (uint64_t)P * 4);
  hipLaunchKernelGGL(k_sign_row, dim3((unsigned)grid), dim3(64 * SR_WAVES), 0, (hipStream_t)stream, x, base,
                     residual, P, NB, bits, scales, residual_out);
  return check_launch("fsg_sign_row");
}
