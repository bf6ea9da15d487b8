// vote_reduce.hip — MI355X (gfx950) kernels of the majority-vote sign path (include/fedvote.h):
//   * fvt_count: per-column set-bit counts over client uploads staged as one sign bit per column and nothing else —
//     1/8 byte per parameter per staged row.  A lane reads one dword of a row (32 columns) and keeps the counts of
//     its 32 columns BIT-SLICED: plane j of the counter is one register whose bit i is bit j of column i's count.  A
//     row dword is then added to all 32 counters at once by carry-save adders (two v_bitop3_b32 each), 16 rows
//     through a Harley-Seal tree of 15 adders: about 5 vector operations per row and 32 columns, where
//     fsg_reduce (sign_reduce.hip) spends 96.  The planes are expanded to integers once, in the epilogue;
//   * fvt_count_plan: the launches it makes and the row split, as a host-only function of (CU count, n, P);
//   * fvt_finish: the vote margin into the new model, one streaming pass;
//   * fvt_sign_row: the executor-side encoder, one fp32 row (minus the round's base model) into bits.
//
// Numerics: the tally is integer and exact; the finish's fp32 ops are rounded to nearest and never contracted into
// an FMA, the division is correctly rounded, the default denormal modes are kept.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fedvote.h"
#include "fa_device.h"
#include "fa_common.h"

// Tuning knobs (tools/vote_reduce_measure.py per library, FEDAGG_LIB).  FVT_L0_V: the strips per wave of
// levels 0 and 1.  FVT_L0_U: the rows whose loads are issued together, 8 or 16 (half or all of an adder group).
// FVT_L0_CAP: level 0's grid cap, workgroups per 100 CUs.
#if defined(FVT_L0_V) || defined(FVT_L0_U) || defined(FVT_L0_CAP)
#if !defined(FA_TUNING) || !FA_TUNING
#error "FVT_L0_V / FVT_L0_U / FVT_L0_CAP are tuning knobs: build with -DFA_TUNING=1"
#endif
#endif
#ifndef FVT_L0_V
#define FVT_L0_V 1
#endif
#ifndef FVT_L0_U
#define FVT_L0_U 16
#endif
#ifndef FVT_L0_CAP
#define FVT_L0_CAP 800
#endif

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// fvt_count
// ------------------------------------------------------------------------------------------------
constexpr int FVT_WAVES = 4;   // waves per workgroup, each owning V strips of a tile
constexpr int FVT_GROUP = 16;  // rows of one pass through the adder tree
constexpr int FVT_LOW = 4;     // the planes ones, twos, fours, eights that the tree keeps

struct VoteArgs {
  const uint32_t* w;  // the bit rows, in dwords (32 columns)
  int64_t ldw;        // bit row stride in dwords
  int64_t Pw;         // dwords to read, ceil(P / 32)
  int64_t P;          // columns to write
  int64_t c0;         // first dword column of this launch
  int64_t ntiles;     // tiles of this launch; LOOP: workgroup b takes tiles b, b + grid, ...
  int n;              // rows
  int S;              // workgroups that share one tile's rows
  int rps;            // rows of one such workgroup, a multiple of FVT_GROUP when S > 1
  int accumulate;     // cnt += (a split launch always adds: cnt was zeroed before it)
  uint32_t* cnt;
};

// A full adder on 32 columns at once: lo is the sum bit a ^ b ^ c, hi the carry, the bitwise majority.  gfx950 has
// v_bitop3_b32, any boolean function of three registers by its truth table: 0x96 is the three-way xor and 0xe8 the
// majority, so an adder is two vector operations.  Written with xors and a select ("c where a and b differ, else a",
// a v_bfi_b32) the compiler finds bitop3 too, but first reassociates the tree: 95 operations per 16 rows, not 50.
__device__ __forceinline__ void csa(uint32_t& hi, uint32_t& lo, uint32_t a, uint32_t b, uint32_t c) {
  hi = __builtin_amdgcn_bitop3_b32(a, b, c, 0xe8);
  lo = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// Eight row dwords onto the low planes p[0..2] (ones, twos, fours): seven adders; returns the word of weight eight
// they emit.
__device__ __forceinline__ uint32_t half8(uint32_t* p, const uint32_t* d) {
  uint32_t t2a, t2b, t4a, t4b, t8;
  csa(t2a, p[0], p[0], d[0], d[1]);
  csa(t2b, p[0], p[0], d[2], d[3]);
  csa(t4a, p[1], p[1], t2a, t2b);
  csa(t2a, p[0], p[0], d[4], d[5]);
  csa(t2b, p[0], p[0], d[6], d[7]);
  csa(t4b, p[1], p[1], t2a, t2b);
  csa(t8, p[2], p[2], t4a, t4b);
  return t8;
}

// The two weight-eight words of a group of 16 rows onto eights (the tree's 15th adder); the one word of weight
// sixteen it emits ripples into the H high planes as a chain of half adders (an and and an xor per plane).  H planes
// above the four low ones count to 2^(4 + H) - 1.
template <int H>
__device__ __forceinline__ void close16(uint32_t* p, uint32_t t8a, uint32_t t8b) {
  uint32_t carry;
  csa(carry, p[3], p[3], t8a, t8b);
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const uint32_t t = p[FVT_LOW + h] & carry;
    p[FVT_LOW + h] ^= carry;
    carry = t;
  }
}

// a streamed dword at a uniform base plus the lane's 32-bit byte offset
__device__ __forceinline__ uint32_t ld32(const char* base, uint32_t off) {
  return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(base + off));
}

// One tile over the rows [r0, r1): each of the workgroup's waves owns V strips (64 lanes x one dword: 2048 contiguous
// columns of a row each).  A lane holds (4 + H) V plane registers and 16 V row dwords; no LDS, no cross-lane traffic.
// A strip past ceil(P / 32) is masked without a branch in the row loop: its lanes read the row's first dword instead
// (always inside the row), and nothing of what they count is stored.  The ragged last r % 16 rows go through the same
// adders, the missing rows as zero words (the row test is wave-uniform).
template <int V, int U, int H, bool ATOMIC>
__device__ __forceinline__ void vote_tile(const VoteArgs& r, int64_t tile, int r0, int r1, int lane, int wave) {
  static_assert(U == 8 || U == 16, "U is half or all of an adder group");
  constexpr int NP = FVT_LOW + H;
  const int64_t c0 = r.c0 + (tile * FVT_WAVES + wave) * (64LL * V) + lane;
  bool ok[V];
  uint32_t ow[V];  // the lane's dword of a row as a 32-bit BYTE offset from the row's uniform base
#pragma unroll
  for (int j = 0; j < V; ++j) {
    ok[j] = (c0 + 64 * j) < r.Pw;
    ow[j] = ok[j] ? 4u * (uint32_t)(c0 + 64 * j) : 0u;
  }
  uint32_t p[V][NP];
#pragma unroll
  for (int j = 0; j < V; ++j)
#pragma unroll
    for (int q = 0; q < NP; ++q) p[j][q] = 0u;

  const int64_t ldw = 4 * r.ldw;  // row stride in bytes
  const char* row = reinterpret_cast<const char*>(r.w) + (int64_t)r0 * ldw;
  int k = r0;
  for (; k + FVT_GROUP <= r1; k += FVT_GROUP) {
    uint32_t d[V][FVT_GROUP], t8[2][V];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (U == 8 || half == 0) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int j = 0; j < V; ++j) d[j][8 * half + u] = ld32(row + (8 * half + u) * ldw, ow[j]);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) t8[half][j] = half8(p[j], d[j] + 8 * half);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) close16<H>(p[j], t8[0][j], t8[1][j]);
    row += FVT_GROUP * ldw;
  }
  if (k < r1) {
    uint32_t d[V][FVT_GROUP];
#pragma unroll
    for (int u = 0; u < FVT_GROUP; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) d[j][u] = (k + u < r1) ? ld32(row + u * ldw, ow[j]) : 0u;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const uint32_t a = half8(p[j], d[j]), b = half8(p[j], d[j] + 8);
      close16<H>(p[j], a, b);
    }
  }

  // the planes into 32 integers per lane and strip, four columns at a time: a v_bfe_u32 and a v_lshl_or_b32 per plane
  // and column, once per tile.  8 x 16 bytes per lane, 128 bytes lane stride.
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (!ok[j]) continue;
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      uint32_t c[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        c[i] = 0u;
#pragma unroll
        for (int q = 0; q < NP; ++q) c[i] |= ((p[j][q] >> (4 * h + i)) & 1u) << q;
      }
      const int64_t col = 32 * (c0 + 64 * j) + 4 * h;
      if (ATOMIC) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (col + i < r.P && c[i]) atomicAdd(r.cnt + col + i, c[i]);
      } else if (col + 4 <= r.P) {
        u4 v = u4{c[0], c[1], c[2], c[3]};
        if (r.accumulate) v += *reinterpret_cast<const u4*>(r.cnt + col);
        *reinterpret_cast<u4*>(r.cnt + col) = v;
      } else {  // the last, partial group of four: columns >= P are neither read nor written
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (col + i < r.P) r.cnt[col + i] = c[i] + (r.accumulate ? r.cnt[col + i] : 0u);
      }
    }
  }
}

// LOOP = true: a capped grid, workgroup b counts all rows of tiles b, b + grid, ... (never split).  Otherwise
// workgroup b counts slice b % S of the rows of tile b / S; with S > 1 (ATOMIC) the slices meet in cnt by atomic adds.
template <int V, int U, int H, bool LOOP, bool ATOMIC>
__global__ __launch_bounds__(64 * FVT_WAVES) void k_vote_count(VoteArgs r) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (LOOP) {
    for (int64_t tile = blockIdx.x; tile < r.ntiles; tile += gridDim.x)
      vote_tile<V, U, H, false>(r, tile, 0, r.n, lane, wave);
  } else if (ATOMIC) {
    const int s = (int)(blockIdx.x % (unsigned)r.S);
    const int r0 = s * r.rps;
    const int r1 = r0 + r.rps < r.n ? r0 + r.rps : r.n;
    if (r0 < r1) vote_tile<V, U, H, true>(r, blockIdx.x / (unsigned)r.S, r0, r1, lane, wave);
  } else {
    vote_tile<V, U, H, false>(r, blockIdx.x, 0, r.n, lane, wave);
  }
}

__global__ __launch_bounds__(256) void k_vote_zero(uint32_t* cnt, int64_t P) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) cnt[p] = 0u;
}

// Launch plan: strip_plan (fa_common.h) over strips of 2048 columns (64 lanes x one dword), as fsg_reduce's.  The
// kernel is meant to be bounded by its bytes; a lane holds 16 V planes and 16 V row dwords, so V = 1 leaves room for
// eight waves per SIMD, and level 0's grid is capped at eight workgroups per CU: all of them resident at once
// (measured register counts: DESIGN.md; no kernel uses scratch).  All three levels run the V = 1 tile and differ in
// their grids only.
//
// Row split.  A bucket whose tiles do not fill the card (fewer tiles than CUs, so no capped launch) spreads the rows
// of every tile over S workgroups: S = min(2 cus / tiles, n / 256) — twice the CUs in workgroups, and at least 256 rows
// per slice: a slice ends with 32 atomic adds per lane at a 128-byte lane stride, which cost more than they save on
// shorter slices (at 32 rows per slice 100 x 1 M took 0.12 ms, 3.6 x fsg_reduce, in a run whose log was not kept: the
// figure cannot be reproduced from the tree; transposing the epilogue through LDS would remove the cause) — and a slice is
// rps = round_up(ceil(n / S), 16) rows, S = ceil(n / rps) after rounding: every slice but the last is whole adder
// groups, none is empty.  S is a function of (cus, n, P) alone.
constexpr StripGeo FVT_GEO{FVT_WAVES, {FVT_L0_V, FVT_L0_V, 1}, {FVT_L0_U, FVT_L0_U, 16}, FVT_L0_CAP, 2048};
constexpr int FVT_SLICE_ROWS = 256;

int64_t vote_strips(int64_t P) { return ((P + 31) / 32 + 63) / 64; }

struct VotePlan {
  StripLaunch l[3];
  int nl, S, rps;
};

VotePlan vote_plan(int64_t cus, int n, int64_t P) {
  VotePlan v{};
  v.nl = strip_plan(cus, vote_strips(P), FVT_GEO, v.l);
  v.S = 1;
  v.rps = n;
  int64_t tiles = 0;
  bool capped = false;
  for (int i = 0; i < v.nl; ++i) {
    tiles += v.l[i].tiles;
    capped |= v.l[i].grid < v.l[i].tiles;
  }
  if (tiles > 0 && tiles < cus && !capped) {
    int64_t want = 2 * cus / tiles;
    if (want > n / FVT_SLICE_ROWS) want = n / FVT_SLICE_ROWS;
    if (want > 1) {
      const int64_t per = (n + want - 1) / want;
      v.rps = (int)((per + FVT_GROUP - 1) / FVT_GROUP * FVT_GROUP);
      v.S = (n + v.rps - 1) / v.rps;
    }
  }
  return v;
}

template <int V, int U, int H>
void launch_h(const VoteArgs& r, const StripLaunch& l, hipStream_t st) {
  const dim3 blk(64 * FVT_WAVES);
  if (l.grid < l.tiles)  // only level 0 runs on a capped grid, and a plan with one is never split
    hipLaunchKernelGGL((k_vote_count<V, U, H, true, false>), dim3((unsigned)l.grid), blk, 0, st, r);
  else if (r.S > 1) {
    // a slice is at least FVT_SLICE_ROWS = 256 rows, so no split launch counts on four high planes: that atomic
    // kernel is not instantiated
    if constexpr (H > 4 || FVT_SLICE_ROWS < 256)
      hipLaunchKernelGGL((k_vote_count<V, U, H, false, true>), dim3((unsigned)(l.grid * r.S)), blk, 0, st, r);
  } else
    hipLaunchKernelGGL((k_vote_count<V, U, H, false, false>), dim3((unsigned)l.grid), blk, 0, st, r);
}

// the high planes from the rows ONE workgroup counts: 4 + H planes hold up to 2^(4 + H) - 1
template <int V, int U>
void launch_one(VoteArgs r, const StripLaunch& l, hipStream_t st) {
  r.c0 = l.strip0 * 64;
  r.ntiles = l.tiles;
  if (r.rps < 256)
    launch_h<V, U, 4>(r, l, st);
  else if (r.rps < 4096)
    launch_h<V, U, 8>(r, l, st);
  else
    launch_h<V, U, 12>(r, l, st);
}

void launch_level(const VoteArgs& r, const StripLaunch& l, hipStream_t st) {
  if (l.level < 2)
    launch_one<FVT_GEO.V[0], FVT_GEO.U[0]>(r, l, st);
  else
    launch_one<FVT_GEO.V[2], FVT_GEO.U[2]>(r, l, st);
}

// ------------------------------------------------------------------------------------------------
// fvt_finish
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float vote1(uint32_t c, float l, int K, float fK, float eta, bool mean) {
  const int v = K - 2 * (int)c;
  const float s = mean ? eta * __fdiv_rn((float)v, fK) : (v > 0 ? eta : (v < 0 ? -eta : 0.0f));
  return l + s;
}

__global__ __launch_bounds__(256) void k_vote_finish(const uint32_t* cnt, const float* L, int64_t P, int K, float eta,
                                                     int mode, float* out, float* mirror) {
  const bool mean = mode == FVT_MEAN;
  const float fK = (float)K;
  const int64_t P4 = (P + 3) / 4;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < P4; g += (int64_t)gridDim.x * 256) {
    const int64_t p = 4 * g;
    if (p + 4 <= P) {
      const u4 c = __builtin_nontemporal_load(reinterpret_cast<const u4*>(cnt + p));
      const f4 l = *reinterpret_cast<const f4*>(L + p);
      f4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = vote1(c[i], l[i], K, fK, eta, mean);
      *reinterpret_cast<f4*>(out + p) = o;
      if (mirror) *reinterpret_cast<f4*>(mirror + p) = o;
    } else {  // the last, partial float4 column: columns >= P are neither read nor written
      for (int i = 0; i < (int)(P - p); ++i) {
        const float o = vote1(cnt[p + i], L[p + i], K, fK, eta, mean);
        out[p + i] = o;
        if (mirror) mirror[p + i] = o;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// fvt_sign_row
// ------------------------------------------------------------------------------------------------
constexpr int VR_WAVES = 4;   // waves per workgroup
constexpr int VR_COLS = 256;  // columns per wave: four ballots, 32 bytes

// Lane l holds the columns l, l + 64, l + 128 and l + 192 of its wave's 256, so each of the four loads of a row is
// one contiguous 256-byte run and a quarter's 64 sign bits are one __ballot mask.  Lane t < 32 then stores byte t of
// the wave's 32: byte t & 7 of quarter t >> 3.  A missing column counts +0.0, bit 0; bytes past ceil(P / 8) are not
// written.  No LDS, no barrier.
__global__ __launch_bounds__(64 * VR_WAVES) void k_vote_row(const float* x, const float* base, int64_t P, int64_t PB,
                                                            int64_t NW, uint8_t* bits) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * VR_WAVES + (threadIdx.x >> 6);
  if (b >= NW) return;  // whole waves leave together
  uint64_t m[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t p = b * VR_COLS + 64 * q + lane;
    uint32_t e = 0u;
    if (p < P) {
      float v = x[p];
      if (base) v = v - base[p];
      e = __builtin_bit_cast(uint32_t, v);
    }
    m[q] = __ballot((e >> 31) != 0u);
  }
  if (lane < 32) {
    const int q = lane >> 3;
    const uint64_t mine = q == 0 ? m[0] : (q == 1 ? m[1] : (q == 2 ? m[2] : m[3]));
    const int64_t byte = b * (VR_COLS / 8) + lane;
    if (byte < PB) bits[byte] = (uint8_t)(mine >> (8 * (lane & 7)));
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedvote.h)
// ------------------------------------------------------------------------------------------------
static_assert(FVT_PLAN_FIELDS == STRIP_PLAN_FIELDS + 1, "fvt_count_plan's row is strip_plan_export's plus S");

extern "C" int32_t fvt_abi_version(void) { return FVT_ABI_VERSION; }

extern "C" int64_t fvt_count_plan(int32_t cus, int32_t n, int64_t P, int64_t* plan_out, int32_t cap) {
  if (cus <= 0 || n < 0 || n > FVT_MAX_ROWS || P < 0 || cap < 0 || (cap > 0 && !plan_out))
    return refuse(FA_E_ARG, "fvt_count_plan: bad arguments (cus=%d n=%d P=%lld cap=%d)", cus, n, (long long)P, cap);
  const VotePlan v = vote_plan(cus, n, P);
  int64_t six[3 * STRIP_PLAN_FIELDS];
  const int nl = strip_plan_export(cus, vote_strips(P), FVT_GEO, six, 3);
  for (int i = 0; i < nl && i < cap; ++i) {
    for (int f = 0; f < STRIP_PLAN_FIELDS; ++f) plan_out[FVT_PLAN_FIELDS * i + f] = six[STRIP_PLAN_FIELDS * i + f];
    plan_out[FVT_PLAN_FIELDS * i + STRIP_PLAN_FIELDS] = v.S;
  }
  return nl;
}

extern "C" int fvt_count(const uint8_t* bits, int64_t ldb, int32_t n, int64_t P, uint32_t* cnt, int32_t flags,
                         fa_stream_t stream) {
  if (flags & ~FA_ACCUMULATE) return refuse(FA_E_ARG, "fvt_count: unknown flags %d (0 or FA_ACCUMULATE)", flags);
  if (n < 0 || P < 0) return refuse(FA_E_ARG, "fvt_count: negative n=%d or P=%lld", n, (long long)P);
  if (n > FVT_MAX_ROWS) return refuse(FA_E_RANGE, "fvt_count: n=%d rows, at most %d per call", n, FVT_MAX_ROWS);
  const int64_t PB = (P + 7) / 8, Pw = (P + 31) / 32;
  if (ldb < PB)
    return refuse(FA_E_ARG, "fvt_count: ldb=%lld < ceil(P / 8)=%lld bytes per row", (long long)ldb, (long long)PB);
  if (ldb % 16 != 0) return refuse(FA_E_ARG, "fvt_count: ldb=%lld must be a multiple of 16 bytes", (long long)ldb);
  if (n > 0 && !bits) return refuse(FA_E_ARG, "fvt_count: bits is NULL");
  if (!cnt) return refuse(FA_E_ARG, "fvt_count: cnt is NULL");
  if (!aligned16(bits) || !aligned16(cnt)) return refuse(FA_E_ARG, "fvt_count: bits and cnt must be 16-byte aligned");
  if (P == 0) return FA_OK;
  if (Pw * 4 > 0xffffffffLL) return refuse(FA_E_RANGE, "fvt_count: P too large (row offsets are 32-bit)");
  const bool acc = (flags & FA_ACCUMULATE) != 0;
  if (n == 0 && acc) return FA_OK;
  FA_DEVICE_SCOPE("fvt_count", stream, cnt);
  FA_OPERAND("bits", bits, n > 0 ? (uint64_t)((int64_t)(n - 1) * ldb + Pw * 4) : 0);
  FA_OPERAND("cnt", cnt, (uint64_t)P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fvt_count launch plan: no CU count for device %d", fa_scope_device());
  const VotePlan v = vote_plan(cus, n, P);
  if (n == 0 || (v.S > 1 && !acc)) {
    int64_t g = (P + 255) / 256;
    if (g > (int64_t)cus * 8) g = (int64_t)cus * 8;
    hipLaunchKernelGGL(k_vote_zero, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, cnt, P);
    const int e = check_launch("fvt_count (zero)");
    if (e || n == 0) return e;
  }
  VoteArgs r{};
  r.w = reinterpret_cast<const uint32_t*>(bits);
  r.ldw = ldb / 4; r.Pw = Pw; r.P = P;
  r.n = n; r.S = v.S; r.rps = v.rps; r.accumulate = acc; r.cnt = cnt;
  for (int i = 0; i < v.nl; ++i) {
    launch_level(r, v.l[i], (hipStream_t)stream);
    const int e = check_launch("fvt_count");
    if (e) return e;
  }
  return FA_OK;
}

extern "C" int fvt_finish(const uint32_t* cnt, const float* L, int64_t P, int32_t K, float eta, int32_t mode,
                          float* out, float* mirror, fa_stream_t stream) {
  if (P < 0) return refuse(FA_E_ARG, "fvt_finish: negative P=%lld", (long long)P);
  if (K < 1 || K > FVT_MAX_CLIENTS) return refuse(FA_E_ARG, "fvt_finish: K=%d must be in 1..2^24", K);
  if (!(eta > 0.0f) || !__builtin_isfinite(eta))
    return refuse(FA_E_ARG, "fvt_finish: eta=%g must be finite and > 0", (double)eta);
  if (mode != FVT_MAJORITY && mode != FVT_MEAN)
    return refuse(FA_E_ARG, "fvt_finish: unknown mode %d (FVT_MAJORITY or FVT_MEAN)", mode);
  if (!cnt || !L || !out) return refuse(FA_E_ARG, "fvt_finish: cnt, L or out is NULL");
  if (!aligned16(cnt) || !aligned16(L) || !aligned16(out) || !aligned16(mirror))
    return refuse(FA_E_ARG, "fvt_finish: cnt, L, out and mirror must be 16-byte aligned");
  if (P == 0) return FA_OK;
  FA_DEVICE_SCOPE("fvt_finish", stream, out);
  FA_OPERAND("cnt", cnt, (uint64_t)P * 4);
  FA_OPERAND("L", L, (uint64_t)P * 4);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  FA_HOST_OK_OPERAND("mirror", mirror, (uint64_t)P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fvt_finish: no CU count for device %d", fa_scope_device());
  int64_t g = ((P + 3) / 4 + 255) / 256;
  if (g > (int64_t)cus * 8) g = (int64_t)cus * 8;
  hipLaunchKernelGGL(k_vote_finish, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, cnt, L, P, K, eta, mode, out,
                     mirror);
  return check_launch("fvt_finish");
}

extern "C" int fvt_sign_row(const float* x, const float* base, int64_t P, uint8_t* bits, fa_stream_t stream) {
  if (P < 0) return refuse(FA_E_ARG, "fvt_sign_row: negative P=%lld", (long long)P);
  if (P == 0) return FA_OK;
  if (!x || !bits) return refuse(FA_E_ARG, "fvt_sign_row: x or bits is NULL");
  if (((uintptr_t)x | (uintptr_t)base) & 3u) return refuse(FA_E_ARG, "fvt_sign_row: x and base must be 4-byte aligned");
  const int64_t PB = (P + 7) / 8, NW = (P + VR_COLS - 1) / VR_COLS;
  const int64_t grid = (NW + VR_WAVES - 1) / VR_WAVES;
  if (grid > 0x7fffffffLL) return refuse(FA_E_RANGE, "fvt_sign_row: P too large");
  FA_DEVICE_SCOPE("fvt_sign_row", stream, bits);
  FA_OPERAND("x", x, (uint64_t)P * 4);
  FA_OPERAND("base", base, (uint64_t)P * 4);
  FA_OPERAND("bits", bits, (uint64_t)PB);
  hipLaunchKernelGGL(k_vote_row, dim3((unsigned)grid), dim3(64 * VR_WAVES), 0, (hipStream_t)stream, x, base, P, PB, NW,
                     bits);
  return check_launch("fvt_sign_row");
}
