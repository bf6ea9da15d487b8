// deep_trim.hip — MI355X (gfx950) kernel of the deep coordinate-wise trimmed mean (include/feddeeptrim.h):
//   * fdt_reduce: selection at any t, the kept rule, the in-order fp32 chain, the division, the optional mirror and
//                 the per-row drop counts, in ONE kernel over LDS-resident tiles (k_deep_trim);
//   * fdt_plan:   the launch it makes, as a host-only function of the CU count.
//
// Numerics: every fp32 op is rounded to nearest and never contracted into an FMA; the default denormal modes are
// kept (fp32 denormals are not flushed); the division is the IEEE one.  Selection and marking are integer arithmetic
// on the order keys: which lane counts which row never reaches a float.
//
// Tile.  A workgroup of 256 lanes owns all K rows x C columns, dense in LDS ([K][C] words, a row's C columns one
// after the other), C = 2^cl the widest of 64, 32, 16, 8, 4 whose workgroup fits 80 KiB, so that TWO workgroups share
// a CU's 160 KiB and one loads while the other selects (K <= 174: 64; <= 466: 32; <= 1002: 16; <= 1913: 8; beyond: 4;
// geo_of).  Words of a workgroup:  K C (tile) + 128 C (histogram) + 256 (partial sums) + 8 C (column state) + 2 K
// (drop counts).  Above K = 3280 not even C = 4 fits 80 KiB; those rounds take the 104 KiB instantiation, one
// workgroup per CU.
//
// One tile, in five steps (LDS operations per ELEMENT of the tile in brackets):
//   load    every lane issues 8 float4 non-temporal loads before it stores the first key, 32 KiB in flight per
//           workgroup; the staged rows are read from HBM once                              [1/4 write of 16 bytes]
//   select  twice (rank t - 1, rank K - t): a most-significant-digit radix select, 8 bits a pass, 4 passes.  Lane
//           (c, s) = (tid % C, tid / C) scans rows [s R, s R + R) of column c; a key whose upper digits equal the
//           column's prefix adds 1 to its digit's 16-bit counter (two counters a word, K <= 4096 < 2^16).  Then the
//           256 / C lanes of a column each sum their 256 / (256 / C) = C bins, and the lane whose bins hold the rank
//           walks them.  Pass 1 counts every key, later passes only the few that match          [8 reads, <= 2+ adds]
//   mark    with lo, hi, n_lo, n_hi known, lane (c, s) counts the keys EQUAL to lo and to hi in its rows; a prefix
//           over s gives the arrival-order rank of its first tie, so the kept rule is evaluated for every row in
//           parallel and exactly as the sequential walk would.  A dropped element becomes -0.0f, a kept one its
//           float again; a drop adds 1 to its row's LDS counter                              [2 reads, 1 write]
//   chain   lane c < C adds column c's K words in arrival order, starting from -0.0f.  -0.0f + v has the bits of v
//           for every v (round to nearest, denormals kept), so this IS "the first kept value, then + every later
//           kept one": K dependent adds and nothing else on the only sequential path             [1 read]
//   write   out (and mirror) = chain / float(K - 2t).
// 12 reads, 1.25 writes and about 3 integer adds per element and round; a 32-step bisection would be ~34 reads.
//
// Banks.  R = ceil(K / (256 / C)) made odd.  The 64 lanes of a wave hold 64 / C consecutive slices s; slice s starts
// s R C words in, and with R odd s R C mod 64 takes 64 / C distinct multiples of C: the wave's 64 addresses fall
// into 64 distinct banks in every scan, without padding.  (At C = 64 a wave is one row segment.)
//
// Registers: no per-column buffers; the compiler's counts and that neither instantiation uses scratch are in
// DESIGN.md.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/feddeeptrim.h"
#include "fa_device.h"
#include "fa_common.h"

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int FDT_LANES = 256;
constexpr int FDT_U = 8;                 // float4 loads a lane has in flight
constexpr int FDT_WORDS_SMALL = 20480;   // 80 KiB: two workgroups per CU
constexpr int FDT_WORDS_BIG = 26624;     // 104 KiB: one workgroup per CU (K > 3280)

constexpr int64_t lds_words(int64_t K, int64_t C) { return K * C + 128 * C + 256 + 8 * C + 2 * K; }
static_assert(lds_words(FDT_MAX_ROWS, 4) <= FDT_WORDS_BIG, "the largest round fits the large instantiation");
static_assert(2 * FDT_WORDS_SMALL * 4 <= 160 * 1024 && FDT_WORDS_BIG * 4 <= 160 * 1024, "gfx950: 160 KiB per CU");

struct DeepGeo {
  int cl;         // log2 C
  int S, R;       // lanes per column, rows per lane
  int64_t words;  // LDS words of the workgroup
  int wgs;        // workgroups per CU
};

DeepGeo geo_of(int K) {
  int cl = 6;
  while (cl > 2 && lds_words(K, 1 << cl) > FDT_WORDS_SMALL) --cl;
  DeepGeo g;
  g.cl = cl;
  g.S = FDT_LANES >> cl;
  g.R = ((K + g.S - 1) / g.S) | 1;
  g.words = lds_words(K, 1 << cl);
  g.wgs = g.words <= FDT_WORDS_SMALL ? 2 : 1;
  return g;
}

struct DeepArgs {
  const f4* x;     // the rows, in float4 columns
  int64_t ld4;     // row stride in float4 columns
  int64_t P4;      // float4 columns to read, ceil(P / 4)
  int64_t P;       // columns to write
  int64_t ntiles;  // workgroup b takes tiles b, b + grid, ...
  int K, t, cl, R;
  float denom;     // float(K - 2t)
  float* out;
  float* mirror;
  unsigned long long* dropped;  // [K][2] or NULL
};

__device__ __forceinline__ uint32_t key_of(float v) {
  const uint32_t b = __float_as_uint(v);
  const uint32_t k = (b >> 31) ? ~b : (b | 0x80000000u);
  return v != v ? 0xFFFFFFFFu : k;
}
// the float of a key; every NaN comes back as 0x7FFFFFFF (which NaN is not part of the contract)
__device__ __forceinline__ uint32_t bits_of(uint32_t key) { return (key >> 31) ? (key & 0x7FFFFFFFu) : ~key; }

// Column state in LDS, 8 arrays of C words: the select's prefix, remaining rank, keys below, keys in the final bin;
// then lo, hi, n_lo, n_hi.
enum { CS_PREFIX = 0, CS_RANK, CS_BELOW, CS_EQ, CS_LO, CS_HI, CS_NLO, CS_NHI };

// cs[CS_PREFIX][c] <- the key of ascending rank `rank` (0-based) of column c, cs[CS_BELOW][c] <- how many keys are
// smaller, cs[CS_EQ][c] <- how many are equal.  Every lane of the workgroup calls it; it ends on a barrier.
__device__ __forceinline__ void radix_select(const uint32_t* tile, uint32_t* hist, uint32_t* part, uint32_t* cs,
                                             int cl, int c, int s, int k0, int k1, int tid, uint32_t rank) {
  const int C = 1 << cl, S = FDT_LANES >> cl, W = C >> 1;  // W: histogram words (2 bins each) of one lane
  if (tid < C) {
    cs[CS_PREFIX * C + tid] = 0u;
    cs[CS_RANK * C + tid] = rank;
    cs[CS_BELOW * C + tid] = 0u;
  }
  uint32_t* h = hist + c * 128 + s * W;  // this lane's bins: digits [s C, s C + C)
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < 128 * C; i += FDT_LANES) hist[i] = 0u;
    __syncthreads();
    const uint32_t prefix = cs[CS_PREFIX * C + c];
    const uint32_t rk = cs[CS_RANK * C + c];
    for (int k = k0; k < k1; ++k) {
      const uint32_t key = tile[(k << cl) + c];
      const bool match = pass == 0 || (key >> (shift + 8)) == prefix;
      if (match) {
        const uint32_t d = (key >> shift) & 255u;
        atomicAdd(&hist[c * 128 + (d >> 1)], 1u << ((d & 1u) * 16u));
      }
    }
    __syncthreads();
    uint32_t sum = 0;
    for (int j = 0; j < W; ++j) {
      const uint32_t w = h[j];
      sum += (w & 0xFFFFu) + (w >> 16);
    }
    part[c * S + s] = sum;
    __syncthreads();
    uint32_t before = 0;
    for (int s2 = 0; s2 < s; ++s2) before += part[c * S + s2];
    if (rk >= before && rk < before + sum) {  // exactly one lane of the column: the matching keys number > rk
      uint32_t cum = before, d = 0, eq = 0;
      bool found = false;
      for (int j = 0; j < W; ++j) {
        const uint32_t w = h[j];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const uint32_t n = half ? (w >> 16) : (w & 0xFFFFu);
          if (!found && rk < cum + n) {
            found = true;
            d = (uint32_t)(s * C + 2 * j + half);
            eq = n;
          }
          if (!found) cum += n;
        }
      }
      cs[CS_PREFIX * C + c] = (prefix << 8) | d;
      cs[CS_RANK * C + c] = rk - cum;
      cs[CS_BELOW * C + c] += cum;  // keys of smaller digits under the same prefix
      cs[CS_EQ * C + c] = eq;
    }
    __syncthreads();
  }
}

template <int WORDS>
__global__ __launch_bounds__(FDT_LANES) void k_deep_trim(DeepArgs r) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[WORDS];
  const int tid = threadIdx.x;
  const int K = r.K, cl = r.cl, C = 1 << cl, S = FDT_LANES >> cl;
  uint32_t* tile = lds;            // [K][C]
  uint32_t* hist = tile + K * C;   // [C][128]
  uint32_t* part = hist + 128 * C; // [C][S]
  uint32_t* cs = part + 256;       // [8][C]
  uint32_t* cnt = cs + 8 * C;      // [K][2]
  const int c = tid & (C - 1), s = tid >> cl;
  const int k0 = s * r.R < K ? s * r.R : K;
  const int k1 = k0 + r.R < K ? k0 + r.R : K;
  const bool counting = r.dropped != nullptr;
  if (counting)
    for (int i = tid; i < 2 * K; i += FDT_LANES) cnt[i] = 0u;  // (the barriers of the first tile come before its use)
  const int cl4 = cl - 2;   // a row of the tile is 2^cl4 float4 columns
  const int n4 = K << cl4;  // float4 words of the tile
  const f4 z4 = f4{0.f, 0.f, 0.f, 0.f};

  for (int64_t tl = blockIdx.x; tl < r.ntiles; tl += gridDim.x) {
    // ---- load: float4 word i of the tile is row i >> cl4, float4 column (tl << cl4) + (i & mask) --------------
    const int64_t col4 = tl << cl4;
    for (int base = tid; base < n4; base += FDT_LANES * FDT_U) {
      f4 v[FDT_U];
#pragma unroll
      for (int u = 0; u < FDT_U; ++u) {
        const int i = base + FDT_LANES * u;
        const int64_t j = col4 + (i & ((1 << cl4) - 1));
        const bool ok = i < n4 && j < r.P4;
        v[u] = ok ? __builtin_nontemporal_load(r.x + (int64_t)(i >> cl4) * r.ld4 + j) : z4;
      }
#pragma unroll
      for (int u = 0; u < FDT_U; ++u) {
        const int i = base + FDT_LANES * u;
        if (i < n4)
          *reinterpret_cast<u4*>(tile + 4 * i) = u4{key_of(v[u][0]), key_of(v[u][1]), key_of(v[u][2]), key_of(v[u][3])};
      }
    }
    __syncthreads();

    // ---- select: lo = rank t - 1, hi = rank K - t ----------------------------------------------------------------
    radix_select(tile, hist, part, cs, cl, c, s, k0, k1, tid, (uint32_t)(r.t - 1));
    if (tid < C) {
      cs[CS_LO * C + tid] = cs[CS_PREFIX * C + tid];
      cs[CS_NLO * C + tid] = (uint32_t)r.t - cs[CS_BELOW * C + tid];
    }
    radix_select(tile, hist, part, cs, cl, c, s, k0, k1, tid, (uint32_t)(K - r.t));
    if (tid < C) {
      const uint32_t above = (uint32_t)K - cs[CS_BELOW * C + tid] - cs[CS_EQ * C + tid];
      cs[CS_HI * C + tid] = cs[CS_PREFIX * C + tid];
      cs[CS_NHI * C + tid] = (uint32_t)r.t - above;
    }
    __syncthreads();

    // ---- mark: the kept rule with exact arrival-order tie ranks --------------------------------------------------
    const uint32_t lo = cs[CS_LO * C + c], hi = cs[CS_HI * C + c];
    const uint32_t nlo = cs[CS_NLO * C + c], nhi = cs[CS_NHI * C + c];
    uint32_t elo = 0, ehi = 0;
    for (int k = k0; k < k1; ++k) {
      const uint32_t key = tile[(k << cl) + c];
      elo += key == lo ? 1u : 0u;
      ehi += key == hi ? 1u : 0u;
    }
    part[c * S + s] = elo | (ehi << 16);
    __syncthreads();
    uint32_t bl = 0, bh = 0;  // rows before this lane's, in arrival order, equal to lo / to hi
    for (int s2 = 0; s2 < s; ++s2) {
      const uint32_t w = part[c * S + s2];
      bl += w & 0xFFFFu;
      bh += w >> 16;
    }
    // lo == hi: the column's j-th such row is dropped low for j < n_lo and high for n_lo <= j < n_lo + n_hi
    const uint32_t skip = lo == hi ? nlo : 0u;
    const bool live = (tl << cl) + c < r.P;  // a column at or past P: nothing of it is counted or stored
    for (int k = k0; k < k1; ++k) {
      const uint32_t key = tile[(k << cl) + c];
      const bool eql = key == lo, eqh = key == hi;
      const bool low = key < lo || (eql && bl < nlo);
      const bool high = !low && (key > hi || (eqh && bh - skip < nhi));
      bl += eql ? 1u : 0u;
      bh += eqh ? 1u : 0u;
      tile[(k << cl) + c] = (low || high) ? 0x80000000u : bits_of(key);
      if (counting && live) {  // integer counts: any order of adds gives the same values
        if (low) atomicAdd(&cnt[2 * k], 1u);
        if (high) atomicAdd(&cnt[2 * k + 1], 1u);
      }
    }
    __syncthreads();

    // ---- chain and write: one lane per column, rows in arrival order --------------------------------------------
    if (tid < C && live) {
      float chain = -0.0f;
#pragma unroll 8
      for (int k = 0; k < K; ++k) chain = chain + __uint_as_float(tile[(k << cl) + tid]);
      const float m = __fdiv_rn(chain, r.denom);
      const int64_t p = (tl << cl) + tid;
      r.out[p] = m;
      if (r.mirror) r.mirror[p] = m;
    }
    __syncthreads();  // the next tile's load overwrites the tile
  }
  if (counting) {
    for (int i = tid; i < 2 * K; i += FDT_LANES) {
      const uint32_t n = cnt[i];
      if (n) atomicAdd(&r.dropped[i], (unsigned long long)n);
    }
  }
}

// what both entry points refuse of (K, P, t); 0 when the triple is fine
int check_sizes(const char* who, int32_t K, int64_t P, int32_t t) {
  if (K < 0 || P < 0) return refuse(FA_E_ARG, "%s: negative K=%d or P=%lld", who, K, (long long)P);
  if (t < 1) return refuse(FA_E_ARG, "%s: t=%d, needs t >= 1 (t = 0 is plain FedAvg: ft_reduce)", who, t);
  if (2 * (int64_t)t >= K) return refuse(FA_E_ARG, "%s: t=%d needs 2t < K=%d", who, t, K);
  if (K > FDT_MAX_ROWS) return refuse(FA_E_ARG, "%s: K=%d exceeds fdt_max_rows()=%d", who, K, FDT_MAX_ROWS);
  return 0;
}

int64_t grid_of(int64_t cus, int64_t tiles, const DeepGeo& g) {
  const int64_t cap = cus * g.wgs;
  return tiles < cap ? tiles : cap;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/feddeeptrim.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t fdt_abi_version(void) { return FDT_ABI_VERSION; }

extern "C" int32_t fdt_max_rows(void) { return FDT_MAX_ROWS; }

extern "C" int fdt_plan(int32_t cus, int32_t K, int64_t P, int32_t t, int64_t* plan_out) {
  if (cus <= 0 || !plan_out) return refuse(FA_E_ARG, "fdt_plan: bad arguments (cus=%d)", cus);
  if (const int e = check_sizes("fdt_plan", K, P, t)) return e;
  const DeepGeo g = geo_of(K);
  const int64_t C = 1 << g.cl, tiles = (P + C - 1) / C;
  plan_out[0] = C;
  plan_out[1] = g.S;
  plan_out[2] = g.R;
  plan_out[3] = g.words * 4;
  plan_out[4] = tiles;
  plan_out[5] = grid_of(cus, tiles, g);
  plan_out[6] = g.wgs;
  return FA_OK;
}

extern "C" int fdt_reduce(const float* x, int64_t ld, int32_t K, int64_t P, int32_t t, float* out, float* mirror,
                          int64_t* dropped, int32_t cus, fa_stream_t stream) {
  if (const int e = check_sizes("fdt_reduce", K, P, t)) return e;
  if (cus < 0) return refuse(FA_E_ARG, "fdt_reduce: negative cus=%d", cus);
  if (ld < P) return refuse(FA_E_ARG, "fdt_reduce: ld=%lld < P=%lld", (long long)ld, (long long)P);
  if (ld % 4 != 0) return refuse(FA_E_ARG, "fdt_reduce: ld=%lld must be a multiple of 4 elements", (long long)ld);
  if (!x) return refuse(FA_E_ARG, "fdt_reduce: x is NULL");
  if (!aligned16(x)) return refuse(FA_E_ARG, "fdt_reduce: x must be 16-byte aligned");
  if (!out) return refuse(FA_E_ARG, "fdt_reduce: out is NULL");
  if (!aligned16(out) || !aligned16(mirror))
    return refuse(FA_E_ARG, "fdt_reduce: out and mirror must be 16-byte aligned");
  if ((uintptr_t)dropped & 7u) return refuse(FA_E_ARG, "fdt_reduce: dropped must be 8-byte aligned");
  if (P == 0) return FA_OK;
  const int64_t P4 = (P + 3) / 4;
  FA_DEVICE_SCOPE("fdt_reduce", stream, out);
  FA_OPERAND("x", x, (uint64_t)((int64_t)(K - 1) * ld + P4 * 4) * 4);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  FA_HOST_OK_OPERAND("mirror", mirror, (uint64_t)P * 4);
  FA_OPERAND("dropped", dropped, (uint64_t)K * 16);
  if (cus == 0) cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fdt_reduce launch plan: no CU count for device %d", fa_scope_device());
  const DeepGeo g = geo_of(K);
  const int64_t C = 1 << g.cl;
  DeepArgs r{};
  r.x = reinterpret_cast<const f4*>(x); r.ld4 = ld / 4; r.P4 = P4; r.P = P;
  r.ntiles = (P + C - 1) / C;
  r.K = K; r.t = t; r.cl = g.cl; r.R = g.R;
  r.denom = (float)(K - 2 * t);
  r.out = out; r.mirror = mirror;
  r.dropped = reinterpret_cast<unsigned long long*>(dropped);
  const dim3 grid((unsigned)grid_of(cus, r.ntiles, g)), blk(FDT_LANES);
  if (g.wgs == 2)
    hipLaunchKernelGGL((k_deep_trim<FDT_WORDS_SMALL>), grid, blk, 0, (hipStream_t)stream, r);
  else
    hipLaunchKernelGGL((k_deep_trim<FDT_WORDS_BIG>), grid, blk, 0, (hipStream_t)stream, r);
  return check_launch("fdt_reduce");
}
