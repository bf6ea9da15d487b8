// trim_reduce.hip — MI355X (gfx950) kernels of the coordinate-wise trimmed mean (include/fedtrim.h):
//   * ft_select: per column the t-th smallest and t-th largest order key of the K staged rows, and how many rows
//                equal to each are dropped (k_trim_select);
//   * ft_reduce: the in-order fp32 chain of the kept rows, the division, the optional mirror and the per-row drop
//                counts, in one kernel (k_trim_reduce);
//   * ft_plan:   the launches both make, as a host-only function of the CU count.
//
// Numerics: every fp32 op is rounded to nearest and never contracted into an FMA; the default denormal modes are
// kept; the division is the IEEE one.  The selection is integer arithmetic on the order keys.
//
// Sentinels.  A column's T smallest keys start as 0xFFFFFFFF and its T largest as 0.  Key 0 never occurs, so the
// low sentinel of the `largest` buffer is below every real key and is pushed out by the first T rows.  The high
// sentinel EQUALS the key of a NaN; that is safe because only slot t - 1 <= T - 1 and the slots before it are read,
// after K > 2t >= t + 1 rows went in: those slots hold the t smallest real keys, and a 0xFFFFFFFF among them is a
// real NaN's key (there are then fewer than t non-NaN rows) — a sentinel and a NaN's key are the same number, and
// only the number is used.
//
// Registers, per lane (a lane owns 4V columns: V float4 loads per row, U rows loaded ahead):
//   k_trim_select<T, V, U>   buffers 2 * T * 4V, loads 4UV, plus ~20 of addresses and masks
//     T = 1   V = 4,2,1  U = 2,4,8     32 + 32 at level 0
//     T = 2   V = 4,2,1  U = 2,4,8     64 + 32
//     T = 4   V = 4,2,1  U = 2,4,8    128 + 32: 2 waves per SIMD at level 0, which the grid cap of 2 workgroups
//                                      per CU asks for; levels 1 and 2 (64 + 32, 32 + 32) hold more
//     T = 8   V = 1      U = 4         64 + 16
//     T = 16  V = 1      U = 4        128 + 16: 3 waves per SIMD (<= 168 allocated), the grid cap of 3 workgroups
//                                      per CU; wider tiles at T >= 8 would leave one wave per SIMD on a kernel
//                                      that is bound by its integer min / max chain (4 T operations per element)
//   k_trim_reduce<V, U, TRIM> lo, hi, ties, chain per column: 16V, loads 4UV; V = 4,2,1  U = 2,4,8: 64 + 32
// The compiler's counts per instantiation (it spends spare registers on keys computed ahead: 60 to 180 for the
// selection, 63 to 118 for the reduce), and that none uses scratch, are in DESIGN.md §4.
//
// Both kernels skip their per-element rule where a whole wave agrees that it cannot change anything: the selection
// when no lane's key enters a buffer (T >= 4), the reduce when every lane's key lies strictly between its lo and hi.
// The reduce without its skip took 29.9 ms at 1000 x 25 M for every t, with it 18.4 ms at t = 1.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fedtrim.h"
#include "fa_device.h"
#include "fa_common.h"

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int FT_WAVES = 4;  // waves per workgroup, each owning V strips of a tile
// T <= 4 and the reduce: three tile widths; the cap is 2 workgroups (8 waves) per CU
constexpr StripGeo FT_GEO_NARROW{FT_WAVES, {4, 2, 1}, {2, 4, 8}, 200, 256};
// T >= 8: one strip per wave at every level (the levels differ in their grids only); 3 workgroups per CU
constexpr StripGeo FT_GEO_DEEP{FT_WAVES, {1, 1, 1}, {4, 4, 4}, 300, 256};
constexpr int FT_LDS_ROWS = 4096;  // rows whose drop counts a workgroup gathers in LDS (at most 32 KiB)

constexpr int depth_of(int t) { return t <= 1 ? 1 : t <= 2 ? 2 : t <= 4 ? 4 : t <= 8 ? 8 : 16; }
constexpr const StripGeo& select_geo(int T) { return T >= 8 ? FT_GEO_DEEP : FT_GEO_NARROW; }

__device__ __forceinline__ uint32_t key_of(float v) {
  const uint32_t b = __float_as_uint(v);
  const uint32_t k = (b >> 31) ? ~b : (b | 0x80000000u);
  return v != v ? 0xFFFFFFFFu : k;
}
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

struct TrimArgs {
  const f4* x;      // the rows, in float4 columns
  int64_t ld4;      // row stride in float4 columns
  int64_t P4;       // float4 columns to read, ceil(P / 4)
  int64_t P;        // columns to write
  int64_t c0;       // first float4 column of this launch
  int64_t ntiles;   // tiles of this launch; workgroup b takes tiles b, b + grid, ...
  int K, t;
  uint32_t* lo;     // select: written; reduce: read
  uint32_t* hi;
  uint32_t* ties;
  float denom;      // float(K - 2t)
  float* out;
  float* mirror;
  unsigned long long* dropped;  // [K][2] or NULL
  int lds_rows;     // K when the counts are gathered in LDS, 0 when they go straight to `dropped`
};

// ------------------------------------------------------------------------------------------------
// k_trim_select
// ------------------------------------------------------------------------------------------------
// One column's two buffers: s[] ascending (the T smallest so far), h[] descending (the T largest).  Inserting x
// is a chain of min / max pairs that carries the displaced key along; a key that enters neither buffer leaves
// both as they were, so skipping the chain when no lane of the wave has such a key changes nothing.
template <int T>
__device__ __forceinline__ void insert(uint32_t (&s)[T], uint32_t (&h)[T], uint32_t key) {
  uint32_t a = key, b = key;
#pragma unroll
  for (int i = 0; i < T; ++i) {
    const uint32_t m = umin(s[i], a);
    a = umax(s[i], a);
    s[i] = m;
    const uint32_t M = umax(h[i], b);
    b = umin(h[i], b);
    h[i] = M;
  }
}

template <int T, int V>
__device__ __forceinline__ void select_row(uint32_t (&s)[V][4][T], uint32_t (&h)[V][4][T], const f4 (&v)[V]) {
#pragma unroll
  for (int j = 0; j < V; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t key = key_of(v[j][c]);
      if (T >= 4) {  // wave-uniform: the chain costs 4 T operations, the test 3
        const bool enters = key < s[j][c][T - 1] || key > h[j][c][T - 1];
        if (__builtin_amdgcn_ballot_w64(enters) == 0) continue;
      }
      insert<T>(s[j][c], h[j][c], key);
    }
}

template <int T, int V, int U>
__device__ __forceinline__ void select_tile(const TrimArgs& r, int64_t tile, int lane, int wave) {
  const int64_t c0 = r.c0 + (tile * FT_WAVES + wave) * (64LL * V) + lane;
  const f4 z4 = f4{0.f, 0.f, 0.f, 0.f};
  bool ok[V];
  uint32_t s[V][4][T], h[V][4][T];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    ok[j] = (c0 + 64 * j) < r.P4;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < T; ++i) {
        s[j][c][i] = 0xFFFFFFFFu;
        h[j][c][i] = 0u;
      }
  }
  const f4* row = r.x + c0;
  int k = 0;
  for (; k + U <= r.K; k += U) {
    f4 v[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) v[u][j] = ok[j] ? __builtin_nontemporal_load(row + u * r.ld4 + 64 * j) : z4;
#pragma unroll
    for (int u = 0; u < U; ++u) select_row<T, V>(s, h, v[u]);
    row += U * r.ld4;
  }
  for (; k < r.K; ++k) {
    f4 v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = ok[j] ? __builtin_nontemporal_load(row + 64 * j) : z4;
    select_row<T, V>(s, h, v);
    row += r.ld4;
  }
  const int t = r.t;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (!ok[j]) continue;
    uint32_t lo[4], hi[4], ties[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      uint32_t l = 0, g = 0;
#pragma unroll
      for (int i = 0; i < T; ++i) {  // slot t - 1, picked without indexing the registers
        l = (i == t - 1) ? s[j][c][i] : l;
        g = (i == t - 1) ? h[j][c][i] : g;
      }
      uint32_t below = 0, above = 0;
#pragma unroll
      for (int i = 0; i < T; ++i) {
        below += (i < t && s[j][c][i] < l) ? 1u : 0u;
        above += (i < t && h[j][c][i] > g) ? 1u : 0u;
      }
      lo[c] = l;
      hi[c] = g;
      ties[c] = ((uint32_t)t - below) | (((uint32_t)t - above) << 16);
    }
    const int64_t p = 4 * (c0 + 64 * j);
    if (p + 4 <= r.P) {
      *reinterpret_cast<u4*>(r.lo + p) = u4{lo[0], lo[1], lo[2], lo[3]};
      *reinterpret_cast<u4*>(r.hi + p) = u4{hi[0], hi[1], hi[2], hi[3]};
      *reinterpret_cast<u4*>(r.ties + p) = u4{ties[0], ties[1], ties[2], ties[3]};
    } else {  // the last, partial float4 column: columns >= P are not written
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (p + c < r.P) {
          r.lo[p + c] = lo[c];
          r.hi[p + c] = hi[c];
          r.ties[p + c] = ties[c];
        }
    }
  }
}

// workgroup b selects over tiles b, b + grid, ... (one tile each unless the grid is capped)
template <int T, int V, int U>
__global__ __launch_bounds__(64 * FT_WAVES) void k_trim_select(TrimArgs r) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  for (int64_t tile = blockIdx.x; tile < r.ntiles; tile += gridDim.x) select_tile<T, V, U>(r, tile, lane, wave);
}

// ------------------------------------------------------------------------------------------------
// k_trim_reduce
// ------------------------------------------------------------------------------------------------
// A column's state: lo, hi, the two tie counters in one register as ft_select packs them (n_lo in the low half,
// n_hi in the high), the chain, and whether the chain has started.  cl / ch: this lane's drops of the row.
struct ColState {
  uint32_t lo, hi, ties;
  float chain;
  bool started;
};

template <bool TRIM>
__device__ __forceinline__ void reduce_one(ColState& q, float v, uint32_t& cl, uint32_t& ch) {
  bool keep = true;
  if (TRIM) {
    const uint32_t key = key_of(v);
    // wave-uniform: a value strictly between lo and hi is kept and moves no counter, so when that holds in every
    // lane the rule below is skipped — the same result for a third of the operations
    const bool edge = key <= q.lo || key >= q.hi;
    if (__builtin_amdgcn_ballot_w64(edge) != 0) {
      const bool tie_lo = key == q.lo && (q.ties & 0xFFFFu) != 0;
      const bool low = key < q.lo || tie_lo;
      const bool tie_hi = !low && key == q.hi && (q.ties >> 16) != 0;
      const bool high = !low && (key > q.hi || tie_hi);
      q.ties -= (tie_lo ? 1u : 0u) + (tie_hi ? 0x10000u : 0u);
      cl += low ? 1u : 0u;
      ch += high ? 1u : 0u;
      keep = !low && !high;
    }
  }
  const float sum = q.chain + v;
  q.chain = keep ? (q.started ? sum : v) : q.chain;
  q.started = q.started || keep;
}

template <int V, bool TRIM>
__device__ __forceinline__ void reduce_row(const TrimArgs& r, ColState (&q)[V][4], const f4 (&v)[V], int k,
                                           uint32_t* lds) {
  uint32_t cl = 0, ch = 0;
#pragma unroll
  for (int j = 0; j < V; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) reduce_one<TRIM>(q[j][c], v[j][c], cl, ch);
  if (TRIM && r.dropped) {  // integer counts: any order of adds gives the same values
    if (r.lds_rows) {
      if (cl) atomicAdd(&lds[2 * k], cl);
      if (ch) atomicAdd(&lds[2 * k + 1], ch);
    } else {
      if (cl) atomicAdd(&r.dropped[2 * (int64_t)k], (unsigned long long)cl);
      if (ch) atomicAdd(&r.dropped[2 * (int64_t)k + 1], (unsigned long long)ch);
    }
  }
}

template <int V, int U, bool TRIM>
__device__ __forceinline__ void reduce_tile(const TrimArgs& r, int64_t tile, int lane, int wave, uint32_t* lds) {
  const int64_t c0 = r.c0 + (tile * FT_WAVES + wave) * (64LL * V) + lane;
  const f4 z4 = f4{0.f, 0.f, 0.f, 0.f};
  bool ok[V];
  ColState q[V][4];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    ok[j] = (c0 + 64 * j) < r.P4;
    u4 lo = u4{0u, 0u, 0u, 0u}, hi = u4{~0u, ~0u, ~0u, ~0u}, ties = u4{0u, 0u, 0u, 0u};
    if (TRIM && ok[j]) {
      lo = *reinterpret_cast<const u4*>(r.lo + 4 * (c0 + 64 * j));
      hi = *reinterpret_cast<const u4*>(r.hi + 4 * (c0 + 64 * j));
      ties = *reinterpret_cast<const u4*>(r.ties + 4 * (c0 + 64 * j));
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      // a column at or past P keeps every row: nothing of it is counted (and nothing of it is stored)
      const bool live = ok[j] && 4 * (c0 + 64 * j) + c < r.P;
      q[j][c] = ColState{live ? lo[c] : 0u, live ? hi[c] : ~0u, live ? ties[c] : 0u, 0.0f, false};
    }
  }
  const f4* row = r.x + c0;
  int k = 0;
  for (; k + U <= r.K; k += U) {
    f4 v[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) v[u][j] = ok[j] ? __builtin_nontemporal_load(row + u * r.ld4 + 64 * j) : z4;
#pragma unroll
    for (int u = 0; u < U; ++u) reduce_row<V, TRIM>(r, q, v[u], k + u, lds);
    row += U * r.ld4;
  }
  for (; k < r.K; ++k) {
    f4 v[V];
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = ok[j] ? __builtin_nontemporal_load(row + 64 * j) : z4;
    reduce_row<V, TRIM>(r, q, v, k, lds);
    row += r.ld4;
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (!ok[j]) continue;
    float m[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) m[c] = __fdiv_rn(q[j][c].chain, r.denom);
    const int64_t p = 4 * (c0 + 64 * j);
    if (p + 4 <= r.P) {
      const f4 o = f4{m[0], m[1], m[2], m[3]};
      *reinterpret_cast<f4*>(r.out + p) = o;
      if (r.mirror) *reinterpret_cast<f4*>(r.mirror + p) = o;
    } else {  // the last, partial float4 column: columns >= P are not written
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (p + c < r.P) {
          r.out[p + c] = m[c];
          if (r.mirror) r.mirror[p + c] = m[c];
        }
    }
  }
}

template <int V, int U, bool TRIM>
__global__ __launch_bounds__(64 * FT_WAVES) void k_trim_reduce(TrimArgs r) {
  extern __shared__ uint32_t lds[];  // [lds_rows][2] drop counts of this workgroup
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const bool counting = TRIM && r.dropped && r.lds_rows;
  if (counting) {
    for (int i = threadIdx.x; i < 2 * r.lds_rows; i += 64 * FT_WAVES) lds[i] = 0u;
    __syncthreads();
  }
  for (int64_t tile = blockIdx.x; tile < r.ntiles; tile += gridDim.x) reduce_tile<V, U, TRIM>(r, tile, lane, wave, lds);
  if (counting) {
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * r.lds_rows; i += 64 * FT_WAVES) {
      const uint32_t n = lds[i];
      if (n) atomicAdd(&r.dropped[i], (unsigned long long)n);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------------
int64_t trim_strips(int64_t P) { return ((P + 3) / 4 + 63) / 64; }

void place(TrimArgs& r, const StripLaunch& l) {
  r.c0 = l.strip0 * 64;
  r.ntiles = l.tiles;
}

template <int T>
void launch_select(TrimArgs r, const StripLaunch& l, hipStream_t st) {
  place(r, l);
  const dim3 grid((unsigned)l.grid), blk(64 * FT_WAVES);
  if constexpr (T >= 8) {
    hipLaunchKernelGGL((k_trim_select<T, 1, 4>), grid, blk, 0, st, r);
  } else {
    if (l.level == 0)
      hipLaunchKernelGGL((k_trim_select<T, 4, 2>), grid, blk, 0, st, r);
    else if (l.level == 1)
      hipLaunchKernelGGL((k_trim_select<T, 2, 4>), grid, blk, 0, st, r);
    else
      hipLaunchKernelGGL((k_trim_select<T, 1, 8>), grid, blk, 0, st, r);
  }
}

template <bool TRIM>
void launch_reduce(TrimArgs r, const StripLaunch& l, hipStream_t st) {
  place(r, l);
  const dim3 grid((unsigned)l.grid), blk(64 * FT_WAVES);
  const size_t lds = (TRIM && r.dropped) ? (size_t)r.lds_rows * 8 : 0;
  if (l.level == 0)
    hipLaunchKernelGGL((k_trim_reduce<4, 2, TRIM>), grid, blk, lds, st, r);
  else if (l.level == 1)
    hipLaunchKernelGGL((k_trim_reduce<2, 4, TRIM>), grid, blk, lds, st, r);
  else
    hipLaunchKernelGGL((k_trim_reduce<1, 8, TRIM>), grid, blk, lds, st, r);
}

static_assert(FT_GEO_NARROW.V[0] == 4 && FT_GEO_NARROW.U[0] == 2 && FT_GEO_NARROW.V[1] == 2 &&
                  FT_GEO_NARROW.U[1] == 4 && FT_GEO_NARROW.V[2] == 1 && FT_GEO_NARROW.U[2] == 8 &&
                  FT_GEO_DEEP.V[0] == 1 && FT_GEO_DEEP.U[0] == 4,
              "the launchers above name the geometries' (V, U) pairs");
static_assert(depth_of(FT_MAX_TRIM) == FT_MAX_TRIM, "the deepest instantiation is FT_MAX_TRIM");

// what every entry point refuses of (K, P, t); 0 when the triple is fine
int check_sizes(const char* who, int32_t K, int64_t P, int32_t t) {
  if (K < 0 || P < 0 || t < 0) return refuse(FA_E_ARG, "%s: negative K=%d, P=%lld or t=%d", who, K, (long long)P, t);
  if (2 * (int64_t)t >= K) return refuse(FA_E_ARG, "%s: t=%d needs 2t < K=%d", who, t, K);
  if (t > FT_MAX_TRIM) return refuse(FA_E_ARG, "%s: t=%d exceeds ft_max_trim()=%d", who, t, FT_MAX_TRIM);
  return 0;
}

int check_rows(const char* who, const float* x, int64_t ld, int64_t P) {
  if (ld < P) return refuse(FA_E_ARG, "%s: ld=%lld < P=%lld", who, (long long)ld, (long long)P);
  if (ld % 4 != 0) return refuse(FA_E_ARG, "%s: ld=%lld must be a multiple of 4 elements", who, (long long)ld);
  if (!x) return refuse(FA_E_ARG, "%s: x is NULL", who);
  if (!aligned16(x)) return refuse(FA_E_ARG, "%s: x must be 16-byte aligned", who);
  if (((P + 3) / 4) / (64 * FT_WAVES) > 0x7fffffffLL) return refuse(FA_E_RANGE, "%s: P too large", who);
  return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedtrim.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t ft_abi_version(void) { return FT_ABI_VERSION; }

extern "C" int32_t ft_max_trim(void) { return FT_MAX_TRIM; }

extern "C" int64_t ft_plan(int32_t cus, int32_t K, int64_t P, int32_t t, int64_t* plan_out, int32_t cap) {
  if (cus <= 0 || cap < 0 || (cap > 0 && !plan_out))
    return refuse(FA_E_ARG, "ft_plan: bad arguments (cus=%d cap=%d)", cus, cap);
  if (const int e = check_sizes("ft_plan", K, P, t)) return e;
  int n = 0;
  StripLaunch l[3];
  for (int kernel = t > 0 ? FT_KERNEL_SELECT : FT_KERNEL_REDUCE; kernel <= FT_KERNEL_REDUCE; ++kernel) {
    const int T = kernel == FT_KERNEL_SELECT ? depth_of(t) : 0;
    const StripGeo& g = kernel == FT_KERNEL_SELECT ? select_geo(T) : FT_GEO_NARROW;
    const int nl = strip_plan(cus, trim_strips(P), g, l);
    for (int i = 0; i < nl; ++i, ++n) {
      if (n >= cap) continue;
      int64_t* o = plan_out + (int64_t)FT_PLAN_FIELDS * n;
      o[0] = kernel;
      o[1] = T;
      o[2] = g.V[l[i].level];
      o[3] = g.U[l[i].level];
      o[4] = l[i].strip0 * g.strip_cols;
      o[5] = l[i].tiles;
      o[6] = l[i].grid;
    }
  }
  return n;
}

extern "C" int ft_select(const float* x, int64_t ld, int32_t K, int64_t P, int32_t t, uint32_t* lo, uint32_t* hi,
                         uint32_t* ties, fa_stream_t stream) {
  if (const int e = check_sizes("ft_select", K, P, t)) return e;
  if (t < 1) return refuse(FA_E_ARG, "ft_select: t=%d, needs t >= 1 (t = 0 has no thresholds)", t);
  if (const int e = check_rows("ft_select", x, ld, P)) return e;
  if (!lo || !hi || !ties) return refuse(FA_E_ARG, "ft_select: lo, hi or ties is NULL");
  if (!aligned16(lo) || !aligned16(hi) || !aligned16(ties))
    return refuse(FA_E_ARG, "ft_select: lo, hi and ties must be 16-byte aligned");
  if (P == 0) return FA_OK;
  const int64_t P4 = (P + 3) / 4;
  FA_DEVICE_SCOPE("ft_select", stream, lo);
  FA_OPERAND("x", x, (uint64_t)((int64_t)(K - 1) * ld + P4 * 4) * 4);
  FA_OPERAND("lo", lo, (uint64_t)P * 4);
  FA_OPERAND("hi", hi, (uint64_t)P * 4);
  FA_OPERAND("ties", ties, (uint64_t)P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "ft_select launch plan: no CU count for device %d", fa_scope_device());
  TrimArgs r{};
  r.x = reinterpret_cast<const f4*>(x); r.ld4 = ld / 4; r.P4 = P4; r.P = P; r.K = K; r.t = t;
  r.lo = lo; r.hi = hi; r.ties = ties;
  const int T = depth_of(t);
  StripLaunch l[3];
  const int nl = strip_plan(cus, trim_strips(P), select_geo(T), l);
  for (int i = 0; i < nl; ++i) {
    hipStream_t st = (hipStream_t)stream;
    switch (T) {
      case 1: launch_select<1>(r, l[i], st); break;
      case 2: launch_select<2>(r, l[i], st); break;
      case 4: launch_select<4>(r, l[i], st); break;
      case 8: launch_select<8>(r, l[i], st); break;
      default: launch_select<16>(r, l[i], st); break;
    }
    const int e = check_launch("ft_select");
    if (e) return e;
  }
  return FA_OK;
}

extern "C" int ft_reduce(const float* x, int64_t ld, int32_t K, int64_t P, int32_t t, const uint32_t* lo,
                         const uint32_t* hi, const uint32_t* ties, float* out, float* mirror, int64_t* dropped,
                         fa_stream_t stream) {
  if (const int e = check_sizes("ft_reduce", K, P, t)) return e;
  if (const int e = check_rows("ft_reduce", x, ld, P)) return e;
  if (t == 0 && (lo || hi || ties))
    return refuse(FA_E_ARG, "ft_reduce: t=0 takes no thresholds: lo, hi and ties must be NULL");
  if (t > 0 && (!lo || !hi || !ties)) return refuse(FA_E_ARG, "ft_reduce: lo, hi or ties is NULL with t=%d", t);
  if (!aligned16(lo) || !aligned16(hi) || !aligned16(ties))
    return refuse(FA_E_ARG, "ft_reduce: lo, hi and ties must be 16-byte aligned");
  if (!out) return refuse(FA_E_ARG, "ft_reduce: out is NULL");
  if (!aligned16(out) || !aligned16(mirror))
    return refuse(FA_E_ARG, "ft_reduce: out and mirror must be 16-byte aligned");
  if ((uintptr_t)dropped & 7u) return refuse(FA_E_ARG, "ft_reduce: dropped must be 8-byte aligned");
  if (P == 0) return FA_OK;
  const int64_t P4 = (P + 3) / 4;
  FA_DEVICE_SCOPE("ft_reduce", stream, out);
  FA_OPERAND("x", x, (uint64_t)((int64_t)(K - 1) * ld + P4 * 4) * 4);
  FA_OPERAND("lo", lo, (uint64_t)P4 * 16);
  FA_OPERAND("hi", hi, (uint64_t)P4 * 16);
  FA_OPERAND("ties", ties, (uint64_t)P4 * 16);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  FA_HOST_OK_OPERAND("mirror", mirror, (uint64_t)P * 4);
  FA_OPERAND("dropped", dropped, (uint64_t)K * 16);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "ft_reduce launch plan: no CU count for device %d", fa_scope_device());
  TrimArgs r{};
  r.x = reinterpret_cast<const f4*>(x); r.ld4 = ld / 4; r.P4 = P4; r.P = P; r.K = K; r.t = t;
  r.lo = const_cast<uint32_t*>(lo); r.hi = const_cast<uint32_t*>(hi); r.ties = const_cast<uint32_t*>(ties);
  r.denom = (float)(K - 2 * t);
  r.out = out; r.mirror = mirror;
  r.dropped = reinterpret_cast<unsigned long long*>(dropped);
  r.lds_rows = K <= FT_LDS_ROWS ? K : 0;
  StripLaunch l[3];
  const int nl = strip_plan(cus, trim_strips(P), FT_GEO_NARROW, l);
  for (int i = 0; i < nl; ++i) {
    if (t > 0)
      launch_reduce<true>(r, l[i], (hipStream_t)stream);
    else
      launch_reduce<false>(r, l[i], (hipStream_t)stream);
    const int e = check_launch("ft_reduce");
    if (e) return e;
  }
  return FA_OK;
}
