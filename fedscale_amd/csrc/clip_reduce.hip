// clip_reduce.hip — MI355X (gfx950) kernels of norm-clipped FedAvg (include/fedclip.h):
//   * fcl_row_sqnorms: per-client squared norms of (upload - starting model) in fp64, in a fixed add order;
//   * fcl_clip_coefs:  the clip coefficient of each client (clip_norm.py:57-60) and the count of rejected rows;
//   * fcl_reduce:      the in-order fp32 chain of the clipped updates, shaped like fh_reduce (reduce_half.hip);
//   * fcl_reduce_plan: the launches it makes, as a host-only function of the CU count;
//   * fcl_finish:      divide, optional Gaussian noise, re-base on the starting model.
//
// Numerics: every fp32 op is rounded to nearest and never contracted into an FMA; the default denormal modes are
// kept; divisions and the fp64 square root are the IEEE ones.  The only fused operation is the fp64 accumulation of
// an fp32 difference's square, whose product is exact in fp64 (fused and unfused adds give the same bits).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fedclip.h"
#include "fa_device.h"
#include "fa_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// fcl_row_sqnorms
// ------------------------------------------------------------------------------------------------
// Tile geometry (compile-time constants and P alone; only the grid depends on the CU count): a wave owns V strips of
// 64 float4 columns, keeps its tile of `last` in 4V registers and walks the rows with U rows' loads (4UV registers)
// issued ahead of their sums.  Per lane and row: the strips in order, x y z w within a float4, into one fp64
// accumulator; then the butterfly over the lanes.  Two geometries, chosen by P (profiles/clip_reduce_variants.log):
//   wide    P >= 4 Mi columns: 4 waves x V = 16, U = 2 (4096-column tiles) on 0.75 workgroups per CU, k_reduce's
//           shape — few concurrent column streams read fastest over long rows (1000 x 25 M: 14.9 against 16.4 ms)
//   narrow  shorter rows: 2 waves x V = 8, U = 4 (2048-column tiles) on up to 4 workgroups per CU — config 2 needs the
//           parallelism (100 x 1 M: 0.097 against 0.163 ms)
struct NormGeo {
  int V, U, waves, grid_pct;  // grid cap: workgroups per 100 CUs
};
constexpr NormGeo NQ_NARROW{8, 4, 2, 400};
constexpr NormGeo NQ_WIDE{16, 2, 4, 75};
constexpr int64_t NQ_WIDE_MIN_P = 4LL << 20;
constexpr NormGeo norm_geo(int64_t P) { return P >= NQ_WIDE_MIN_P ? NQ_WIDE : NQ_NARROW; }

struct NormArgs {
  const f4* x;      // the rows, in float4 columns
  int64_t ld4;      // row stride in float4 columns
  int64_t P4f;      // whole float4 columns, floor(P / 4): the <= 3 columns after them belong to the second launch
  int64_t tiles;    // wave tiles, ceil(P4f / (64 V))
  int n;
  const f4* last;
  double* ws;       // [n, tiles]
};

__device__ __forceinline__ double sq_acc(double acc, f4 t, f4 l) {
  const f4 d = t - l;
  acc = __builtin_fma((double)d.x, (double)d.x, acc);
  acc = __builtin_fma((double)d.y, (double)d.y, acc);
  acc = __builtin_fma((double)d.z, (double)d.z, acc);
  acc = __builtin_fma((double)d.w, (double)d.w, acc);
  return acc;
}

template <int NQ_V, int NQ_U, int NQ_WAVES>
__global__ __launch_bounds__(64 * NQ_WAVES) void k_row_sqnorm(NormArgs r) {
  constexpr int64_t NQ_TILE4 = 64 * NQ_V;  // float4 columns of one wave tile
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const f4 z4 = f4{0.f, 0.f, 0.f, 0.f};
  for (int64_t wt = (int64_t)blockIdx.x * NQ_WAVES + wave; wt < r.tiles; wt += (int64_t)gridDim.x * NQ_WAVES) {
    const int64_t c0 = wt * NQ_TILE4 + lane;
    bool ok[NQ_V];
    f4 l[NQ_V];
#pragma unroll
    for (int j = 0; j < NQ_V; ++j) {
      ok[j] = (c0 + 64 * j) < r.P4f;
      l[j] = ok[j] ? r.last[c0 + 64 * j] : z4;  // a masked strip: 0 - 0, adds +0.0
    }
    const f4* row = r.x + c0;
    double* w = r.ws + wt;
    int k = 0;
    for (; k + NQ_U <= r.n; k += NQ_U) {
      f4 t[NQ_U][NQ_V];
#pragma unroll
      for (int u = 0; u < NQ_U; ++u)
#pragma unroll
        for (int j = 0; j < NQ_V; ++j) t[u][j] = ok[j] ? __builtin_nontemporal_load(row + u * r.ld4 + 64 * j) : z4;
#pragma unroll
      for (int u = 0; u < NQ_U; ++u) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < NQ_V; ++j) acc = sq_acc(acc, t[u][j], l[j]);
        acc = wave_sum(acc);
        if (lane == 0) w[(int64_t)(k + u) * r.tiles] = acc;
      }
      row += NQ_U * r.ld4;
    }
    for (; k < r.n; ++k) {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < NQ_V; ++j)
        acc = sq_acc(acc, ok[j] ? __builtin_nontemporal_load(row + 64 * j) : z4, l[j]);
      acc = wave_sum(acc);
      if (lane == 0) w[(int64_t)k * r.tiles] = acc;
      row += r.ld4;
    }
  }
}

// One wave per row: lane l adds the row's partials of tiles l, l + 64, ... in order, the lanes meet in the
// butterfly, and the columns [4 P4f, P) follow in order.
__global__ __launch_bounds__(64) void k_sqnorm_sum(const double* __restrict__ ws, int64_t tiles,
                                                   const float* __restrict__ x, int64_t ld, int64_t P4f, int64_t P,
                                                   const float* __restrict__ last, double* __restrict__ sq) {
  const int64_t k = blockIdx.x;
  const int lane = threadIdx.x;
  double acc = 0.0;
  for (int64_t t = lane; t < tiles; t += 64) acc = acc + ws[k * tiles + t];
  acc = wave_sum(acc);
  if (lane == 0) {
    for (int64_t p = 4 * P4f; p < P; ++p) {
      const float d = x[k * ld + p] - last[p];
      acc = __builtin_fma((double)d, (double)d, acc);
    }
    sq[k] = acc;
  }
}

int64_t norm_tiles(int64_t P) {
  const int64_t tile4 = 64 * norm_geo(P).V;
  return (P / 4 + tile4 - 1) / tile4;
}
int64_t norm_grid(int64_t cus, int64_t P) {
  const NormGeo g = norm_geo(P);
  const int64_t wgs = (norm_tiles(P) + g.waves - 1) / g.waves;
  const int64_t cap = cus * g.grid_pct / 100 > 0 ? cus * g.grid_pct / 100 : 1;
  return wgs < cap ? wgs : cap;
}

// ------------------------------------------------------------------------------------------------
// fcl_clip_coefs
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_clip_coef(const double* __restrict__ sq, int n, double M,
                                                   float* __restrict__ c, int32_t* rejected) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double s = sq[i];
  float ck = 0.0f;
  if (!__builtin_isfinite(s)) {
    atomicAdd(rejected, 1);  // an integer count: any order gives the same value
  } else {
    const double rk = M / (sqrt(s) + 1e-6);
    ck = rk < 1.0 ? (float)rk : 1.0f;
  }
  c[i] = ck;
}

// ------------------------------------------------------------------------------------------------
// fcl_reduce
// ------------------------------------------------------------------------------------------------
constexpr int FCL_WAVES = 4;  // waves per workgroup, each owning V strips of a tile

struct ClipArgs {
  const f4* x;     // the rows, in float4 columns
  int64_t ld4;     // row stride in float4 columns
  int64_t P4;      // float4 columns to read, ceil(P / 4)
  int64_t P;       // columns to write
  int64_t c0;      // first float4 column of this launch
  int64_t ntiles;  // tiles of this launch; workgroup b takes tiles b, b + grid, ...
  int n;
  int flags;
  const f4* last;
  const float* coef;
  const f4* acc_in;
  float* out;
};

// One tile, as fh_reduce's: each of the workgroup's waves owns V strips (64 lanes x one float4: 256 contiguous
// columns of a row each) and walks all n rows, U rows' loads issued ahead of their adds.  A lane holds its columns
// of `last` (4V registers), the chain (4V) and 4UV load registers.  The coefficient is a per-row scalar, so the skip
// of a rejected row is wave-uniform.
template <int V, int U>
__device__ __forceinline__ void clip_tile(const ClipArgs& r, int64_t tile, int lane, int wave) {
  const int64_t c0 = r.c0 + (tile * FCL_WAVES + wave) * (64LL * V) + lane;
  const f4 z4 = f4{0.f, 0.f, 0.f, 0.f};
  bool ok[V];
  f4 l[V], s[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    ok[j] = (c0 + 64 * j) < r.P4;
    l[j] = ok[j] ? r.last[c0 + 64 * j] : z4;
    s[j] = ((r.flags & FA_ACCUMULATE) && ok[j]) ? r.acc_in[c0 + 64 * j] : z4;
  }
  const f4* row = r.x + c0;
  int k = 0;
  for (; k + U <= r.n; k += U) {
    f4 t[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) t[u][j] = ok[j] ? __builtin_nontemporal_load(row + u * r.ld4 + 64 * j) : z4;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float ck = r.coef[k + u];
      if (ck != 0.0f) {
#pragma unroll
        for (int j = 0; j < V; ++j) s[j] = s[j] + ck * (t[u][j] - l[j]);
      }
    }
    row += U * r.ld4;
  }
  for (; k < r.n; ++k) {
    const float ck = r.coef[k];
    if (ck != 0.0f) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const f4 t = ok[j] ? __builtin_nontemporal_load(row + 64 * j) : z4;
        s[j] = s[j] + ck * (t - l[j]);
      }
    }
    row += r.ld4;
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (!ok[j]) continue;
    const int64_t p = 4 * (c0 + 64 * j);
    if (p + 4 <= r.P) {
      *reinterpret_cast<f4*>(r.out + p) = s[j];
    } else {  // the last, partial float4 column: columns >= P are not written
      r.out[p] = s[j].x;
      if (p + 1 < r.P) r.out[p + 1] = s[j].y;
      if (p + 2 < r.P) r.out[p + 2] = s[j].z;
    }
  }
}

// LOOP = false: workgroup b reduces tile b.  LOOP = true: a capped grid, workgroup b reduces tiles b, b + grid, ...
template <int V, int U, bool LOOP>
__global__ __launch_bounds__(64 * FCL_WAVES) void k_reduce_clip(ClipArgs r) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (LOOP) {
    for (int64_t tile = blockIdx.x; tile < r.ntiles; tile += gridDim.x) clip_tile<V, U>(r, tile, lane, wave);
  } else {
    clip_tile<V, U>(r, blockIdx.x, lane, wave);
  }
}

// Launch plan: strip_plan (fa_common.h) over strips of 256 columns, fh_reduce's plan with fp32 rows.  Its three
// variants, sized by registers — a lane holds 8V registers of `last` and chain plus 4UV of loads in flight:
//   level 0  V = 16, U = 1   128 + 64 registers, one wave per SIMD: the widest contiguous run per row (16 KiB)
//   level 1  V =  8, U = 4    64 + 128 registers, two waves per SIMD
//   level 2  V =  2, U = 8    16 +  64 registers: short rows need the parallelism
// K does not enter the plan today; it is a parameter because fa_reduce's plan depends on it.
constexpr StripGeo FCL_GEO{FCL_WAVES, {16, 8, 2}, {1, 4, 8}, 75, 256};
static_assert(FCL_PLAN_FIELDS == STRIP_PLAN_FIELDS, "fcl_reduce_plan's row is strip_plan_export's");

int64_t clip_strips(int64_t P) { return ((P + 3) / 4 + 63) / 64; }

template <int V, int U>
void launch_one(ClipArgs r, const StripLaunch& l, hipStream_t st) {
  r.c0 = l.strip0 * 64;
  r.ntiles = l.tiles;
  const dim3 grid((unsigned)l.grid), blk(64 * FCL_WAVES);
  if constexpr (V == FCL_GEO.V[0]) {  // only level 0 runs on a capped grid
    if (l.grid < l.tiles) {
      hipLaunchKernelGGL((k_reduce_clip<V, U, true>), grid, blk, 0, st, r);
      return;
    }
  }
  hipLaunchKernelGGL((k_reduce_clip<V, U, false>), grid, blk, 0, st, r);
}

void launch_level(const ClipArgs& r, const StripLaunch& l, hipStream_t st) {
  if (l.level == 0)
    launch_one<FCL_GEO.V[0], FCL_GEO.U[0]>(r, l, st);
  else if (l.level == 1)
    launch_one<FCL_GEO.V[1], FCL_GEO.U[1]>(r, l, st);
  else
    launch_one<FCL_GEO.V[2], FCL_GEO.U[2]>(r, l, st);
}

// ------------------------------------------------------------------------------------------------
// fcl_finish
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float finish1(float ch, float l, float z, float sigma, float denom, bool noise,
                                         float& m) {
  m = __fdiv_rn(ch, denom);
  if (noise) m = m + sigma * z;
  return l + m;
}

__global__ __launch_bounds__(256) void k_clip_finish(const f4* __restrict__ chain, const f4* __restrict__ last,
                                                     const f4* __restrict__ z, float sigma, float denom, int64_t P,
                                                     float* out, float* mean_delta, float* mirror) {
  const bool noise = sigma > 0.0f;
  const int64_t P4 = (P + 3) / 4;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < P4; c += (int64_t)gridDim.x * 256) {
    const f4 ch = chain[c], l = last[c];
    const f4 zz = noise ? z[c] : f4{0.f, 0.f, 0.f, 0.f};
    float mm[4], oo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) oo[i] = finish1(ch[i], l[i], zz[i], sigma, denom, noise, mm[i]);
    const f4 m = f4{mm[0], mm[1], mm[2], mm[3]}, o = f4{oo[0], oo[1], oo[2], oo[3]};
    const int64_t p = 4 * c;
    if (p + 4 <= P) {
      *reinterpret_cast<f4*>(out + p) = o;
      if (mean_delta) *reinterpret_cast<f4*>(mean_delta + p) = m;
      if (mirror) *reinterpret_cast<f4*>(mirror + p) = o;
    } else {  // the last, partial float4 column: columns >= P are not written
      for (int i = 0; i < (int)(P - p); ++i) {
        out[p + i] = oo[i];
        if (mean_delta) mean_delta[p + i] = mm[i];
        if (mirror) mirror[p + i] = oo[i];
      }
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedclip.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t fcl_abi_version(void) { return FCL_ABI_VERSION; }

extern "C" int64_t fcl_workspace_bytes(int32_t n, int64_t P) {
  if (n < 0 || P < 0) return refuse(FA_E_ARG, "fcl_workspace_bytes: negative n=%d or P=%lld", n, (long long)P);
  const int64_t b = (int64_t)n * norm_tiles(P) * 8;
  return b > 8 ? b : 8;
}

extern "C" int64_t fcl_norm_plan(int32_t cus, int64_t P, int64_t* plan_out) {
  if (cus <= 0 || P < 0 || !plan_out)
    return refuse(FA_E_ARG, "fcl_norm_plan: bad arguments (cus=%d P=%lld)", cus, (long long)P);
  const int64_t tiles = norm_tiles(P);
  plan_out[0] = tiles;
  plan_out[1] = norm_grid(cus, P);
  plan_out[2] = norm_geo(P).waves;
  plan_out[3] = 256 * norm_geo(P).V;
  return tiles > 0 ? 2 : 1;
}

extern "C" int fcl_row_sqnorms(const float* x, int64_t ld, int32_t n, int64_t P, const float* last, double* sq,
                               double* workspace, int64_t workspace_bytes, fa_stream_t stream) {
  if (n <= 0) return refuse(FA_E_ARG, "fcl_row_sqnorms: n=%d rows, needs n >= 1", n);
  if (P < 0 || ld < P) return refuse(FA_E_ARG, "fcl_row_sqnorms: ld=%lld < P=%lld or negative P", (long long)ld, (long long)P);
  if (ld % 4 != 0) return refuse(FA_E_ARG, "fcl_row_sqnorms: ld=%lld must be a multiple of 4 elements", (long long)ld);
  if (!x || !last || !sq || !workspace) return refuse(FA_E_ARG, "fcl_row_sqnorms: x, last, sq or workspace is NULL");
  if (!aligned16(x) || !aligned16(last)) return refuse(FA_E_ARG, "fcl_row_sqnorms: x and last must be 16-byte aligned");
  if (((uintptr_t)sq & 7u) || ((uintptr_t)workspace & 7u))
    return refuse(FA_E_ARG, "fcl_row_sqnorms: sq and workspace must be 8-byte aligned");
  const int64_t tiles = norm_tiles(P);
  const int64_t need = fcl_workspace_bytes(n, P);
  if (workspace_bytes < need)
    return refuse(FA_E_ARG, "fcl_row_sqnorms: workspace of %lld bytes, needs %lld (fcl_workspace_bytes)",
                  (long long)workspace_bytes, (long long)need);
  const int64_t P4c = (P + 3) / 4;
  FA_DEVICE_SCOPE("fcl_row_sqnorms", stream, sq);
  FA_OPERAND("x", x, (uint64_t)((int64_t)(n - 1) * ld + P4c * 4) * 4);
  FA_OPERAND("last", last, (uint64_t)P4c * 16);
  FA_OPERAND("sq", sq, (uint64_t)n * 8);
  FA_OPERAND("workspace", workspace, (uint64_t)need);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fcl_row_sqnorms: no CU count for device %d", fa_scope_device());
  hipStream_t st = (hipStream_t)stream;
  if (tiles > 0) {
    NormArgs r{};
    r.x = reinterpret_cast<const f4*>(x); r.ld4 = ld / 4; r.P4f = P / 4; r.tiles = tiles; r.n = n;
    r.last = reinterpret_cast<const f4*>(last); r.ws = workspace;
    const dim3 grid((unsigned)norm_grid(cus, P));
    if (P >= NQ_WIDE_MIN_P)
      hipLaunchKernelGGL((k_row_sqnorm<NQ_WIDE.V, NQ_WIDE.U, NQ_WIDE.waves>), grid, dim3(64 * NQ_WIDE.waves), 0, st, r);
    else
      hipLaunchKernelGGL((k_row_sqnorm<NQ_NARROW.V, NQ_NARROW.U, NQ_NARROW.waves>), grid, dim3(64 * NQ_NARROW.waves),
                         0, st, r);
    const int e = check_launch("fcl_row_sqnorms");
    if (e) return e;
  }
  hipLaunchKernelGGL(k_sqnorm_sum, dim3((unsigned)n), dim3(64), 0, st, workspace, tiles, x, ld, P / 4, P, last, sq);
  return check_launch("fcl_row_sqnorms");
}

extern "C" int fcl_clip_coefs(const double* sq, int32_t n, double max_norm, float* c, int32_t* rejected,
                              fa_stream_t stream) {
  if (n <= 0) return refuse(FA_E_ARG, "fcl_clip_coefs: n=%d rows, needs n >= 1", n);
  if (!(max_norm > 0.0) || !__builtin_isfinite(max_norm))
    return refuse(FA_E_ARG, "fcl_clip_coefs: max_norm=%g must be finite and > 0", max_norm);
  if (!sq || !c || !rejected) return refuse(FA_E_ARG, "fcl_clip_coefs: sq, c or rejected is NULL");
  if (((uintptr_t)sq & 7u) || ((uintptr_t)c & 3u) || ((uintptr_t)rejected & 3u))
    return refuse(FA_E_ARG, "fcl_clip_coefs: sq must be 8-byte, c and rejected 4-byte aligned");
  FA_DEVICE_SCOPE("fcl_clip_coefs", stream, c);
  FA_OPERAND("sq", sq, (uint64_t)n * 8);
  FA_OPERAND("c", c, (uint64_t)n * 4);
  FA_OPERAND("rejected", rejected, 4);
  hipLaunchKernelGGL(k_clip_coef, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sq, n,
                     max_norm, c, rejected);
  return check_launch("fcl_clip_coefs");
}

extern "C" int64_t fcl_reduce_plan(int32_t cus, int32_t K, int64_t P, int64_t* plan_out, int32_t cap) {
  if (cus <= 0 || K < 0 || P < 0 || cap < 0 || (cap > 0 && !plan_out))
    return refuse(FA_E_ARG, "fcl_reduce_plan: bad arguments (cus=%d K=%d P=%lld cap=%d)", cus, K, (long long)P, cap);
  return strip_plan_export(cus, clip_strips(P), FCL_GEO, plan_out, cap);
}

extern "C" int fcl_reduce(const float* x, int64_t ld, int32_t n, int64_t P, const float* last, const float* c,
                          const float* acc_in, float* out, int32_t flags, fa_stream_t stream) {
  if (flags & ~FA_ACCUMULATE) return refuse(FA_E_ARG, "fcl_reduce: unknown flags %d (0 or FA_ACCUMULATE)", flags);
  if (n < 0 || P < 0 || ld < P) return refuse(FA_E_ARG, "fcl_reduce: ld=%lld < P=%lld, or negative n=%d / P", (long long)ld, (long long)P, n);
  if (ld % 4 != 0) return refuse(FA_E_ARG, "fcl_reduce: ld=%lld must be a multiple of 4 elements", (long long)ld);
  if ((flags & FA_ACCUMULATE) && !acc_in) return refuse(FA_E_ARG, "fcl_reduce: FA_ACCUMULATE without acc_in");
  if (n == 0 && !(flags & FA_ACCUMULATE)) return refuse(FA_E_ARG, "fcl_reduce: n=0 rows with nothing to accumulate");
  if (n > 0 && (!x || !c)) return refuse(FA_E_ARG, "fcl_reduce: x or c is NULL");
  if (!last || !out) return refuse(FA_E_ARG, "fcl_reduce: last or out is NULL");
  if (!aligned16(x) || !aligned16(last)) return refuse(FA_E_ARG, "fcl_reduce: x and last must be 16-byte aligned");
  if (!aligned16(out) || !aligned16(acc_in)) return refuse(FA_E_ARG, "fcl_reduce: out and acc_in must be 16-byte aligned");
  if ((uintptr_t)c & 3u) return refuse(FA_E_ARG, "fcl_reduce: c must be 4-byte aligned");
  if (P == 0) return FA_OK;
  const int64_t P4 = (P + 3) / 4;
  if (P4 / (64 * FCL_WAVES) > 0x7fffffffLL) return refuse(FA_E_RANGE, "fcl_reduce: P too large");
  FA_DEVICE_SCOPE("fcl_reduce", stream, out);
  FA_OPERAND("x", x, n > 0 ? (uint64_t)((int64_t)(n - 1) * ld + P4 * 4) * 4 : 0);
  FA_OPERAND("last", last, (uint64_t)P4 * 16);
  FA_OPERAND("c", c, (uint64_t)n * 4);
  FA_OPERAND("acc_in", (flags & FA_ACCUMULATE) ? acc_in : nullptr, (uint64_t)P4 * 16);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fcl_reduce launch plan: no CU count for device %d", fa_scope_device());
  ClipArgs r{};
  r.x = reinterpret_cast<const f4*>(x); r.ld4 = ld / 4; r.P4 = P4; r.P = P; r.n = n; r.flags = flags;
  r.last = reinterpret_cast<const f4*>(last); r.coef = c; r.acc_in = reinterpret_cast<const f4*>(acc_in);
  r.out = out;
  StripLaunch l[3];
  const int nl = strip_plan(cus, clip_strips(P), FCL_GEO, l);
  for (int i = 0; i < nl; ++i) {
    launch_level(r, l[i], (hipStream_t)stream);
    const int e = check_launch("fcl_reduce");
    if (e) return e;
  }
  return FA_OK;
}

extern "C" int fcl_finish(const float* chain, const float* last, const float* z, float sigma, float denom, int64_t P,
                          float* out, float* mean_delta_out, float* mirror, fa_stream_t stream) {
  if (P < 0) return refuse(FA_E_ARG, "fcl_finish: negative P=%lld", (long long)P);
  if (!(sigma >= 0.0f) || !__builtin_isfinite(sigma)) return refuse(FA_E_ARG, "fcl_finish: sigma=%g must be finite and >= 0", (double)sigma);
  if (!(denom > 0.0f)) return refuse(FA_E_ARG, "fcl_finish: denom=%g must be > 0", (double)denom);
  if (!chain || !last || !out) return refuse(FA_E_ARG, "fcl_finish: chain, last or out is NULL");
  if (sigma > 0.0f && !z) return refuse(FA_E_ARG, "fcl_finish: sigma > 0 without z");
  if (!aligned16(chain) || !aligned16(last) || !aligned16(z))
    return refuse(FA_E_ARG, "fcl_finish: chain, last and z must be 16-byte aligned");
  if (!aligned16(out) || !aligned16(mean_delta_out) || !aligned16(mirror))
    return refuse(FA_E_ARG, "fcl_finish: out, mean_delta_out and mirror must be 16-byte aligned");
  if (P == 0) return FA_OK;
  const int64_t P4 = (P + 3) / 4;
  FA_DEVICE_SCOPE("fcl_finish", stream, out);
  FA_OPERAND("chain", chain, (uint64_t)P4 * 16);
  FA_OPERAND("last", last, (uint64_t)P4 * 16);
  FA_OPERAND("z", sigma > 0.0f ? z : nullptr, (uint64_t)P4 * 16);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  FA_OPERAND("mean_delta_out", mean_delta_out, (uint64_t)P * 4);
  FA_HOST_OK_OPERAND("mirror", mirror, (uint64_t)P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fcl_finish: no CU count for device %d", fa_scope_device());
  int64_t g = (P4 + 255) / 256;
  if (g > (int64_t)cus * 8) g = (int64_t)cus * 8;
  hipLaunchKernelGGL(k_clip_finish, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const f4*>(chain), reinterpret_cast<const f4*>(last),
                     reinterpret_cast<const f4*>(z), sigma, denom, P, out, mean_delta_out, mirror);
  return check_launch("fcl_finish");
}
