// secagg.hip — MI355X (gfx950) kernels of the secure-aggregation data path (include/fedsecagg.h):
//   * fsa_encode_row: the executor-side encoder, one fp32 row (minus the round's base model) into fixed-point words
//     mod 2^32, with the counts of clamped and NaN elements;
//   * fsa_mask_sum: a sum of ChaCha20 keystreams (RFC 8439 section 2.3, one block of 16 columns per lane and key)
//     added to or subtracted from a row mod 2^32 — the executor's masking and the server's unmasking;
//   * fsa_reduce: the modular sum of the staged rows, and fsa_reduce_plan, the launches it makes;
//   * fsa_finish: the unmasked sum back to fp32 on the round's starting model, with the range check's count.
//
// Numerics: the integer arithmetic is mod 2^32, so no launch plan changes a bit; every fp32 / fp64 op is rounded to
// nearest and never contracted into an FMA.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fedsecagg.h"
#include "fa_device.h"
#include "fa_common.h"

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

// the 64 lanes' counts added up (every lane ends with the sum)
__device__ __forceinline__ int wave_count(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// a count added to a device int64 by one lane: a vector atomic on integers, so any order gives the same value
__device__ __forceinline__ void count_add(int64_t* dst, int v) {
  __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)v, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------
// fsa_encode_row
// ------------------------------------------------------------------------------------------------
constexpr int ENC_THREADS = 256;  // 4 columns per thread

// one element; cl / nn count what the clamp and the NaN rule touched
__device__ __forceinline__ uint32_t encode1(float d, float scale, double B, int& cl, int& nn) {
  const float r = __builtin_rintf(d * scale);
  if (r != r) {
    ++nn;
    return 0u;
  }
  double v = (double)r;
  if (v > B) {
    v = B;
    ++cl;
  } else if (v < -B) {
    v = -B;
    ++cl;
  }
  return (uint32_t)(int32_t)v;
}

__global__ __launch_bounds__(ENC_THREADS) void k_encode_row(const float* __restrict__ x, const float* __restrict__ base,
                                                            int64_t P, float scale, double B,
                                                            uint32_t* __restrict__ out, int64_t* stats) {
  const int64_t p = 4 * ((int64_t)blockIdx.x * ENC_THREADS + threadIdx.x);
  int cl = 0, nn = 0;
  if (p + 4 <= P) {
    f4 d = *reinterpret_cast<const f4*>(x + p);
    if (base) d = d - *reinterpret_cast<const f4*>(base + p);
    u4 q;
    q.x = encode1(d.x, scale, B, cl, nn);
    q.y = encode1(d.y, scale, B, cl, nn);
    q.z = encode1(d.z, scale, B, cl, nn);
    q.w = encode1(d.w, scale, B, cl, nn);
    *reinterpret_cast<u4*>(out + p) = q;
  } else {  // the row's last columns; columns >= P are neither read nor written
    for (int64_t c = p; c < P; ++c) out[c] = encode1(base ? x[c] - base[c] : x[c], scale, B, cl, nn);
  }
  cl = wave_count(cl);
  nn = wave_count(nn);
  if ((threadIdx.x & 63) == 0) {
    if (cl) count_add(stats, cl);
    if (nn) count_add(stats + 1, nn);
  }
}

// ------------------------------------------------------------------------------------------------
// fsa_mask_sum
// ------------------------------------------------------------------------------------------------
constexpr int MS_THREADS = 256;  // one ChaCha20 block (16 columns) per lane: FSA_MASK_TILE columns per workgroup
static_assert(MS_THREADS * 16 == FSA_MASK_TILE, "a workgroup of fsa_mask_sum covers FSA_MASK_TILE columns per sweep");

__device__ __forceinline__ uint32_t rotl(uint32_t v, int n) { return __builtin_rotateleft32(v, n); }

#define FSA_QR(a, b, c, d)                    \
  a += b; d ^= a; d = rotl(d, 16);            \
  c += d; b ^= c; b = rotl(b, 12);            \
  a += b; d ^= a; d = rotl(d, 8);             \
  c += d; b ^= c; b = rotl(b, 7)

// the ChaCha20 block of (key k, counter ctr, nonce n0..n2) added to (SUB: subtracted from) the lane's 16 words; the
// key and the nonce are wave-uniform, the counter is the lane's
template <bool SUB>
__device__ __forceinline__ void mask_block(const uint32_t* __restrict__ k, uint32_t ctr, uint32_t n0, uint32_t n1,
                                           uint32_t n2, uint32_t a[16]) {
  uint32_t in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, k[0], k[1], k[2], k[3],
                     k[4],        k[5],        k[6],        k[7],        ctr,  n0,   n1,   n2};
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = in[i];
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    FSA_QR(x[0], x[4], x[8], x[12]);
    FSA_QR(x[1], x[5], x[9], x[13]);
    FSA_QR(x[2], x[6], x[10], x[14]);
    FSA_QR(x[3], x[7], x[11], x[15]);
    FSA_QR(x[0], x[5], x[10], x[15]);
    FSA_QR(x[1], x[6], x[11], x[12]);
    FSA_QR(x[2], x[7], x[8], x[13]);
    FSA_QR(x[3], x[4], x[9], x[14]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t w = x[i] + in[i];
    a[i] = SUB ? a[i] - w : a[i] + w;
  }
}
#undef FSA_QR

// Block g of the call (columns [16g, 16g + 16)) belongs to lane g % 256 of workgroup (g / 256) % grid.  The lane
// loads its 16 words (four 16-byte loads; the row's last, partial block word by word), walks the keys with the words
// in registers and stores them once.
__global__ __launch_bounds__(MS_THREADS) void k_mask_sum(const uint32_t* __restrict__ keys, int n_add, int n_sub,
                                                         uint32_t n0, uint32_t n1, uint32_t n2, uint32_t blk0,
                                                         int64_t nblk, int64_t P, const uint32_t* acc_in,
                                                         uint32_t* out) {
  for (int64_t g = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; g < nblk; g += (int64_t)gridDim.x * MS_THREADS) {
    const int64_t p = 16 * g;
    const bool whole = p + 16 <= P;
    uint32_t a[16];
    if (whole) {
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const u4 v = *reinterpret_cast<const u4*>(acc_in + p + 4 * h);
        a[4 * h] = v.x; a[4 * h + 1] = v.y; a[4 * h + 2] = v.z; a[4 * h + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) a[i] = p + i < P ? acc_in[p + i] : 0u;
    }
    const uint32_t ctr = blk0 + (uint32_t)g;  // col0 + P <= 2^36: no block counter of a call wraps
    int m = 0;
    for (; m < n_add; ++m) mask_block<false>(keys + 8 * (int64_t)m, ctr, n0, n1, n2, a);
    for (; m < n_add + n_sub; ++m) mask_block<true>(keys + 8 * (int64_t)m, ctr, n0, n1, n2, a);
    if (whole) {
#pragma unroll
      for (int h = 0; h < 4; ++h)
        *reinterpret_cast<u4*>(out + p + 4 * h) = u4{a[4 * h], a[4 * h + 1], a[4 * h + 2], a[4 * h + 3]};
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (p + i < P) out[p + i] = a[i];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// fsa_reduce
// ------------------------------------------------------------------------------------------------
constexpr int FSA_WAVES = 4;  // waves per workgroup, each owning V strips of a tile

struct SumArgs {
  const u4* y;     // the rows, in 16-byte columns (4 words)
  int64_t ld4;     // row stride in 16-byte columns
  int64_t P4;      // 16-byte columns to read, ceil(P / 4)
  int64_t P;       // columns to write
  int64_t c0;      // first 16-byte column of this launch
  int64_t ntiles;  // tiles of this launch; workgroup b takes tiles b, b + grid, ...
  int n;
  int flags;
  const u4* acc_in;
  uint32_t* out;
};

// One tile, as fcl_reduce's: each of the workgroup's waves owns V strips (64 lanes x one 16-byte load: 256 contiguous
// columns of a row each) and walks all n rows, U rows' loads issued ahead of their adds.  A lane holds 4V words of
// the sum and 4UV load registers.  Strips past ceil(P / 4) are masked: nothing of them is loaded or stored.
template <int V, int U>
__device__ __forceinline__ void sum_tile(const SumArgs& r, int64_t tile, int lane, int wave) {
  const int64_t c0 = r.c0 + (tile * FSA_WAVES + wave) * (64LL * V) + lane;
  const u4 z4 = u4{0u, 0u, 0u, 0u};
  bool ok[V];
  u4 s[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    ok[j] = (c0 + 64 * j) < r.P4;
    s[j] = ((r.flags & FA_ACCUMULATE) && ok[j]) ? r.acc_in[c0 + 64 * j] : z4;
  }
  const u4* row = r.y + c0;
  int k = 0;
  for (; k + U <= r.n; k += U) {
    u4 t[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) t[u][j] = ok[j] ? __builtin_nontemporal_load(row + u * r.ld4 + 64 * j) : z4;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) s[j] = s[j] + t[u][j];
    row += U * r.ld4;
  }
  for (; k < r.n; ++k) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const u4 t = ok[j] ? __builtin_nontemporal_load(row + 64 * j) : z4;
      s[j] = s[j] + t;
    }
    row += r.ld4;
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (!ok[j]) continue;
    const int64_t p = 4 * (c0 + 64 * j);
    if (p + 4 <= r.P) {
      *reinterpret_cast<u4*>(r.out + p) = s[j];
    } else {  // the last, partial 16-byte column: columns >= P are not written
      r.out[p] = s[j].x;
      if (p + 1 < r.P) r.out[p + 1] = s[j].y;
      if (p + 2 < r.P) r.out[p + 2] = s[j].z;
    }
  }
}

// LOOP = false: workgroup b reduces tile b.  LOOP = true: a capped grid, workgroup b reduces tiles b, b + grid, ...
template <int V, int U, bool LOOP>
__global__ __launch_bounds__(64 * FSA_WAVES) void k_reduce_masked(SumArgs r) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (LOOP) {
    for (int64_t tile = blockIdx.x; tile < r.ntiles; tile += gridDim.x) sum_tile<V, U>(r, tile, lane, wave);
  } else {
    sum_tile<V, U>(r, blockIdx.x, lane, wave);
  }
}

// Launch plan: strip_plan (fa_common.h) over strips of 256 columns, fcl_reduce's plan without its `last` registers —
// a lane holds 4V words of the sum plus 4UV of loads in flight:
//   level 0  V = 16, U = 2    64 + 128 registers, two waves per SIMD: the widest contiguous run per row (16 KiB)
//   level 1  V =  8, U = 4    32 + 128 registers, two waves per SIMD
//   level 2  V =  2, U = 8     8 +  64 registers: short rows need the parallelism
// K does not enter the plan today; it is a parameter because fa_reduce's plan depends on it.
constexpr StripGeo FSA_GEO{FSA_WAVES, {16, 8, 2}, {2, 4, 8}, 75, 256};
static_assert(FSA_PLAN_FIELDS == STRIP_PLAN_FIELDS, "fsa_reduce_plan's row is strip_plan_export's");

int64_t sum_strips(int64_t P) { return ((P + 3) / 4 + 63) / 64; }

template <int V, int U>
void launch_one(SumArgs r, const StripLaunch& l, hipStream_t st) {
  r.c0 = l.strip0 * 64;
  r.ntiles = l.tiles;
  const dim3 grid((unsigned)l.grid), blk(64 * FSA_WAVES);
  if constexpr (V == FSA_GEO.V[0]) {  // only level 0 runs on a capped grid
    if (l.grid < l.tiles) {
      hipLaunchKernelGGL((k_reduce_masked<V, U, true>), grid, blk, 0, st, r);
      return;
    }
  }
  hipLaunchKernelGGL((k_reduce_masked<V, U, false>), grid, blk, 0, st, r);
}

void launch_level(const SumArgs& r, const StripLaunch& l, hipStream_t st) {
  if (l.level == 0)
    launch_one<FSA_GEO.V[0], FSA_GEO.U[0]>(r, l, st);
  else if (l.level == 1)
    launch_one<FSA_GEO.V[1], FSA_GEO.U[1]>(r, l, st);
  else
    launch_one<FSA_GEO.V[2], FSA_GEO.U[2]>(r, l, st);
}

// ------------------------------------------------------------------------------------------------
// fsa_finish
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_secagg_finish(const u4* __restrict__ sum, const f4* __restrict__ last,
                                                       int64_t P, double inv_scale, double n, int64_t bound,
                                                       float* out, float* mirror, int64_t* out_of_range) {
  const int64_t P4 = (P + 3) / 4;
  int bad = 0;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < P4; c += (int64_t)gridDim.x * 256) {
    const u4 sv = sum[c];
    const f4 l = last[c];
    const int64_t p = 4 * c;
    const int live = p + 4 <= P ? 4 : (int)(P - p);
    float oo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int32_t s = (int32_t)sv[i];
      const int64_t mag = s < 0 ? -(int64_t)s : (int64_t)s;
      if (i < live && mag > bound) ++bad;
      const float m = (float)(((double)s * inv_scale) / n);
      oo[i] = l[i] + m;
    }
    if (live == 4) {
      const f4 o = f4{oo[0], oo[1], oo[2], oo[3]};
      *reinterpret_cast<f4*>(out + p) = o;
      if (mirror) *reinterpret_cast<f4*>(mirror + p) = o;
    } else {  // the last, partial float4 column: columns >= P are neither counted nor written
      for (int i = 0; i < live; ++i) {
        out[p + i] = oo[i];
        if (mirror) mirror[p + i] = oo[i];
      }
    }
  }
  bad = wave_count(bad);
  if ((threadIdx.x & 63) == 0 && bad) count_add(out_of_range, bad);
}

bool spec_ok(int32_t frac_bits, int32_t mag_bits) {
  return frac_bits >= 0 && frac_bits <= FSA_MAX_FRAC_BITS && mag_bits >= 1 && mag_bits <= FSA_MAX_MAG_BITS;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedsecagg.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t fsa_abi_version(void) { return FSA_ABI_VERSION; }

extern "C" int fsa_encode_row(const float* x, const float* base, int64_t P, int32_t frac_bits, int32_t mag_bits,
                              uint32_t* out_u32, int64_t* stats, fa_stream_t stream) {
  if (P < 0) return refuse(FA_E_ARG, "fsa_encode_row: negative P=%lld", (long long)P);
  if (!spec_ok(frac_bits, mag_bits))
    return refuse(FA_E_ARG, "fsa_encode_row: frac_bits=%d must be in [0, %d] and mag_bits=%d in [1, %d]", frac_bits,
                  FSA_MAX_FRAC_BITS, mag_bits, FSA_MAX_MAG_BITS);
  if (!stats) return refuse(FA_E_ARG, "fsa_encode_row: stats is NULL");
  if ((uintptr_t)stats & 7u) return refuse(FA_E_ARG, "fsa_encode_row: stats must be 8-byte aligned");
  if (P > 0 && (!x || !out_u32)) return refuse(FA_E_ARG, "fsa_encode_row: x or out_u32 is NULL");
  if (!aligned16(x) || !aligned16(base) || !aligned16(out_u32))
    return refuse(FA_E_ARG, "fsa_encode_row: x, base and out_u32 must be 16-byte aligned");
  const int64_t grid = ((P + 3) / 4 + ENC_THREADS - 1) / ENC_THREADS;
  if (grid > 0x7fffffffLL) return refuse(FA_E_RANGE, "fsa_encode_row: P too large");
  FA_DEVICE_SCOPE("fsa_encode_row", stream, stats);
  FA_OPERAND("x", x, (uint64_t)P * 4);
  FA_OPERAND("base", base, (uint64_t)P * 4);
  FA_OPERAND("out_u32", out_u32, (uint64_t)P * 4);
  FA_OPERAND("stats", stats, 16);
  if (hipMemsetAsync(stats, 0, 16, (hipStream_t)stream) != hipSuccess)
    return fail(FA_E_HIP, "fsa_encode_row: clearing stats failed: %s", hipGetErrorString(hipGetLastError()));
  if (P == 0) return FA_OK;
  const float scale = __builtin_bit_cast(float, (uint32_t)(127 + frac_bits) << 23);  // 2^f
  const double B = (double)((1LL << mag_bits) - 1);
  hipLaunchKernelGGL(k_encode_row, dim3((unsigned)grid), dim3(ENC_THREADS), 0, (hipStream_t)stream, x, base, P, scale,
                     B, out_u32, stats);
  return check_launch("fsa_encode_row");
}

extern "C" int fsa_mask_sum(const uint32_t* keys, int32_t n_add, int32_t n_sub, uint32_t nonce0, uint32_t nonce1,
                            uint32_t nonce2, int64_t col0, int64_t P, const uint32_t* acc_in, uint32_t* out,
                            fa_stream_t stream) {
  if (P < 0 || n_add < 0 || n_sub < 0)
    return refuse(FA_E_ARG, "fsa_mask_sum: negative P=%lld, n_add=%d or n_sub=%d", (long long)P, n_add, n_sub);
  const int64_t M = (int64_t)n_add + n_sub;
  if (M > FSA_MAX_KEYS)
    return refuse(FA_E_ARG, "fsa_mask_sum: %lld keys exceed the limit FSA_MAX_KEYS = %d", (long long)M, FSA_MAX_KEYS);
  if (col0 < 0 || col0 % 16 != 0)
    return refuse(FA_E_ARG, "fsa_mask_sum: col0=%lld must be a multiple of 16, >= 0", (long long)col0);
  if (col0 > (1LL << 36) || P > (1LL << 36) - col0)
    return refuse(FA_E_ARG, "fsa_mask_sum: col0 + P = %lld + %lld exceeds 2^36 columns (the 32-bit block counter)",
                  (long long)col0, (long long)P);
  if (M > 0 && !keys) return refuse(FA_E_ARG, "fsa_mask_sum: keys is NULL");
  if ((uintptr_t)keys & 3u) return refuse(FA_E_ARG, "fsa_mask_sum: keys must be 4-byte aligned");
  if (P > 0 && (!acc_in || !out)) return refuse(FA_E_ARG, "fsa_mask_sum: acc_in or out is NULL");
  if (!aligned16(acc_in) || !aligned16(out))
    return refuse(FA_E_ARG, "fsa_mask_sum: acc_in and out must be 16-byte aligned");
  if (acc_in != out && P > 0) {
    const uintptr_t a = (uintptr_t)acc_in, o = (uintptr_t)out, bytes = (uintptr_t)P * 4;
    if (a < o + bytes && o < a + bytes)
      return refuse(FA_E_ARG, "fsa_mask_sum: out overlaps acc_in without being the same pointer");
  }
  if (P == 0) return FA_OK;
  const int64_t nblk = (P + 15) / 16;
  FA_DEVICE_SCOPE("fsa_mask_sum", stream, out);
  FA_OPERAND("keys", keys, (uint64_t)M * 32);
  FA_OPERAND("acc_in", acc_in, (uint64_t)P * 4);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fsa_mask_sum: no CU count for device %d", fa_scope_device());
  int64_t g = (nblk + MS_THREADS - 1) / MS_THREADS;
  if (g > (int64_t)cus * FSA_MASK_GRID_PER_CU) g = (int64_t)cus * FSA_MASK_GRID_PER_CU;
  hipLaunchKernelGGL(k_mask_sum, dim3((unsigned)g), dim3(MS_THREADS), 0, (hipStream_t)stream, keys, n_add, n_sub,
                     nonce0, nonce1, nonce2, (uint32_t)(col0 / 16), nblk, P, acc_in, out);
  return check_launch("fsa_mask_sum");
}

extern "C" int64_t fsa_reduce_plan(int32_t cus, int32_t K, int64_t P, int64_t* plan_out, int32_t cap) {
  if (cus <= 0 || K < 0 || P < 0 || cap < 0 || (cap > 0 && !plan_out))
    return refuse(FA_E_ARG, "fsa_reduce_plan: bad arguments (cus=%d K=%d P=%lld cap=%d)", cus, K, (long long)P, cap);
  return strip_plan_export(cus, sum_strips(P), FSA_GEO, plan_out, cap);
}

extern "C" int fsa_reduce(const uint32_t* y, int64_t ld, int32_t n, int64_t P, const uint32_t* acc_in, uint32_t* out,
                          int32_t flags, fa_stream_t stream) {
  if (flags & ~FA_ACCUMULATE) return refuse(FA_E_ARG, "fsa_reduce: unknown flags %d (0 or FA_ACCUMULATE)", flags);
  if (n < 0 || P < 0 || ld < P)
    return refuse(FA_E_ARG, "fsa_reduce: ld=%lld < P=%lld, or negative n=%d / P", (long long)ld, (long long)P, n);
  if (ld % 64 != 0) return refuse(FA_E_ARG, "fsa_reduce: ld=%lld must be a multiple of 64 words", (long long)ld);
  if ((flags & FA_ACCUMULATE) && !acc_in) return refuse(FA_E_ARG, "fsa_reduce: FA_ACCUMULATE without acc_in");
  if (n == 0 && !(flags & FA_ACCUMULATE)) return refuse(FA_E_ARG, "fsa_reduce: n=0 rows with nothing to accumulate");
  if (n > 0 && !y) return refuse(FA_E_ARG, "fsa_reduce: y is NULL");
  if (!out) return refuse(FA_E_ARG, "fsa_reduce: out is NULL");
  if (!aligned16(y)) return refuse(FA_E_ARG, "fsa_reduce: y must be 16-byte aligned");
  if (!aligned16(out) || !aligned16(acc_in)) return refuse(FA_E_ARG, "fsa_reduce: out and acc_in must be 16-byte aligned");
  if (P == 0) return FA_OK;
  const int64_t P4 = (P + 3) / 4;
  if (P4 / (64 * FSA_WAVES) > 0x7fffffffLL) return refuse(FA_E_RANGE, "fsa_reduce: P too large");
  FA_DEVICE_SCOPE("fsa_reduce", stream, out);
  FA_OPERAND("y", y, n > 0 ? (uint64_t)((int64_t)(n - 1) * ld + P4 * 4) * 4 : 0);
  FA_OPERAND("acc_in", (flags & FA_ACCUMULATE) ? acc_in : nullptr, (uint64_t)P4 * 16);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fsa_reduce launch plan: no CU count for device %d", fa_scope_device());
  SumArgs r{};
  r.y = reinterpret_cast<const u4*>(y); r.ld4 = ld / 4; r.P4 = P4; r.P = P; r.n = n; r.flags = flags;
  r.acc_in = reinterpret_cast<const u4*>(acc_in); r.out = out;
  StripLaunch l[3];
  const int nl = strip_plan(cus, sum_strips(P), FSA_GEO, l);
  for (int i = 0; i < nl; ++i) {
    launch_level(r, l[i], (hipStream_t)stream);
    const int e = check_launch("fsa_reduce");
    if (e) return e;
  }
  return FA_OK;
}

extern "C" int fsa_finish(const uint32_t* sum, const float* last, int64_t P, int32_t frac_bits, int32_t mag_bits,
                          int32_t n, float* out, float* mirror, int64_t* out_of_range, fa_stream_t stream) {
  if (P < 0) return refuse(FA_E_ARG, "fsa_finish: negative P=%lld", (long long)P);
  if (!spec_ok(frac_bits, mag_bits))
    return refuse(FA_E_ARG, "fsa_finish: frac_bits=%d must be in [0, %d] and mag_bits=%d in [1, %d]", frac_bits,
                  FSA_MAX_FRAC_BITS, mag_bits, FSA_MAX_MAG_BITS);
  const int64_t B = (1LL << mag_bits) - 1;
  if (n < 1 || (int64_t)n * B > 0x7fffffffLL)
    return refuse(FA_E_ARG, "fsa_finish: n=%d arrivals must be >= 1 with n * (2^%d - 1) <= 2^31 - 1", n, mag_bits);
  if (!out_of_range) return refuse(FA_E_ARG, "fsa_finish: out_of_range is NULL");
  if ((uintptr_t)out_of_range & 7u) return refuse(FA_E_ARG, "fsa_finish: out_of_range must be 8-byte aligned");
  if (P > 0 && (!sum || !last || !out)) return refuse(FA_E_ARG, "fsa_finish: sum, last or out is NULL");
  if (!aligned16(sum) || !aligned16(last)) return refuse(FA_E_ARG, "fsa_finish: sum and last must be 16-byte aligned");
  if (!aligned16(out) || !aligned16(mirror)) return refuse(FA_E_ARG, "fsa_finish: out and mirror must be 16-byte aligned");
  const int64_t P4 = (P + 3) / 4;
  FA_DEVICE_SCOPE("fsa_finish", stream, out_of_range);
  FA_OPERAND("sum", sum, (uint64_t)P4 * 16);
  FA_OPERAND("last", last, (uint64_t)P4 * 16);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  FA_HOST_OK_OPERAND("mirror", mirror, (uint64_t)P * 4);
  FA_OPERAND("out_of_range", out_of_range, 8);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fsa_finish: no CU count for device %d", fa_scope_device());
  if (hipMemsetAsync(out_of_range, 0, 8, (hipStream_t)stream) != hipSuccess)
    return fail(FA_E_HIP, "fsa_finish: clearing out_of_range failed: %s", hipGetErrorString(hipGetLastError()));
  if (P == 0) return FA_OK;
  int64_t g = (P4 + 255) / 256;
  if (g > (int64_t)cus * 8) g = (int64_t)cus * 8;
  const double inv_scale = __builtin_bit_cast(double, (uint64_t)(1023 - frac_bits) << 52);  // 2^-f
  hipLaunchKernelGGL(k_secagg_finish, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const u4*>(sum), reinterpret_cast<const f4*>(last), P, inv_scale, (double)n,
                     (int64_t)n * B, out, mirror, out_of_range);
  return check_launch("fsa_finish");
}
