// sparse_reduce.hip — MI355X (gfx950) kernels of the top-k sparse delta-upload path (include/fedsparse.h):
//   * fs_reduce: the in-order fp32 column chain over client deltas staged as (index, value) rows.  A wave owns a tile
//     of FS_TILE columns of the chain in LDS and walks every row's segment of that tile in arrival order; the segment
//     bounds come from fs_row_offsets.  The LDS operations of one wave complete in order and the indices of a row are
//     unique, so the read-add-write per pair needs no atomic and no barrier, and the arrival order holds;
//   * fs_row_offsets, fs_check_rows: the per-row side data made when a row is staged;
//   * fs_reduce_plan: the launches fs_reduce makes, as a host-only function of the CU count;
//   * fs_topk_row: the executor-side handler, a radix select of the k-th largest magnitude and an ordered emit.
//
// Numerics: every fp32 op is rounded to nearest and never contracted into an FMA; the default denormal modes are
// kept, so subnormal values and sums survive.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fedsparse.h"
#include "fa_device.h"
#include "fa_common.h"

// Tuning knob (tools/sparse_reduce_measure.py per library, FEDAGG_LIB): the rows in flight.
#if defined(FS_ROWS_AHEAD) && (!defined(FA_TUNING) || !FA_TUNING)
#error "FS_ROWS_AHEAD is a tuning knob: build with -DFA_TUNING=1"
#endif
#ifndef FS_ROWS_AHEAD
#define FS_ROWS_AHEAD 16
#endif

namespace {

// ------------------------------------------------------------------------------------------------
// fs_reduce
// ------------------------------------------------------------------------------------------------
constexpr int FS_U = FS_ROWS_AHEAD;  // rows whose first 64 pairs of the segment are loaded ahead of their adds
constexpr int FS_TAIL = 4;       // 64-pair groups of a longer segment loaded ahead of their adds
constexpr int FS_WG_PER_CU = 8;  // workgroups (one wave, 16 KiB of LDS each) the plan puts on a CU: 128 of 160 KiB
static_assert(FS_TILE % 256 == 0 && FS_TILE * 4 * FS_WG_PER_CU <= 160 * 1024, "a CU's LDS holds the plan's tiles");
static_assert(64 % FS_U == 0, "a batch of 64 rows is walked FS_U rows at a time");

struct SparseArgs {
  const uint32_t* idx;
  const float* val;
  int64_t ldk;
  const int32_t* nnz;
  const int32_t* off;  // [boundary][row], row stride 1, boundary stride ldo
  int64_t ldo;
  const int32_t* rflags;
  int n;
  int flags;
  int64_t P;
  int64_t ntiles;
  const float* acc_in;
  float* out;
};

// the compiler keeps the LDS accesses of consecutive pairs in program order (they may alias); the hardware completes
// one wave's LDS operations in order
__device__ __forceinline__ void wave_order() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// one pair onto the tile: the index is an address only after the unsigned range test (a masked lane carries
// 0xFFFFFFFF, which no tile of a P <= 2^31 - 1 bucket holds)
__device__ __forceinline__ void add_pair(float* tile, uint32_t base, uint32_t i, float v) {
  const uint32_t c = i - base;
  if (c < (uint32_t)FS_TILE) tile[c] = tile[c] + v;
}

__device__ __forceinline__ void sparse_tile(const SparseArgs& r, int64_t t, int lane, float* tile) {
  const int64_t c0 = t * FS_TILE;
  const uint32_t base = (uint32_t)c0;
  const f4 z4 = f4{0.f, 0.f, 0.f, 0.f};
  f4* t4 = reinterpret_cast<f4*>(tile);
  const f4* ain = reinterpret_cast<const f4*>(r.acc_in);
  for (int i = lane; i < FS_TILE / 4; i += 64) {
    const int64_t p = c0 + 4 * i;
    t4[i] = ((r.flags & FA_ACCUMULATE) && p < r.P) ? ain[p >> 2] : z4;  // acc_in holds round_up(P, 4) floats
  }
  wave_order();

  const int32_t* o0 = r.off + t * r.ldo;
  const int32_t* o1 = o0 + r.ldo;
  for (int k0 = 0; k0 < r.n; k0 += 64) {
    // this lane's row of the batch: its segment [lo, hi) of the tile, clamped into the row whatever the offsets hold
    int lo = 0, hi = 0;
    if (k0 + lane < r.n) {
      const int k = k0 + lane;
      int cap = r.nnz[k];
      cap = cap < 0 ? 0 : ((int64_t)cap > r.ldk ? (int)r.ldk : cap);
      lo = o0[k];
      hi = o1[k];
      hi = hi < 0 ? 0 : (hi > cap ? cap : hi);
      lo = lo < 0 ? 0 : (lo > hi ? hi : lo);
      if (r.rflags[k] != 0) hi = lo;  // a flagged row: an empty segment for the whole wave
    }
    const int m = r.n - k0 < 64 ? r.n - k0 : 64;
    for (int u0 = 0; u0 < m; u0 += FS_U) {
      uint32_t ci[FS_U];
      float cv[FS_U];
      int slo[FS_U], shi[FS_U];
#pragma unroll
      for (int u = 0; u < FS_U; ++u) {  // (lanes of rows >= n hold lo = hi = 0)
        slo[u] = __builtin_amdgcn_readlane(lo, u0 + u);
        shi[u] = __builtin_amdgcn_readlane(hi, u0 + u);
        const int j = slo[u] + lane;
        const bool ok = j < shi[u];
        const int64_t at = (int64_t)(k0 + u0 + u) * r.ldk + j;
        ci[u] = ok ? __builtin_nontemporal_load(r.idx + at) : 0xFFFFFFFFu;
        cv[u] = ok ? __builtin_nontemporal_load(r.val + at) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < FS_U; ++u) {
        add_pair(tile, base, ci[u], cv[u]);
        wave_order();
        if (slo[u] + 64 < shi[u]) {  // wave-uniform: the rest of a segment longer than one group
          const int64_t row = (int64_t)(k0 + u0 + u) * r.ldk;
          for (int j0 = slo[u] + 64; j0 < shi[u]; j0 += 64 * FS_TAIL) {
            uint32_t ti[FS_TAIL];
            float tv[FS_TAIL];
#pragma unroll
            for (int g = 0; g < FS_TAIL; ++g) {
              const int j = j0 + 64 * g + lane;
              const bool ok = j < shi[u];
              ti[g] = ok ? __builtin_nontemporal_load(r.idx + row + j) : 0xFFFFFFFFu;
              tv[g] = ok ? __builtin_nontemporal_load(r.val + row + j) : 0.f;
            }
#pragma unroll
            for (int g = 0; g < FS_TAIL; ++g) {
              add_pair(tile, base, ti[g], tv[g]);
              wave_order();
            }
          }
        }
      }
    }
  }
  wave_order();

  for (int i = lane; i < FS_TILE / 4; i += 64) {
    const int64_t p = c0 + 4 * i;
    const f4 s = t4[i];
    if (p + 4 <= r.P) {
      *reinterpret_cast<f4*>(r.out + p) = s;
    } else if (p < r.P) {  // the last, partial float4 column: columns >= P are not written
      r.out[p] = s.x;
      if (p + 1 < r.P) r.out[p + 1] = s.y;
      if (p + 2 < r.P) r.out[p + 2] = s.z;
    }
  }
  wave_order();  // the tile is reused by this wave's next tile
}

// workgroup b (one wave) reduces tiles b, b + grid, ...
__global__ __launch_bounds__(64) void k_reduce_sparse(SparseArgs r) {
  __shared__ __attribute__((aligned(16))) float tile[FS_TILE];
  const int lane = threadIdx.x;
  for (int64_t t = blockIdx.x; t < r.ntiles; t += gridDim.x) sparse_tile(r, t, lane, tile);
}

// Launch plan: one launch.  Up to FS_WG_PER_CU tiles per CU are resident (LDS); a longer bucket runs on a capped
// grid whose workgroups walk the same number of tiles, the last round ragged.  K does not enter the plan.
struct SparseLaunch {
  int64_t tiles, per, grid;
};
int64_t sparse_tiles(int64_t P) { return (P + FS_TILE - 1) / FS_TILE; }
SparseLaunch sparse_plan(int64_t cus, int64_t P) {
  SparseLaunch l{sparse_tiles(P), 1, 0};
  const int64_t cap = cus * FS_WG_PER_CU;
  l.per = (l.tiles + cap - 1) / cap;
  if (l.per < 1) l.per = 1;
  l.grid = (l.tiles + l.per - 1) / l.per;
  return l;
}

// ------------------------------------------------------------------------------------------------
// fs_row_offsets, fs_check_rows
// ------------------------------------------------------------------------------------------------
constexpr int RO_THREADS = 256;
__device__ __forceinline__ int row_count(const int32_t* nnz, int row, int64_t ldk) {
  const int c = nnz[row];
  return c < 0 ? 0 : ((int64_t)c > ldk ? (int)ldk : c);
}

// thread (b, row): lower bound of b * FS_TILE in the row (row fastest: coalesced stores)
__global__ __launch_bounds__(RO_THREADS) void k_row_offsets(const uint32_t* __restrict__ idx, int64_t ldk,
                                                            const int32_t* __restrict__ nnz, int n, int64_t nb,
                                                            int32_t* __restrict__ off, int64_t ldo) {
  const int64_t t = (int64_t)blockIdx.x * RO_THREADS + threadIdx.x;
  if (t >= nb * n) return;
  const int row = (int)(t % n);
  const int64_t b = t / n;
  const uint64_t target = (uint64_t)b * FS_TILE;
  const uint32_t* r = idx + (int64_t)row * ldk;
  int lo = 0, hi = row_count(nnz, row, ldk);
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)r[mid] < target) lo = mid + 1; else hi = mid;
  }
  off[b * ldo + row] = lo;
}

constexpr int CK_THREADS = 256, CK_PER = 16;  // a block checks 4096 pairs of one row
__global__ __launch_bounds__(CK_THREADS) void k_check_rows(const uint32_t* __restrict__ idx, int64_t ldk,
                                                           const int32_t* __restrict__ nnz, int64_t P,
                                                           int32_t* __restrict__ flags) {
  const int row = blockIdx.y;
  const int raw = nnz[row];
  if (blockIdx.x == 0 && threadIdx.x == 0 && (raw < 0 || (int64_t)raw > ldk)) flags[row] = 1;
  const int c = row_count(nnz, row, ldk);
  const uint32_t* r = idx + (int64_t)row * ldk;
  const int64_t j0 = (int64_t)blockIdx.x * (CK_THREADS * CK_PER) + threadIdx.x;
  bool bad = false;
#pragma unroll 4
  for (int i = 0; i < CK_PER; ++i) {
    const int64_t j = j0 + (int64_t)i * CK_THREADS;
    if (j < c) {
      const uint32_t v = r[j];
      bad = bad || (uint64_t)v >= (uint64_t)P || (j > 0 && r[j - 1] >= v);
    }
  }
  if (bad) flags[row] = 1;  // (every writer stores the same value)
}

// ------------------------------------------------------------------------------------------------
// fs_topk_row
// ------------------------------------------------------------------------------------------------
// Workspace, in 32-bit words: the running prefix of tau (TK_PREFIX), the rank still looked for among the keys that
// match it (TK_KREM), the 256-bin histogram of a pass (TK_HIST), and from TK_CNT two words per tile of TK_TILE
// columns: (keys > tau, keys == tau), turned into exclusive prefixes by the scan.
constexpr int TK_PREFIX = 0, TK_KREM = 1, TK_HIST = 16, TK_CNT = 512;
constexpr int TK_THREADS = 256, TK_TILE = 4 * TK_THREADS;
constexpr int TK_SCAN = 1024;

int64_t topk_tiles(int64_t P) { return (P + TK_TILE - 1) / TK_TILE; }

__device__ __forceinline__ float delta_of(const float* x, const float* base, const float* rin, int64_t p) {
  float e = x[p];
  if (base) e = e - base[p];
  if (rin) e = e + rin[p];
  return e;
}
__device__ __forceinline__ uint32_t key_of(float e) { return __builtin_bit_cast(uint32_t, e) & 0x7fffffffu; }

__global__ __launch_bounds__(TK_THREADS) void k_topk_init(uint32_t* ws, uint32_t k) {
  ws[TK_HIST + threadIdx.x] = 0u;
  if (threadIdx.x == 0) {
    ws[TK_PREFIX] = 0u;
    ws[TK_KREM] = k;
  }
}

// histogram of the digit at `shift` over the keys whose higher bits equal the prefix's
__global__ __launch_bounds__(TK_THREADS) void k_topk_hist(const float* __restrict__ x, const float* __restrict__ base,
                                                          const float* __restrict__ rin, int64_t P, uint32_t* ws,
                                                          int shift) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const uint64_t want = (uint64_t)ws[TK_PREFIX] >> (shift + 8);
  for (int64_t p = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x; p < P; p += (int64_t)gridDim.x * TK_THREADS) {
    const uint32_t key = key_of(delta_of(x, base, rin, p));
    if (((uint64_t)key >> (shift + 8)) == want) atomicAdd(&h[(key >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&ws[TK_HIST + threadIdx.x], h[threadIdx.x]);
}

// the digit that holds the rank looked for, from the top bin down; clears the histogram for the next pass
__global__ __launch_bounds__(TK_THREADS) void k_topk_pick(uint32_t* ws, int shift) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = ws[TK_HIST + threadIdx.x];
  ws[TK_HIST + threadIdx.x] = 0u;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t krem = ws[TK_KREM];
    uint32_t above = 0u;
    int d = 255;
    for (; d > 0; --d) {
      if (above + h[d] >= krem) break;
      above += h[d];
    }
    ws[TK_PREFIX] |= (uint32_t)d << shift;
    ws[TK_KREM] = krem - above;
  }
}

// inclusive scan of one 64-bit value per thread over a block of N threads (two packed 32-bit counters)
template <int N>
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
#pragma unroll
  for (int d = 1; d < N; d <<= 1) {
    const uint64_t o = t >= d ? sh[t - d] : 0ull;
    __syncthreads();
    v += o;
    sh[t] = v;
    __syncthreads();
  }
  return v;
}

__global__ __launch_bounds__(TK_THREADS) void k_topk_count(const float* __restrict__ x, const float* __restrict__ base,
                                                           const float* __restrict__ rin, int64_t P, uint32_t* ws) {
  __shared__ uint32_t c[2];
  if (threadIdx.x < 2) c[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t tau = ws[TK_PREFIX];
  const int64_t p0 = (int64_t)blockIdx.x * TK_TILE + 4 * threadIdx.x;
  uint32_t gt = 0u, eq = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (p0 + i < P) {
      const uint32_t key = key_of(delta_of(x, base, rin, p0 + i));
      gt += key > tau;
      eq += key == tau;
    }
  if (gt) atomicAdd(&c[0], gt);
  if (eq) atomicAdd(&c[1], eq);
  __syncthreads();
  if (threadIdx.x < 2) ws[TK_CNT + 2 * (int64_t)blockIdx.x + threadIdx.x] = c[threadIdx.x];
}

// exclusive prefixes of the per-tile counts, in place (one workgroup)
__global__ __launch_bounds__(TK_SCAN) void k_topk_scan(uint32_t* ws, int64_t ntiles) {
  __shared__ uint64_t sh[TK_SCAN];
  uint32_t* cnt = ws + TK_CNT;
  uint64_t carry = 0ull;
  for (int64_t b = 0; b < ntiles; b += TK_SCAN) {
    const int64_t i = b + threadIdx.x;
    const uint64_t own = i < ntiles ? ((uint64_t)cnt[2 * i] << 32 | cnt[2 * i + 1]) : 0ull;
    const uint64_t inc = block_scan<TK_SCAN>(own, sh);
    const uint64_t ex = carry + inc - own;
    if (i < ntiles) {
      cnt[2 * i] = (uint32_t)(ex >> 32);
      cnt[2 * i + 1] = (uint32_t)ex;
    }
    carry += sh[TK_SCAN - 1];
    __syncthreads();
  }
}

// the kept pairs in index order: a tie is taken only while its rank among all ties is below the number still needed
__global__ __launch_bounds__(TK_THREADS) void k_topk_emit(const float* __restrict__ x, const float* __restrict__ base,
                                                          const float* rin, int64_t P, const uint32_t* __restrict__ ws,
                                                          uint32_t kcap, uint32_t* __restrict__ idx_out,
                                                          float* __restrict__ val_out, float* rout) {
  __shared__ uint64_t sh[TK_THREADS];
  const uint32_t tau = ws[TK_PREFIX], need = ws[TK_KREM];
  const uint32_t gbase = ws[TK_CNT + 2 * (int64_t)blockIdx.x], ebase = ws[TK_CNT + 2 * (int64_t)blockIdx.x + 1];
  const int64_t p0 = (int64_t)blockIdx.x * TK_TILE + 4 * threadIdx.x;
  float e[4];
  uint32_t key[4];
  uint32_t neq = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    e[i] = 0.f;
    key[i] = 0u;
    if (p0 + i < P) {
      e[i] = delta_of(x, base, rin, p0 + i);
      key[i] = key_of(e[i]);
      neq += key[i] == tau;
    }
  }
  uint32_t rank = ebase + (uint32_t)(block_scan<TK_THREADS>(neq, sh) - neq);
  __syncthreads();
  bool keep[4];
  uint32_t nk = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    keep[i] = false;
    if (p0 + i < P) {
      if (key[i] > tau) {
        keep[i] = true;
      } else if (key[i] == tau) {
        keep[i] = rank < need;
        ++rank;
      }
    }
    nk += keep[i];
  }
  uint32_t pos = gbase + (ebase < need ? ebase : need) + (uint32_t)(block_scan<TK_THREADS>(nk, sh) - nk);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (p0 + i < P) {
      if (keep[i]) {
        if (pos < kcap) {  // (always: exactly kcap columns are kept; the outputs hold kcap pairs)
          idx_out[pos] = (uint32_t)(p0 + i);
          val_out[pos] = e[i];
        }
        ++pos;
      }
      if (rout) rout[p0 + i] = keep[i] ? 0.f : e[i];
    }
}

int64_t topk_ws_bytes(int64_t P) { return ((TK_CNT + 2 * topk_tiles(P)) * 4 + 15) / 16 * 16; }

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedsparse.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t fs_abi_version(void) { return FS_ABI_VERSION; }

extern "C" int64_t fs_reduce_plan(int32_t cus, int32_t K, int64_t P, int64_t* plan_out, int32_t cap) {
  if (cus <= 0 || K < 0 || P < 0 || cap < 0 || (cap > 0 && !plan_out))
    return refuse(FA_E_ARG, "fs_reduce_plan: bad arguments (cus=%d K=%d P=%lld cap=%d)", cus, K, (long long)P, cap);
  if (P == 0) return 0;
  const SparseLaunch l = sparse_plan(cus, P);
  if (cap > 0) {
    plan_out[0] = FS_TILE;
    plan_out[1] = FS_U;
    plan_out[2] = 0;
    plan_out[3] = l.tiles;
    plan_out[4] = l.per;
    plan_out[5] = l.grid;
  }
  return 1;
}

static int check_rows_args(const char* what, const void* idx, int64_t ldk, const void* nnz, int32_t n, int64_t P) {
  if (n < 0 || P < 0 || ldk < 0)
    return refuse(FA_E_ARG, "%s: negative n=%d, P=%lld or ldk=%lld", what, n, (long long)P, (long long)ldk);
  if (P > 0x7fffffffLL) return refuse(FA_E_RANGE, "%s: P=%lld exceeds 2^31 - 1 columns", what, (long long)P);
  if (ldk % 4 != 0 || ldk > 0x40000000LL)  // (positions in a row, plus a wave's lanes, stay inside an int)
    return refuse(FA_E_ARG, "%s: ldk=%lld must be a multiple of 4, at most 2^30", what, (long long)ldk);
  if (n > 0 && (!idx || !nnz)) return refuse(FA_E_ARG, "%s: idx or nnz is NULL", what);
  if (!aligned16(idx)) return refuse(FA_E_ARG, "%s: idx must be 16-byte aligned", what);
  if (((uintptr_t)nnz & 3u) != 0) return refuse(FA_E_ARG, "%s: nnz must be 4-byte aligned", what);
  return FA_OK;
}

extern "C" int fs_row_offsets(const uint32_t* idx, int64_t ldk, const int32_t* nnz, int32_t n, int64_t P,
                              int32_t* offsets, int64_t ldo, fa_stream_t stream) {
  const int e0 = check_rows_args("fs_row_offsets", idx, ldk, nnz, n, P);
  if (e0) return e0;
  if (ldo < n) return refuse(FA_E_ARG, "fs_row_offsets: ldo=%lld < n=%d rows", (long long)ldo, n);
  if (!offsets) return refuse(FA_E_ARG, "fs_row_offsets: offsets is NULL");
  if (((uintptr_t)offsets & 3u) != 0) return refuse(FA_E_ARG, "fs_row_offsets: offsets must be 4-byte aligned");
  if (n == 0) return FA_OK;
  const int64_t nb = sparse_tiles(P) + 1;
  const int64_t grid = (nb * n + RO_THREADS - 1) / RO_THREADS;
  if (grid > 0x7fffffffLL) return refuse(FA_E_RANGE, "fs_row_offsets: n x boundaries too large");
  FA_DEVICE_SCOPE("fs_row_offsets", stream, offsets);
  FA_OPERAND("idx", idx, (uint64_t)n * ldk * 4);
  FA_OPERAND("nnz", nnz, (uint64_t)n * 4);
  FA_OPERAND("offsets", offsets, (uint64_t)((nb - 1) * ldo + n) * 4);
  hipLaunchKernelGGL(k_row_offsets, dim3((unsigned)grid), dim3(RO_THREADS), 0, (hipStream_t)stream, idx, ldk, nnz, n,
                     nb, offsets, ldo);
  return check_launch("fs_row_offsets");
}

extern "C" int fs_check_rows(const uint32_t* idx, int64_t ldk, const int32_t* nnz, int32_t n, int64_t P,
                             int32_t* flags, fa_stream_t stream) {
  const int e0 = check_rows_args("fs_check_rows", idx, ldk, nnz, n, P);
  if (e0) return e0;
  if (!flags) return refuse(FA_E_ARG, "fs_check_rows: flags is NULL");
  if (((uintptr_t)flags & 3u) != 0) return refuse(FA_E_ARG, "fs_check_rows: flags must be 4-byte aligned");
  if (n > 65535) return refuse(FA_E_RANGE, "fs_check_rows: n=%d exceeds 65535 rows per call", n);
  if (n == 0) return FA_OK;
  FA_DEVICE_SCOPE("fs_check_rows", stream, flags);
  FA_OPERAND("idx", idx, (uint64_t)n * ldk * 4);
  FA_OPERAND("nnz", nnz, (uint64_t)n * 4);
  FA_OPERAND("flags", flags, (uint64_t)n * 4);
  if (hipMemsetAsync(flags, 0, (size_t)n * 4, (hipStream_t)stream) != hipSuccess)
    return fail(FA_E_HIP, "fs_check_rows: clearing the flags failed: %s", hipGetErrorString(hipGetLastError()));
  const int64_t gx = (ldk + CK_THREADS * CK_PER - 1) / (CK_THREADS * CK_PER);
  hipLaunchKernelGGL(k_check_rows, dim3((unsigned)(gx > 0 ? gx : 1), (unsigned)n), dim3(CK_THREADS), 0,
                     (hipStream_t)stream, idx, ldk, nnz, P, flags);
  return check_launch("fs_check_rows");
}

extern "C" int fs_reduce(const uint32_t* idx, const float* val, int64_t ldk, const int32_t* nnz,
                         const int32_t* offsets, int64_t ldo, const int32_t* row_flags, int32_t n, int64_t P,
                         const float* acc_in, float* out, int32_t flags, fa_stream_t stream) {
  if (flags & ~FA_ACCUMULATE) return refuse(FA_E_ARG, "fs_reduce: unknown flags %d (0 or FA_ACCUMULATE)", flags);
  const int e0 = check_rows_args("fs_reduce", idx, ldk, nnz, n, P);
  if (e0) return e0;
  if (ldo < n) return refuse(FA_E_ARG, "fs_reduce: ldo=%lld < n=%d rows", (long long)ldo, n);
  if ((flags & FA_ACCUMULATE) && !acc_in) return refuse(FA_E_ARG, "fs_reduce: FA_ACCUMULATE without acc_in");
  if (n == 0 && !(flags & FA_ACCUMULATE)) return refuse(FA_E_ARG, "fs_reduce: n=0 rows with nothing to accumulate");
  if (n > 0 && (!val || !offsets || !row_flags)) return refuse(FA_E_ARG, "fs_reduce: val, offsets or row_flags is NULL");
  if (!out) return refuse(FA_E_ARG, "fs_reduce: out is NULL");
  if (!aligned16(val)) return refuse(FA_E_ARG, "fs_reduce: val must be 16-byte aligned");
  if ((((uintptr_t)offsets | (uintptr_t)row_flags) & 3u) != 0)
    return refuse(FA_E_ARG, "fs_reduce: offsets and row_flags must be 4-byte aligned");
  if (!aligned16(out) || !aligned16(acc_in)) return refuse(FA_E_ARG, "fs_reduce: out and acc_in must be 16-byte aligned");
  if (P == 0) return FA_OK;
  const int64_t nb = sparse_tiles(P) + 1, P4 = (P + 3) / 4;
  FA_DEVICE_SCOPE("fs_reduce", stream, out);
  FA_OPERAND("idx", idx, (uint64_t)n * ldk * 4);
  FA_OPERAND("val", val, (uint64_t)n * ldk * 4);
  FA_OPERAND("nnz", nnz, (uint64_t)n * 4);
  FA_OPERAND("offsets", offsets, n > 0 ? (uint64_t)((nb - 1) * ldo + n) * 4 : 0);
  FA_OPERAND("row_flags", row_flags, (uint64_t)n * 4);
  FA_OPERAND("acc_in", (flags & FA_ACCUMULATE) ? acc_in : nullptr, (uint64_t)P4 * 16);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fs_reduce launch plan: no CU count for device %d", fa_scope_device());
  const SparseLaunch l = sparse_plan(cus, P);
  SparseArgs r{};
  r.idx = idx; r.val = val; r.ldk = ldk; r.nnz = nnz; r.off = offsets; r.ldo = ldo; r.rflags = row_flags;
  r.n = n; r.flags = flags; r.P = P; r.ntiles = l.tiles; r.acc_in = acc_in; r.out = out;
  hipLaunchKernelGGL(k_reduce_sparse, dim3((unsigned)l.grid), dim3(64), 0, (hipStream_t)stream, r);
  return check_launch("fs_reduce");
}

extern "C" int64_t fs_topk_workspace(int64_t P) {
  if (P < 0) return refuse(FA_E_ARG, "fs_topk_workspace: negative P=%lld", (long long)P);
  return topk_ws_bytes(P);
}

extern "C" int fs_topk_row(const float* x, const float* base, const float* r_in, int64_t P, int64_t k,
                           void* workspace, uint32_t* idx_out, float* val_out, float* r_out, fa_stream_t stream) {
  if (P < 0 || k < 1) return refuse(FA_E_ARG, "fs_topk_row: negative P=%lld or k=%lld < 1", (long long)P, (long long)k);
  if (P > 0x7fffffffLL) return refuse(FA_E_RANGE, "fs_topk_row: P=%lld exceeds 2^31 - 1 columns", (long long)P);
  if (P == 0) return FA_OK;
  if (!x || !workspace || !idx_out || !val_out)
    return refuse(FA_E_ARG, "fs_topk_row: x, workspace, idx_out or val_out is NULL");
  if (!aligned16(x) || !aligned16(base) || !aligned16(r_in) || !aligned16(r_out) || !aligned16(workspace) ||
      !aligned16(idx_out) || !aligned16(val_out))
    return refuse(FA_E_ARG, "fs_topk_row: every operand must be 16-byte aligned");
  if (k > P) k = P;
  const int64_t nt = topk_tiles(P);
  FA_DEVICE_SCOPE("fs_topk_row", stream, idx_out);
  FA_OPERAND("x", x, (uint64_t)P * 4);
  FA_OPERAND("base", base, (uint64_t)P * 4);
  FA_OPERAND("r_in", r_in, (uint64_t)P * 4);
  FA_OPERAND("workspace", workspace, (uint64_t)topk_ws_bytes(P));
  FA_OPERAND("idx_out", idx_out, (uint64_t)k * 4);
  FA_OPERAND("val_out", val_out, (uint64_t)k * 4);
  FA_OPERAND("r_out", r_out, (uint64_t)P * 4);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* ws = static_cast<uint32_t*>(workspace);
  const int64_t hb = (P + TK_THREADS * 8 - 1) / (TK_THREADS * 8);
  const dim3 hgrid((unsigned)(hb < 2048 ? hb : 2048)), blk(TK_THREADS);
  hipLaunchKernelGGL(k_topk_init, dim3(1), blk, 0, st, ws, (uint32_t)k);
  for (int shift = 24; shift >= 0; shift -= 8) {  // the 31 key bits, 8 at a time from the top
    hipLaunchKernelGGL(k_topk_hist, hgrid, blk, 0, st, x, base, r_in, P, ws, shift);
    hipLaunchKernelGGL(k_topk_pick, dim3(1), blk, 0, st, ws, shift);
  }
  hipLaunchKernelGGL(k_topk_count, dim3((unsigned)nt), blk, 0, st, x, base, r_in, P, ws);
  hipLaunchKernelGGL(k_topk_scan, dim3(1), dim3(TK_SCAN), 0, st, ws, nt);
  hipLaunchKernelGGL(k_topk_emit, dim3((unsigned)nt), blk, 0, st, x, base, r_in, P, ws, (uint32_t)k, idx_out,
                     val_out, r_out);
  return check_launch("fs_topk_row");
}
