// bulyan.hip — MI355X (gfx950) kernels of Bulyan (include/fedbulyan.h):
//   * fbl_select: Krum iterated theta times in K-space — every row's distances sorted once (k_bulyan_sort), then one
//                 small launch per iteration (k_bulyan_iter) that re-derives the previous pick, rebuilds the removed
//                 set and re-adds the surviving head of its sorted row; no workgroup ever waits on another;
//   * fbl_reduce: per column the mean of the beta selected values closest to their median, in ONE kernel (k_bulyan)
//                 whose two selections run on register-resident keys with neither a barrier nor an LDS atomic;
//   * fbl_plan:   the launch fbl_reduce makes, as a host-only function of the CU count.
//
// Numerics: every fp32 op is rounded to nearest and never contracted into an FMA; the default denormal modes are
// kept (fp32 denormals are not flushed); the division is the IEEE one.  The selections are integer arithmetic on order
// keys: which lane counts which row never reaches a float.  The scores are sequential fp64 adds by one lane.
//
// k_bulyan, one tile of theta rows x W columns (W = 2^wl <= 64, geo_of), in four steps:
//   load    through sel, coalesced: every lane issues 8 float4 non-temporal loads before it stores the first key; the
//           selected rows are read from HBM once.  The keys go to LDS transposed into sub-tiles of N = 64 / G columns,
//           [W / N][theta][N] words: sub-tile `sub` is what ONE wave works on in one pass.
//   select  G lanes of one wave own a column (G = 16, 32, 64 by theta); lane g of them holds rows [g R, g R + R) as
//           keys in R registers (R = 5, 17, 33, 65: compile-time, fully unrolled, no scratch; rows >= theta are the
//           largest key and sit behind every real row in rank and in arrival order).  A selection is a 32-step
//           bisection on the key bits: candidate = prefix | bit, every lane counts its register keys below it
//           (v_cmp + add-with-carry per key), the count is summed over the column's lanes by a butterfly inside the
//           wave, and the bit stays when count <= rank.  Where a wave is one column (G = 64) the candidate is
//           wave-uniform and the compare mask is counted on the scalar unit (ballot, then a scalar population count):
//           no cross-lane step at all.  The median's bisection gives med; the registers are rewritten in place as
//           ekey = bits(|v - med|) (the keys themselves stay in LDS); the same bisection gives cut and, from the count
//           at the last accepted bit, the number of keys below it.  4 waves x N columns per pass, W / (4 N) passes.
//   mark    ties at cut take their arrival-order rank from an exclusive scan of the per-lane tie counts over the
//           column's lanes (slices are contiguous in r, so lane order is arrival order).  A kept row's LDS word becomes
//           its float again, a dropped one -0.0f; with `kept`, the N lanes that hold a row add their kept flags inside the
//           wave and one of them adds the sum to the row's LDS counter.
//   chain   lane c < W adds column c's theta words in order of r, starting from -0.0f.  -0.0f + v has the bits of v
//           for every v (round to nearest, denormals kept), so this IS "the first kept value, then + every later kept
//           one".  Passing the chain from lane to lane instead would execute the same theta dependent adds as
//           full-wave instructions for N columns at a time; from LDS one wave chains W columns at once, W / N times
//           fewer issue slots, while the CU's second workgroup selects.
// The only workgroup barriers are after the load, before the chain and before the next tile's load.
//
// Banks.  R is odd.  The 64 lanes of a wave read, for register i, the words (g R + i) N + c of their sub-tile
// (c < N): g R N mod 64 takes G = 64 / N distinct multiples of N, so the 64 addresses fall into 64 distinct banks.
//
// Registers and scratch: the compiler's counts are in DESIGN.md.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/fedbulyan.h"
#include "fa_device.h"
#include "fa_common.h"

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int FBL_LANES = 256;
constexpr int FBL_U = 8;           // float4 loads a lane has in flight
constexpr int FBL_WORDS = 20480;   // 80 KiB: the largest LDS allocation, two workgroups per CU
constexpr int FBL_MAX_THETA = 4096;
static_assert(FBL_MAX_THETA * (4 + 1) <= FBL_WORDS && FBL_MAX_THETA <= 64 * 65 && FBL_MAX_THETA == FK_MAX_K,
              "the largest round fits the narrowest tile and the deepest instantiation");

// LDS words an instantiation allocates (static): its largest theta at the widest tile, inside FBL_WORDS
constexpr int lds_words(int G, int R) { return G * R * 65 < FBL_WORDS ? G * R * 65 : FBL_WORDS; }

struct BulGeo {
  int G, R;  // lanes per column, rows per lane
  int wl;    // log2 W
  int wgs;   // workgroups per CU the grid is planned for: what LDS and registers leave room for
};

BulGeo geo_of(int theta) {
  BulGeo g;
  if (theta <= 16 * 5) { g.G = 16; g.R = 5; g.wgs = 4; }  // 20.3 KiB and 86 VGPRs
  else if (theta <= 16 * 17) { g.G = 16; g.R = 17; g.wgs = 2; }
  else if (theta <= 32 * 33) { g.G = 32; g.R = 33; g.wgs = 2; }
  else { g.G = 64; g.R = 65; g.wgs = 1; }  // 303 registers: one wave per SIMD
  const int C = FBL_LANES / g.G;  // columns of one pass
  g.wl = 6;
  while ((1 << g.wl) > C && (int64_t)theta * ((1 << g.wl) + 1) > FBL_WORDS) --g.wl;
  return g;
}

struct BulArgs {
  const f4* x;     // the rows, in float4 columns
  int64_t ld4;     // row stride in float4 columns
  int64_t P4;      // float4 columns to read, ceil(P / 4)
  int64_t P;       // columns to write
  int64_t ntiles;  // workgroup b takes tiles b, b + grid, ...
  const int* sel;
  const int* n_sel;
  const float* last;
  int K, theta, beta, wl;
  float denom;     // float(beta)
  float* out;
  float* mirror;
  unsigned long long* kept;  // [K] or NULL
};

__device__ __forceinline__ uint32_t key_of(float v) {
  const uint32_t b = __float_as_uint(v);
  const uint32_t k = (b >> 31) ? ~b : (b | 0x80000000u);
  return v != v ? 0xFFFFFFFFu : k;
}
// the float of a key; every NaN comes back as 0x7FFFFFFF (which NaN is not part of the contract)
__device__ __forceinline__ uint32_t bits_of(uint32_t key) { return (key >> 31) ? (key & 0x7FFFFFFFu) : ~key; }

// how many of the column's keys are below cand: this lane's R registers, then the column's G lanes (N columns a wave)
template <int G, int R>
__device__ __forceinline__ uint32_t count_below(const uint32_t (&k)[R], uint32_t cand) {
  uint32_t c = 0;
  if constexpr (G == 64) {  // cand is wave-uniform: the mask of every compare is counted on the scalar unit
#pragma unroll
    for (int i = 0; i < R; ++i) c += (uint32_t)__popcll(__ballot(k[i] < cand));
  } else {
#pragma unroll
    for (int i = 0; i < R; ++i) c += k[i] < cand ? 1u : 0u;
#pragma unroll
    for (int m = 64 / G; m < 64; m <<= 1) c += (uint32_t)__shfl_xor((int)c, m, 64);
  }
  return c;
}

// the key of ascending rank `rank` (0-based) among the column's keys; below <- how many keys are smaller
template <int G, int R>
__device__ __forceinline__ uint32_t select_rank(const uint32_t (&k)[R], uint32_t rank, uint32_t& below) {
  uint32_t prefix = 0;
  below = 0;
#pragma unroll 1
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t cand = prefix | (1u << bit);
    const uint32_t c = count_below<G, R>(k, cand);
    if (c <= rank) {  // the rank's key is >= cand
      prefix = cand;
      below = c;
    }
  }
  return prefix;
}

template <int G, int R>
__global__ __launch_bounds__(FBL_LANES) void k_bulyan(BulArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[lds_words(G, R)];
  constexpr int N = 64 / G;  // columns of a wave per pass
  constexpr int C = 4 * N;   // columns of the workgroup per pass
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int cw = lane % N, g = lane / N;
  const int theta = a.theta, W = 1 << a.wl;
  if (*a.n_sel != theta) {  // a refused round: the model stays as it was
    for (int64_t tl = blockIdx.x; tl < a.ntiles; tl += gridDim.x) {
      const int64_t p = (tl << a.wl) + tid;
      if (tid < W && p < a.P) {
        const float l = a.last[p];
        a.out[p] = l;
        if (a.mirror) a.mirror[p] = l;
      }
    }
    return;
  }
  uint32_t* tile = lds;              // [W / N][theta][N]
  uint32_t* cnt = lds + theta * W;   // [theta]
  const bool counting = a.kept != nullptr;
  if (counting)
    for (int i = tid; i < theta; i += FBL_LANES) cnt[i] = 0u;  // (the load's barrier comes before its use)
  const int wl4 = a.wl - 2;     // a row of the tile is 2^wl4 float4 columns
  const int n4 = theta << wl4;  // float4 words of the tile
  const f4 z4 = f4{0.f, 0.f, 0.f, 0.f};
  const uint32_t rank_med = (uint32_t)(theta - 1) >> 1, rank_cut = (uint32_t)a.beta - 1u;

  for (int64_t tl = blockIdx.x; tl < a.ntiles; tl += gridDim.x) {
    // ---- load: float4 word i of the tile is selected row i >> wl4, float4 column (tl << wl4) + (i & mask) -------
    const int64_t col4 = tl << wl4;
    for (int base = tid; base < n4; base += FBL_LANES * FBL_U) {
      int src[FBL_U];
      f4 v[FBL_U];
#pragma unroll
      for (int u = 0; u < FBL_U; ++u) {
        const int i = base + FBL_LANES * u;
        const bool ok = i < n4 && col4 + (i & ((1 << wl4) - 1)) < a.P4;
        src[u] = ok ? a.sel[i >> wl4] : -1;
      }
#pragma unroll
      for (int u = 0; u < FBL_U; ++u) {
        const int i = base + FBL_LANES * u;
        const bool ok = (unsigned)src[u] < (unsigned)a.K;  // never a row outside the staging
        v[u] = ok ? __builtin_nontemporal_load(a.x + (int64_t)src[u] * a.ld4 + col4 + (i & ((1 << wl4) - 1))) : z4;
      }
#pragma unroll
      for (int u = 0; u < FBL_U; ++u) {
        const int i = base + FBL_LANES * u;
        if (i < n4) {
          const int row = i >> wl4, c0 = (i & ((1 << wl4) - 1)) * 4;
          if constexpr (N == 4) {
            *reinterpret_cast<u4*>(tile + ((c0 >> 2) * theta + row) * 4) =
                u4{key_of(v[u][0]), key_of(v[u][1]), key_of(v[u][2]), key_of(v[u][3])};
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[(((c0 + e) / N) * theta + row) * N + (c0 + e) % N] = key_of(v[u][e]);
          }
        }
      }
    }
    __syncthreads();

    // ---- select and mark: a wave works on sub-tile ps * 4 + wave, alone ------------------------------------------
    for (int ps = 0; ps < W / C; ++ps) {
      const int sub = ps * 4 + wave;
      uint32_t* my = tile + sub * theta * N + cw;  // row r of this lane's column: my[r * N]
      const bool live = (tl << a.wl) + sub * N + cw < a.P;  // a column at or past P: nothing of it is counted
      uint32_t k[R];
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int r = g * R + i;
        k[i] = r < theta ? my[r * N] : 0xFFFFFFFFu;
      }
      uint32_t below;
      const float med = __uint_as_float(bits_of(select_rank<G, R>(k, rank_med, below)));
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const float e = fabsf(__uint_as_float(bits_of(k[i])) - med);
        k[i] = (e != e || g * R + i >= theta) ? 0xFFFFFFFFu : __float_as_uint(e);
      }
      const uint32_t cut = select_rank<G, R>(k, rank_cut, below);
      const uint32_t n_cut = (uint32_t)a.beta - below;  // rows EQUAL to cut that are kept, in 1..
      uint32_t ties = 0;
#pragma unroll
      for (int i = 0; i < R; ++i) ties += k[i] == cut ? 1u : 0u;
      uint32_t before = ties;  // inclusive scan over the column's lanes, then made exclusive
#pragma unroll
      for (int d = 1; d < G; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)before, d * N, 64);
        if (g >= d) before += up;
      }
      before -= ties;
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int r = g * R + i;
        const bool eq = k[i] == cut;
        const bool keep = k[i] < cut || (eq && before < n_cut);
        before += eq ? 1u : 0u;
        if (r < theta) my[r * N] = keep ? bits_of(my[r * N]) : 0x80000000u;
        if (counting) {  // the N lanes of a row add up inside the wave: one LDS add per row, wave and pass
          uint32_t n = (live && keep && r < theta) ? 1u : 0u;
#pragma unroll
          for (int m = 1; m < N; m <<= 1) n += (uint32_t)__shfl_xor((int)n, m, 64);
          if (cw == 0 && n) atomicAdd(&cnt[r], n);  // integer counts: any order gives the same values
        }
      }
    }
    __syncthreads();

    // ---- chain and write: one lane per column, rows in order of r -------------------------------------------------
    const int64_t p = (tl << a.wl) + tid;
    if (tid < W && p < a.P) {
      const uint32_t* col = tile + (tid / N) * theta * N + tid % N;
      float chain = -0.0f;
#pragma unroll 8
      for (int r = 0; r < theta; ++r) chain = chain + __uint_as_float(col[r * N]);
      const float m = __fdiv_rn(chain, a.denom);
      a.out[p] = m;
      if (a.mirror) a.mirror[p] = m;
    }
    __syncthreads();  // the next tile's load overwrites the tile
  }
  if (counting) {
    for (int i = tid; i < theta; i += FBL_LANES) {
      const uint32_t n = cnt[i];
      const int row = a.sel[i];
      if (n && (unsigned)row < (unsigned)a.K) atomicAdd(&a.kept[row], (unsigned long long)n);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// fbl_select
// ------------------------------------------------------------------------------------------------
// One workgroup per row i: the K - 1 pairs (dist2, j) go to LDS, padded with (+inf, INT_MAX) to n (a power of two),
// and are sorted ascending by (dist2, j) — k_krum_scores's bitonic sort, carrying the index.  dist2 is never NaN and
// never -0, so the order is total; which of two equal distances comes first cannot change a sum of the smallest m.
__global__ __launch_bounds__(256) void k_bulyan_sort(const double* __restrict__ gram, int K, int n,
                                                     double* __restrict__ sd_out, int* __restrict__ sj_out) {
  extern __shared__ double sd[];  // [n] distances, then [n] neighbours
  int* sj = reinterpret_cast<int*>(sd + n);
  const int i = blockIdx.x;
  const double gii = gram[(int64_t)i * K + i];
  for (int s = threadIdx.x; s < n; s += 256) {
    double d = INFINITY;
    int j = 0x7FFFFFFF;
    if (s < K - 1) {
      j = s < i ? s : s + 1;
      const double v = (gii + gram[(int64_t)j * K + j]) - 2.0 * gram[(int64_t)i * K + j];
      d = v != v ? (double)INFINITY : (v > 0.0 ? v : 0.0);
    }
    sd[s] = d;
    sj[s] = j;
  }
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int s = threadIdx.x; s < n; s += 256) {
        const int o = s ^ j;
        if (o > s) {
          const double da = sd[s], db = sd[o];
          const int ja = sj[s], jb = sj[o];
          const bool up = (s & k) == 0;
          const bool gt = da > db || (da == db && ja > jb);
          const bool lt = da < db || (da == db && ja < jb);
          if (up ? gt : lt) {
            sd[s] = db; sd[o] = da;
            sj[s] = jb; sj[o] = ja;
          }
        }
      }
      __syncthreads();
    }
  const int64_t row = (int64_t)i * (K - 1);
  for (int s = threadIdx.x; s < K - 1; s += 256) {
    sd_out[row + s] = sd[s];
    sj_out[row + s] = sj[s];
  }
}

struct IterArgs {
  const double* sd;  // [K][K - 1] sorted distances
  const int* sj;     // [K][K - 1] their neighbours
  double* score;     // [2][K]: iteration s writes half s & 1; a removed row's score is -1
  int* picks;        // [theta]
  int* sel;          // [theta]   (written by the closing launch)
  int* n_sel;
  int K, f, theta, s;
};

// lexicographic (score, row) minimum of two candidates; row INT_MAX: none
__device__ __forceinline__ void take_min(double& bs, int& bi, double s, int i) {
  if (i != 0x7FFFFFFF && (bi == 0x7FFFFFFF || s < bs || (s == bs && i < bi))) {
    bs = s;
    bi = i;
  }
}

// Launch s of theta + 1, grid K (the closing launch s = theta: grid 1).  Every workgroup rebuilds the removed set:
// picks[0 .. s - 2] from memory (recorded by earlier launches) and pick s - 1 as the argmin of the previous launch's
// scores, which workgroup 0 records.  Then the workgroup of a remaining row i scores it against R_s.
__global__ __launch_bounds__(256) void k_bulyan_iter(IterArgs a) {
  __shared__ double cd[FK_MAX_K];          // the compacted distances
  __shared__ unsigned char gone[FK_MAX_K]; // the removed set
  __shared__ double ws[4];
  __shared__ int wi[4];
  __shared__ int part[256];
  __shared__ int stopped;
  const int tid = threadIdx.x, K = a.K, s = a.s, i = blockIdx.x;
  for (int k = tid; k < K; k += 256) gone[k] = 0;
  if (tid == 0) stopped = 0;
  __syncthreads();
  if (s > 0) {
    for (int j = tid; j < s - 1; j += 256) {
      const int p = a.picks[j];
      if (p < 0) stopped = 1;  // (every writer writes the same value)
      else gone[p] = 1;
    }
    const double* prev = a.score + (int64_t)((s - 1) & 1) * K;
    double bs = 0.0;
    int bi = 0x7FFFFFFF;
    for (int k = tid; k < K; k += 256) {
      const double v = prev[k];
      if (v >= 0.0) take_min(bs, bi, v, k);  // (a removed row's -1 is skipped; a score is never NaN)
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double os = __shfl_xor(bs, m, 64);
      const int oi = __shfl_xor(bi, m, 64);
      take_min(bs, bi, os, oi);
    }
    if ((tid & 63) == 0) {
      ws[tid >> 6] = bs;
      wi[tid >> 6] = bi;
    }
    __syncthreads();  // (also: stopped and gone of the recorded picks)
    bs = ws[0];
    bi = wi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) take_min(bs, bi, ws[w], wi[w]);
    const bool finite = bi != 0x7FFFFFFF && bs < (double)INFINITY;
    const int pick = (stopped || !finite) ? -1 : bi;
    __syncthreads();  // every lane has read `stopped` before it changes
    if (tid == 0) {
      if (pick < 0) stopped = 1;
      else gone[pick] = 1;
      if (i == 0) a.picks[s - 1] = pick;
    }
    __syncthreads();
  }
  if (s == a.theta) {  // the closing launch: sel <- the removed set in ascending order, then -1; n_sel <- its size
    const int chunk = (K + 255) / 256;
    const int k0 = tid * chunk < K ? tid * chunk : K, k1 = k0 + chunk < K ? k0 + chunk : K;
    int n = 0;
    for (int k = k0; k < k1; ++k) n += gone[k];
    part[tid] = n;
    __syncthreads();
    int pos = 0, total = 0;
    for (int t = 0; t < 256; ++t) {
      pos += t < tid ? part[t] : 0;
      total += part[t];
    }
    for (int k = k0; k < k1; ++k)
      if (gone[k] && pos < a.theta) a.sel[pos++] = k;
    for (int t = total + tid; t < a.theta; t += 256) a.sel[t] = -1;
    if (tid == 0) *a.n_sel = total;
    return;
  }
  double* cur = a.score + (int64_t)(s & 1) * K;
  if (gone[i] || stopped) {  // a removed row; or the picks have run out: no score is finite any more
    if (tid == 0) cur[i] = gone[i] ? -1.0 : (double)INFINITY;
    return;
  }
  // the first m surviving distances of the sorted row, compacted in order
  const int m = K - s - a.f - 2, L = K - 1;
  const int64_t row = (int64_t)i * L;
  const int chunk = (L + 255) / 256;
  const int q0 = tid * chunk < L ? tid * chunk : L, q1 = q0 + chunk < L ? q0 + chunk : L;
  int n = 0;
  for (int q = q0; q < q1; ++q) n += gone[a.sj[row + q]] ? 0 : 1;
  part[tid] = n;
  __syncthreads();
  int pos = 0;
  for (int t = 0; t < tid; ++t) pos += part[t];
  for (int q = q0; q < q1 && pos < m; ++q)
    if (!gone[a.sj[row + q]]) cd[pos++] = a.sd[row + q];
  __syncthreads();
  if (tid == 0) {
    double sc = 0.0;
    for (int q = 0; q < m; ++q) sc = sc + cd[q];
    cur[i] = sc;
  }
}

int check_theta(const char* who, int32_t theta, int64_t P) {
  if (P < 0) return refuse(FA_E_ARG, "%s: negative P=%lld", who, (long long)P);
  if (theta < 1 || theta > FBL_MAX_THETA)
    return refuse(FA_E_ARG, "%s: theta=%d must satisfy 1 <= theta <= %d (FK_MAX_K)", who, theta, FBL_MAX_THETA);
  return 0;
}

int64_t select_bytes(int64_t K) { return K * (K - 1) * 12 + 2 * K * 8 + 8; }
int64_t sorted_j_offset(int64_t K) { return K * (K - 1) * 8 + 2 * K * 8; }

bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

template <int G, int R>
void launch_reduce(const BulArgs& a, unsigned grid, hipStream_t st) {
  hipLaunchKernelGGL((k_bulyan<G, R>), dim3(grid), dim3(FBL_LANES), 0, st, a);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedbulyan.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t fbl_abi_version(void) { return FBL_ABI_VERSION; }

extern "C" int64_t fbl_select_workspace_bytes(int32_t K) {
  if (K < 1 || K > FK_MAX_K)
    return refuse(FA_E_ARG, "fbl_select_workspace_bytes: K=%d must satisfy 1 <= K <= %d (FK_MAX_K)", K, FK_MAX_K);
  return select_bytes(K);
}

extern "C" int fbl_select(const double* gram, int32_t K, int32_t f, int32_t* picks, int32_t* sel, int32_t* n_sel,
                          void* workspace, int64_t workspace_bytes, fa_stream_t stream) {
  if (K < 1 || K > FK_MAX_K)
    return refuse(FA_E_ARG, "fbl_select: K=%d must satisfy 1 <= K <= %d (FK_MAX_K)", K, FK_MAX_K);
  if (f < 0 || 4 * (int64_t)f + 3 > K)
    return refuse(FA_E_ARG, "fbl_select: f=%d needs 0 <= f and 4f + 3 <= K=%d", f, K);
  if (!gram || !picks || !sel || !n_sel || !workspace)
    return refuse(FA_E_ARG, "fbl_select: gram, picks, sel, n_sel or workspace is NULL");
  if (!aligned8(gram) || !aligned8(workspace))
    return refuse(FA_E_ARG, "fbl_select: gram and workspace must be 8-byte aligned");
  if (!aligned4(picks) || !aligned4(sel) || !aligned4(n_sel))
    return refuse(FA_E_ARG, "fbl_select: picks, sel and n_sel must be 4-byte aligned");
  const int64_t need = select_bytes(K);
  if (workspace_bytes < need)
    return refuse(FA_E_ARG, "fbl_select: workspace of %lld bytes, K=%d needs %lld (fbl_select_workspace_bytes)",
                  (long long)workspace_bytes, K, (long long)need);
  const int theta = K - 2 * f - 2;
  FA_DEVICE_SCOPE("fbl_select", stream, picks);
  FA_OPERAND("gram", gram, (uint64_t)K * K * 8);
  FA_OPERAND("picks", picks, (uint64_t)theta * 4);
  FA_OPERAND("sel", sel, (uint64_t)theta * 4);
  FA_OPERAND("n_sel", n_sel, 4);
  FA_OPERAND("workspace", workspace, (uint64_t)need);
  hipStream_t st = (hipStream_t)stream;
  IterArgs a{};
  a.sd = (const double*)workspace;
  a.score = (double*)workspace + (int64_t)K * (K - 1);
  int* sj = reinterpret_cast<int*>((char*)workspace + sorted_j_offset(K));
  a.sj = sj;
  a.picks = picks; a.sel = sel; a.n_sel = n_sel;
  a.K = K; a.f = f; a.theta = theta;
  int n = 2;
  while (n < K - 1) n <<= 1;
  hipLaunchKernelGGL(k_bulyan_sort, dim3((unsigned)K), dim3(256), (size_t)n * 12, st, gram, (int)K, n,
                     (double*)workspace, sj);
  if (const int e = check_launch("fbl_select (sort)")) return e;
  for (int s = 0; s <= theta; ++s) {
    a.s = s;
    hipLaunchKernelGGL(k_bulyan_iter, dim3(s < theta ? (unsigned)K : 1u), dim3(256), 0, st, a);
    if (const int e = check_launch("fbl_select (iteration)")) return e;
  }
  return FA_OK;
}

extern "C" int fbl_plan(int32_t cus, int32_t theta, int64_t P, int64_t* plan_out) {
  if (cus <= 0 || !plan_out) return refuse(FA_E_ARG, "fbl_plan: bad arguments (cus=%d)", cus);
  if (const int e = check_theta("fbl_plan", theta, P)) return e;
  const BulGeo g = geo_of(theta);
  const int64_t W = 1 << g.wl, tiles = (P + W - 1) / W;
  plan_out[0] = g.G;
  plan_out[1] = g.R;
  plan_out[2] = W;
  plan_out[3] = W * g.G / FBL_LANES;
  plan_out[4] = (int64_t)lds_words(g.G, g.R) * 4;
  plan_out[5] = tiles;
  plan_out[6] = tiles < g.wgs * (int64_t)cus ? tiles : g.wgs * (int64_t)cus;
  return FA_OK;
}

extern "C" int fbl_reduce(const float* x, int64_t ld, int32_t K, int64_t P, const int32_t* sel, const int32_t* n_sel,
                          int32_t theta, int32_t beta, const float* last, float* out, float* mirror, int64_t* kept,
                          int32_t cus, fa_stream_t stream) {
  if (const int e = check_theta("fbl_reduce", theta, P)) return e;
  if (K < theta || K > FK_MAX_K)
    return refuse(FA_E_ARG, "fbl_reduce: K=%d must satisfy theta=%d <= K <= %d (FK_MAX_K)", K, theta, FK_MAX_K);
  if (beta < 1 || beta > theta) return refuse(FA_E_ARG, "fbl_reduce: beta=%d needs 1 <= beta <= theta=%d", beta, theta);
  if (cus < 0) return refuse(FA_E_ARG, "fbl_reduce: negative cus=%d", cus);
  if (ld < P) return refuse(FA_E_ARG, "fbl_reduce: ld=%lld < P=%lld", (long long)ld, (long long)P);
  if (ld % 4 != 0) return refuse(FA_E_ARG, "fbl_reduce: ld=%lld must be a multiple of 4 elements", (long long)ld);
  if (!x || !sel || !n_sel || !last || !out) return refuse(FA_E_ARG, "fbl_reduce: x, sel, n_sel, last or out is NULL");
  if (!aligned16(x) || !aligned16(last)) return refuse(FA_E_ARG, "fbl_reduce: x and last must be 16-byte aligned");
  if (!aligned16(out) || !aligned16(mirror))
    return refuse(FA_E_ARG, "fbl_reduce: out and mirror must be 16-byte aligned");
  if (!aligned4(sel) || !aligned4(n_sel)) return refuse(FA_E_ARG, "fbl_reduce: sel and n_sel must be 4-byte aligned");
  if (!aligned8(kept)) return refuse(FA_E_ARG, "fbl_reduce: kept must be 8-byte aligned");
  if (P == 0) return FA_OK;
  const int64_t P4 = (P + 3) / 4;
  FA_DEVICE_SCOPE("fbl_reduce", stream, out);
  FA_OPERAND("x", x, (uint64_t)((int64_t)(K - 1) * ld + P4 * 4) * 4);
  FA_OPERAND("sel", sel, (uint64_t)theta * 4);
  FA_OPERAND("n_sel", n_sel, 4);
  FA_OPERAND("last", last, (uint64_t)P4 * 16);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  FA_HOST_OK_OPERAND("mirror", mirror, (uint64_t)P * 4);
  FA_OPERAND("kept", kept, (uint64_t)K * 8);
  if (cus == 0) cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "fbl_reduce launch plan: no CU count for device %d", fa_scope_device());
  const BulGeo g = geo_of(theta);
  BulArgs a{};
  a.x = reinterpret_cast<const f4*>(x); a.ld4 = ld / 4; a.P4 = P4; a.P = P;
  a.ntiles = (P + (1 << g.wl) - 1) >> g.wl;
  a.sel = sel; a.n_sel = n_sel; a.last = last;
  a.K = K; a.theta = theta; a.beta = beta; a.wl = g.wl;
  a.denom = (float)beta;
  a.out = out; a.mirror = mirror;
  a.kept = reinterpret_cast<unsigned long long*>(kept);
  const unsigned grid = (unsigned)(a.ntiles < g.wgs * (int64_t)cus ? a.ntiles : g.wgs * (int64_t)cus);
  hipStream_t st = (hipStream_t)stream;
  if (g.R == 5) launch_reduce<16, 5>(a, grid, st);
  else if (g.R == 17) launch_reduce<16, 17>(a, grid, st);
  else if (g.R == 33) launch_reduce<32, 33>(a, grid, st);
  else launch_reduce<64, 65>(a, grid, st);
  return check_launch("fbl_reduce");
}
