// lowrank_reduce.hip — MI355X (gfx950) kernel of the low-rank delta-upload path (include/fedlowrank.h):
//   * flr_reduce: every client's staged factors Ut [r2, O4], V [r2, I4] multiplied out onto the fp32 chain,
//     sum over (client, j) of Ut[j, o] * V[j, i], on the fp32 matrix unit (v_mfma_f32_32x32x2_f32); the bucket's
//     unfactored entries are chained by the same launch;
//   * flr_reduce_plan, flr_reduce_table: the tile table of that launch, a host-only function of (CU count, rank,
//     entry shapes);
//   * flr_row_layout: where an entry's factors lie in a staged row.
//
// One launch per staged chunk, one workgroup per row of the tile table: (entry, tile row, tile column, kind).
//
// The matrix tile.  T x T outputs (T = 128, or 64 for buckets whose 128-tiles would leave CUs idle), a workgroup of four waves,
// each wave a (T/2) x (T/2) quadrant as B x B blocks of the 32 x 32 x 2 instruction (B = T / 64) whose accumulators
// stay in registers through the whole inner loop (64 VGPRs at T = 128).  Both operands are read inner-major — a
// staged row Ut[j, o0 : o0 + T], V[j, i0 : i0 + T] is contiguous — so a stage of FLR_DEPTH inner rows goes
// global -> registers -> LDS as [D][U: T | V: T] with 16-byte accesses and no transposition; the registers of
// stage s + 1 are loaded before the matrix instructions of stage s are issued and written to the other LDS buffer
// after them (one barrier per stage).  Lane l of a wave reads its operand of inner pair h at
// LDS[2h + l / 32][32 b + l % 32]: 32 consecutive words per half wave.  The instruction's A operand is V and its B
// operand Ut: the accumulator's register r of lane l is then d[o = l % 32][i = 8 (r / 4) + 4 (l / 32) + r % 4], four
// consecutive i per lane, stored as a float4 wherever (chain offset + o * I + i) is 16-byte aligned.
// The inner dimension is never split and never padded: an inner tail n * r2 mod D runs as a shorter stage, over the
// staged rows only (the next client's slot is not this chunk's).
//
// Numerics: the order of the inner index is ascending and the same for every tile shape, so an output element's
// bits are a function of the data alone; what the matrix unit does inside one instruction is the hardware's
// (include/fedlowrank.h).  The dense tile's adds are fp32, rounded to nearest, never fused.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/fedlowrank.h"
#include "fa_device.h"
#include "fa_common.h"

// this unit's device code is compiled without the packed fp32 VALU forms (v_pk_add_f32, v_pk_mul_f32, v_pk_fma_f32)
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace {

typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int D = FLR_DEPTH;  // inner rows of one stage
constexpr int DENSE_U = 8;    // rows of a dense tile loaded ahead of their adds
constexpr int32_t MAGIC = 0x31524c46;  // "FLR1"
static_assert(D % 2 == 0 && D >= 2, "an instruction takes two inner rows");
static_assert(sizeof(flr_head_t) == 64 && sizeof(flr_entry_t) == 64 && sizeof(flr_tile_t) == 16, "table layout");

struct ReduceArgs {
  const float* staged;
  int64_t ldf;
  int n, r2, flags, n_entries;
  const unsigned char* table;
  const float* acc_in;
  float* out;
};

// four consecutive chain elements from `at`, the first nv of them inside the entry's row: one 16-byte access where
// the address allows, scalars otherwise
__device__ __forceinline__ f4 chain_load(const float* p, int64_t at, int nv) {
  f4 v = f4{0.f, 0.f, 0.f, 0.f};
  if (nv == 4 && (at & 3) == 0) {
    v = *reinterpret_cast<const f4*>(p + at);
  } else {
    if (nv > 0) v.x = p[at];
    if (nv > 1) v.y = p[at + 1];
    if (nv > 2) v.z = p[at + 2];
    if (nv > 3) v.w = p[at + 3];
  }
  return v;
}
__device__ __forceinline__ void chain_store(float* p, int64_t at, int nv, f4 v) {
  if (nv == 4 && (at & 3) == 0) {
    *reinterpret_cast<f4*>(p + at) = v;
  } else {
    if (nv > 0) p[at] = v.x;
    if (nv > 1) p[at + 1] = v.y;
    if (nv > 2) p[at + 2] = v.z;
    if (nv > 3) p[at + 3] = v.w;
  }
}

template <int B>
__device__ __forceinline__ void matrix_tile(const ReduceArgs& a, const flr_entry_t& e, int tr, int tc, float* lds) {
  constexpr int T = 64 * B;          // outputs each way
  constexpr int C4 = T / 4;          // float4 pieces of one operand's staged row
  constexpr int PITCH = 2 * T;       // LDS floats of one inner row: [Ut: T | V: T]
  constexpr int PER = D * 2 * C4 / 256;  // float4 pieces of a stage per thread
  static_assert(PER >= 1 && D * 2 * C4 % 256 == 0, "a stage is a whole number of pieces per thread");
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wi = wave >> 1, wj = wave & 1;
  const int lrow = lane >> 5, lcol = lane & 31;
  const int o0 = tr * T, i0 = tc * T;
  const int G = a.n * a.r2;  // the inner dimension (even)
  const int stages = (G + D - 1) / D;
  const f4 zero = f4{0.f, 0.f, 0.f, 0.f};

  f4 reg[PER];
  auto fetch = [&](int s) {
#pragma unroll
    for (int p = 0; p < PER; ++p) {
      const int idx = tid + 256 * p;
      const int d = idx / (2 * C4), c = idx % (2 * C4);
      const int g = s * D + d;
      reg[p] = zero;
      if (g < G) {  // a row past the chunk's last is not read: it is not this chunk's
        const int k = g / a.r2, j = g - k * a.r2;
        const float* row = a.staged + (int64_t)k * a.ldf;
        if (c < C4) {
          const int col = o0 + 4 * c;  // (a multiple of 4: whole float4s lie below O4)
          if (col < e.O4) reg[p] = *reinterpret_cast<const f4*>(row + e.ut_off + (int64_t)j * e.O4 + col);
        } else {
          const int col = i0 + 4 * (c - C4);
          if (col < e.I4) reg[p] = *reinterpret_cast<const f4*>(row + e.v_off + (int64_t)j * e.I4 + col);
        }
      }
    }
  };
  auto put = [&](float* buf) {
#pragma unroll
    for (int p = 0; p < PER; ++p) *reinterpret_cast<f4*>(buf + 4 * (tid + 256 * p)) = reg[p];
  };

  // the accumulators: block (bo, bi) of this wave's quadrant, register 4 q + c of lane l = d[o][i + c]
  f16v acc[B][B];
  const int ow = o0 + wi * 32 * B + lcol, iw = i0 + wj * 32 * B + lrow * 4;
#pragma unroll
  for (int bo = 0; bo < B; ++bo)
#pragma unroll
    for (int bi = 0; bi < B; ++bi)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f4 v = zero;
        if (a.flags & FA_ACCUMULATE) {
          const int o = ow + 32 * bo, i = iw + 32 * bi + 8 * q;
          const int left = e.I - i;
          const int nv = o < e.O ? (left >= 4 ? 4 : (left > 0 ? left : 0)) : 0;
          v = chain_load(a.acc_in, e.chain_off + (int64_t)o * e.I + i, nv);
        }
        acc[bo][bi][4 * q] = v.x;
        acc[bo][bi][4 * q + 1] = v.y;
        acc[bo][bi][4 * q + 2] = v.z;
        acc[bo][bi][4 * q + 3] = v.w;
      }

  auto pair = [&](const float* buf, int h) {
    const float* r = buf + (2 * h + lrow) * PITCH + lcol;
    float u[B], v[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      u[b] = r[wi * 32 * B + 32 * b];
      v[b] = r[T + wj * 32 * B + 32 * b];
    }
#pragma unroll
    for (int bo = 0; bo < B; ++bo)
#pragma unroll
      for (int bi = 0; bi < B; ++bi)
        acc[bo][bi] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[bi], u[bo], acc[bo][bi], 0, 0, 0);
  };

  if (stages > 0) {
    fetch(0);
    put(lds);
  }
  __syncthreads();
  for (int s = 0; s < stages; ++s) {  // (uniform over the workgroup)
    const float* buf = lds + (s & 1) * (D * PITCH);
    const bool more = s + 1 < stages;
    if (more) fetch(s + 1);  // in flight under the matrix instructions
    const int rows = G - s * D < D ? G - s * D : D;
    if (rows == D) {
#pragma unroll
      for (int h = 0; h < D / 2; ++h) pair(buf, h);
    } else {
      for (int h = 0; h < rows / 2; ++h) pair(buf, h);
    }
    if (more) put(lds + ((s + 1) & 1) * (D * PITCH));
    __syncthreads();
  }

#pragma unroll
  for (int bo = 0; bo < B; ++bo)
#pragma unroll
    for (int bi = 0; bi < B; ++bi)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int o = ow + 32 * bo, i = iw + 32 * bi + 8 * q;
        const int left = e.I - i;
        const int nv = o < e.O ? (left >= 4 ? 4 : (left > 0 ? left : 0)) : 0;
        const f4 v = f4{acc[bo][bi][4 * q], acc[bo][bi][4 * q + 1], acc[bo][bi][4 * q + 2], acc[bo][bi][4 * q + 3]};
        chain_store(a.out, e.chain_off + (int64_t)o * e.I + i, nv, v);
      }
}

// one column per thread through the n rows, DENSE_U loads ahead of their adds; a row past n adds nothing (not a zero)
__device__ __forceinline__ void dense_tile(const ReduceArgs& a, const flr_entry_t& e, int tc) {
  const int64_t p = (int64_t)tc * FLR_DENSE_COLS + threadIdx.x;
  if (p >= e.O) return;
  const float* x = a.staged + e.ut_off + p;
  const int64_t at = e.chain_off + p;
  float acc = (a.flags & FA_ACCUMULATE) ? a.acc_in[at] : 0.0f;
  for (int k0 = 0; k0 < a.n; k0 += DENSE_U) {
    float v[DENSE_U];
#pragma unroll
    for (int u = 0; u < DENSE_U; ++u) v[u] = k0 + u < a.n ? x[(int64_t)(k0 + u) * a.ldf] : 0.0f;
#pragma unroll
    for (int u = 0; u < DENSE_U; ++u)
      if (k0 + u < a.n) acc = acc + v[u];
  }
  a.out[at] = acc;
}

__global__ __launch_bounds__(256) void k_reduce_lowrank(ReduceArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[2 * D * 2 * 128];
  static_assert(FLR_DENSE_COLS == 256, "a dense tile is one column per thread");
  const flr_entry_t* ents = reinterpret_cast<const flr_entry_t*>(a.table + sizeof(flr_head_t));
  const flr_tile_t* tiles = reinterpret_cast<const flr_tile_t*>(a.table + sizeof(flr_head_t) +
                                                                (size_t)a.n_entries * sizeof(flr_entry_t));
  const flr_tile_t t = tiles[blockIdx.x];
  const flr_entry_t e = ents[t.entry];
  if (t.kind == FLR_KIND_LARGE) {
    matrix_tile<2>(a, e, t.tr, t.tc, lds);
  } else if (t.kind == FLR_KIND_SMALL) {
    matrix_tile<1>(a, e, t.tr, t.tc, lds);
  } else {
    dense_tile(a, e, t.tc);
  }
}

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

// ------------------------------------------------------------------------------------------------
// the plan (host)
// ------------------------------------------------------------------------------------------------
struct Plan {
  std::vector<flr_entry_t> ents;
  int64_t n_tiles = 0, ldf = 64, P = 0, row_floats = 0;
  int rank = 0, r2 = 0;
};

constexpr int64_t I31 = 0x7fffffffLL;
int64_t up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// the staged offsets and chain offsets (cus == 0: no tiles), then the tiles
int make_plan(const char* who, int64_t cus, int32_t rank, int32_t n_entries, const int64_t* dims, int32_t force,
              Plan& pl) {
  if (rank < 1 || rank > FLR_MAX_RANK)
    return refuse(FA_E_ARG, "%s: rank=%d outside 1..%d", who, rank, FLR_MAX_RANK);
  if (n_entries < 0 || (n_entries > 0 && !dims)) return refuse(FA_E_ARG, "%s: n_entries=%d or dims is NULL", who, n_entries);
  if (cus < 0 || (force != 0 && force != 64 && force != 128))
    return refuse(FA_E_ARG, "%s: cus=%lld or force_tile=%d (0, 64 or 128)", who, (long long)cus, force);
  pl.rank = rank;
  pl.r2 = (rank + 1) / 2 * 2;
  pl.ents.resize(n_entries);
  int64_t off = 0, chain = 0;
  for (int i = 0; i < n_entries; ++i) {
    const int64_t O = dims[2 * i], I = dims[2 * i + 1];
    if (O < 0 || I < 0 || (I > 0 && O < 1)) return refuse(FA_E_ARG, "%s: entry %d has dims (%lld, %lld)", who, i, (long long)O, (long long)I);
    if (O > I31 - 3 || I > I31 - 3) return refuse(FA_E_RANGE, "%s: entry %d exceeds 2^31 - 1 floats", who, i);
    flr_entry_t& e = pl.ents[i];
    memset(&e, 0, sizeof(e));
    off = up(off, 4);
    e.chain_off = chain;
    e.ut_off = off;
    e.O = (int32_t)O;
    if (I > 0) {
      e.I = (int32_t)I;
      e.O4 = (int32_t)up(O, 4);
      e.I4 = (int32_t)up(I, 4);
      e.v_off = off + (int64_t)pl.r2 * e.O4;
      off = e.v_off + (int64_t)pl.r2 * e.I4;
      chain += O * I;
    } else {
      off += O;
      chain += O;
    }
    if (off > I31 - 64 || chain > I31) return refuse(FA_E_RANGE, "%s: the bucket or a staged row exceeds 2^31 - 1 floats", who);
  }
  pl.P = chain;
  pl.row_floats = off;
  pl.ldf = off > 0 ? up(off, 64) : 64;
  if (cus == 0) return FA_OK;
  // the large tile when the factored entries together give every CU one (they share the launch); the small one
  // otherwise — 1.6 x and 2 x apart, either way, in profiles/lowrank_measure.json
  int64_t nl = 0;
  for (const auto& e : pl.ents)
    if (e.I > 0) nl += ((int64_t)e.O + 127) / 128 * (((int64_t)e.I + 127) / 128);
  const bool large = force == 128 || (force == 0 && nl >= cus);
  for (auto& e : pl.ents) {
    if (e.I > 0) {
      e.kind = large ? FLR_KIND_LARGE : FLR_KIND_SMALL;
      e.tile = large ? 128 : 64;
      e.ntr = (e.O + e.tile - 1) / e.tile;
      e.ntc = (e.I + e.tile - 1) / e.tile;
    } else {
      e.kind = FLR_KIND_DENSE;
      e.tile = FLR_DENSE_COLS;
      e.ntc = (int32_t)(((int64_t)e.O + FLR_DENSE_COLS - 1) / FLR_DENSE_COLS);
      e.ntr = e.ntc > 0 ? 1 : 0;
    }
  }
  int64_t t = 0;
  for (int kind : {FLR_KIND_LARGE, FLR_KIND_SMALL, FLR_KIND_DENSE})  // the longest tiles first
    for (auto& e : pl.ents)
      if (e.kind == kind) {
        e.first_tile = t;
        t += (int64_t)e.ntr * e.ntc;
      }
  if (t > I31) return refuse(FA_E_RANGE, "%s: %lld tiles exceed one launch", who, (long long)t);
  pl.n_tiles = t;
  return FA_OK;
}

int64_t table_bytes(const Plan& pl) {
  return (int64_t)sizeof(flr_head_t) + (int64_t)pl.ents.size() * sizeof(flr_entry_t) + pl.n_tiles * sizeof(flr_tile_t);
}

void write_table(const Plan& pl, unsigned char* out) {
  flr_head_t h;
  memset(&h, 0, sizeof(h));
  h.magic = MAGIC;
  h.rank = pl.rank;
  h.r2 = pl.r2;
  h.n_entries = (int32_t)pl.ents.size();
  h.n_tiles = pl.n_tiles;
  h.ldf = pl.ldf;
  h.P = pl.P;
  h.row_floats = pl.row_floats;
  memcpy(out, &h, sizeof(h));
  if (!pl.ents.empty()) memcpy(out + sizeof(h), pl.ents.data(), pl.ents.size() * sizeof(flr_entry_t));
  flr_tile_t* tiles = reinterpret_cast<flr_tile_t*>(out + sizeof(h) + pl.ents.size() * sizeof(flr_entry_t));
  for (size_t i = 0; i < pl.ents.size(); ++i) {
    const flr_entry_t& e = pl.ents[i];
    flr_tile_t* t = tiles + e.first_tile;
    for (int tr = 0; tr < e.ntr; ++tr)
      for (int tc = 0; tc < e.ntc; ++tc) *t++ = flr_tile_t{(int32_t)i, tr, tc, e.kind};
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedlowrank.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t flr_abi_version(void) { return FLR_ABI_VERSION; }

extern "C" int64_t flr_row_layout(int32_t rank, int32_t n_entries, const int64_t* dims, int64_t* off_out) {
  Plan pl;
  if (const int e = make_plan("flr_row_layout", 0, rank, n_entries, dims, 0, pl)) return e;
  if (off_out)
    for (int i = 0; i < n_entries; ++i) {
      off_out[2 * i] = pl.ents[i].ut_off;
      off_out[2 * i + 1] = pl.ents[i].v_off;
    }
  return pl.ldf;
}

extern "C" int64_t flr_reduce_plan(int32_t cus, int32_t rank, int32_t n_entries, const int64_t* dims,
                                   int32_t force_tile, int64_t* plan_out) {
  if (cus <= 0) return refuse(FA_E_ARG, "flr_reduce_plan: cus=%d", cus);
  Plan pl;
  if (const int e = make_plan("flr_reduce_plan", cus, rank, n_entries, dims, force_tile, pl)) return e;
  if (plan_out)
    for (int i = 0; i < n_entries; ++i) {
      const flr_entry_t& e = pl.ents[i];
      int64_t* o = plan_out + (int64_t)FLR_PLAN_FIELDS * i;
      o[0] = e.kind;
      o[1] = e.tile;
      o[2] = (int64_t)e.ntr * e.ntc;
      o[3] = e.first_tile;
    }
  return pl.n_tiles;
}

extern "C" int64_t flr_reduce_table(int32_t cus, int32_t rank, int32_t n_entries, const int64_t* dims,
                                    int32_t force_tile, void* table_out, int64_t cap_bytes) {
  if (cus <= 0) return refuse(FA_E_ARG, "flr_reduce_table: cus=%d", cus);
  Plan pl;
  if (const int e = make_plan("flr_reduce_table", cus, rank, n_entries, dims, force_tile, pl)) return e;
  const int64_t need = table_bytes(pl);
  if (table_out && cap_bytes >= need) write_table(pl, static_cast<unsigned char*>(table_out));
  return need;
}

extern "C" int flr_reduce(const float* staged, int64_t ldf, int32_t n, int32_t rank, int32_t n_entries,
                          const int64_t* dims, int32_t force_tile, const void* table_dev, const void* table_host,
                          int64_t table_bytes_in, const float* acc_in, float* out, int32_t flags,
                          fa_stream_t stream) {
  if (flags & ~FA_ACCUMULATE) return refuse(FA_E_ARG, "flr_reduce: unknown flags %d (0 or FA_ACCUMULATE)", flags);
  if (n < 0 || n > (1 << 24)) return refuse(FA_E_ARG, "flr_reduce: n=%d rows (0 .. 2^24)", n);
  Plan lay;
  if (const int e = make_plan("flr_reduce", 0, rank, n_entries, dims, force_tile, lay)) return e;
  if (ldf != lay.ldf)
    return refuse(FA_E_ARG, "flr_reduce: ldf=%lld, the rows of these shapes have %lld (flr_row_layout)",
                  (long long)ldf, (long long)lay.ldf);
  if ((flags & FA_ACCUMULATE) && !acc_in) return refuse(FA_E_ARG, "flr_reduce: FA_ACCUMULATE without acc_in");
  if (n == 0 && !(flags & FA_ACCUMULATE)) return refuse(FA_E_ARG, "flr_reduce: n=0 rows with nothing to accumulate");
  if (n > 0 && !staged) return refuse(FA_E_ARG, "flr_reduce: staged is NULL");
  if (!out || !table_dev || !table_host) return refuse(FA_E_ARG, "flr_reduce: out, table_dev or table_host is NULL");
  if (!aligned16(staged) || !aligned16(table_dev))
    return refuse(FA_E_ARG, "flr_reduce: staged and table_dev must be 16-byte aligned");
  if (!aligned16(out) || !aligned16(acc_in)) return refuse(FA_E_ARG, "flr_reduce: out and acc_in must be 16-byte aligned");
  if (lay.P == 0) return FA_OK;
  FA_DEVICE_SCOPE("flr_reduce", stream, out);
  FA_OPERAND("staged", staged, (uint64_t)n * ldf * 4);
  FA_OPERAND("table_dev", table_dev, (uint64_t)(table_bytes_in > 0 ? table_bytes_in : 0));
  FA_OPERAND("acc_in", (flags & FA_ACCUMULATE) ? acc_in : nullptr, (uint64_t)lay.P * 4);
  FA_OPERAND("out", out, (uint64_t)lay.P * 4);
  const int cus = cu_count();
  if (cus <= 0) return fail(FA_E_HIP, "flr_reduce launch plan: no CU count for device %d", fa_scope_device());
  Plan pl;
  if (const int e = make_plan("flr_reduce", cus, rank, n_entries, dims, force_tile, pl)) return e;
  const int64_t need = table_bytes(pl);
  std::vector<unsigned char> want((size_t)need);
  write_table(pl, want.data());
  if (table_bytes_in != need || memcmp(want.data(), table_host, (size_t)need) != 0)
    return refuse(FA_E_ARG, "flr_reduce: the tile table (%lld bytes) is not the table of these shapes at rank %d on "
                  "%d CUs (%lld bytes; flr_reduce_table)", (long long)table_bytes_in, rank, cus, (long long)need);
  if (pl.n_tiles == 0) return FA_OK;
  ReduceArgs a{};
  a.staged = staged; a.ldf = ldf; a.n = n; a.r2 = pl.r2; a.flags = flags; a.n_entries = n_entries;
  a.table = static_cast<const unsigned char*>(table_dev); a.acc_in = acc_in; a.out = out;
  hipLaunchKernelGGL(k_reduce_lowrank, dim3((unsigned)pl.n_tiles), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("flr_reduce");
}
