// rotate.hip — MI355X (gfx950) kernels of the randomised block Hadamard rotation (include/fedrotate.h):
//   * frt_rotate: e = x - base, the seed's sign diagonal, the 4096-point fast Walsh-Hadamard transform in the
//     contract's stage order, and the scale 2^-6, into all P' columns;
//   * frt_unrotate: the same transform, the scale, the diagonal, into columns [0, P).
// One wave owns one block and keeps it in registers: no LDS, no barrier, nothing crosses waves.  Lane l loads the
// float4 at columns 4l + 256i, i < 16 — sixteen coalesced 1 KiB runs per wave — so of the twelve index bits it holds
// bits 0-1 (the float4's components) and 8-11 (i) in its 64 registers, and bits 2-7 are the lane number.  Stages
// h = 1, 2 and h = 256 ... 2048 are adds between a lane's own registers; stages h = 4 ... 128 pair lane l with lane
// l ^ (h / 4) and cost one cross-lane move per register: a DPP quad permute for l ^ 1 and l ^ 2, a swizzle for
// l ^ 4, l ^ 8 and l ^ 16, and a permute for l ^ 32.  The kernels are byte-bound.
//
// Numerics: every fp32 op is rounded to nearest and never contracted into an FMA; the default denormal modes are
// kept.  A butterfly's difference is lower minus upper.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fedrotate.h"
#include "fa_device.h"
#include "fa_common.h"

// Tuning knob (tools/rotate_measure.py per library, FEDAGG_LIB).  FRT_PERMUTE_ONLY: every cross-lane
// stage through the general permute instead of DPP and swizzle moves.
#if defined(FRT_PERMUTE_ONLY)
#if !defined(FA_TUNING) || !FA_TUNING
#error "FRT_PERMUTE_ONLY is a tuning knob: build with -DFA_TUNING=1"
#endif
#endif
#ifndef FRT_PERMUTE_ONLY
#define FRT_PERMUTE_ONLY 0
#endif

namespace {

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));  // a float4 at a 4-byte aligned address

constexpr int FRT_WAVES = 4;  // blocks per workgroup: one wave transforms one block of 4096 columns

// A float's bits and back.  By value, on purpose: __builtin_bit_cast applied directly to a vector's component (v.y)
// reads the vector's first component with this compiler.
__device__ __forceinline__ uint32_t fbits(float f) { return __builtin_bit_cast(uint32_t, f); }
__device__ __forceinline__ float bfloat(uint32_t u) { return __builtin_bit_cast(float, u); }

// the 64 diagonal bits of the 64-column word w (splitmix64)
__device__ __forceinline__ uint64_t diag_word(uint64_t seed, uint64_t w) {
  uint64_t z = seed + (w + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the float4 at column c (a multiple of 4) under the diagonal: d[c + j] xored into component j's sign bit
__device__ __forceinline__ f4 diag_apply(f4 v, uint64_t seed, int64_t c) {
  const uint32_t d = (uint32_t)(diag_word(seed, (uint64_t)c >> 6) >> (c & 63));
  v.x = bfloat(fbits(v.x) ^ ((d & 1u) << 31));
  v.y = bfloat(fbits(v.y) ^ ((d & 2u) << 30));
  v.z = bfloat(fbits(v.z) ^ ((d & 4u) << 29));
  v.w = bfloat(fbits(v.w) ^ ((d & 8u) << 28));
  return v;
}

// lane l's value of v in lane l ^ M
template <int M>
__device__ __forceinline__ float lane_xor(float v) {
  const int x = __builtin_bit_cast(int, v);
#if FRT_PERMUTE_ONLY
  return __builtin_bit_cast(float, __shfl_xor(x, M, 64));
#else
  if (M == 1) return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false));  // quad_perm:[1,0,3,2]
  if (M == 2) return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false));  // quad_perm:[2,3,0,1]
  if (M == 4 || M == 8 || M == 16)  // bit mode: source lane = (l & 0x1f) ^ M, inside each half of the wave
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(x, (M << 10) | 0x1F));
  return __builtin_bit_cast(float, __shfl_xor(x, M, 64));
#endif
}

// one cross-lane stage over the lane's 64 registers: the lower lane of a pair takes a + b, the upper a - b.  The
// upper lane holds b and receives a: a - b is a + (-b) bit for bit (IEEE subtraction), so it flips its own sign bit
// and both lanes add — an xor and an add per register instead of two adds and a select
template <int M>
__device__ __forceinline__ void lane_stage(f4 v[16], int lane) {
  const uint32_t flip = (lane & M) ? 0x80000000u : 0u;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const f4 o = f4{lane_xor<M>(v[i].x), lane_xor<M>(v[i].y), lane_xor<M>(v[i].z), lane_xor<M>(v[i].w)};
    v[i].x = o.x + bfloat(fbits(v[i].x) ^ flip);
    v[i].y = o.y + bfloat(fbits(v[i].y) ^ flip);
    v[i].z = o.z + bfloat(fbits(v[i].z) ^ flip);
    v[i].w = o.w + bfloat(fbits(v[i].w) ^ flip);
  }
}

// the twelve stages in the contract's order, then the scale
__device__ __forceinline__ void fwht4096(f4 v[16], int lane) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {  // h = 1, 2: the float4's components
    const f4 a = v[i];
    const f4 s = f4{a.x + a.y, a.x - a.y, a.z + a.w, a.z - a.w};
    v[i] = f4{s.x + s.z, s.y + s.w, s.x - s.z, s.y - s.w};
  }
  lane_stage<1>(v, lane);   // h = 4
  lane_stage<2>(v, lane);   // h = 8
  lane_stage<4>(v, lane);   // h = 16
  lane_stage<8>(v, lane);   // h = 32
  lane_stage<16>(v, lane);  // h = 64
  lane_stage<32>(v, lane);  // h = 128
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) {  // h = 256 ... 2048: the lane's own float4s i and i + m
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i & m) continue;
      const f4 a = v[i], b = v[i + m];
      v[i] = a + b;
      v[i + m] = a - b;
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = v[i] * 0.015625f;
}

// INV = false: in = x (4-byte aligned, P columns, minus base when BASE), out = y (P' columns, all written).
// INV = true:  in = y (16-byte aligned, P' columns), out written in [0, P); out may be in: the wave has read its
// whole block before it stores any of it, and no other wave touches the block.
// Whether a block lies wholly below P is uniform over its wave: every block but the last takes the branch-free
// loads and stores, all sixteen loads (thirty-two with a base) in flight at once.
template <bool INV, bool BASE>
__global__ __launch_bounds__(64 * FRT_WAVES) void k_fwht(const float* in, const float* base, int64_t P, int64_t NB,
                                                         uint64_t seed, float* out) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * FRT_WAVES + (threadIdx.x >> 6);
  if (b >= NB) return;  // whole waves leave together
  const bool whole = (b + 1) * FRT_BLOCK <= P;
  const int64_t c0 = b * FRT_BLOCK + 4 * lane;
  f4 v[16];
  if (INV) {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = *reinterpret_cast<const f4*>(in + c0 + 256 * i);
  } else if (whole) {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = *reinterpret_cast<const f4u*>(in + c0 + 256 * i);
    if (BASE) {
      f4 l[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) l[i] = *reinterpret_cast<const f4u*>(base + c0 + 256 * i);
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = v[i] - l[i];
    }
  } else {  // the tail block: loads masked at P, the padding +0.0
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t c = c0 + 256 * i;
      float e[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c + j < P) e[j] = BASE ? in[c + j] - base[c + j] : in[c + j];
      v[i] = f4{e[0], e[1], e[2], e[3]};
    }
  }
  if (!INV) {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = diag_apply(v[i], seed, c0 + 256 * i);
  }
  fwht4096(v, lane);
  if (INV) {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = diag_apply(v[i], seed, c0 + 256 * i);
  }
  if (!INV || whole) {
#pragma unroll
    for (int i = 0; i < 16; ++i) *reinterpret_cast<f4*>(out + c0 + 256 * i) = v[i];
  } else {  // the inverse's tail block: stores masked at P
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t c = c0 + 256 * i;
      if (c + 4 <= P) {
        *reinterpret_cast<f4*>(out + c) = v[i];
      } else if (c < P) {  // the last, partial float4: columns >= P are not written
        out[c] = v[i].x;
        if (c + 1 < P) out[c + 1] = v[i].y;
        if (c + 2 < P) out[c + 2] = v[i].z;
      }
    }
  }
}

template <bool INV, bool BASE>
int launch(const char* what, const float* in, const float* base, int64_t P, uint64_t seed, float* out,
           hipStream_t st) {
  const int64_t NB = (P + FRT_BLOCK - 1) / FRT_BLOCK;
  const int64_t grid = (NB + FRT_WAVES - 1) / FRT_WAVES;
  hipLaunchKernelGGL((k_fwht<INV, BASE>), dim3((unsigned)grid), dim3(64 * FRT_WAVES), 0, st, in, base, P, NB, seed,
                     out);
  return check_launch(what);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedrotate.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t frt_abi_version(void) { return FRT_ABI_VERSION; }

extern "C" int64_t frt_padded(int64_t P) {
  if (P < 0) return refuse(FA_E_ARG, "frt_padded: negative P=%lld", (long long)P);
  return (P + FRT_BLOCK - 1) / FRT_BLOCK * FRT_BLOCK;
}

extern "C" int frt_rotate(const float* x, const float* base, int64_t P, uint64_t seed, float* y,
                          fa_stream_t stream) {
  if (P < 0) return refuse(FA_E_ARG, "frt_rotate: negative P=%lld", (long long)P);
  if (P == 0) return FA_OK;
  if (!x || !y) return refuse(FA_E_ARG, "frt_rotate: x or y is NULL");
  if (((uintptr_t)x | (uintptr_t)base) & 3u) return refuse(FA_E_ARG, "frt_rotate: x and base must be 4-byte aligned");
  if (!aligned16(y)) return refuse(FA_E_ARG, "frt_rotate: y must be 16-byte aligned");
  const int64_t Pp = (P + FRT_BLOCK - 1) / FRT_BLOCK * FRT_BLOCK;
  if (Pp / FRT_BLOCK / FRT_WAVES >= 0x7fffffffLL) return refuse(FA_E_RANGE, "frt_rotate: P too large");
  FA_DEVICE_SCOPE("frt_rotate", stream, y);
  FA_OPERAND("x", x, (uint64_t)P * 4);
  FA_OPERAND("base", base, (uint64_t)P * 4);
  FA_OPERAND("y", y, (uint64_t)Pp * 4);
  return base ? launch<false, true>("frt_rotate", x, base, P, seed, y, (hipStream_t)stream)
              : launch<false, false>("frt_rotate", x, nullptr, P, seed, y, (hipStream_t)stream);
}

extern "C" int frt_unrotate(const float* y, int64_t P, uint64_t seed, float* out, fa_stream_t stream) {
  if (P < 0) return refuse(FA_E_ARG, "frt_unrotate: negative P=%lld", (long long)P);
  if (P == 0) return FA_OK;
  if (!y || !out) return refuse(FA_E_ARG, "frt_unrotate: y or out is NULL");
  if (!aligned16(y) || !aligned16(out)) return refuse(FA_E_ARG, "frt_unrotate: y and out must be 16-byte aligned");
  const int64_t Pp = (P + FRT_BLOCK - 1) / FRT_BLOCK * FRT_BLOCK;
  if (Pp / FRT_BLOCK / FRT_WAVES >= 0x7fffffffLL) return refuse(FA_E_RANGE, "frt_unrotate: P too large");
  FA_DEVICE_SCOPE("frt_unrotate", stream, out);
  FA_OPERAND("y", y, (uint64_t)Pp * 4);
  FA_OPERAND("out", out, (uint64_t)P * 4);
  return launch<true, false>("frt_unrotate", y, nullptr, P, seed, out, (hipStream_t)stream);
}
