// fa_common.h — what the .hip translation units of libfedagg.so share on the host side (internal to the library):
// error plumbing, the CU count of the scope's device, the 64-lane fp64 butterfly, and the strip launch plan of
// fh_reduce and fcl_reduce.  Included after fa_device.h.  The host-only units (ingress_host.cpp, ingress_dma.cpp,
// rccl_comm.cpp) keep their own small helpers, and fa_device.h does not include this header: tests/csrc compiles
// it against a mock runtime that has no device attributes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "fa_device.h"

typedef float f4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// error plumbing (the thread-local last-error string lives in fedagg.hip, behind fa_internal_set_error)
// ------------------------------------------------------------------------------------------------
__attribute__((format(printf, 2, 3))) static inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return fa_internal_set_error(code, buf);
}
// an argument refused before the device scope opens: the same closing words as DevScope's operand errors
__attribute__((format(printf, 2, 3))) static inline int refuse(int code, const char* fmt, ...) {
  char msg[400], buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof(msg), fmt, ap);
  va_end(ap);
  snprintf(buf, sizeof(buf), "%s (nothing was launched)", msg);
  return fa_internal_set_error(code, buf);
}
static inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FA_E_HIP, "%s: launch failed: %s", what, hipGetErrorString(e));
  return FA_OK;
}
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// CU count of the device the running entry point works on (its DevScope), not the thread's current device.  A
// failed query is not a launch failure: its error is cleared, so that a later check_launch does not report it.
static inline int cu_count() {
  static int cache[64];  // per device ordinal (idempotent, benign race)
  const int dev = fa_scope_device();
  if (dev < 0 || dev >= 64) return 0;
  if (cache[dev] > 0) return cache[dev];
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  cache[dev] = cus;
  return cus;
}

// the 64 lanes' doubles added as a butterfly: every lane ends with the same sum (IEEE addition commutes), in an
// order that is a function of the lane numbering alone — the same on every run
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------
// strip launch plan (fh_reduce, fcl_reduce)
// ------------------------------------------------------------------------------------------------
// A row is cut into strips: what the 64 lanes of a wave read with one 16-byte load each (strip_cols columns).  A
// workgroup of `waves` waves reduces a tile, each wave owning V strips of it and issuing U rows' loads ahead of their
// adds.  Three (V, U) variants trade the contiguous run per row against the waves a SIMD can hold; each kernel file
// writes down its own register arithmetic per level.  The plan over S strips, a host-only function of the CU count:
//   * with at least 0.85 x cap level-0 tiles (cap = cap_pct % of the CUs) the bucket is ONE level-0 launch on a grid
//     of at most cap workgroups, each walking the same number of tiles, the last tile ragged — k_reduce's
//     measurements carry over in their shape (profiles/r01_tune_grid_sweep.log: wide tiles on fewer concurrent
//     column streams read fastest);
//   * a shorter bucket gives its whole level-1 tiles to level 1 when they cover at least half the CUs,
//   * and what is left (all of it otherwise) to level 2.
// K and the weights do not enter this plan; fa_reduce's own plan (fedagg.hip) depends on them and is another one.
struct StripGeo {
  int waves;       // waves per workgroup
  int V[3], U[3];  // per level
  int cap_pct;     // level 0's grid cap: workgroups per 100 CUs
  int strip_cols;  // columns of one strip
};
struct StripLaunch {
  int level;
  int64_t strip0, tiles, grid;
};

static inline int strip_plan(int64_t cus, int64_t strips, const StripGeo& g, StripLaunch out[3]) {
  if (strips <= 0 || cus <= 0) return 0;
  const int64_t S = strips;
  const int64_t cap = cus * g.cap_pct / 100 > 0 ? cus * g.cap_pct / 100 : 1;
  const int64_t span0 = (int64_t)g.waves * g.V[0], span1 = (int64_t)g.waves * g.V[1],
                span2 = (int64_t)g.waves * g.V[2];
  const int64_t t0 = (S + span0 - 1) / span0;
  if (t0 * 100 >= cap * 85) {
    const int64_t rounds = (t0 + cap - 1) / cap;
    out[0] = StripLaunch{0, 0, t0, (t0 + rounds - 1) / rounds};
    return 1;
  }
  int n = 0;
  int64_t s = 0;
  const int64_t n1 = S / span1;
  if (n1 > 0 && 2 * n1 >= cus) {
    out[n++] = StripLaunch{1, 0, n1, n1};
    s = n1 * span1;
  }
  if (s < S) {
    const int64_t t2 = (S - s + span2 - 1) / span2;
    out[n++] = StripLaunch{2, s, t2, t2};
  }
  return n;
}

// the plan as fh_reduce_plan / fcl_reduce_plan report it: six fields per launch (FH_PLAN_FIELDS, FCL_PLAN_FIELDS),
// the first `cap` launches written; returns the number of launches
constexpr int STRIP_PLAN_FIELDS = 6;
static inline int strip_plan_export(int64_t cus, int64_t strips, const StripGeo& g, int64_t* plan_out, int cap) {
  StripLaunch l[3];
  const int n = strip_plan(cus, strips, g, l);
  for (int i = 0; i < n && i < cap; ++i) {
    int64_t* o = plan_out + (int64_t)STRIP_PLAN_FIELDS * i;
    o[0] = g.V[l[i].level];
    o[1] = g.U[l[i].level];
    o[2] = l[i].strip0 * g.strip_cols;
    o[3] = l[i].tiles;
    o[4] = g.V[l[i].level];
    o[5] = l[i].grid;
  }
  return n;
}
