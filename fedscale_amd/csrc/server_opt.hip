// server_opt.hip — MI355X (gfx950) kernel of the adaptive server optimizers (include/fedserveropt.h): FedAdam,
// FedAdagrad and FedAvgM as one streaming pass over the round's mean, the last model and the optimizer state.
// Modelled on k_yogi_step (fedagg.hip): 256 threads, grid-stride float4, the grid capped at 8192 workgroups.  The
// kernel is byte-bound: FSO_ADAM and FSO_ADAGRAD move 28 bytes per parameter, FSO_AVGM 20 — it has no
// v stream and never forms an address from v.
//
// Numerics: every fp32 op is rounded to nearest and never contracted into an FMA; the default denormal modes are
// kept.  sqrt is __builtin_sqrtf and the division the plain operator: with this build's flags both compile to the
// correctly rounded sequences (v_sqrt_f32 plus the fma refinement; v_div_scale / v_div_fmas / v_div_fixup), so the
// results equal a numpy float32 restatement bit for bit.  No reciprocal: __frcp_rn(x) * y cannot be restated.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fedserveropt.h"
#include "fa_device.h"
#include "fa_common.h"

namespace {

struct Hp {  // the step's scalars, as fp32
  float eta, tau, beta, omb, beta2, omb2, v0;
};

constexpr int FSO_BLOCK = 256;
constexpr int64_t FSO_MAX_GRID = 8192;  // 256 CUs x 32 workgroups: grid-stride the rest (stride_grid, fedagg.hip)

__host__ __device__ constexpr int streams_of(int rule) { return rule == FSO_AVGM ? 5 : 7; }

template <bool NT, typename T>
__device__ __forceinline__ T ld_s(const T* p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}
template <bool NT, typename T>
__device__ __forceinline__ void st_s(T* p, T v) {
  if (NT)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}

// one parameter's step; the operation order is the contract's (include/fedserveropt.h)
template <int RULE>
__device__ __forceinline__ float step_elem(float cur, float last, float& m, float& v, const Hp& h) {
  const float g = cur - last;
  if (RULE == FSO_AVGM) {
    m = h.beta * m + g;
    return last + h.eta * m;
  }
  const float g2 = g * g;
  m = h.beta * m + h.omb * g;
  if (RULE == FSO_ADAM)
    v = h.beta2 * v + h.omb2 * g2;
  else
    v = v + g2;
  const float den = __builtin_sqrtf(v) + h.tau;
  return last + h.eta * (m / den);
}

template <int RULE>
__device__ __forceinline__ f4 step4(f4 cur, f4 last, f4& M, f4& V, const Hp& h) {
  float m[4] = {M.x, M.y, M.z, M.w}, v[4] = {V.x, V.y, V.z, V.w};
  float c[4] = {cur.x, cur.y, cur.z, cur.w}, l[4] = {last.x, last.y, last.z, last.w}, o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = step_elem<RULE>(c[i], l[i], m[i], v[i], h);
  M = f4{m[0], m[1], m[2], m[3]};
  V = f4{v[0], v[1], v[2], v[3]};
  return f4{o[0], o[1], o[2], o[3]};
}

// out may alias cur (no __restrict__ on either): a thread loads its float4 of cur before it stores that float4 of
// out.  Every index is below P4, the float4 count the host checked each operand's allocation against.
template <int RULE, bool NT>
__global__ __launch_bounds__(FSO_BLOCK) void k_fso_step(const f4* cur, const f4* last, f4* m, f4* v, f4* out,
                                                        int64_t P4, Hp h, int init) {
  constexpr bool HAS_V = RULE != FSO_AVGM;
  for (int64_t i = (int64_t)blockIdx.x * FSO_BLOCK + threadIdx.x; i < P4; i += (int64_t)gridDim.x * FSO_BLOCK) {
    const f4 C = ld_s<NT>(cur + i), L = ld_s<NT>(last + i);
    f4 M = init ? f4{0.f, 0.f, 0.f, 0.f} : ld_s<NT>(m + i);
    f4 V = f4{h.v0, h.v0, h.v0, h.v0};
    if (HAS_V && !init) V = ld_s<NT>(v + i);
    const f4 o = step4<RULE>(C, L, M, V, h);
    st_s<NT>(m + i, M);
    if (HAS_V) st_s<NT>(v + i, V);
    st_s<NT>(out + i, o);
  }
}

// The launch of one step.  The non-temporal threshold is k_yogi_step's (FA_YOGI_NT_MIN_BYTES, fedagg.hip): a step
// whose streams fit the 256 MiB Infinity Cache keeps the hits the nt policy gives up.  That threshold was measured for
// YoGi's seven streams only (profiles/r05_yogi_step_probe.log); tools/serveropt_measure.py times every rule with the
// policy forced on and off at 1 M and 25 M parameters (profiles/serveropt_measure.json).
struct Plan {
  int64_t P4, grid, trips, bytes;
  bool nt;
};

Plan plan_of(int rule, int64_t P, int flags) {
  Plan p;
  p.P4 = (P + 3) / 4;
  const int64_t b = (p.P4 + FSO_BLOCK - 1) / FSO_BLOCK;
  p.grid = b > FSO_MAX_GRID ? FSO_MAX_GRID : b;
  p.trips = p.grid ? (p.P4 + p.grid * FSO_BLOCK - 1) / (p.grid * FSO_BLOCK) : 0;
  const int s = streams_of(rule);
  p.nt = (flags & FSO_NT_ON) ? true : (flags & FSO_NT_OFF) ? false : p.P4 * 16 * s > FSO_NT_MIN_BYTES;
  const int unread = (flags & FSO_INIT) ? (rule == FSO_AVGM ? 1 : 2) : 0;  // the state streams FSO_INIT does not read
  p.bytes = p.P4 * 16 * (s - unread);
  return p;
}

// what fso_step refuses of (rule, P, flags)
int check_shape(const char* what, int rule, int64_t P, int flags) {
  if (rule != FSO_ADAM && rule != FSO_ADAGRAD && rule != FSO_AVGM)
    return refuse(FA_E_ARG, "%s: unknown rule %d", what, rule);
  if (flags & ~(FSO_INIT | FSO_NT_ON | FSO_NT_OFF)) return refuse(FA_E_ARG, "%s: unknown flags 0x%x", what, flags);
  if ((flags & FSO_NT_ON) && (flags & FSO_NT_OFF))
    return refuse(FA_E_ARG, "%s: FSO_NT_ON and FSO_NT_OFF are both set", what);
  if (P < 0) return refuse(FA_E_ARG, "%s: negative P=%lld", what, (long long)P);
  return FA_OK;
}

// NULL and alignment checks of one step's pointers
int check_ptrs(const char* what, int rule, const float* cur, const float* last, const float* m, const float* v,
               const float* out) {
  const bool has_v = rule != FSO_AVGM;
  if (!cur || !last || !m || !out || (has_v && !v)) return refuse(FA_E_ARG, "%s: NULL pointer", what);
  if (!aligned16(cur) || !aligned16(last) || !aligned16(m) || !aligned16(out) || (has_v && !aligned16(v)))
    return refuse(FA_E_ARG, "%s: pointers must be 16-byte aligned", what);
  return FA_OK;
}

typedef void (*StepKernel)(const f4*, const f4*, f4*, f4*, f4*, int64_t, Hp, int);

StepKernel kernel_of(int rule, bool nt) {
  switch (rule) {
    case FSO_ADAM: return nt ? k_fso_step<FSO_ADAM, true> : k_fso_step<FSO_ADAM, false>;
    case FSO_ADAGRAD: return nt ? k_fso_step<FSO_ADAGRAD, true> : k_fso_step<FSO_ADAGRAD, false>;
    default: return nt ? k_fso_step<FSO_AVGM, true> : k_fso_step<FSO_AVGM, false>;
  }
}

int launch(const char* what, int rule, const float* cur, const float* last, float* m, float* v, float* out,
           int64_t P, const Hp& h, int flags, hipStream_t st) {
  const Plan p = plan_of(rule, P, flags);
  hipLaunchKernelGGL(kernel_of(rule, p.nt), dim3((unsigned)p.grid), dim3(FSO_BLOCK), 0, st, (const f4*)cur,
                     (const f4*)last, (f4*)m, rule == FSO_AVGM ? nullptr : (f4*)v, (f4*)out, p.P4, h,
                     (flags & FSO_INIT) ? 1 : 0);
  return check_launch(what);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI (include/fedserveropt.h)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t fso_abi_version(void) { return FSO_ABI_VERSION; }

extern "C" int fso_step_plan(int32_t rule, int64_t P, int32_t flags, int64_t* fields) {
  const int e = check_shape("fso_step_plan", rule, P, flags);
  if (e) return e;
  if (!fields) return refuse(FA_E_ARG, "fso_step_plan: fields is NULL");
  const Plan p = plan_of(rule, P, flags);
  fields[0] = p.grid;
  fields[1] = p.trips;
  fields[2] = P > 0 && p.nt ? 1 : 0;
  fields[3] = p.bytes;
  return FA_OK;
}

extern "C" int fso_step(int32_t rule, const float* cur, const float* last, float* m, float* v, float* out, int64_t P,
                        float eta, float tau, float beta, float omb, float beta2, float omb2, float v0,
                        int32_t flags, fa_stream_t stream) {
  int e = check_shape("fso_step", rule, P, flags);
  if (e) return e;
  if (P == 0) return FA_OK;
  e = check_ptrs("fso_step", rule, cur, last, m, v, out);
  if (e) return e;
  FA_DEVICE_SCOPE("fso_step", stream, out);
  const uint64_t b = (uint64_t)((P + 3) / 4) * 16;
  FA_OPERAND("cur", cur, b);
  FA_OPERAND("last", last, b);
  FA_OPERAND("m", m, b);
  FA_OPERAND("v", rule == FSO_AVGM ? nullptr : v, b);
  FA_OPERAND("out", out, b);
  const Hp h{eta, tau, beta, omb, beta2, omb2, v0};
  return launch("fso_step", rule, cur, last, m, v, out, P, h, flags, (hipStream_t)stream);
}

extern "C" int fso_step_parts(int32_t n, int32_t rule, const float* const* cur, const float* const* last,
                              float* const* m, float* const* v, float* const* out, const int64_t* P, float eta,
                              float tau, float beta, float omb, float beta2, float omb2, float v0, int32_t flags,
                              fa_stream_t const* streams) {
  if (n < 1 || !cur || !last || !m || !out || !P || !streams)
    return refuse(FA_E_ARG, "fso_step_parts: NULL table or n < 1");
  const int e0 = check_shape("fso_step_parts", rule, 0, flags);
  if (e0) return e0;
  if (rule != FSO_AVGM && !v) return refuse(FA_E_ARG, "fso_step_parts: NULL table v");
  char what[48], nm[24];
  for (int i = 0; i < n; ++i) {
    snprintf(what, sizeof(what), "fso_step_parts[%d]", i);
    int e = check_shape(what, rule, P[i], flags);
    if (e) return e;
    if (P[i] == 0) continue;
    const float* vi = (rule == FSO_AVGM || !v) ? nullptr : v[i];
    if (!streams[i]) return refuse(FA_E_ARG, "%s: NULL stream", what);
    e = check_ptrs(what, rule, cur[i], last[i], m[i], vi, out[i]);
    if (e) return e;
    FA_DEVICE_SCOPE(what, streams[i], out[i]);
    const uint64_t b = (uint64_t)((P[i] + 3) / 4) * 16;
    const void* ops[5] = {cur[i], last[i], m[i], vi, out[i]};
    const char* names[5] = {"cur", "last", "m", "v", "out"};
    for (int j = 0; j < 5; ++j) {
      snprintf(nm, sizeof(nm), "%s[%d]", names[j], i);
      FA_OPERAND(nm, ops[j], b);
    }
  }
  const Hp h{eta, tau, beta, omb, beta2, omb2, v0};
  for (int i = 0; i < n; ++i) {
    if (P[i] == 0) continue;
    snprintf(what, sizeof(what), "fso_step_parts[%d]", i);
    FA_DEVICE_SCOPE(what, streams[i], out[i]);
    float* vi = (rule == FSO_AVGM || !v) ? nullptr : v[i];
    const int e = launch(what, rule, cur[i], last[i], m[i], vi, out[i], P[i], h, flags, (hipStream_t)streams[i]);
    if (e) return e;
  }
  return FA_OK;
}
