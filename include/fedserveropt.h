/*
 * fedserveropt.h — C ABI of the adaptive server optimizers on MI355X (gfx950): FedAdam and FedAdagrad (Reddi et
 * al., "Adaptive Federated Optimization", ICLR 2021, Algorithm 2 — the two rules beside FedYoGi) and FedAvgM
 * (Hsu et al., 2019: server momentum, also the server step of FedBuff's paper).  One streaming pass over the
 * round's mean, the last model and the optimizer state, into the new model.
 *
 * Built into the same libfedagg.so as fedagg.h and following its conventions (0 / negative FA_E* codes,
 * fa_last_error_string(), asynchronous on `stream`, no implicit synchronisation, caller-owned memory, stateless, no
 * atomics, the call's GPU taken from its stream or its output, every operand checked before anything is queued).
 * The entry points of this header are bound by fedscale_amd/_native_serveropt.py; the header has its own version
 * (fso_abi_version), FA_ABI_VERSION is not touched by it.
 *
 * What is replaced (reference): nothing — the reference's server steps are FedYoGi and q-FedAvg (optimizers.py:43-108).
 *
 * The contract.  All arithmetic is fp32, every operation rounded once to nearest, nothing contracted into an FMA,
 * fp32 denormals kept.  The scalars arrive as fp32: omb = fp32(1 - beta) and omb2 = fp32(1 - beta2), the differences
 * formed in double by the host.  Per parameter, with g = cur - last (cur is the round's mean):
 *
 *   rule          m                    v                         out
 *   FSO_ADAM      beta*m + omb*g       beta2*v + omb2*(g*g)      last + eta * (m / (sqrt(v) + tau))
 *   FSO_ADAGRAD   beta*m + omb*g       v + g*g                   last + eta * (m / (sqrt(v) + tau))
 *   FSO_AVGM      beta*m + g           (not used)                last + eta * m
 *
 * Each product, sum, square root and quotient above is one IEEE operation, evaluated as written (beta*m, then omb*g,
 * then their sum; g*g before omb2 multiplies it; sqrt(v), + tau, m / that, eta * that, last + that).  The square
 * root and the division are the correctly rounded ones; there is no reciprocal-then-multiply, which could not be
 * restated exactly.  So m, v and out equal a numpy float32 restatement bit for bit (tests/serveropt_fixtures.py).
 *
 * First step (FSO_INIT): m is taken as 0 and v as v0 without being read, so state buffers need no clearing.  The
 * paper asks v_{-1} >= tau^2; the Python layer's default is v0 = fp32(tau*tau), the product formed in double.
 *
 * A rule touches only its own streams: FSO_ADAM and FSO_ADAGRAD read cur, last, m, v and write m, v, out (28 bytes
 * per parameter, 20 under FSO_INIT); FSO_AVGM reads cur, last, m and writes m, out (20 bytes, 16 under FSO_INIT) and
 * never dereferences v, which may be NULL.  m and v are updated in place.  out may alias cur: a thread reads its
 * float4 of cur before it writes that float4 of out, and no other thread touches it.
 *
 * FSO_AVGM with beta = 0 and eta = 1 gives last + (cur - last), which in fp32 is not always cur.
 *
 * Non-finite values propagate as IEEE does; nothing is rejected or replaced.
 *
 * Buffers hold round_up(P, 4) floats: the kernel works in float4, and columns [P, round_up(P, 4)) are read, stepped
 * and written like any other (the bucket layout pads every buffer so).
 */
#ifndef FEDSERVEROPT_H
#define FEDSERVEROPT_H

#include <stdint.h>

#include "fedagg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FSO_ABI_VERSION 1

enum { /* rule */
  FSO_ADAM = 0,
  FSO_ADAGRAD = 1,
  FSO_AVGM = 2,
};

enum { /* flags (bitwise or) */
  FSO_INIT = 1,   /* first step: m := 0 and v := v0, neither is read */
  FSO_NT_ON = 2,  /* non-temporal loads and stores whatever the size */
  FSO_NT_OFF = 4, /* cached loads and stores whatever the size */
};

/* Without an override a step takes non-temporal loads and stores when the bytes of the rule's streams,
 * round_up(P, 4) * 4 * streams (7 for FSO_ADAM / FSO_ADAGRAD, 5 for FSO_AVGM), exceed this: the Infinity Cache. */
#define FSO_NT_MIN_BYTES (256LL << 20)

#define FSO_PLAN_FIELDS 4 /* fso_step_plan: blocks, grid-stride trips, non-temporal 0/1, bytes moved */

int32_t fso_abi_version(void);

/*
 * One step of `rule` over P parameters (the table above).
 *   cur, last  device memory of round_up(P, 4) floats, 16-byte aligned; read.
 *   m, v       device memory of round_up(P, 4) floats, 16-byte aligned; read (unless FSO_INIT) and written.  v is
 *              ignored, and may be NULL, for FSO_AVGM.
 *   out        device memory of round_up(P, 4) floats, 16-byte aligned; written.  May be cur.
 *   beta2, omb2, tau, v0   ignored by the rules that do not use them.
 * P == 0 queues nothing and returns FA_OK.  Refused (FA_E_ARG, nothing launched, fa_last_error_string names the
 * call): a negative P, an unknown rule, unknown flag bits, FSO_NT_ON together with FSO_NT_OFF, a NULL or misaligned
 * pointer, an operand that is not device memory of the call's GPU or is shorter than round_up(P, 4) floats.
 */
int fso_step(int32_t rule, const float* cur, const float* last, float* m, float* v, float* out, int64_t P, float eta,
             float tau, float beta, float omb, float beta2, float omb2, float v0, int32_t flags, fa_stream_t stream);

/*
 * fso_step over every part of a model sharded across the GPUs of one process, in one call: part i steps cur[i],
 * last[i], m[i], v[i] -> out[i] (P[i] columns) on streams[i] (never NULL), the same rule, scalars and flags for every
 * part.  v may be NULL (the table itself) for FSO_AVGM.  Every part is checked before anything launches; a part with
 * P[i] == 0 is skipped.
 */
int fso_step_parts(int32_t n, int32_t rule, const float* const* cur, const float* const* last, float* const* m,
                   float* const* v, float* const* out, const int64_t* P, float eta, float tau, float beta, float omb,
                   float beta2, float omb2, float v0, int32_t flags, fa_stream_t const* streams);

/*
 * What fso_step(rule, ..., P, ..., flags) launches (host only, no GPU needed): fields[0] workgroups of 256 threads,
 * fields[1] grid-stride trips of the busiest thread, fields[2] 1 when the loads and stores are non-temporal,
 * fields[3] bytes read plus bytes written.  P == 0 gives four zeros.  FA_E_ARG for what fso_step refuses of
 * (rule, P, flags), or a NULL fields.
 */
int fso_step_plan(int32_t rule, int64_t P, int32_t flags, int64_t* fields);

#ifdef __cplusplus
}
#endif
#endif /* FEDSERVEROPT_H */
