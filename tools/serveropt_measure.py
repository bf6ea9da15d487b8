"""Time fso_step (include/fedserveropt.h) for FedAdam, FedAdagrad and FedAvgM beside k_yogi_step, with the
non-temporal policy forced on and off, and the whole device-resident round under fed-adam beside fed-yogi, in one
process.

    python -u tools/serveropt_measure.py [--reps 30] [--round-reps 5] [--out profiles/serveropt_measure.json]

Steps, at 1 M and 25 M parameters, every buffer resident in HBM and reused by every call: device events around each
wrapper call, three warm-up calls, then ``--reps`` (>= 20) timed calls per variant, the variants alternating back to
back so that drift of the machine falls on all of them; median, min and max.  k_yogi_step takes its own size policy
(cached at 1 M, non-temporal at 25 M); each fso rule is timed with FSO_NT_ON and with FSO_NT_OFF.

Round, at 1000 x 25 M, the rows resident in HBM: fa_reduce into the mean buffer, then the step — fa_yogi_step for
fed-yogi, fso_step(adam) for fed-adam — as TorchModelAdapter._apply_round issues them.

The predictions, written into the result before anything is timed: by bytes, adam and adagrad take k_yogi_step's
time (the same 28 B per parameter) and avgm takes 20/28 of it.  A prediction is met when the time it predicts for
k_yogi_step — the rule's median by the size policy, scaled by 28 / the rule's bytes — lies inside the min-to-max
spread of k_yogi_step's repeats in the same run.  Misses are reported as misses.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedscale_amd import _native  # noqa: E402
from fedscale_amd import kernels as kx  # noqa: E402
from fedscale_amd import kernels_serveropt as kso  # noqa: E402

STEP_P = (1_000_000, 25_000_000)
ROUND = (1000, 25_000_000)
RULES = ("adam", "adagrad", "avgm")
BYTES = {"adam": 28, "adagrad": 28, "avgm": 20, "yogi": 28}  # per parameter, read plus written
HP = dict(eta=0.01, tau=1e-3, beta=0.9, omb=float(np.float32(0.1)), beta2=0.99, omb2=float(np.float32(0.01)),
          v0=1e-6)
YOGI_HP = dict(eta=0.01, tau=1e-3, beta=0.9, omb=float(np.float32(0.1)), omb2=float(np.float32(0.01)))
BLOCK = 50  # rows filled at a time

PREDICTIONS = {
    "adam": "takes k_yogi_step's time: the same 28 B per parameter",
    "adagrad": "takes k_yogi_step's time: the same 28 B per parameter",
    "avgm": "takes 20/28 of k_yogi_step's time: 20 B per parameter",
    "met_when": "the k_yogi_step time the rule's median implies (median x 28 / the rule's bytes) lies inside the "
                "min-to-max spread of k_yogi_step's repeats in the same run",
}


def timed(fns, reps: int):
    """(median, min, max) ms of each call of ``fns``, timed alternately after three warm-up calls of each."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]


def entry(ms, nbytes) -> dict:
    med, lo, hi = ms
    return {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes": int(nbytes),
            "TBps": round(nbytes / (med * 1e-3) / 1e12, 3)}


def steps(P: int, reps: int) -> dict:
    dev = torch.device("cuda:0")
    ld = (P + 63) // 64 * 64
    cur = torch.empty(ld, device=dev).normal_(0.0, 1.0)
    last = torch.empty(ld, device=dev).normal_(0.0, 1.0)
    m = torch.zeros(ld, device=dev)
    v = torch.full((ld,), 1e-6, device=dev)
    out = torch.empty(ld, device=dev)
    names, fns = ["k_yogi_step"], [lambda: kx.yogi_step(cur, last, m, v, out, P, init=False, **YOGI_HP)]
    for rule in RULES:
        for nt in (True, False):
            names.append(f"{rule}_nt_{'on' if nt else 'off'}")
            fns.append(lambda rule=rule, nt=nt: kso.step(rule, cur, last, m, v, out, P, init=False, nt=nt, **HP))
    times = dict(zip(names, timed(fns, reps)))
    res = {"P": P, "reps": reps, "buffers_reused_by_every_call": True,
           "k_yogi_step": dict(entry(times["k_yogi_step"], BYTES["yogi"] * P),
                               nt=bool(P * 28 > (256 << 20)))}
    y = res["k_yogi_step"]
    print(f"[P={P}] k_yogi_step {y}", flush=True)
    for rule in RULES:
        on, off = entry(times[f"{rule}_nt_on"], BYTES[rule] * P), entry(times[f"{rule}_nt_off"], BYTES[rule] * P)
        policy_nt = kso.plan(rule, P)["nt"]
        chosen = on if policy_nt else off
        implied = chosen["ms_median"] * 28 / BYTES[rule]
        res[rule] = {
            "nt_on": on, "nt_off": off, "policy_nt": bool(policy_nt),
            "policy_takes_the_faster_path": bool(chosen["ms_median"] <= (off if policy_nt else on)["ms_median"]),
            "predicted_ms": round(y["ms_median"] * BYTES[rule] / 28, 4),
            "implied_yogi_ms": round(implied, 4),
            "yogi_spread_ms": [y["ms_min"], y["ms_max"]],
            "prediction": "met" if y["ms_min"] <= implied <= y["ms_max"] else "missed",
        }
        print(f"[P={P}] {rule} {res[rule]}", flush=True)
    return res


def whole_round(K: int, P: int, reps: int) -> dict:
    dev = torch.device("cuda:0")
    ld = (P + 63) // 64 * 64
    x = torch.empty(K, ld, device=dev)
    for k0 in range(0, K, BLOCK):
        x[k0:k0 + BLOCK].normal_(0.0, 0.01)
    last = torch.empty(ld, device=dev).normal_(0.0, 1.0)
    mean = torch.empty(ld, device=dev)
    m = torch.zeros(ld, device=dev)
    v = torch.full((ld,), 1e-6, device=dev)
    out = torch.empty(ld, device=dev)
    den = float(np.float32(K))

    def yogi():
        kx.reduce(x, K, P, mean, denom=den, finalize=True)
        kx.yogi_step(mean, last, m, v, out, P, init=False, **YOGI_HP)

    def adam():
        kx.reduce(x, K, P, mean, denom=den, finalize=True)
        kso.step("adam", mean, last, m, v, out, P, init=False, **HP)

    ty, ta = timed([yogi, adam], reps)
    res = {"K": K, "P": P, "reps": reps, "fed_yogi_round": entry(ty, 4 * K * P + 4 * P + 28 * P),
           "fed_adam_round": entry(ta, 4 * K * P + 4 * P + 28 * P),
           "predicted": "the fed-adam round takes the fed-yogi round's time",
           "prediction": "met" if ty[1] <= ta[0] <= ty[2] else "missed"}
    print(f"[round {K} x {P}] {res}", flush=True)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--round-reps", type=int, default=5)
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("serveropt_measure: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("serveropt_measure: needs a GPU (a CPU run gives no time)")
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "build_defs": _native.build_info().get("defs", ""), "calls_per_median": a.reps,
           "bytes_per_parameter": BYTES, "predictions": PREDICTIONS}
    print(f"[predictions] {PREDICTIONS}", flush=True)  # on record before anything is timed
    res["steps"] = [steps(P, a.reps) for P in STEP_P]
    torch.cuda.empty_cache()
    res["round"] = whole_round(*ROUND, a.round_reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
