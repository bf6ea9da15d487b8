"""Time fvt_count + fvt_finish (majority-vote sign rows, include/fedvote.h) beside fsg_reduce (sign1) and fa_reduce
(fp32) in one process ("Majority-vote tally").

    python -u tools/vote_reduce_measure.py [--configs c2,mid,head] [--reps 30] [--out profiles/vote_reduce_measure.json]

Per shape (c2: config 2's 100 x 1 M; mid: 100 x 25 M; head: 1000 x 25 M, the headline) the stagings are filled on the
device: random bits, scales near 0.01, N(0, 0.01^2) fp32 rows.  Device events around each wrapper call, three warm-up
calls, then ``--reps`` (>= 20) timed calls per kernel, the kernels alternating back to back so that drift of the
machine falls on all of them; medians with min and max.  For fvt_count: the bytes it reads and writes against the
7.23 TB/s stream-read ceiling (profiles/r01_hbm_stream_read_ceiling.json), the vector lane-operations of its row loop
(5 per row and dword, the figure of the prediction; the compiled loop has 4.8) per second against the 78.6 T lane-operations/s of the spec sheet
(256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz), and at the headline the ratios to the two times predicted before the kernel
existed — 0.45 ms from its bytes, 0.05 ms from its operations — with a verdict each: met within 10 %, or missed.
Before anything is timed, fvt_count's result at the shape is compared with a tally of the same rows by torch integer
ops on the device (``device_tally``); a mismatch ends the run.
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
from fedscale_amd import kernels_sign as kg  # noqa: E402
from fedscale_amd import kernels_vote as kv  # noqa: E402

READ_CEILING = 7.23e12  # B/s
LANE_OPS = 78.6e12      # vector lane-operations/s
OPS_PER_ROW_DWORD = 5   # the prediction's figure for the row loop (the compiled loop has 4.8: DESIGN.md)
SHAPES = {"c2": (100, 1_000_000), "mid": (100, 25_000_000), "head": (1000, 25_000_000)}
PREDICTED_MS = {"bytes": 0.45, "operations": 0.05}  # fvt_count at the headline, made before the kernel existed
BLOCK = 50  # rows filled at a time


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
    floor_ms = nbytes / READ_CEILING * 1e3
    return {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes": int(nbytes),
            "TBps": round(nbytes / (med * 1e-3) / 1e12, 3), "byte_floor_ms": round(floor_ms, 4),
            "share_of_read_ceiling": round(floor_ms / med, 4)}


def device_tally(bits: torch.Tensor, n: int, P: int, rows: int = 16) -> torch.Tensor:
    """int32 [P]: the set bits per column of bits[:n], by torch integer ops, ``rows`` rows at a time."""
    PB = (P + 7) // 8
    acc = torch.zeros(PB, 8, dtype=torch.int32, device=bits.device)
    for k in range(0, n, rows):
        b = bits[k:min(n, k + rows), :PB]
        for i in range(8):
            acc[:, i] += ((b >> i) & 1).sum(0, dtype=torch.int32)
    return acc.reshape(-1)[:P]


def measure(name: str, K: int, P: int, reps: int, with_fp32: bool) -> dict:
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ld = (P + 63) // 64 * 64
    bits = torch.empty(K, kv.bit_stride(P), dtype=torch.uint8, device=dev)
    scales = torch.empty(K, kg.scale_stride(P), device=dev).uniform_(0.005, 0.015)
    x32 = torch.empty(K, ld, device=dev) if with_fp32 else None
    for k0 in range(0, K, BLOCK):
        bits[k0:k0 + BLOCK].random_(0, 256)
        if with_fp32:
            x32[k0:k0 + BLOCK].normal_(0.0, 0.01)
    cnt = torch.zeros(ld, dtype=torch.int32, device=dev)
    L = torch.randn(ld, device=dev)
    out = [torch.empty(ld, device=dev) for _ in range(3)]
    den = float(np.float32(K))
    fns = [lambda: kv.count_votes(bits, K, P, cnt), lambda: kv.finish_vote(cnt, L, P, K, 0.01, out[0]),
           lambda: kg.reduce_sign(bits, scales, K, P, out[1])]
    if with_fp32:
        fns.append(lambda: kx.reduce(x32, K, P, out[2], denom=den, finalize=True))
    fns[0]()
    if not torch.equal(cnt[:P], device_tally(bits, K, P)):
        raise SystemExit(f"[{name}] fvt_count differs from the torch tally of the same rows")
    t = timed(fns, reps)
    res = {"config": name, "K": K, "P": P, "reps": reps, "fvt_count_plan": kv.count_votes_plan(cus, K, P),
           "fvt_count_equals_torch_tally": True, "fvt_count": entry(t[0], K * kv.bit_bytes(P) + 4 * P), "fvt_finish": entry(t[1], 12 * P),
           "fsg_reduce": entry(t[2], K * (kg.bit_bytes(P) + 4 * kg.blocks(P)) + 4 * P)}
    if with_fp32:
        res["fa_reduce"] = entry(t[3], 4 * K * P + 4 * P)
    c = res["fvt_count"]
    ops = OPS_PER_ROW_DWORD * K * ((P + 31) // 32)
    c.update(lane_operations=ops, lane_ops_per_s_over_spec=round(ops / (t[0][0] * 1e-3) / LANE_OPS, 4),
             count_plus_finish_ms=round(t[0][0] + t[1][0], 4), ratio_to_fsg_reduce=round(t[0][0] / t[2][0], 4))
    if name == "head":
        c["predicted_ms"] = dict(PREDICTED_MS)
        c["ratio_to_predictions"] = {k: round(t[0][0] / v, 3) for k, v in PREDICTED_MS.items()}
        c["verdicts"] = {k: "met" if t[0][0] <= 1.1 * v else "missed" for k, v in PREDICTED_MS.items()}
        c["bytes_bind"] = bool(c["share_of_read_ceiling"] >= 0.9)
    for k in res:
        if isinstance(res[k], dict):
            print(f"[{name}] {k} {res[k]}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,mid,head")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-fp32-at-head", action="store_true", help="skip fa_reduce's 100 GB staging at the headline")
    ap.add_argument("--out", default="profiles/vote_reduce_measure.json")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be >= 20")
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "build_defs": _native.build_info().get("defs", ""), "read_ceiling_Bps": READ_CEILING,
           "lane_ops_per_s": LANE_OPS, "lane_ops_per_row_dword": OPS_PER_ROW_DWORD, "shapes": []}
    for name in a.configs.split(","):
        K, P = SHAPES[name]
        res["shapes"].append(measure(name, K, P, a.reps, not (name == "head" and a.no_fp32_at_head)))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out, flush=True)


if __name__ == "__main__":
    main()
