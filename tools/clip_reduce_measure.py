"""Time the kernels of norm-clipped aggregation (include/fedclip.h) beside fa_reduce over the same rows, in one
process.

    python -u tools/clip_reduce_measure.py [--configs head,c2] [--reps 30] [--out profiles/clip_reduce_measure.json]

Per shape (head: 1000 x 25 M, the headline; c2: config 2's 100 x 1 M) the device-resident rows are x_k = L + noise
whose length grows with k, clipped at the median norm (half of the rows clipped).  Three warm-up calls, then
``--reps`` (>= 20) timed calls each of
    fa_reduce        weighted (the coefficients as weights), no finalize   4 K P + 4 P bytes
    fcl_reduce       the clipped chain                                     4 K P + 8 P bytes
    fcl_row_sqnorms  the norm pass                                         4 K P + 4 P bytes
    fa_reduce        once more: the spread this run itself shows for the same kernel
alternating in that order, so that drift of the machine falls on all of them; device events around each wrapper
call; medians.  Reported per kernel: ms per call, TB/s on its algorithmic bytes, the share of the 7.23 TB/s
stream-read ceiling (profiles/r01_hbm_stream_read_ceiling.json); fcl_reduce's and fcl_row_sqnorms' ratio to fa_reduce
of the same run, and fa_reduce's second series' ratio to its first.  Then the whole finish of a device-resident round:
``ClippedRound.finalize_mean`` (norms, coefficients, chain, finish) against ``DeviceRound.finalize_mean`` (one
finalising fa_reduce), alternating, ``--round-reps`` each.
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
from fedscale_amd import kernels_clip as kc  # noqa: E402

READ_CEILING = 7.23e12  # B/s
SHAPES = {"head": (1000, 25_000_000), "c2": (100, 1_000_000)}
BLOCK = 50  # rows filled at a time: no second K x ld temporary


def fill(x: torch.Tensor, last: torch.Tensor):
    """x_k = last + N(0, 0.01^2) * (1 + k / K): norms spread over a factor of two around their median."""
    K = x.shape[0]
    for k0 in range(0, K, BLOCK):
        b = x[k0:k0 + BLOCK]
        b.normal_(0.0, 0.01)
        s = 1.0 + torch.arange(k0, k0 + b.shape[0], device=x.device, dtype=torch.float32) / K
        b.mul_(s[:, None])
        b.add_(last)


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


def entry(ms, nbytes=None, base=None) -> dict:
    med, lo, hi = ms
    r = {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
    if nbytes is not None:
        r.update({"bytes": int(nbytes), "TBps": round(nbytes / (med * 1e-3) / 1e12, 3),
                  "share_of_read_ceiling": round(nbytes / (med * 1e-3) / READ_CEILING, 3)})
    if base is not None:
        r["ratio_to_fa_reduce"] = round(med / base, 4)
    return r


def measure(name: str, K: int, P: int, reps: int, round_reps: int) -> dict:
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.clip_round import ClippedRound, ClipSpec
    from fedscale_amd.round import DeviceRound

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    st = ClientStaging(L, dev, K, bulk=False)
    x, ld = st.x, L.ld
    last = torch.empty(ld, device=dev).normal_(0.0, 1.0)
    fill(x, last)
    sq = torch.empty(K, dtype=torch.float64, device=dev)
    ws = kc.workspace(K, P, dev)
    kc.row_sqnorms(x, K, P, last, sq, ws)
    M = float(sq.sqrt().median())
    c = torch.empty(K, dtype=torch.float32, device=dev)
    rej = torch.zeros(1, dtype=torch.int32, device=dev)
    kc.clip_coefs(sq, K, M, c, rej)
    out_a, out_c = torch.empty(ld, device=dev), torch.empty(ld, device=dev)
    res = {"config": name, "K": K, "P": P, "ld": ld, "reps": reps, "max_norm": M,
           "rows_clipped": int((c < 1).sum()), "rows_rejected": int(rej.cpu()[0]),
           "workspace_bytes": kc.workspace_bytes(K, P),
           "launches": {"fa_reduce": kx.reduce_launches(K, P, True), "fcl_reduce": len(kc.reduce_clip_plan(cus, K, P)),
                        "fcl_row_sqnorms": kc.norm_plan(cus, P)["launches"]},
           "fcl_reduce_plan": kc.reduce_clip_plan(cus, K, P), "fcl_norm_plan": kc.norm_plan(cus, P)}
    t = timed([lambda: kx.reduce(x, K, P, out_a, a=c),
               lambda: kc.reduce_clip(x, K, P, last, c, out_c),
               lambda: kc.row_sqnorms(x, K, P, last, sq, ws),
               lambda: kx.reduce(x, K, P, out_a, a=c)], reps)
    rows = 4 * K * P
    res["fa_reduce_weighted"] = entry(t[0], rows + 4 * P)
    res["fcl_reduce"] = entry(t[1], rows + 8 * P, t[0][0])
    res["fcl_row_sqnorms"] = entry(t[2], rows + 4 * P, t[0][0])
    res["fa_reduce_weighted_again"] = entry(t[3], rows + 4 * P, t[0][0])
    res["fa_reduce_spread"] = round(abs(t[3][0] / t[0][0] - 1.0), 4)
    for k in ("fa_reduce_weighted", "fcl_reduce", "fcl_row_sqnorms", "fa_reduce_weighted_again"):
        print(f"[{name}] {k} {res[k]}", flush=True)
    del sq, ws, out_a, out_c
    # the whole finish of a device-resident round
    den = float(np.float32(K))
    out = torch.empty(ld, device=dev)
    side = torch.zeros(L.ldq, dtype=torch.float64, device=dev)
    spec = ClipSpec(M)

    def plain_round():
        r = DeviceRound(L, dev, K, "fedavg", capacity=K, staging=st)
        r.adopt_resident(K)
        return lambda: r.finalize_mean(den, float(K), out=out, cur_side=side)

    def clipped_round():
        r = ClippedRound(L, dev, K, spec, staging=st, last_f32=last, capacity=K)
        r.adopt_resident(K)
        return lambda: r.finalize_mean(den, float(K), out=out, cur_side=side)

    if round_reps <= 0:
        return res
    ms = ([], [])
    for rep in range(2 + round_reps):  # two warm-up rounds of each
        for i, make in enumerate((plain_round, clipped_round)):
            fin = make()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fin()
            b.record()
            b.synchronize()
            if rep >= 2:
                ms[i].append(a.elapsed_time(b))
    tp, tc = [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]
    res["device_round_finish"] = entry(tp)
    res["clipped_round_finish"] = entry(tc)
    res["clipped_round_finish"]["ratio_to_device_round_finish"] = round(tc[0] / tp[0], 4)
    res["round_reps"] = round_reps
    print(f"[{name}] device_round_finish {res['device_round_finish']}", flush=True)
    print(f"[{name}] clipped_round_finish {res['clipped_round_finish']}", flush=True)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="head,c2")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--round-reps", type=int, default=10)
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("clip_reduce_measure: --reps must be at least 20")
    for c in a.configs.split(","):
        if c not in SHAPES:
            raise SystemExit(f"clip_reduce_measure: unknown config {c!r} (known: {', '.join(SHAPES)})")
    if not torch.cuda.is_available():
        raise SystemExit("clip_reduce_measure: needs a GPU (a CPU run gives no time)")
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "read_ceiling_Bps": READ_CEILING, "shapes": []}
    for c in a.configs.split(","):
        K, P = SHAPES[c]
        res["shapes"].append(measure(c, K, P, a.reps, a.round_reps))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
