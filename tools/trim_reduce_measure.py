"""Time the kernels of the coordinate-wise trimmed mean (include/fedtrim.h) beside fa_reduce over the same rows, in
one process.

    python -u tools/trim_reduce_measure.py [--configs head,c2] [--reps 30] [--out profiles/trim_reduce_measure.json]

Per shape (head: 1000 x 25 M, the headline; c2: config 2's 100 x 1 M) the device-resident rows are x_k = L + noise.
Three warm-up calls, then ``--reps`` (>= 20) timed calls each of
    fa_reduce            weighted, no finalize                         4 K P +  4 P bytes
    ft_select            at t = 1, 4, 16 (depths T = 1, 4, 16)          4 K P + 12 P bytes
    ft_reduce            at the same t, without the drop counts        4 K P + 16 P bytes
    ft_reduce + dropped  the same with the int64 [K, 2] table
    fa_reduce            once more: the spread this run itself shows for the same kernel
alternating in that order, so that drift of the machine falls on all of them; device events around each wrapper
call; medians.  Reported per kernel: ms per call, TB/s on its algorithmic bytes, the share of the 7.23 TB/s
stream-read ceiling (profiles/r01_hbm_stream_read_ceiling.json) and the ratio to fa_reduce of the same run.  Then the
whole finish of a device-resident round (``adopt_resident``): ``TrimmedRound.finalize_mean`` (select, reduce with the
drop counts) at each t against ``DeviceRound.finalize_mean`` (one finalising fa_reduce), alternating, ``--round-reps``
each.
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
from fedscale_amd import kernels_trim as kt  # noqa: E402

READ_CEILING = 7.23e12  # B/s
SHAPES = {"head": (1000, 25_000_000), "c2": (100, 1_000_000)}
TRIMS = (1, 4, 16)
BLOCK = 50  # rows filled at a time: no second K x ld temporary


def fill(x: torch.Tensor, last: torch.Tensor):
    """x_k = last + N(0, 0.01^2)."""
    for k0 in range(0, x.shape[0], BLOCK):
        b = x[k0:k0 + BLOCK]
        b.normal_(0.0, 0.01)
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
    from fedscale_amd.round import DeviceRound
    from fedscale_amd.trim_round import TrimmedRound, TrimSpec

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    st = ClientStaging(L, dev, K, bulk=False)
    x, ld = st.x, L.ld
    last = torch.empty(ld, device=dev).normal_(0.0, 1.0)
    fill(x, last)
    w = torch.ones(K, dtype=torch.float32, device=dev)
    out_a, out_t = torch.empty(ld, device=dev), torch.empty(ld, device=dev)
    thr = {t: kt.thresholds(P, dev) for t in TRIMS}
    dropped = torch.zeros((K, 2), dtype=torch.int64, device=dev)
    res = {"config": name, "K": K, "P": P, "ld": ld, "reps": reps, "cus": cus,
           "launches": {"fa_reduce": kx.reduce_launches(K, P, True)},
           "ft_plan": {str(t): kt.plan(cus, K, P, t) for t in TRIMS}}

    def select(t):
        return lambda: kt.select(x, K, P, t, *thr[t])

    def reduce(t, counts):
        lo, hi, ties = thr[t]
        return lambda: kt.reduce_trim(x, K, P, t, out_t, lo=lo, hi=hi, ties=ties, dropped=dropped if counts else None)

    fns, names = [lambda: kx.reduce(x, K, P, out_a, a=w)], ["fa_reduce_weighted"]
    rows = 4 * K * P
    nbytes = [rows + 4 * P]
    for t in TRIMS:
        fns += [select(t), reduce(t, False), reduce(t, True)]
        names += [f"ft_select_t{t}", f"ft_reduce_t{t}", f"ft_reduce_dropped_t{t}"]
        nbytes += [rows + 12 * P, rows + 16 * P, rows + 16 * P]
    fns.append(fns[0])
    names.append("fa_reduce_weighted_again")
    nbytes.append(rows + 4 * P)
    ts = timed(fns, reps)
    for k, tm, nb in zip(names, ts, nbytes):
        res[k] = entry(tm, nb, None if k == "fa_reduce_weighted" else ts[0][0])
        print(f"[{name}] {k} {res[k]}", flush=True)
    res["fa_reduce_spread"] = round(abs(ts[-1][0] / ts[0][0] - 1.0), 4)
    res["dropped_sum_check"] = bool(int(dropped.sum()) % (2 * P) == 0)  # every call adds 2 t P
    del out_a, out_t, thr
    if round_reps <= 0:
        return res
    # the whole finish of a device-resident round
    den = float(np.float32(K))
    out = torch.empty(ld, device=dev)
    side = torch.zeros(L.ldq, dtype=torch.float64, device=dev)

    def plain_round():
        r = DeviceRound(L, dev, K, "fedavg", capacity=K, staging=st)
        r.adopt_resident(K)
        return lambda: r.finalize_mean(den, float(K), out=out, cur_side=side)

    def trimmed_round(t):
        def make():
            r = TrimmedRound(L, dev, K, TrimSpec(t), staging=st, capacity=K)
            r.adopt_resident(K)
            return lambda: r.finalize_mean(den, float(K), out=out, cur_side=side)
        return make

    makers = [plain_round] + [trimmed_round(t) for t in TRIMS]
    ms = [[] for _ in makers]
    for rep in range(2 + round_reps):  # two warm-up rounds of each
        for i, make in enumerate(makers):
            fin = make()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fin()
            b.record()
            b.synchronize()
            if rep >= 2:
                ms[i].append(a.elapsed_time(b))
    tm = [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]
    res["device_round_finish"] = entry(tm[0])
    print(f"[{name}] device_round_finish {res['device_round_finish']}", flush=True)
    for t, v in zip(TRIMS, tm[1:]):
        k = f"trimmed_round_finish_t{t}"
        res[k] = entry(v)
        res[k]["ratio_to_device_round_finish"] = round(v[0] / tm[0][0], 4)
        print(f"[{name}] {k} {res[k]}", flush=True)
    res["round_reps"] = round_reps
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="head,c2")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--round-reps", type=int, default=10)
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("trim_reduce_measure: --reps must be at least 20")
    for c in a.configs.split(","):
        if c not in SHAPES:
            raise SystemExit(f"trim_reduce_measure: unknown config {c!r} (known: {', '.join(SHAPES)})")
    if not torch.cuda.is_available():
        raise SystemExit("trim_reduce_measure: needs a GPU (a CPU run gives no time)")
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "read_ceiling_Bps": READ_CEILING, "trims": list(TRIMS), "shapes": []}
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
