"""Time the finish of a deep trimmed-mean round (include/feddeeptrim.h) beside the register-selection trimmed round
and the plain round over the same device-resident rows, in one process ("Deep trimmed mean").

    python -u tools/deep_trim_measure.py [--configs c2,wide,head,rows] [--reps 20] [--out profiles/deep_trim_measure.json]

Per shape (c2: 100 x 1 M; wide: 100 x 25 M; head: 1000 x 25 M; rows: 4096 x 2 M) the rows are x_k = L + noise, staged
through ``adopt_resident``.  Two warm-up rounds, then ``--reps`` (>= 20) timed rounds each of
    DeviceRound.finalize_mean        one finalising fa_reduce                    4 K P + 4 P bytes
    TrimmedRound.finalize_mean       ft_select + ft_reduce at t = 1, 4, 16       8 K P + ...   (where 2t < K)
    DeepTrimmedRound.finalize_mean   fdt_reduce at the shape's deep trims        4 K P + 4 P bytes
alternating in that order, so that drift of the machine falls on all of them; device events around each finish;
medians.  Reported per finish: ms, TB/s on 4 K P bytes, the share of the 7.23 TB/s stream-read ceiling
(profiles/r01_hbm_stream_read_ceiling.json), the ratio to the plain finish of the same run, and for the deep rounds
the verdict on the prediction "one read of the rows at the ceiling": met within 1.15 x, else "missed, n x".
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
from fedscale_amd import kernels_deeptrim as kd  # noqa: E402

READ_CEILING = 7.23e12  # B/s
SHAPES = {"c2": (100, 1_000_000, (1, 16, 20, 49)), "wide": (100, 25_000_000, (1, 16, 20, 49)),
          "head": (1000, 25_000_000, (1, 16, 100, 200, 499)), "rows": (4096, 2_000_000, (1, 16, 409, 2047))}
OLD_TRIMS = (1, 4, 16)
BLOCK = 50  # rows filled at a time: no second K x ld temporary


def fill(x: torch.Tensor, last: torch.Tensor):
    """x_k = last + N(0, 0.01^2)."""
    for k0 in range(0, x.shape[0], BLOCK):
        b = x[k0:k0 + BLOCK]
        b.normal_(0.0, 0.01)
        b.add_(last)


def measure(name: str, K: int, P: int, deep_trims, reps: int) -> dict:
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.deep_trim_round import DeepTrimmedRound, DeepTrimSpec
    from fedscale_amd.round import DeviceRound
    from fedscale_amd.trim_round import TrimmedRound, TrimSpec

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    st = ClientStaging(L, dev, K, bulk=False)
    fill(st.x, torch.empty(L.ld, device=dev).normal_(0.0, 1.0))
    den = float(np.float32(K))
    out = torch.empty(L.ld, device=dev)
    side = torch.zeros(L.ldq, dtype=torch.float64, device=dev)

    def maker(cls, *spec):
        def make():
            r = cls(L, dev, K, *spec, staging=st, capacity=K)
            r.adopt_resident(K)
            return lambda: r.finalize_mean(den, float(K), out=out, cur_side=side)
        return make

    names = ["device_round_finish"]
    makers = [maker(DeviceRound, "fedavg")]
    for t in OLD_TRIMS:
        if 2 * t < K:
            names.append(f"trimmed_round_finish_t{t}")
            makers.append(maker(TrimmedRound, TrimSpec(t)))
    for t in deep_trims:
        names.append(f"deep_trimmed_round_finish_t{t}")
        makers.append(maker(DeepTrimmedRound, DeepTrimSpec(t)))
    ms = [[] for _ in makers]
    for rep in range(2 + reps):  # two warm-up rounds of each
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
    rows = 4 * K * P
    floor_ms = rows / READ_CEILING * 1e3
    res = {"config": name, "K": K, "P": P, "ld": L.ld, "reps": reps, "cus": cus, "fdt_plan": kd.plan(cus, K, P, 1),
           "floor_ms_one_read_at_ceiling": round(floor_ms, 4)}
    base = float(np.median(ms[0]))
    for k, m in zip(names, ms):
        med = float(np.median(m))
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(m), 4), "ms_max": round(max(m), 4),
                  "TBps_on_4KP": round(rows / (med * 1e-3) / 1e12, 3),
                  "share_of_read_ceiling": round(rows / (med * 1e-3) / READ_CEILING, 3),
                  "ratio_to_device_round_finish": round(med / base, 4)}
        if k.startswith("deep"):
            n = med / floor_ms
            res[k]["one_read_at_ceiling"] = "met" if n <= 1.15 else f"missed, {n:.2f} x"
        print(f"[{name}] {k} {res[k]}", flush=True)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="c2,wide,head,rows")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("deep_trim_measure: --reps must be at least 20")
    for c in a.configs.split(","):
        if c not in SHAPES:
            raise SystemExit(f"deep_trim_measure: unknown config {c!r} (known: {', '.join(SHAPES)})")
    if not torch.cuda.is_available():
        raise SystemExit("deep_trim_measure: needs a GPU (a CPU run gives no time)")
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "read_ceiling_Bps": READ_CEILING, "shapes": []}
    for c in a.configs.split(","):
        K, P, trims = SHAPES[c]
        res["shapes"].append(measure(c, K, P, trims, a.reps))
        torch.cuda.empty_cache()
        if a.out:  # after every shape: a later shape that runs out of time loses nothing
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
