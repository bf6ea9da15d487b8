"""Time fh_reduce (16-bit client rows, include/fedhalf.h) beside fa_reduce (fp32 rows) over the same values, in one
process.

    python -u tools/half_reduce_measure.py [--configs head,c2] [--reps 30] [--out profiles/half_reduce_measure.json]

Per shape (head: 1000 x 25 M, the headline; c2: config 2's 100 x 1 M) the device-resident finalising reduction
(FedAvg: unweighted, FA_FINALIZE) is timed on fp32 rows and on float16 and bfloat16 rows holding the SAME values
(the fp32 rows are filled with values both 16-bit formats hold exactly, so the three means must be — and are
checked to be — the same bits).  Device events around each call, three warm-up calls, then ``--reps`` (>= 20)
timed calls per kernel, interleaved fp32 / 16-bit so that drift of the machine falls on both; the median is
reported.  Bytes are what the algorithm needs: K x P row elements read once plus P fp32 results written.
Reported per kernel: ms per call, TB/s on those bytes, the share of the 7.23 TB/s stream-read ceiling
(profiles/r01_hbm_stream_read_ceiling.json) and the ratio to the fp32 time of the same run.

``--pcie K`` adds the PCIe-inclusive round of the headline's model from pickled executor payloads, per upload dtype
in the same process: K times ``ingress.loads`` of one payload (100 MB of float32, or 50 MB of float16 / bfloat16
bits) + the staging's ``put`` (host gather into a pinned row, H2D), then the finalising reduce; host wall clock from
the first ``loads`` to a device synchronise after the reduce, after 5 warm-up uploads.  Updates/s and GB/s of payload.
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
from fedscale_amd import kernels_half as kh  # noqa: E402

READ_CEILING = 7.23e12  # B/s
SHAPES = {"head": (1000, 25_000_000), "c2": (100, 1_000_000)}
BLOCK = 50  # rows filled / converted at a time: no second K x ld temporary


def fill(x: torch.Tensor):
    """N(0, 0.01) rounded to values float16 AND bfloat16 hold exactly: 8 significant bits, nothing below 2^-14."""
    for k0 in range(0, x.shape[0], BLOCK):
        b = x[k0:k0 + BLOCK]
        b.normal_(0.0, 0.01)
        b.copy_(b.to(torch.bfloat16))
        b.masked_fill_(b.abs() < 2.0 ** -14, 0.0)


def narrowed(x: torch.Tensor, dtype) -> torch.Tensor:
    x16 = torch.empty(x.shape, dtype=dtype, device=x.device)
    for k0 in range(0, x.shape[0], BLOCK):
        x16[k0:k0 + BLOCK].copy_(x[k0:k0 + BLOCK])
    return x16


def timed_pair(f32, f16, reps: int):
    """Median ms of each of two calls, timed alternately after three warm-up calls of each."""
    for _ in range(3):
        f32()
        f16()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(reps):
        for i, fn in enumerate((f32, f16)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]


def entry(ms, nbytes, ms32=None) -> dict:
    med, lo, hi = ms
    r = {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes": int(nbytes),
         "TBps": round(nbytes / (med * 1e-3) / 1e12, 3),
         "share_of_read_ceiling": round(nbytes / (med * 1e-3) / READ_CEILING, 3)}
    if ms32 is not None:
        r["ratio_to_fp32"] = round(med / ms32, 4)
    return r


def measure(name: str, K: int, P: int, reps: int) -> dict:
    dev = torch.device("cuda:0")
    ld = (P + 63) // 64 * 64
    den = float(np.float32(K))
    x = torch.empty(K, ld, dtype=torch.float32, device=dev)
    fill(x)
    out32, out16 = torch.empty(ld, device=dev), torch.empty(ld, device=dev)
    res = {"config": name, "K": K, "P": P, "ld": ld, "reps": reps,
           "launches": {"fa_reduce": kx.reduce_launches(K, P), "fh_reduce": kh.reduce16_launches(K, P)},
           "fh_reduce_plan": kh.reduce16_plan(torch.cuda.get_device_properties(0).multi_processor_count, K, P)}
    b32, b16 = 4 * K * P + 4 * P, 2 * K * P + 4 * P
    for key, dtype in (("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        x16 = narrowed(x, dtype)
        t32, t16 = timed_pair(lambda: kx.reduce(x, K, P, out32, denom=den, finalize=True),
                              lambda: kh.reduce16(x16, K, P, out16, denom=den, finalize=True), reps)
        if not torch.equal(out32[:P], out16[:P]):
            raise SystemExit(f"half_reduce_measure: {name} {key}: the 16-bit mean differs from the fp32 mean")
        res[f"fa_reduce_fp32_beside_{key}"] = entry(t32, b32)
        res[f"fh_reduce_{key}"] = entry(t16, b16, t32[0])
        print(f"[{name}] fp32 {res[f'fa_reduce_fp32_beside_{key}']}", flush=True)
        print(f"[{name}] {key} {res[f'fh_reduce_{key}']}", flush=True)
        del x16
        torch.cuda.empty_cache()
    res["means_bit_identical"] = True
    return res


def pcie_round(K: int, P: int) -> dict:
    """Updates/s of one K-upload round from pickled payloads, float32 (ClientStaging) and 16-bit (HalfStaging)."""
    import pickle
    import time

    from fedscale_amd import ingress
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.half_round import HalfStaging

    dev = torch.device("cuda:0")
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    w = np.random.default_rng(0).standard_normal(P, dtype=np.float32) * np.float32(0.01)
    den = float(np.float32(K))
    out = torch.empty(L.ld, device=dev)
    res = {"K": K, "P": P}
    for key in ("float32", "float16", "bfloat16"):
        if key == "float32":
            arr, st = w, ClientStaging(L, dev, K, bulk=False)
        else:
            arr = w.astype(np.float16) if key == "float16" else (w.view(np.uint32) >> 16).astype(np.uint16)
            st = HalfStaging(L, dev, K, key)
        payload = pickle.dumps({"client_id": 1, "update_weight": {"w": arr}, "moving_loss": 0.5})

        def upload(k):
            st.put(k, ingress.loads(payload)["update_weight"])

        for k in range(5):
            upload(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(K):
            upload(k)
        if key == "float32":
            st.drain()
            kx.reduce(st.x, K, P, out, denom=den, finalize=True)
        else:
            kh.reduce16(st.x16, K, P, out, denom=den, finalize=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[key] = {"payload_bytes": len(payload), "seconds": round(dt, 4), "updates_per_s": round(K / dt, 1),
                    "payload_GBps": round(K * len(payload) / dt / 1e9, 1)}
        print(f"[pcie] {key} {res[key]}", flush=True)
        del st
        torch.cuda.empty_cache()
    for key in ("float16", "bfloat16"):
        res[key]["ratio_to_fp32_rate"] = round(res[key]["updates_per_s"] / res["float32"]["updates_per_s"], 3)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="head,c2")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--pcie", type=int, default=0, metavar="K",
                   help="also time a K-upload round of the headline's model from pickled payloads (0: skip)")
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("half_reduce_measure: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("half_reduce_measure: needs a GPU (a CPU run gives no time)")
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "read_ceiling_Bps": READ_CEILING, "pcie_inclusive": "not measured", "shapes": []}
    for c in a.configs.split(","):
        K, P = SHAPES[c]
        res["shapes"].append(measure(c, K, P, a.reps))
        torch.cuda.empty_cache()
    if a.pcie > 0:
        res["pcie_inclusive"] = pcie_round(a.pcie, SHAPES["head"][1])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
