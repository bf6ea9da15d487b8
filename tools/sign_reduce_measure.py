"""Time fsg_reduce (1-bit sign delta rows, include/fedsign.h) beside fq_reduce (MXFP8), fh_reduce (bf16) and fa_reduce
(fp32) in one process.

    python -u tools/sign_reduce_measure.py [--configs c2,mid,head] [--reps 30] [--pcie K] \
        [--out profiles/sign_reduce_measure.json]

Per shape (c2: config 2's 100 x 1 M; mid: 100 x 25 M; head: 1000 x 25 M, the headline) the four stagings are filled
on the device: random sign bits under scales near 0.01, random finite e4m3 codes under scale bytes near 2^-7, and
N(0, 0.01^2) rows in bf16 and fp32.  Device events around each wrapper call, three warm-up calls, then ``--reps``
(>= 20) timed calls per kernel, the kernels alternating back to back so that drift of the machine falls on all of
them; medians.  Per kernel: the time, the bytes it has to read and write over it against the 7.23 TB/s stream-read
ceiling (profiles/r01_hbm_stream_read_ceiling.json); for fsg_reduce also the (row x column) pairs per second against
the 78.6 T lane-operations/s of the spec sheet (256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz), and at the headline the
ratios to the two predictions made before the kernel existed: 0.49 ms from its bytes, 0.95 ms from three vector
operations per pair.  At the headline's width, fsg_sign_row on one row.

``--pcie K`` adds the payload-to-model round of the headline's model from pickled executor payloads, float32 and
sign in the same process: K times ``ingress.loads`` of one payload + the staging's ``put``, then the finishing reduce;
host wall clock from the first ``loads`` to a device synchronise after the reduce, after 5 warm-up uploads.
Updates/s, and what the payload bytes predict against the float32 rate.
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
from fedscale_amd import kernels_half as kh  # noqa: E402
from fedscale_amd import kernels_quant as kq  # noqa: E402
from fedscale_amd import kernels_sign as kg  # noqa: E402

READ_CEILING = 7.23e12  # B/s
LANE_OPS = 78.6e12      # vector lane-operations/s: 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz
SHAPES = {"c2": (100, 1_000_000), "mid": (100, 25_000_000), "head": (1000, 25_000_000)}
PREDICTED_MS = {"bytes": 0.49, "three_vector_ops_per_pair": 0.95}  # at the headline, made before the kernel existed
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


def entry(ms, nbytes=None) -> dict:
    med, lo, hi = ms
    r = {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
    if nbytes is not None:
        floor_ms = nbytes / READ_CEILING * 1e3
        r.update(bytes=int(nbytes), TBps=round(nbytes / (med * 1e-3) / 1e12, 3), byte_floor_ms=round(floor_ms, 4),
                 share_of_read_ceiling=round(floor_ms / med, 4))
    return r


def measure(name: str, K: int, P: int, reps: int) -> dict:
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ld = (P + 63) // 64 * 64
    ldb, lds = kg.bit_stride(P), kg.scale_stride(P)
    den = float(np.float32(K))
    x32 = torch.empty(K, ld, device=dev)
    x16 = torch.empty(K, ld, dtype=torch.bfloat16, device=dev)
    q8 = torch.empty(K, ld, dtype=torch.uint8, device=dev)
    q8s = torch.empty(K, ld // kq.BLOCK, dtype=torch.uint8, device=dev)
    bits = torch.empty(K, ldb, dtype=torch.uint8, device=dev)
    scales = torch.empty(K, lds, device=dev).uniform_(0.005, 0.015)
    for k0 in range(0, K, BLOCK):
        x32[k0:k0 + BLOCK].normal_(0.0, 0.01)
        x16[k0:k0 + BLOCK].copy_(x32[k0:k0 + BLOCK])
        q8[k0:k0 + BLOCK].random_(0, 0x78)  # finite codes
        q8s[k0:k0 + BLOCK].random_(118, 124)
        bits[k0:k0 + BLOCK].random_(0, 256)
    out = [torch.empty(ld, device=dev) for _ in range(4)]
    tg, tq, th, ta = timed([lambda: kg.reduce_sign(bits, scales, K, P, out[0]),
                            lambda: kq.reduce8(q8, q8s, K, P, out[1]),
                            lambda: kh.reduce16(x16, K, P, out[2], denom=den, finalize=True),
                            lambda: kx.reduce(x32, K, P, out[3], denom=den, finalize=True)], reps)
    NB = kg.blocks(P)
    b_sign = K * (kg.bit_bytes(P) + 4 * NB) + 4 * P
    res = {"config": name, "K": K, "P": P, "reps": reps, "fsg_reduce_plan": kg.reduce_sign_plan(cus, K, P),
           "fsg_reduce": entry(tg, b_sign),
           "fq_reduce": entry(tq, K * (P + kq.blocks(P)) + 4 * P),
           "fh_reduce_bf16": entry(th, 2 * K * P + 4 * P),
           "fa_reduce": entry(ta, 4 * K * P + 4 * P)}
    pairs = K * P
    g = res["fsg_reduce"]
    g.update(row_column_pairs=pairs, pairs_per_s=round(pairs / (tg[0] * 1e-3), 1),
             pairs_per_s_over_lane_ops_per_s=round(pairs / (tg[0] * 1e-3) / LANE_OPS, 4),
             lane_ops_per_pair_at_the_spec_rate=round(LANE_OPS * tg[0] * 1e-3 / pairs, 3),
             ratio_to_fq_reduce=round(tg[0] / tq[0], 4), ratio_to_fh_reduce_bf16=round(tg[0] / th[0], 4),
             ratio_to_fa_reduce=round(tg[0] / ta[0], 4),
             bytes_ratio_to_fq_reduce=round(b_sign / res["fq_reduce"]["bytes"], 4))
    if name == "head":
        g["predicted_ms"] = dict(PREDICTED_MS)
        g["ratio_to_predictions"] = {k: round(tg[0] / v, 3) for k, v in PREDICTED_MS.items()}
        g["beats_fq_reduce"] = bool(tg[0] < tq[0])
    for k in ("fsg_reduce", "fq_reduce", "fh_reduce_bf16", "fa_reduce"):
        print(f"[{name}] {k} {res[k]}", flush=True)
    if name == "head":
        x, base, r_in = x32[0], x32[1], x32[2]
        bo = torch.empty(NB * 32, dtype=torch.uint8, device=dev)
        so = torch.empty(NB, device=dev)
        ro = torch.empty(P, device=dev)
        (t,) = timed([lambda: kg.sign_row(x, base, r_in, P, bo, so, ro)], reps)
        res["fsg_sign_row"] = entry(t, 16 * P + NB * 36)  # x, base and the residual read, the residual written
        print(f"[{name}] fsg_sign_row {res['fsg_sign_row']}", flush=True)
    return res


def pcie_round(K: int, P: int) -> dict:
    """Updates/s of one K-upload round from pickled payloads: float32 (ClientStaging) and sign (SignStaging)."""
    import pickle
    import time

    from fedscale_amd import ingress
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.cloud.execution.sign_upload import compress_sign
    from fedscale_amd.sign_round import SignStaging

    dev = torch.device("cuda:0")
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    rng = np.random.default_rng(0)
    base = rng.standard_normal(P, dtype=np.float32)
    w = base + rng.standard_normal(P, dtype=np.float32) * np.float32(0.01)
    den = float(np.float32(K))
    out, chain = torch.empty(L.ld, device=dev), torch.zeros(L.ld, device=dev)
    last = torch.from_numpy(np.concatenate([base, np.zeros(L.ld - P, dtype=np.float32)])).to(dev)
    res = {"K": K, "P": P}
    for key in ("float32", "sign1"):
        if key == "float32":
            up, st = {"w": w}, ClientStaging(L, dev, K, bulk=False)
        else:
            up, st = compress_sign({"w": w}, {"w": base})[0], SignStaging(L, dev, K)
        payload = pickle.dumps({"client_id": 1, "update_weight": up, "moving_loss": 0.5})

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
            kg.reduce_sign(st.bits, st.scales, K, P, chain)
            kc.finish(chain, last, P, den, out)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[key] = {"payload_bytes": len(payload), "seconds": round(dt, 4), "updates_per_s": round(K / dt, 1),
                    "payload_GBps": round(K * len(payload) / dt / 1e9, 2)}
        print(f"[pcie] {key} {res[key]}", flush=True)
        del st
        torch.cuda.empty_cache()
    res["sign1"]["ratio_to_fp32_rate"] = round(res["sign1"]["updates_per_s"] / res["float32"]["updates_per_s"], 3)
    res["sign1"]["byte_prediction_of_that_ratio"] = round(res["float32"]["payload_bytes"] /
                                                          res["sign1"]["payload_bytes"], 3)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="c2,mid,head")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--pcie", type=int, default=0, metavar="K",
                   help="also time a K-upload round of the headline's model from pickled payloads (0: skip)")
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("sign_reduce_measure: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("sign_reduce_measure: needs a GPU (a CPU run gives no time)")
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "build_defs": _native.build_info().get("defs", ""), "read_ceiling_Bps": READ_CEILING,
           "lane_ops_per_s": LANE_OPS, "pcie_inclusive": "not measured", "shapes": []}
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
