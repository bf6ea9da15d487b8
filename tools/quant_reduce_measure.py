"""Time fq_reduce (MXFP8 delta rows, include/fedquant.h) beside fh_reduce (bfloat16 rows) and fa_reduce (fp32 rows) in
one process.

    python -u tools/quant_reduce_measure.py [--configs head,c2] [--reps 30] [--pcie K] \
        [--out profiles/quant_reduce_measure.json]

Per shape (head: 1000 x 25 M, the headline; c2: config 2's 100 x 1 M) three stagings are filled on the device from
the same uploads x_k = L + N(0, 0.01^2): fp32 rows, their bfloat16 rounding, and the MXFP8 quantisation of x_k - L
(fq_quantize_row).  Device events around each call, three warm-up calls, then ``--reps`` (>= 20) timed calls per
kernel, the three kernels alternating so that drift of the machine falls on all of them; medians.  Bytes are what the
algorithm needs: the row elements read once (K x P x 4, x 2, x (1 + 1/32)) plus P fp32 results written.  Reported per
kernel: ms per call, TB/s on those bytes, the share of the 7.23 TB/s stream-read ceiling
(profiles/r01_hbm_stream_read_ceiling.json), the ratio to fa_reduce's and fh_reduce's time of the same run, and the
ratio to what the bytes predict (0.2578 x fa_reduce).  Then the whole finish of a device-resident round —
``QuantRound.finalize_mean`` (chain, fcl_finish), ``HalfRound.finalize_mean`` and ``DeviceRound.finalize_mean`` —
alternating, ``--round-reps`` each.

``--pcie K`` adds the payload-to-model round of the headline's model from pickled executor payloads, per upload format
in the same process: K times ``ingress.loads`` of one payload + the staging's ``put`` (host gather into a pinned row,
H2D), then the finishing reduce; host wall clock from the first ``loads`` to a device synchronise after the reduce,
after 5 warm-up uploads.  Updates/s and GB/s of payload.
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

READ_CEILING = 7.23e12  # B/s
SHAPES = {"head": (1000, 25_000_000), "c2": (100, 1_000_000)}
BLOCK = 50  # rows filled / converted at a time: no second K x ld temporary
BYTES_RATIO = (1 + 1 / 32) / 4  # what the row bytes predict for fq_reduce against fa_reduce


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
        r.update(bytes=int(nbytes), TBps=round(nbytes / (med * 1e-3) / 1e12, 3),
                 share_of_read_ceiling=round(nbytes / (med * 1e-3) / READ_CEILING, 3))
    return r


def measure(name: str, K: int, P: int, reps: int, round_reps: int) -> dict:
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.half_round import HalfRound, HalfStaging
    from fedscale_amd.quant_round import QuantRound, QuantStaging
    from fedscale_amd.round import DeviceRound

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    ld = L.ld
    den = float(np.float32(K))
    s32 = ClientStaging(L, dev, K, bulk=False)
    s16 = HalfStaging(L, dev, K, "bfloat16")
    s8 = QuantStaging(L, dev, K)
    last = torch.empty(ld, device=dev).normal_(0.0, 1.0)
    for k0 in range(0, K, BLOCK):
        b = s32.x[k0:k0 + BLOCK]
        b.normal_(0.0, 0.01)
        b.add_(last)
        s16.x16[k0:k0 + BLOCK].copy_(b)
    for k in range(K):
        kq.quantize_row(s32.x[k], last, P, s8.q8[k], s8.scales[k])
    torch.cuda.synchronize()
    out32, out16, out8 = (torch.empty(ld, device=dev) for _ in range(3))
    res = {"config": name, "K": K, "P": P, "ld": ld, "reps": reps, "fq_reduce_plan": kq.reduce8_plan(cus, K, P)}
    b32, b16, b8 = 4 * K * P + 4 * P, 2 * K * P + 4 * P, K * (P + kq.blocks(P)) + 4 * P
    t32, t16, t8 = timed([lambda: kx.reduce(s32.x, K, P, out32, denom=den, finalize=True),
                          lambda: kh.reduce16(s16.x16, K, P, out16, denom=den, finalize=True),
                          lambda: kq.reduce8(s8.q8, s8.scales, K, P, out8)], reps)
    # what the quantised chain computes, against the fp32 mean of the same uploads: the quantisation error only
    mean8 = torch.empty(ld, device=dev)
    kc.finish(out8, last, P, den, mean8)
    err = (mean8[:P] - out32[:P]).abs().max().item()
    res["fa_reduce_fp32"] = entry(t32, b32)
    res["fh_reduce_bfloat16"] = entry(t16, b16)
    res["fh_reduce_bfloat16"]["ratio_to_fa_reduce"] = round(t16[0] / t32[0], 4)
    res["fq_reduce_mxfp8"] = entry(t8, b8)
    res["fq_reduce_mxfp8"].update(ratio_to_fa_reduce=round(t8[0] / t32[0], 4),
                                  ratio_to_fh_reduce=round(t8[0] / t16[0], 4),
                                  ratio_to_byte_prediction=round(t8[0] / (BYTES_RATIO * t32[0]), 4))
    res["max_abs_difference_of_the_means_mxfp8_vs_fp32"] = err
    for k in ("fa_reduce_fp32", "fh_reduce_bfloat16", "fq_reduce_mxfp8"):
        print(f"[{name}] {k} {res[k]}", flush=True)
    if round_reps <= 0:
        return res
    side = torch.zeros(L.ldq, dtype=torch.float64, device=dev)

    def plain_round():
        r = DeviceRound(L, dev, K, "fedavg", capacity=K, staging=s32)
        r.adopt_resident(K)
        return lambda: r.finalize_mean(den, float(K), out=out32, cur_side=side)

    def half_round():
        r = HalfRound(L, dev, K, "fedavg", staging=s16, capacity=K)
        r.slot = r.n = K  # the uploads are already in the staging slots (as adopt_resident)
        return lambda: r.finalize_mean(den, float(K), out=out16, cur_side=side)

    def quant_round():
        r = QuantRound(L, dev, K, "fedavg", staging=s8, last_f32=last, capacity=K)
        r.adopt_resident(K)
        return lambda: r.finalize_mean(den, float(K), out=out8, cur_side=side)

    ms = ([], [], [])
    for rep in range(2 + round_reps):  # two warm-up rounds of each
        for i, make in enumerate((plain_round, half_round, quant_round)):
            fin = make()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fin()
            b.record()
            b.synchronize()
            if rep >= 2:
                ms[i].append(a.elapsed_time(b))
    tp, th, tq = [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]
    res["device_round_finish"] = entry(tp)
    res["half_round_finish"] = entry(th)
    res["quant_round_finish"] = entry(tq)
    res["half_round_finish"]["ratio_to_device_round_finish"] = round(th[0] / tp[0], 4)
    res["quant_round_finish"]["ratio_to_device_round_finish"] = round(tq[0] / tp[0], 4)
    res["round_reps"] = round_reps
    for k in ("device_round_finish", "half_round_finish", "quant_round_finish"):
        print(f"[{name}] {k} {res[k]}", flush=True)
    return res


def pcie_round(K: int, P: int) -> dict:
    """Updates/s of one K-upload round from pickled payloads: float32 (ClientStaging), bfloat16 (HalfStaging) and
    MXFP8 deltas (QuantStaging)."""
    import pickle
    import time

    from fedscale_amd import ingress
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.cloud.execution.quant_upload import compress_delta
    from fedscale_amd.half_round import HalfStaging
    from fedscale_amd.quant_round import QuantStaging

    dev = torch.device("cuda:0")
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    rng = np.random.default_rng(0)
    base = rng.standard_normal(P, dtype=np.float32)
    w = base + rng.standard_normal(P, dtype=np.float32) * np.float32(0.01)
    den = float(np.float32(K))
    out, chain = torch.empty(L.ld, device=dev), torch.zeros(L.ld, device=dev)
    last = torch.from_numpy(np.concatenate([base, np.zeros(L.ld - P, dtype=np.float32)])).to(dev)
    res = {"K": K, "P": P}
    for key in ("float32", "bfloat16", "mxfp8"):
        if key == "float32":
            up, st = {"w": w}, ClientStaging(L, dev, K, bulk=False)
        elif key == "bfloat16":
            up, st = {"w": (w.view(np.uint32) >> 16).astype(np.uint16)}, HalfStaging(L, dev, K, key)
        else:
            up, st = compress_delta({"w": w}, {"w": base}), QuantStaging(L, dev, K)
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
        elif key == "bfloat16":
            kh.reduce16(st.x16, K, P, out, denom=den, finalize=True)
        else:
            kq.reduce8(st.q8, st.scales, K, P, chain)
            kc.finish(chain, last, P, den, out)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[key] = {"payload_bytes": len(payload), "seconds": round(dt, 4), "updates_per_s": round(K / dt, 1),
                    "payload_GBps": round(K * len(payload) / dt / 1e9, 1)}
        print(f"[pcie] {key} {res[key]}", flush=True)
        del st
        torch.cuda.empty_cache()
    for key in ("bfloat16", "mxfp8"):
        res[key]["ratio_to_fp32_rate"] = round(res[key]["updates_per_s"] / res["float32"]["updates_per_s"], 3)
    res["mxfp8"]["byte_prediction_of_that_ratio"] = round(4 / (1 + 1 / 32), 3)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="head,c2")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--round-reps", type=int, default=10)
    p.add_argument("--pcie", type=int, default=0, metavar="K",
                   help="also time a K-upload round of the headline's model from pickled payloads (0: skip)")
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("quant_reduce_measure: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("quant_reduce_measure: needs a GPU (a CPU run gives no time)")
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "build_defs": _native.build_info().get("defs", ""), "read_ceiling_Bps": READ_CEILING,
           "byte_prediction_fq_over_fa": round(BYTES_RATIO, 4), "pcie_inclusive": "not measured", "shapes": []}
    for c in a.configs.split(","):
        K, P = SHAPES[c]
        res["shapes"].append(measure(c, K, P, a.reps, a.round_reps))
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
