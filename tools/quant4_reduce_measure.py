"""Time fq4_reduce (MXFP4 delta rows, include/fedquant4.h) beside fq_reduce (MXFP8), fsg_reduce (sign1) and fa_reduce
(fp32 rows) in one process, and compute the fidelity of the three lossy encoders on the CPU.

    python -u tools/quant4_reduce_measure.py [--configs c2,mid,head] [--reps 30] [--pcie K] \
        [--out profiles/quant4_reduce_measure.json]
    python -u tools/quant4_reduce_measure.py --fidelity-only          # no GPU needed

Per shape (c2: 100 x 1 M, mid: 100 x 25 M, head: 1000 x 25 M, the headline) four stagings are filled on the device
from the same uploads x_k = L + N(0, 0.01^2): fp32 rows and the MXFP8 and MXFP4 encodings of x_k - L
(fq_quantize_row, fq4_quantize_row); the sign1 rows are random bits under scales of that magnitude.  Device events
around each call, three warm-up calls, then ``--reps`` (>= 20) timed calls per kernel, the kernels alternating so
that drift of the machine falls on all of them; medians.  Bytes are what the algorithm needs: the staged rows read once plus P fp32 results written.  Reported per
kernel: ms per call, TB/s on those bytes, the share of the 7.23 TB/s stream-read ceiling
(profiles/r01_hbm_stream_read_ceiling.json), and for fq4_reduce the ratios to the other kernels of the same run and to
the two times predicted before the kernel ran:

    by bytes        (17/32 K P + 4 P) B / 7.23 TB/s                       1.85 ms at the headline
    by operations   K P lane-operations (16 scaled converts and 16 packed adds per 32 columns: one per column)
                    / 78.6 T lane-operations/s                            0.32 ms at the headline

with a verdict each (met: within 10 %).  Then the whole finish of a device-resident round — ``Quant4Round``,
``QuantRound``, ``SignRound`` and ``DeviceRound`` ``.finalize_mean`` — alternating, ``--round-reps`` each.

``--pcie K`` adds the payload-to-model round of the headline's model from pickled executor payloads, float32 against
MXFP4: K times ``ingress.loads`` of one payload + the staging's ``put``, then the finishing reduce; host wall clock to a
device synchronise after the reduce, after 5 warm-up uploads.

Fidelity (always, on the CPU, from the host encoders of the three formats): the share of the update's energy the
dequantised upload keeps, 1 - |d - deq|^2 / |d|^2, and the relative error |d - deq| / |d|, for a Gaussian, a
Student-t (1.5 degrees of freedom) and a 1 %-non-zero Gaussian update of 2^20 parameters, seeded.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

READ_CEILING = 7.23e12  # B/s
LANE_OPS = 78.6e12      # vector lane-operations/s (the spec sheet's)
SHAPES = {"c2": (100, 1_000_000), "mid": (100, 25_000_000), "head": (1000, 25_000_000)}
BYTES_PER_COLUMN = 17 / 32
OPS_PER_COLUMN = 1.0


def predictions(K: int, P: int) -> dict:
    """ms of fq4_reduce at (K, P), written before the kernel ran on a card."""
    return {"bytes": (BYTES_PER_COLUMN * K * P + 4 * P) / READ_CEILING * 1e3,
            "operations": OPS_PER_COLUMN * K * P / LANE_OPS * 1e3}


def fidelity(n: int = 1 << 20, seed: int = 0) -> dict:
    """Energy kept and relative error of MXFP4, MXFP8 and sign1 on three update distributions (CPU)."""
    from fedscale_amd.cloud.execution import quant4_upload, quant_upload, sign_upload

    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n)
    updates = {"gaussian": g * 0.01, "student_t_1.5": rng.standard_t(1.5, n) * 0.01,
               "one_percent_nonzero": np.where(rng.random(n) < 0.01, g, 0.0) * 0.01}
    out = {}
    for name, d in updates.items():
        d = d.astype(np.float32)
        codes, s = quant_upload.quantize_host(d)
        deq8 = (torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
                * np.repeat(np.ldexp(1.0, s.astype(np.int64) - 127), 32))[:n]
        errs = {"mxfp4": quant4_upload.quantize_host(d)[2].astype(np.float64), "mxfp8": d - deq8,
                "sign1": sign_upload.encode_host(d)[2].astype(np.float64)}
        e2 = float((d.astype(np.float64) ** 2).sum())
        out[name] = {k: {"energy_kept": round(1 - float((r ** 2).sum()) / e2, 4),
                         "relative_error": round(float(np.sqrt((r ** 2).sum() / e2)), 4)} for k, r in errs.items()}
        print(f"[fidelity] {name} {out[name]}", flush=True)
    return out


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


def measure(P: int, names, reps: int, round_reps: int) -> list:
    """The shapes ``names`` (all of P columns) over one set of stagings filled for the largest K."""
    from fedscale_amd import kernels as kx
    from fedscale_amd import kernels_clip as kc
    from fedscale_amd import kernels_quant as kq
    from fedscale_amd import kernels_quant4 as kq4
    from fedscale_amd import kernels_sign as kg
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.quant4_round import Quant4Round, Quant4Staging
    from fedscale_amd.quant_round import QuantRound, QuantStaging
    from fedscale_amd.round import DeviceRound
    from fedscale_amd.sign_round import SignRound, SignStaging

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Kmax = max(SHAPES[n][0] for n in names)
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    ld = L.ld
    s32, s8 = ClientStaging(L, dev, Kmax, bulk=False), QuantStaging(L, dev, Kmax)
    s4, s1 = Quant4Staging(L, dev, Kmax), SignStaging(L, dev, Kmax)
    last = torch.empty(ld, device=dev).normal_(0.0, 1.0)
    for k in range(Kmax):
        row = s32.x[k]
        row.normal_(0.0, 0.01)
        row.add_(last)
        kq.quantize_row(row, last, P, s8.q8[k], s8.scales[k])
        kq4.quantize_row4(row, last, None, P, s4.q4[k], s4.scales[k])
    s1.bits.random_(0, 256)  # (a staged sign row is narrower than what fsg_sign_row writes for a partial last block;
    s1.scales.uniform_(0.005, 0.015)  # random bits under scales of the updates' magnitude take the same time)
    torch.cuda.synchronize()
    o32, o8, o4, o1 = (torch.empty(ld, device=dev) for _ in range(4))
    side = torch.zeros(L.ldq, dtype=torch.float64, device=dev)
    results = []
    for name in names:
        K = SHAPES[name][0]
        den = float(np.float32(K))
        res = {"config": name, "K": K, "P": P, "ld": ld, "reps": reps, "fq4_reduce_plan": kq4.reduce4_plan(cus, K, P)}
        nbytes = {"fa_reduce_fp32": 4 * K * P + 4 * P, "fq_reduce_mxfp8": K * (P + kq.blocks(P)) + 4 * P,
                  "fq4_reduce_mxfp4": K * (kq4.code_bytes(P) + kq4.blocks(P)) + 4 * P,
                  "fsg_reduce_sign1": K * (kg.bit_bytes(P) + 4 * kg.blocks(P)) + 4 * P}
        t = dict(zip(nbytes, timed([lambda: kx.reduce(s32.x, K, P, o32, denom=den, finalize=True),
                                    lambda: kq.reduce8(s8.q8, s8.scales, K, P, o8),
                                    lambda: kq4.reduce4(s4.q4, s4.scales, K, P, o4),
                                    lambda: kg.reduce_sign(s1.bits, s1.scales, K, P, o1)], reps)))
        for k, ms in t.items():
            res[k] = entry(ms, nbytes[k])
        t4 = t["fq4_reduce_mxfp4"][0]
        pred = predictions(K, P)
        c = res["fq4_reduce_mxfp4"]
        c.update({f"ratio_to_{k.split('_')[0]}_reduce": round(t4 / ms[0], 4) for k, ms in t.items()
                  if k != "fq4_reduce_mxfp4"})
        c.update(lane_ops_per_s_over_spec=round(OPS_PER_COLUMN * K * P / (t4 * 1e-3) / LANE_OPS, 4),
                 predicted_ms={k: round(v, 4) for k, v in pred.items()},
                 ratio_to_predictions={k: round(t4 / v, 3) for k, v in pred.items()},
                 verdicts={k: "met" if t4 <= 1.1 * v else "missed" for k, v in pred.items()})
        # what the 4-bit chain computes, against the fp32 mean of the same uploads: the quantisation error only
        mean4 = torch.empty(ld, device=dev)
        kc.finish(o4, last, P, den, mean4)
        res["max_abs_difference_of_the_means_mxfp4_vs_fp32"] = (mean4[:P] - o32[:P]).abs().max().item()
        for k in nbytes:
            print(f"[{name}] {k} {res[k]}", flush=True)
        if round_reps > 0:
            def rnd(cls, st, out, **kw):
                def make():
                    r = cls(L, dev, K, "fedavg", staging=st, capacity=K, **kw)
                    r.adopt_resident(K)
                    return lambda: r.finalize_mean(den, float(K), out=out, cur_side=side)
                return make

            makers = {"device_round_finish": rnd(DeviceRound, s32, o32),
                      "quant_round_finish": rnd(QuantRound, s8, o8, last_f32=last),
                      "quant4_round_finish": rnd(Quant4Round, s4, o4, last_f32=last),
                      "sign_round_finish": rnd(SignRound, s1, o1, last_f32=last)}
            ms = {k: [] for k in makers}
            for rep in range(2 + round_reps):  # two warm-up rounds of each
                for k, make in makers.items():
                    fin = make()
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fin()
                    b.record()
                    b.synchronize()
                    if rep >= 2:
                        ms[k].append(a.elapsed_time(b))
            for k, m in ms.items():
                res[k] = entry((float(np.median(m)), float(min(m)), float(max(m))))
                res[k]["ratio_to_device_round_finish"] = round(res[k]["ms_median"] /
                                                               float(np.median(ms["device_round_finish"])), 4)
                print(f"[{name}] {k} {res[k]}", flush=True)
            res["round_reps"] = round_reps
        results.append(res)
    return results


def pcie_round(K: int, P: int) -> dict:
    """Updates/s of one K-upload round from pickled payloads: float32 (ClientStaging) and MXFP4 (Quant4Staging)."""
    import pickle
    import time

    from fedscale_amd import ingress
    from fedscale_amd import kernels as kx
    from fedscale_amd import kernels_clip as kc
    from fedscale_amd import kernels_quant4 as kq4
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.cloud.execution.quant4_upload import compress_delta4
    from fedscale_amd.quant4_round import Quant4Staging

    dev = torch.device("cuda:0")
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    rng = np.random.default_rng(0)
    base = rng.standard_normal(P, dtype=np.float32)
    w = base + rng.standard_normal(P, dtype=np.float32) * np.float32(0.01)
    den = float(np.float32(K))
    out, chain = torch.empty(L.ld, device=dev), torch.zeros(L.ld, device=dev)
    last = torch.from_numpy(np.concatenate([base, np.zeros(L.ld - P, dtype=np.float32)])).to(dev)
    res = {"K": K, "P": P}
    for key in ("float32", "mxfp4"):
        if key == "float32":
            up, st = {"w": w}, ClientStaging(L, dev, K, bulk=False)
        else:
            up, st = compress_delta4({"w": w}, {"w": base})[0], Quant4Staging(L, dev, K)
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
            kq4.reduce4(st.q4, st.scales, K, P, chain)
            kc.finish(chain, last, P, den, out)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[key] = {"payload_bytes": len(payload), "seconds": round(dt, 4), "updates_per_s": round(K / dt, 1),
                    "payload_GBps": round(K * len(payload) / dt / 1e9, 1)}
        print(f"[pcie] {key} {res[key]}", flush=True)
        del st
        torch.cuda.empty_cache()
    res["mxfp4"]["ratio_to_fp32_rate"] = round(res["mxfp4"]["updates_per_s"] / res["float32"]["updates_per_s"], 3)
    res["mxfp4"]["byte_prediction_of_that_ratio"] = round(4 / BYTES_PER_COLUMN, 3)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="c2,mid,head")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--round-reps", type=int, default=10)
    p.add_argument("--pcie", type=int, default=0, metavar="K",
                   help="also time a K-upload round of the headline's model from pickled payloads (0: skip)")
    p.add_argument("--fidelity-only", action="store_true", help="the CPU part alone (no GPU needed)")
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("quant4_reduce_measure: --reps must be at least 20")
    if a.fidelity_only:
        print(json.dumps({"fidelity": fidelity()}))
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("quant4_reduce_measure: needs a GPU (a CPU run gives no time)")
    from fedscale_amd import _native

    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "build_defs": _native.build_info().get("defs", ""), "read_ceiling_Bps": READ_CEILING,
           "lane_ops_per_s": LANE_OPS, "bytes_per_column": BYTES_PER_COLUMN, "lane_ops_per_column": OPS_PER_COLUMN,
           "pcie_inclusive": "not measured", "shapes": []}
    names = a.configs.split(",")
    for P in sorted({SHAPES[n][1] for n in names}):
        res["shapes"] += measure(P, [n for n in names if SHAPES[n][1] == P], a.reps, a.round_reps)
        torch.cuda.empty_cache()
    if a.pcie > 0:
        res["pcie_inclusive"] = pcie_round(a.pcie, SHAPES["head"][1])
    res["fidelity"] = fidelity()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
