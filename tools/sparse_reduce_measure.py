"""Time fs_reduce (top-k sparse delta rows, include/fedsparse.h) beside the weighted fa_reduce (fp32 rows) in one
process.

    python -u tools/sparse_reduce_measure.py [--configs head,c2] [--densities 0.001,0.01,0.1] [--reps 30] \
        [--pcie K] [--out profiles/sparse_reduce_measure.json]

Per shape (head: 1000 x 25 M, the headline; c2: config 2's 100 x 1 M) a dense fp32 staging is filled on the device
with x_k = L + N(0, 0.01^2), and per density a sparse staging with random index sets (every column kept with
probability ``density``, so a row holds about density x P pairs) and N(0, 0.01^2) values.  Device events around each
wrapper call, three warm-up calls, then ``--reps`` (>= 20) timed calls per kernel, the kernels alternating so that
drift of the machine falls on all of them; medians.  Per density: fs_reduce, fs_row_offsets + fs_check_rows over
all rows, and the whole finish of a device-resident round (``SparseRound.finalize_mean``: chain, fcl_finish), each
beside the weighted fa_reduce and ``DeviceRound.finalize_mean`` of the same run and against its byte floor,
(8 x sum nnz + 4 x P) / the 7.23 TB/s stream-read ceiling (profiles/r01_hbm_stream_read_ceiling.json).  At the
headline's width, fs_topk_row on one row.

``--pcie K`` adds the payload-to-model round of the headline's model from pickled executor payloads, per upload format
in the same process (float32, MXFP8 deltas, top-k pairs at 1 %): K times ``ingress.loads`` of one payload + the
staging's ``put``, then the finishing reduce; host wall clock from the first ``loads`` to a device synchronise after
the reduce, after 5 warm-up uploads.  Updates/s, and what the payload bytes predict against the float32 rate.
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
from fedscale_amd import kernels_quant as kq  # noqa: E402
from fedscale_amd import kernels_sparse as ks  # noqa: E402

READ_CEILING = 7.23e12  # B/s
SHAPES = {"head": (1000, 25_000_000), "c2": (100, 1_000_000)}
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
                 ratio_to_byte_floor=round(med / floor_ms, 2))
    return r


def fill_sparse(st, K: int, P: int, density: float):
    """Random rows written on the device into the staging's slots [0, K); returns the pairs staged in all."""
    total = 0
    for k in range(K):
        cols = torch.nonzero(torch.rand(P, device=st.device) < density).reshape(-1)[:st.ldk].to(torch.int32)
        n = cols.numel()
        st.idx[k, :n] = cols
        st.val[k, :n].normal_(0.0, 0.01)
        st.nnz[k] = n
        total += n
    return total


def measure(name: str, K: int, P: int, densities, reps: int, round_reps: int) -> dict:
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.round import DeviceRound
    from fedscale_amd.sparse_round import SparseRound, SparseStaging

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    ld = L.ld
    den = float(np.float32(K))
    s32 = ClientStaging(L, dev, K, bulk=False)
    last = torch.empty(ld, device=dev).normal_(0.0, 1.0)
    for k0 in range(0, K, BLOCK):
        b = s32.x[k0:k0 + BLOCK]
        b.normal_(0.0, 0.01)
        b.add_(last)
    w = torch.full((K,), 1.0, device=dev)
    out32, outs = torch.empty(ld, device=dev), torch.empty(ld, device=dev)
    side = torch.zeros(L.ldq, dtype=torch.float64, device=dev)
    res = {"config": name, "K": K, "P": P, "ld": ld, "reps": reps, "fs_reduce_plan": ks.reduce_sparse_plan(cus, K, P),
           "densities": []}
    b32 = 4 * K * P + 4 * P
    for density in densities:
        st = SparseStaging(L, dev, K, min(1.0, density * 1.05 + 64.0 / P))  # room for the binomial spread of a row
        pairs = fill_sparse(st, K, P, density)
        st.index_rows(0, K)
        torch.cuda.synchronize()
        assert int((st.flags != 0).sum().item()) == 0
        nb = 8 * pairs + 4 * P
        t32, ts, ti = timed([lambda: kx.reduce(s32.x, K, P, out32, a=w, denom=den, finalize=True),
                             lambda: ks.reduce_sparse(st.idx, st.val, st.nnz, st.offsets, st.flags, K, P, outs),
                             lambda: st.index_rows(0, K)], reps)
        d = {"density": density, "pairs": pairs, "ldk": st.ldk,
             "fa_reduce_fp32_weighted": entry(t32, b32), "fs_reduce": entry(ts, nb),
             "fs_row_offsets_and_check_rows": entry(ti, 4 * pairs)}
        d["fs_reduce"].update(ratio_to_fa_reduce=round(ts[0] / t32[0], 4),
                              bytes_ratio_to_fa_reduce=round(nb / b32, 4))
        for k in ("fa_reduce_fp32_weighted", "fs_reduce", "fs_row_offsets_and_check_rows"):
            print(f"[{name} d={density}] {k} {d[k]}", flush=True)
        if round_reps > 0:
            def plain_round():
                r = DeviceRound(L, dev, K, "fedavg", capacity=K, staging=s32)
                r.adopt_resident(K)
                return lambda: r.finalize_mean(den, float(K), out=out32, cur_side=side)

            def sparse_round():
                r = SparseRound(L, dev, K, "fedavg", staging=st, last_f32=last, capacity=K)
                r.slot = r.n = K  # the rows and their offsets are already in the staging slots
                return lambda: r.finalize_mean(den, float(K), out=outs, cur_side=side)

            ms = ([], [])
            for rep in range(2 + round_reps):  # two warm-up rounds of each
                for i, make in enumerate((plain_round, sparse_round)):
                    fin = make()
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fin()
                    b.record()
                    b.synchronize()
                    if rep >= 2:
                        ms[i].append(a.elapsed_time(b))
            tp, tq = [(float(np.median(m)), float(min(m)), float(max(m))) for m in ms]
            d["device_round_finish"] = entry(tp)
            d["sparse_round_finish"] = entry(tq, nb + 12 * P)  # + fcl_finish: chain and L read, the model written
            d["sparse_round_finish"]["ratio_to_device_round_finish"] = round(tq[0] / tp[0], 4)
            for k in ("device_round_finish", "sparse_round_finish"):
                print(f"[{name} d={density}] {k} {d[k]}", flush=True)
        res["densities"].append(d)
        del st
        torch.cuda.empty_cache()
    if name == "head":
        x = s32.x[0]
        ws = torch.empty(ks.topk_workspace(P), dtype=torch.uint8, device=dev)
        rout = torch.empty(P, device=dev)
        res["fs_topk_row"] = []
        for density in densities:
            k = max(1, int(np.ceil(density * P)))
            io = torch.empty(k + 4, dtype=torch.int32, device=dev)
            vo = torch.empty(k + 4, device=dev)
            (t,) = timed([lambda: ks.topk_row(x, last, None, P, k, ws, io, vo, rout)], reps)
            e = entry(t, 6 * 8 * P + 4 * P + 8 * k)  # six passes over x and base, the residual and the pairs written
            e["density"] = density
            res["fs_topk_row"].append(e)
            print(f"[{name} d={density}] fs_topk_row {e}", flush=True)
    return res


def pcie_round(K: int, P: int, density: float) -> dict:
    """Updates/s of one K-upload round from pickled payloads: float32 (ClientStaging), MXFP8 deltas (QuantStaging) and
    top-k pairs (SparseStaging)."""
    import pickle
    import time

    from fedscale_amd import ingress
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.cloud.execution.quant_upload import compress_delta
    from fedscale_amd.cloud.execution.sparse_upload import compress_topk
    from fedscale_amd.quant_round import QuantStaging
    from fedscale_amd.sparse_round import SparseStaging

    dev = torch.device("cuda:0")
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    rng = np.random.default_rng(0)
    base = rng.standard_normal(P, dtype=np.float32)
    w = base + rng.standard_normal(P, dtype=np.float32) * np.float32(0.01)
    den = float(np.float32(K))
    out, chain = torch.empty(L.ld, device=dev), torch.zeros(L.ld, device=dev)
    last = torch.from_numpy(np.concatenate([base, np.zeros(L.ld - P, dtype=np.float32)])).to(dev)
    res = {"K": K, "P": P, "density": density}
    for key in ("float32", "mxfp8", "topk"):
        if key == "float32":
            up, st = {"w": w}, ClientStaging(L, dev, K, bulk=False)
        elif key == "mxfp8":
            up, st = compress_delta({"w": w}, {"w": base}), QuantStaging(L, dev, K)
        else:
            up, st = compress_topk({"w": w}, {"w": base}, density=density)[0], SparseStaging(L, dev, K, density)
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
        elif key == "mxfp8":
            kq.reduce8(st.q8, st.scales, K, P, chain)
            kc.finish(chain, last, P, den, out)
        else:
            ks.reduce_sparse(st.idx, st.val, st.nnz, st.offsets, st.flags, K, P, chain)
            kc.finish(chain, last, P, den, out)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[key] = {"payload_bytes": len(payload), "seconds": round(dt, 4), "updates_per_s": round(K / dt, 1),
                    "payload_GBps": round(K * len(payload) / dt / 1e9, 2)}
        print(f"[pcie] {key} {res[key]}", flush=True)
        del st
        torch.cuda.empty_cache()
    for key in ("mxfp8", "topk"):
        res[key]["ratio_to_fp32_rate"] = round(res[key]["updates_per_s"] / res["float32"]["updates_per_s"], 3)
        res[key]["byte_prediction_of_that_ratio"] = round(res["float32"]["payload_bytes"] /
                                                          res[key]["payload_bytes"], 3)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="head,c2")
    p.add_argument("--densities", default="0.001,0.01,0.1")
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--round-reps", type=int, default=10)
    p.add_argument("--pcie", type=int, default=0, metavar="K",
                   help="also time a K-upload round of the headline's model from pickled payloads (0: skip)")
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("sparse_reduce_measure: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("sparse_reduce_measure: needs a GPU (a CPU run gives no time)")
    densities = [float(d) for d in a.densities.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "build_defs": _native.build_info().get("defs", ""), "read_ceiling_Bps": READ_CEILING,
           "tile_columns": ks.TILE, "pcie_inclusive": "not measured", "shapes": []}
    for c in a.configs.split(","):
        K, P = SHAPES[c]
        res["shapes"].append(measure(c, K, P, densities, a.reps, a.round_reps))
        torch.cuda.empty_cache()
    if a.pcie > 0:
        res["pcie_inclusive"] = pcie_round(a.pcie, SHAPES["head"][1], 0.01)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
