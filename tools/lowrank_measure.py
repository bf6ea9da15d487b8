"""Time flr_reduce (low-rank factor rows on the matrix unit, include/fedlowrank.h) beside fa_reduce over dense fp32
rows of the same layout, in one process.

    python -u tools/lowrank_measure.py [--configs t25,c2] [--clients 100,1000] [--ranks 4,8,32] [--reps 20] \
        [--tiles 0,64,128] [--pcie K] [--out profiles/lowrank_measure.json]

Layouts: t25, transformer-like matrices summing to about 25 M parameters (an embedding, six blocks of qkv / proj / two
ffn matrices with their biases, a head); c2, config 2's 1 M.  Per (layout, clients, rank) the staging is filled on
the device with N(0, 0.01^2) factors; device events around each wrapper call, three warm-up calls, then ``--reps``
(>= 20) timed calls per kernel, the kernels alternating so that drift of the machine falls on all of them;
min - median - max.  ``--tiles`` times the plan's own choice (0) beside every factored entry forced to one tile.

The predictions, stated before the run and stored beside each time:
  * time >= 2 n r2 sum(O I) FLOP over the fp32 matrix peak of the data sheet (157.3 TFLOP/s);
  * bytes read ~ the factors times their re-read count through L2 — Ut once per tile column, V once per tile row —
    plus the chain written once; over the 7.23 TB/s stream-read ceiling this is the byte floor of a run whose re-reads
    all missed L2.
``--pcie K`` adds the payload-to-model round of t25 from pickled executor payloads, float32 beside rank-8 factors:
K times ``ingress.loads`` + the staging's ``put``, then the finishing reduce; host wall clock, after 5 warm-up uploads.
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
from fedscale_amd import kernels_lowrank as kl  # noqa: E402

MATRIX_PEAK = 157.3e12  # FLOP/s, fp32 matrix, MI355X data sheet
READ_CEILING = 7.23e12  # B/s (profiles/r01_hbm_stream_read_ceiling.json)
BLOCK = 50


def layout_shapes(name: str):
    if name == "c2":
        return [("fc.weight", (1000, 1000)), ("fc.bias", (1000,))]
    d, out = 512, [("embed.weight", (8192, 512))]
    for b in range(6):
        for n, s in (("qkv", (3 * d, d)), ("proj", (d, d)), ("ffn1", (4 * d, d)), ("ffn2", (d, 4 * d))):
            out += [(f"block{b}.{n}.weight", s), (f"block{b}.{n}.bias", (s[0],))]
    return out + [("head.weight", (4096, 512)), ("head.bias", (4096,))]


def timed(fns, reps: int):
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
    return [{"ms_min": round(float(min(m)), 4), "ms_median": round(float(np.median(m)), 4),
             "ms_max": round(float(max(m)), 4)} for m in ms]


def predictions(table: kl.TileTable, n: int) -> dict:
    head, ents, _ = kl.parse_table(table.host)
    r2 = int(head["r2"])
    flop = read = 0
    for e in ents:
        O, I = int(e["O"]), int(e["I"])
        if I:
            flop += 2 * n * r2 * O * I
            read += 4 * n * r2 * (int(e["O4"]) * int(e["ntc"]) + int(e["I4"]) * int(e["ntr"]))
        else:
            read += 4 * n * O
    nbytes = read + 4 * int(head["P"])
    return {"flop": flop, "flop_floor_ms": round(flop / MATRIX_PEAK * 1e3, 4), "bytes_with_rereads": nbytes,
            "byte_floor_ms": round(nbytes / READ_CEILING * 1e3, 4), "tiles": table.tiles}


def measure(name: str, clients, ranks, tiles, reps: int) -> dict:
    from fedscale_amd.bucket import BucketLayout, ClientStaging

    dev = torch.device("cuda:0")
    shapes = layout_shapes(name)
    L = BucketLayout([n for n, _ in shapes], [s for _, s in shapes], [torch.float32] * len(shapes))
    res = {"layout": name, "P": L.P, "entries": len(shapes), "runs": []}
    for K in clients:
        s32 = ClientStaging(L, dev, K, bulk=False)
        for k0 in range(0, K, BLOCK):
            s32.x[k0:k0 + BLOCK].normal_(0.0, 0.01)
        out32, out = torch.empty(L.ld, device=dev), torch.empty(L.ld, device=dev)
        den = float(np.float32(K))
        for r in ranks:
            dims = kl.entry_dims([s for _, s in shapes], r)
            tabs = [kl.TileTable(dims, r, dev, t) for t in tiles]
            rows = torch.empty(K, tabs[0].ldf, device=dev)
            for k0 in range(0, K, BLOCK):
                rows[k0:k0 + BLOCK].normal_(0.0, 0.01)
            fns = [lambda: kx.reduce(s32.x, K, L.P, out32, denom=den, finalize=True)]
            fns += [lambda t=t: kl.reduce_lowrank(rows, K, t, out) for t in tabs]
            ts = timed(fns, reps)
            run = {"clients": K, "rank": r, "ldf": tabs[0].ldf, "staged_bytes_per_client": 4 * tabs[0].ldf,
                   "dense_bytes_per_client": 4 * L.P, "fa_reduce_fp32": ts[0], "flr_reduce": []}
            for t, tab, tm in zip(tiles, tabs, ts[1:]):
                p = predictions(tab, K)
                tm.update(force_tile=t, **p)
                tm["ratio_to_flop_floor"] = round(tm["ms_median"] / max(p["flop_floor_ms"], 1e-9), 2)
                tm["TFLOPs"] = round(p["flop"] / (tm["ms_median"] * 1e-3) / 1e12, 2)
                tm["ratio_to_fa_reduce"] = round(tm["ms_median"] / ts[0]["ms_median"], 3)
                run["flr_reduce"].append(tm)
            res["runs"].append(run)
            print(f"[{name}] {run}", flush=True)
            del rows, tabs
            torch.cuda.empty_cache()
        del s32
        torch.cuda.empty_cache()
    return res


def pcie_round(K: int, rank: int) -> dict:
    """Updates/s of one K-upload round of t25 from pickled payloads: float32 (ClientStaging) beside rank-``rank``
    factors (LowRankStaging)."""
    import pickle
    import time

    from fedscale_amd import ingress
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.cloud.execution.lowrank_upload import LowRankCompressor
    from fedscale_amd.lowrank_round import LowRankStaging

    dev = torch.device("cuda:0")
    shapes = layout_shapes("t25")
    L = BucketLayout([n for n, _ in shapes], [s for _, s in shapes], [torch.float32] * len(shapes))
    rng = np.random.default_rng(0)
    base = {n: rng.standard_normal(s, dtype=np.float32) for n, s in shapes}
    w = {n: b + rng.standard_normal(b.shape, dtype=np.float32) * np.float32(0.01) for n, b in base.items()}
    den = float(np.float32(K))
    out, chain = torch.empty(L.ld, device=dev), torch.zeros(L.ld, device=dev)
    last = torch.zeros(L.ld, device=dev)
    res = {"K": K, "rank": rank}
    for key in ("float32", "lowrank"):
        if key == "float32":
            up, st = w, ClientStaging(L, dev, K, bulk=False)
        else:
            up = LowRankCompressor(rank).compress({n: torch.from_numpy(v) for n, v in w.items()}, base)
            st = LowRankStaging(L, dev, K, rank)
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
            kx.reduce(st.x, K, L.P, out, denom=den, finalize=True)
        else:
            kl.reduce_lowrank(st.rows, K, st.table, chain)
            kc.finish(chain, last, L.P, den, out)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[key] = {"payload_bytes": len(payload), "seconds": round(dt, 4), "updates_per_s": round(K / dt, 1)}
        print(f"[pcie] {key} {res[key]}", flush=True)
        del st
        torch.cuda.empty_cache()
    res["lowrank"]["ratio_to_fp32_rate"] = round(res["lowrank"]["updates_per_s"] / res["float32"]["updates_per_s"], 3)
    res["lowrank"]["byte_prediction_of_that_ratio"] = round(res["float32"]["payload_bytes"] /
                                                            res["lowrank"]["payload_bytes"], 3)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="t25,c2")
    p.add_argument("--clients", default="100,1000")
    p.add_argument("--ranks", default="4,8,32")
    p.add_argument("--tiles", default="0,64,128")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--pcie", type=int, default=0, metavar="K")
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("lowrank_measure: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("lowrank_measure: needs a GPU (a CPU run gives no time)")
    ints = lambda s: [int(v) for v in s.split(",")]  # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "matrix_peak_FLOPs": MATRIX_PEAK,
           "read_ceiling_Bps": READ_CEILING, "stage_depth": kl.DEPTH, "pcie_inclusive": "not measured", "layouts": []}
    for c in a.configs.split(","):
        res["layouts"].append(measure(c, ints(a.clients), ints(a.ranks), ints(a.tiles), a.reps))
    if a.pcie > 0:
        res["pcie_inclusive"] = pcie_round(a.pcie, 8)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
