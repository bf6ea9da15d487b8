#!/usr/bin/env python3
"""Time the Count-Sketch path (include/fedsketch.h) on the GPU and write profiles/sketch_measure.json.

    python -u tools/sketch_measure.py [--out profiles/sketch_measure.json] [--windows 7] [--pcie 40] [--kernels-only]
    FEDAGG_LIB=<a library built with -DFA_TUNING=1 -DFCS_SHARE_SIGN=1> python tools/sketch_measure.py --kernels-only ...

Kernels, at 25 M columns (R = 5, C = 2^18) and 1 M (C = 2^14): fcs_sketch_row with a base, fcs_estimate and the server
step after the mean (fcs_state_step, fcs_estimate, fs_topk_row at 1 %, fcs_apply, fcs_sketch_row with
FCS_SUBTRACT_FROM).  A timed window is WINDOW launches between two device events, each launch on the next of a ring of
input sets that together exceed the 256 MB Infinity Cache several times, so no launch finds its inputs cached by the
one before; min - median - max of the windows' per-launch times.  Predicted before the first run, over the measured
7.23 TB/s read ceiling (profiles/r01_hbm_stream_read_ceiling.json):

    fcs_sketch_row with a base   R 8 P bytes if no row is served from cache; 8 P + 4 R C if every row after the first is
    fcs_estimate                 4 P + 4 R C bytes
    the sketched round           the staged K R C 4 bytes over the ceiling, plus the server step as measured here

Rounds, at 100 x 1 M and 1000 x 25 M, alternating in one process: the whole finish of a sketched round (fa_reduce over
the staged tables, then the server step), of a dense fp32 round (fa_reduce over K x P) and of a top-k round at 1 %.
``--pcie K``: updates/s of a K-upload round of the 25 M model from pickled payloads, float32 against sketches.

No GPU, no numbers: the script fails without one.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CEILING = 7.23e12      # bytes / s, measured read ceiling
CACHE = 256 << 20      # Infinity Cache
WINDOW = 24            # launches of one timed window
SHAPES = ((1000, 25_000_000, 1 << 18), (100, 1_000_000, 1 << 14))  # K, P, C
R, SEED, RHO = 5, 1, 0.9


def windows(fn, n, torch, launches=WINDOW):
    """min / median / max over n windows of the per-launch time of fn(i), i the launch's number."""
    for i in range(launches):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(launches):
            fn(i)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / launches)
    return {"ms_median": round(float(np.median(ms)), 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5),
            "windows": n, "launches_per_window": launches}


def against(t, **preds):
    t["predicted_bytes"] = preds
    t["predicted_ms"] = {k: round(v / CEILING * 1e3, 5) for k, v in preds.items()}
    t["time_over_prediction"] = {k: round(t["ms_median"] / (v / CEILING * 1e3), 3) for k, v in preds.items()}
    t["verdicts"] = {k: "met" if v <= 1.1 else "missed" for k, v in t["time_over_prediction"].items()}
    return t


def kernels(P, C, n, torch):
    from fedscale_amd import kernels_sketch as kk
    from fedscale_amd import kernels_sparse as ks

    dev = torch.device("cuda:0")
    k = (P + 99) // 100
    sets = max(2, -(-4 * CACHE // (8 * P)))  # rings of inputs and outputs four times the cache
    xs = [torch.randn(P, device=dev) for _ in range(sets)]
    bs = [torch.randn(P, device=dev) for _ in range(sets)]
    ests = [torch.empty(P, device=dev) for _ in range(sets)]
    tables = [torch.randn(R * C, device=dev) for _ in range(sets)]
    su, se, nu, ne = (torch.zeros(R * C, device=dev) for _ in range(4))
    model = torch.empty(P, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    kp = (k + 3) // 4 * 4
    pairs = torch.empty(2 * kp, dtype=torch.int32, device=dev)
    ws = torch.empty(ks.topk_workspace(P), dtype=torch.uint8, device=dev)
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def step(i):
        est = ests[i % sets]
        kk.state_step(tables[i % sets], su, se, RHO, R * C, nu, ne, bad)
        kk.estimate(ne, P, R, C, SEED, est)
        ks.topk_row(est, None, None, P, k, ws, pairs[:kp], pairs[kp:].view(torch.float32))
        kk.apply_pairs(pairs[:k], pairs[kp:kp + k].view(torch.float32), k, P, est, bs[i % sets], model)
        kk.sketch_row(est, None, None, P, R, C, SEED, ne, subtract=True)

    s = windows(lambda i: kk.sketch_row(xs[i % sets], bs[i % sets], None, P, R, C, SEED, tables[i % sets]), n, torch)
    e = windows(lambda i: kk.estimate(tables[i % sets], P, R, C, SEED, ests[i % sets]), n, torch)
    return {"P": P, "R": R, "C": C, "k": k, "input_sets": sets, "plan": kk.sketch_plan(cus, P, R, C),
            "fcs_sketch_row_with_base": against(s, no_row_cached=R * 8 * P, rows_after_the_first_cached=8 * P + 4 * R * C),
            "fcs_estimate": against(e, bytes=4 * P + 4 * R * C),
            "server_step_after_the_mean": windows(step, n, torch, launches=8)}


def rounds(K, P, C, n, step_ms, torch):
    """The whole finish of a sketched, a dense fp32 and a top-k (1 %) round over K resident uploads, alternating."""
    from fedscale_amd import kernels_sparse as ks
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.cloud.execution.sketch_upload import SketchSpec
    from fedscale_amd.round import DeviceRound
    from fedscale_amd.sketch_round import SketchRound, SketchStaging, SketchState
    from fedscale_amd.sparse_round import SparseRound, SparseStaging

    dev = torch.device("cuda:0")
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    spec = SketchSpec(rows=R, cols=C, k=0.01, momentum=RHO, seed=SEED)
    last = torch.empty(L.ld, device=dev).normal_(0.0, 1.0)
    s32, sk, sp = ClientStaging(L, dev, K, bulk=False), SketchStaging(L, dev, K, spec), SparseStaging(L, dev, K, 0.01)
    for r in range(K):
        s32.x[r].normal_(0.0, 0.01).add_(last)
    sk.x.normal_(0.0, 0.01)
    kmax = sp.kmax
    stride = P // kmax
    for r0 in range(0, K, 50):  # strictly increasing indices below P: one per stride of columns
        r1 = min(K, r0 + 50)
        off = torch.randint(0, stride, (r1 - r0, kmax), device=dev, dtype=torch.int32)
        sp.idx[r0:r1, :kmax] = off + torch.arange(kmax, device=dev, dtype=torch.int32) * stride
    sp.val.normal_(0.0, 0.01)
    sp.nnz.fill_(kmax)
    state = SketchState(R, C, dev)
    out = torch.empty(L.ld, device=dev)
    side = torch.zeros(L.ldq, dtype=torch.float64, device=dev)
    den = float(np.float32(K))
    torch.cuda.synchronize()

    def make(cls, st, **kw):
        def m():
            r = cls(L, dev, K, "fedavg", staging=st, capacity=K, **kw)
            r.adopt_resident(K)
            return lambda: r.finalize_mean(den, float(K), out=out, cur_side=side)
        return m

    makers = {"sketch_round_finish": make(SketchRound, sk, spec=spec, last_f32=last, state=state),
              "dense_fp32_round_finish": make(DeviceRound, s32),
              "topk_1pct_round_finish": make(SparseRound, sp, last_f32=last)}
    ms = {k: [] for k in makers}
    for rep in range(2 + n):  # two warm-up rounds of each
        for k, m in makers.items():
            fin = m()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fin()
            b.record()
            b.synchronize()
            if rep >= 2:
                ms[k].append(a.elapsed_time(b))
    staged = {"sketch_round_finish": 4 * K * R * C, "dense_fp32_round_finish": 4 * K * P,
              "topk_1pct_round_finish": 8 * K * ks.row_stride(kmax)}
    res = {"K": K, "P": P, "C": C, "rounds": n}
    for k, m in ms.items():
        med = float(np.median(m))
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(m), 4), "ms_max": round(max(m), 4),
                  "staged_bytes": staged[k], "ratio_to_dense_fp32": round(med / float(np.median(
                      ms["dense_fp32_round_finish"])), 4)}
    pred = staged["sketch_round_finish"] / CEILING * 1e3 + step_ms
    c = res["sketch_round_finish"]
    c["predicted_ms"] = round(pred, 4)
    c["time_over_prediction"] = round(c["ms_median"] / pred, 3)
    c["verdict"] = "met" if c["time_over_prediction"] <= 1.1 else "missed"
    c["includes"] = "one host synchronisation (the non-finite count)"
    print(f"[round {K} x {P}] {res}", flush=True)
    return res


def pcie_round(K, P, C, torch):
    """Updates/s of one K-upload round from pickled payloads: float32 (ClientStaging) and sketches (SketchStaging)."""
    import pickle
    import time

    from fedscale_amd import ingress
    from fedscale_amd import kernels as kx
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.cloud.execution.sketch_upload import SketchSpec, compress_sketch
    from fedscale_amd.sketch_round import SketchStaging

    dev = torch.device("cuda:0")
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    spec = SketchSpec(rows=R, cols=C, seed=SEED)
    rng = np.random.default_rng(0)
    base = rng.standard_normal(P, dtype=np.float32)
    w = base + rng.standard_normal(P, dtype=np.float32) * np.float32(0.01)
    den = float(np.float32(K))
    res = {"K": K, "P": P}
    for key in ("float32", "sketch"):
        if key == "float32":
            up, st, n = {"w": w}, ClientStaging(L, dev, K, bulk=False), P
        else:
            up = compress_sketch({"w": torch.from_numpy(w).to(dev)}, {"w": torch.from_numpy(base).to(dev)}, spec)
            st, n = SketchStaging(L, dev, K, spec), R * C
        out = torch.empty((n + 3) // 4 * 4, device=dev)
        payload = pickle.dumps({"client_id": 1, "update_weight": up, "moving_loss": 0.5})
        for k in range(3):
            st.put(k, ingress.loads(payload)["update_weight"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(K):
            st.put(k, ingress.loads(payload)["update_weight"])
        if key == "float32":
            st.drain()
        kx.reduce(st.x, K, n, out, denom=den, finalize=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[key] = {"payload_bytes": len(payload), "seconds": round(dt, 4), "updates_per_s": round(K / dt, 1),
                    "payload_GBps": round(K * len(payload) / dt / 1e9, 2)}
        print(f"[pcie] {key} {res[key]}", flush=True)
        del st, out
        torch.cuda.empty_cache()
    res["sketch"]["ratio_to_fp32_rate"] = round(res["sketch"]["updates_per_s"] / res["float32"]["updates_per_s"], 2)
    res["sketch"]["byte_prediction_of_that_ratio"] = round(P / (R * C), 2)
    return res


def main(argv=None):
    import torch

    from fedscale_amd import _native

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sketch_measure.json")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--pcie", type=int, default=0, metavar="K")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sketch_measure: no GPU")
    bi = _native.build_info()
    out = {"build_id": bi["build_id"], "build_defs": bi["defs"],
           "device": torch.cuda.get_device_name(0), "read_ceiling_bytes_per_s": CEILING,
           "met_means": "median time at most 1.1 x the predicted time", "kernels": [], "rounds": "not measured",
           "pcie_inclusive": "not measured"}
    for K, P, C in SHAPES:
        out["kernels"].append(kernels(P, C, a.windows, torch))
        print(f"[kernels] {out['kernels'][-1]}", flush=True)
        torch.cuda.empty_cache()
    if not a.kernels_only:
        out["rounds"] = []
        for (K, P, C), kr in zip(SHAPES, out["kernels"]):
            out["rounds"].append(rounds(K, P, C, a.windows, kr["server_step_after_the_mean"]["ms_median"], torch))
            torch.cuda.empty_cache()
        if a.pcie > 0:
            out["pcie_inclusive"] = pcie_round(a.pcie, SHAPES[0][1], SHAPES[0][2], torch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
