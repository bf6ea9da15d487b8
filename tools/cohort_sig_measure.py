"""Time the cohort-signature kernels (include/fedcohort.h) at the BASELINE shapes, beside the host cost of the
reference path they replace.

    python -u tools/cohort_sig_measure.py [--configs c3,head] [--reps 10] [--no-host]

Per shape (K uploads of a P-float model whose tail has ResNet-18's structure: the last 3x3 convolution, its
BatchNorm with the int64 counter, the classifier): fc_signature over all K staged rows, fc_center, fc_normalize
and fc_gram, each timed with device events over ``--reps`` calls after two warm-up calls (the median is
reported).  Bytes and flops are what the algorithm needs, computed from the shapes here.  The host figures time a
restatement of examples/auxo/aggregator.py:293-302 + client_metadata.py:10-17 per upload (get_weights' clone of
the model, per-tensor subtract, concatenate, slice, float16 cast) and of client_manager.py:208-210 per round, on
this machine's CPU, one thread as the aggregator's main loop.  Also reports whether the f16 matrix unit keeps
float16 subnormal inputs (one product that is D / 32 if it does and 0 if it flushes them).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fedscale_amd import cohort_signature as cs  # noqa: E402
from fedscale_amd.bucket import BucketLayout  # noqa: E402

READ_CEILING = 7.23e12  # B/s, profiles/r01_hbm_stream_read_ceiling.json
SHAPES = {"c3": (1000, 11_191_242), "head": (1000, 25_000_000)}


def tail_layout(P: int) -> BucketLayout:
    """A P-float model with one int64 counter whose last 2.39 M elements are ResNet-18's: layer4.1.conv2, bn2
    (weight, bias, running_mean, running_var, num_batches_tracked), fc of 62 classes."""
    tail = [("layer4.1.conv2.weight", (512, 512, 3, 3), torch.float32), ("layer4.1.bn2.weight", (512,), torch.float32),
            ("layer4.1.bn2.bias", (512,), torch.float32), ("layer4.1.bn2.running_mean", (512,), torch.float32),
            ("layer4.1.bn2.running_var", (512,), torch.float32),
            ("layer4.1.bn2.num_batches_tracked", (), torch.int64), ("fc.weight", (62, 512), torch.float32),
            ("fc.bias", (62,), torch.float32)]
    n_tail = sum(int(np.prod(s)) for _, s, d in tail if d == torch.float32)
    spec = [("body", (P - n_tail,), torch.float32)] + tail
    return BucketLayout([n for n, _, _ in spec], [s for _, s, _ in spec], [d for _, _, d in spec])


def timed(fn, reps: int):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def device_side(name: str, K: int, P: int, reps: int) -> dict:
    dev = torch.device("cuda:0")
    L = tail_layout(P)
    plan = cs.signature_plan(L)
    D, ldd = plan.D, plan.ldd
    x = torch.empty(K, L.ld, dtype=torch.float32, device=dev)
    for k0 in range(0, K, 50):  # filled in blocks: no second K x ld temporary
        x[k0:k0 + 50].normal_(0.0, 0.01)
    xi = torch.randint(0, 100, (K, L.ldq), dtype=torch.int64, device=dev)
    last = torch.zeros(L.ld, dtype=torch.float32, device=dev).normal_(0.0, 0.05)
    last_i = torch.full((L.ldq,), 50, dtype=torch.int64, device=dev)
    sig = torch.empty(K, ldd, dtype=torch.float16, device=dev)
    out = {"config": name, "K": K, "P": P, "D": D, "segments": len(plan.segs), "int64_elements": len(plan.isegs)}

    def rate(key, ms, nbytes=None, flops=None):
        med, lo, hi = ms
        r = {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
        if nbytes is not None:
            r["bytes"] = int(nbytes)
            r["GBps"] = round(nbytes / (med * 1e-3) / 1e9, 1)
            r["share_of_read_ceiling"] = round(nbytes / (med * 1e-3) / READ_CEILING, 3)
        if flops is not None:
            r["flop"] = int(flops)
            r["TFLOPs"] = round(flops / (med * 1e-3) / 1e12, 1)
        out[key] = r
        print(f"[{name}] {key}: {r}", flush=True)

    rate("fc_signature", timed(lambda: cs.signature(x, xi, K, last, last_i, plan, sig), reps),
         nbytes=4 * K * D + 4 * D + 2 * K * D)
    del x
    avg, cen, sumsq = cs.center(sig, K, D)
    # two reads of sig (mean pass, centring pass), one write of centered (+ the fp64 partial rows)
    # (the wrapper allocates outputs and workspace from torch's caching allocator per call; timed with it)
    rate("fc_center", timed(lambda: cs.center(sig, K, D), reps), nbytes=2 * (2 * K * D) + 2 * K * D)
    norms = torch.sqrt(sumsq)
    rate("fc_normalize", timed(lambda: cs.normalize(cen, K, D, norms), reps), nbytes=4 * K * D)
    tiles = ((K + 63) // 64) * ((K + 63) // 64 + 1) // 2
    rate("fc_gram", timed(lambda: cs.gram(cen, K, D), reps), flops=tiles * 64 * 64 * 2 * D)
    out["fc_gram"]["flop_full_matrix"] = 2 * K * K * D
    out["gram_d2h_bytes"], out["matrix_d2h_bytes"] = 4 * K * K, 2 * K * D
    return out


def subnormal_probe() -> dict:
    dev = torch.device("cuda:0")
    D = 4096
    c = torch.zeros(2, D, dtype=torch.float16, device=dev)
    c[0] = 2.0 ** -15  # a float16 subnormal
    c[1] = 1024.0
    g = cs.gram(c).cpu().numpy()
    kept = bool(g[1, 0] == D / 32)
    r = {"product": float(g[1, 0]), "exact": D / 32, "subnormal_self_product": float(g[0, 0]),
         "mfma_f16_keeps_subnormal_inputs": kept}
    print(f"[probe] f16 MFMA with subnormal inputs: {r}", flush=True)
    return r


def host_side(name: str, K: int, P: int, end_of_round: bool) -> dict:
    torch.set_num_threads(1)
    L = tail_layout(P)
    rng = np.random.default_rng(0)
    model = [torch.from_numpy(rng.standard_normal(e.numel, dtype=np.float32).reshape(e.shape) * 0.05) if e.kind == "f"
             else torch.tensor(50, dtype=torch.int64) for e in L.entries]
    upload = {e.name: (m.numpy() + np.float32(0.01)) if e.kind == "f" else np.asarray(53, dtype=np.int64)
              for e, m in zip(L.entries, model)}
    t = {}

    def lap(key, t0):
        t[key] = t.get(key, 0.0) + time.perf_counter() - t0

    reps = 3
    for _ in range(reps):
        t0 = time.perf_counter()
        w_old = [p.data.clone() for p in model]                      # get_weights() (torch_model_adapter.py:41-47)
        lap("get_weights_clone", t0)
        t0 = time.perf_counter()
        w_old = [dt.cpu().numpy() for dt in w_old]
        w = [upload[k] for k in upload]
        gradient = [pb - pa for pa, pb in zip(w, w_old)]              # client_metadata.py:13
        lap("subtract", t0)
        t0 = time.perf_counter()
        gradient = np.concatenate([v.flatten() for v in gradient])    # :14 (float64: an int64 entry is present)
        lap("concatenate", t0)
        t0 = time.perf_counter()
        val_len = len(gradient) // 10
        tail = gradient[-val_len:]
        lap("slice", t0)
        t0 = time.perf_counter()
        g16 = np.float16(tail)                                        # :16
        lap("float16_cast", t0)
    out = {"config": name, "per_upload_ms": {k: round(v / reps * 1e3, 2) for k, v in t.items()}}
    out["per_upload_ms"]["total"] = round(sum(t.values()) / reps * 1e3, 2)
    out["per_round_ms_at_K"] = round(sum(t.values()) / reps * 1e3 * K, 0)
    print(f"[{name}] host, per upload: {out['per_upload_ms']}", flush=True)
    if end_of_round:
        from sklearn import preprocessing

        gl = [np.roll(g16, k) for k in range(K)]
        t0 = time.perf_counter()
        avg = np.mean(gl, axis=0)                                     # client_manager.py:208
        t1 = time.perf_counter()
        cen = gl - avg                                                # :209
        t2 = time.perf_counter()
        preprocessing.normalize(cen)                                  # :210
        t3 = time.perf_counter()
        out["end_of_round_ms"] = {"mean": round((t1 - t0) * 1e3, 1), "centre": round((t2 - t1) * 1e3, 1),
                                  "normalize": round((t3 - t2) * 1e3, 1)}
        print(f"[{name}] host, end of round: {out['end_of_round_ms']}", flush=True)
    return out


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="c3,head")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--no-host", action="store_true")
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cohort_sig_measure: needs a GPU (a CPU run gives no time)")
    res = {"device": torch.cuda.get_device_name(0), "read_ceiling_Bps": READ_CEILING, "subnormal_probe": subnormal_probe(),
           "device_side": [], "host_side": []}
    for c in a.configs.split(","):
        K, P = SHAPES[c]
        res["device_side"].append(device_side(c, K, P, a.reps))
        torch.cuda.empty_cache()
    if not a.no_host:
        for c in a.configs.split(","):
            K, P = SHAPES[c]
            res["host_side"].append(host_side(c, K, P, end_of_round=(c == "c3")))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
