"""Time the stages of geometric-median (RFA) aggregation (include/fedgeomed.h) beside fa_reduce over the same rows,
in one process ("Geometric median").

    python -u tools/geomed_measure.py [--configs c2,k100,head] [--reps 20] [--out profiles/geomed_measure.json]

Per shape (c2: 100 x 1 M; k100: 100 x 25 M; head: 1000 x 25 M) the device-resident rows are x_k = L + noise, R = 4
iterations, nu = 1e-6.  Three warm-up calls, then ``--reps`` timed calls each (fewer, at least 5, of a call that takes
more than 200 ms) of
    fa_reduce        weighted, no finalize, the same rows
    fk_gram          the Gram of the Gram method (both launches)
    fgm_start        the start weights from the Gram diagonal
    fgm_gram_dist2   one iteration's distances in K-space (both launches)
    fgm_weights      one iteration's weights
    fcl_row_sqnorms  one iteration's distances of the streamed method, against an fp32 iterate
    fcl_reduce       the chain with the fp32 weights (once in the Gram method, 1 + R times in the streamed one)
    fgm_finish
alternating in that order; device events around each wrapper call; medians.  Then the whole finish of a
device-resident round (``adopt_resident``): ``GeoMedRound.finalize_mean`` by either method against
``DeviceRound.finalize_mean``, alternating, ``--round-reps`` each — and what ``method="auto"`` picks at the shape, with
the ratio of the two methods, which is what a later change would move the constant of the rule by.
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
from fedscale_amd import kernels_geomed as kg  # noqa: E402
from fedscale_amd import kernels_krum as kk  # noqa: E402

SHAPES = {"c2": (100, 1_000_000), "k100": (100, 25_000_000), "head": (1000, 25_000_000)}
BLOCK = 50  # rows filled at a time: no second K x ld temporary
ITERS, NU = 4, 1e-6


def fill(x: torch.Tensor, last: torch.Tensor):
    """x_k = last + N(0, 0.01^2)."""
    for k0 in range(0, x.shape[0], BLOCK):
        b = x[k0:k0 + BLOCK]
        b.normal_(0.0, 0.01)
        b.add_(last)


def _once(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fns, reps: int):
    """(median, min, max, n) ms of each call of ``fns``, timed alternately after three warm-up calls of each; a call
    whose warm-up took more than 200 ms is timed max(5, reps // 4) times."""
    n = []
    for fn in fns:
        w = [_once(fn) for _ in range(3)]
        n.append(reps if min(w) <= 200.0 else max(5, reps // 4))
    ms = [[] for _ in fns]
    for rep in range(max(n)):
        for i, fn in enumerate(fns):
            if rep < n[i]:
                ms[i].append(_once(fn))
    return [(float(np.median(m)), float(min(m)), float(max(m)), len(m)) for m in ms]


def entry(ms, base=None) -> dict:
    med, lo, hi, n = ms
    r = {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "calls": n}
    if base is not None:
        r["ratio_to_fa_reduce"] = round(med / base, 4)
    return r


def measure(name: str, K: int, P: int, reps: int, round_reps: int) -> dict:
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.geomed_round import GeoMedRound, GeoMedSpec
    from fedscale_amd.round import DeviceRound

    dev = torch.device("cuda:0")
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    st = ClientStaging(L, dev, K, bulk=False)
    x, ld = st.x, L.ld
    last = torch.empty(ld, device=dev).normal_(0.0, 1.0)
    fill(x, last)
    ones = torch.ones(K, dtype=torch.float32, device=dev)
    out_a, out_g, chain, z = (torch.empty(ld, device=dev) for _ in range(4))
    z.copy_(last)
    z[:P] += 0.001
    ws = kk.gram_workspace(K, P, dev)
    G = torch.empty(K * K, dtype=torch.float64, device=dev)
    ws2 = kg.dist2_workspace(K, dev)
    wsn = kc.workspace(K, P, dev)
    w = torch.empty(K, dtype=torch.float64, device=dev)
    c = torch.empty(K, dtype=torch.float32, device=dev)
    q = torch.empty(K, dtype=torch.float64, device=dev)
    qs = torch.empty(K, dtype=torch.float64, device=dev)
    obj = torch.zeros(1, dtype=torch.float64, device=dev)
    n_valid = torch.zeros(1, dtype=torch.int32, device=dev)
    auto = GeoMedSpec(ITERS, NU).resolve(K)
    res = {"config": name, "K": K, "P": P, "ld": ld, "iters": ITERS, "nu": NU, "reps": reps, "auto_method": auto,
           "auto_rule_K_max": 12 * (1 + 2 * ITERS), "gram_plan": kk.gram_plan(K, P),
           "dist2_workspace_bytes": kg.dist2_workspace_bytes(K),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count}
    names = ["fa_reduce_weighted", "fk_gram", "fgm_start", "fgm_gram_dist2", "fgm_weights", "fcl_row_sqnorms",
             "fcl_reduce_chain", "fgm_finish", "fa_reduce_weighted_again"]
    fns = [lambda: kx.reduce(x, K, P, out_a, a=ones),
           lambda: kk.gram(x, K, P, last, G, ws),
           lambda: kg.start(G, K, w, c, n_valid, stride=K + 1),
           lambda: kg.gram_dist2(G, K, w, q, ws2),
           lambda: kg.weights(q, K, NU, w, c, obj, n_valid),
           lambda: kc.row_sqnorms(x, K, P, z, qs, wsn),
           lambda: kc.reduce_clip(x, K, P, last, c, chain),
           lambda: kg.finish(chain, last, n_valid, P, out_g)]
    fns.append(fns[0])
    ts = timed(fns, reps)
    for k, tm in zip(names, ts):
        res[k] = entry(tm, None if k == "fa_reduce_weighted" else ts[0][0])
    res["fa_reduce_spread"] = round(abs(ts[-1][0] / ts[0][0] - 1.0), 4)
    res["n_valid"] = int(n_valid.cpu()[0])
    t = {k: res[k]["ms_median"] for k in names}
    # the rounds as sums of their stages' medians (the measured whole rounds follow)
    res["gram_round_from_stages_ms"] = round(
        t["fk_gram"] + t["fgm_start"] + ITERS * (t["fgm_gram_dist2"] + t["fgm_weights"]) + t["fcl_reduce_chain"]
        + t["fgm_finish"], 4)
    res["stream_round_from_stages_ms"] = round(
        (1 + ITERS) * (t["fcl_row_sqnorms"] + t["fcl_reduce_chain"] + t["fgm_finish"]) + t["fgm_start"]
        + ITERS * t["fgm_weights"], 4)
    res["gram_in_plain_passes"] = round(t["fk_gram"] / t["fa_reduce_weighted"], 3)
    for k in names + ["gram_round_from_stages_ms", "stream_round_from_stages_ms", "gram_in_plain_passes"]:
        print(f"[{name}] {k} {res[k]}", flush=True)
    del out_a, out_g, G, ws, ws2, wsn, z, chain
    torch.cuda.empty_cache()
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

    def geomed_round(method):
        def make():
            r = GeoMedRound(L, dev, K, GeoMedSpec(ITERS, NU, method), staging=st, last_f32=last, capacity=K)
            r.adopt_resident(K)
            return lambda: r.finalize_mean(den, float(K), out=out, cur_side=side)
        return make

    makers = [plain_round, geomed_round("gram"), geomed_round("stream")]
    ms = [[] for _ in makers]
    for rep in range(2 + round_reps):  # two warm-up rounds of each
        for i, make in enumerate(makers):
            fin = make()
            torch.cuda.synchronize()
            tt = _once(fin)
            del fin
            if rep >= 2:
                ms[i].append(tt)
    tm = [(float(np.median(v)), float(min(v)), float(max(v)), len(v)) for v in ms]
    res["device_round_finish"] = entry(tm[0])
    for k, v in (("geomed_gram_round_finish", tm[1]), ("geomed_stream_round_finish", tm[2])):
        res[k] = entry(v)
        res[k]["ratio_to_device_round_finish"] = round(v[0] / tm[0][0], 4)
    res["gram_over_stream"] = round(tm[1][0] / tm[2][0], 4)
    res["faster_method"] = "gram" if tm[1][0] <= tm[2][0] else "stream"
    for k in ("device_round_finish", "geomed_gram_round_finish", "geomed_stream_round_finish", "gram_over_stream",
              "faster_method", "auto_method"):
        print(f"[{name}] {k} {res[k]}", flush=True)
    res["round_reps"] = round_reps
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="c2,k100,head")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--round-reps", type=int, default=5)
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("geomed_measure: --reps must be at least 20")
    for c in a.configs.split(","):
        if c not in SHAPES:
            raise SystemExit(f"geomed_measure: unknown config {c!r} (known: {', '.join(SHAPES)})")
    if not torch.cuda.is_available():
        raise SystemExit("geomed_measure: needs a GPU (a CPU run gives no time)")
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"], "shapes": []}
    for c in a.configs.split(","):
        K, P = SHAPES[c]
        res["shapes"].append(measure(c, K, P, a.reps, a.round_reps))
        torch.cuda.empty_cache()
        if a.out:  # (after every shape: a later shape's time limit does not lose the earlier ones)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
