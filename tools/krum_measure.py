"""Time the kernels of Krum / Multi-Krum selection (include/fedkrum.h) beside fa_reduce over the same rows, in one
process ("Multi-Krum").

    python -u tools/krum_measure.py [--configs c2,k100,head] [--reps 20] [--out profiles/krum_measure.json]

Per shape (c2: 100 x 1 M; k100: 100 x 25 M; head: 1000 x 25 M) the device-resident rows are x_k = L + noise and
f = K // 5, m = K - f.  Three warm-up calls, then ``--reps`` timed calls each (fewer, at least 5, of a call that takes
more than 200 ms) of
    fa_reduce      weighted, no finalize, the same rows
    fk_gram        both launches: the tile partials on the fp64 matrix unit, then the split sum
    fk_gram_sum    a proxy — fk_gram at the smallest P with the same nsplit (4 steps per split): the split sum of the
                   same K x K x nsplit partials plus a partial launch of a few microseconds; the C ABI has no entry
                   point for the sum alone
    fk_scores, fk_select, fcl_reduce (the chain over the kept rows), fk_finish
alternating in that order; device events around each wrapper call; medians.  For the Gram partials (fk_gram minus the
proxy) it reports the achieved FLOP/s, counting tiles x 64^2 x P x 2, its share of the 78.6 TF fp64 matrix peak of the
public spec sheet, and the bytes per second the tiles fetch (rows of every tile x P x 4: a diagonal tile fetches its
rows once) with their share of the 7.23 TB/s stream-read ceiling (profiles/r01_hbm_stream_read_ceiling.json).  Then
the whole finish of a device-resident round (``adopt_resident``): ``KrumRound.finalize_mean`` against
``DeviceRound.finalize_mean``, alternating, ``--round-reps`` each.
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
from fedscale_amd import kernels_krum as kk  # noqa: E402

READ_CEILING = 7.23e12   # B/s
FP64_MATRIX_PEAK = 78.6e12  # FLOP/s, the public spec sheet's figure
SHAPES = {"c2": (100, 1_000_000), "k100": (100, 25_000_000), "head": (1000, 25_000_000)}
BLOCK = 50  # rows filled at a time: no second K x ld temporary


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


def tile_rows(K: int) -> int:
    """Rows the lower-triangle tiles fetch per column: a diagonal tile its own rows, another tile both operands'."""
    T = -(-K // 64)
    rows = [min(64, K - 64 * i) for i in range(T)]
    return sum(rows[i] if i == j else rows[i] + rows[j] for i in range(T) for j in range(i + 1))


def measure(name: str, K: int, P: int, reps: int, round_reps: int) -> dict:
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.krum_round import KrumRound, KrumSpec
    from fedscale_amd.round import DeviceRound

    dev = torch.device("cuda:0")
    f = K // 5
    m = K - f
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    st = ClientStaging(L, dev, K, bulk=False)
    x, ld = st.x, L.ld
    last = torch.empty(ld, device=dev).normal_(0.0, 1.0)
    fill(x, last)
    w = torch.ones(K, dtype=torch.float32, device=dev)
    out_a, out_k, chain = torch.empty(ld, device=dev), torch.empty(ld, device=dev), torch.empty(ld, device=dev)
    plan = kk.gram_plan(K, P)
    p_small = plan["nsplit"] * 4 * plan["step_cols"]
    assert kk.gram_plan(K, p_small)["nsplit"] == plan["nsplit"] and p_small <= P
    ws = kk.gram_workspace(K, P, dev)
    G = torch.empty(K * K, dtype=torch.float64, device=dev)
    G2 = torch.empty(K * K, dtype=torch.float64, device=dev)
    score = torch.empty(K, dtype=torch.float64, device=dev)
    c = torch.empty(K, dtype=torch.float32, device=dev)
    n_sel = torch.zeros(1, dtype=torch.int32, device=dev)
    res = {"config": name, "K": K, "P": P, "ld": ld, "f": f, "m": m, "reps": reps, "gram_plan": plan,
           "gram_sum_proxy_P": p_small, "workspace_bytes": kk.gram_workspace_bytes(K, P),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count}
    names = ["fa_reduce_weighted", "fk_gram", "fk_gram_sum_proxy", "fk_scores", "fk_select", "fcl_reduce_chain",
             "fk_finish", "fa_reduce_weighted_again"]
    fns = [lambda: kx.reduce(x, K, P, out_a, a=w),
           lambda: kk.gram(x, K, P, last, G, ws),
           lambda: kk.gram(x, K, p_small, last, G2, ws),
           lambda: kk.scores(G, K, f, score),
           lambda: kk.select(score, K, m, c, n_sel),
           lambda: kc.reduce_clip(x, K, P, last, c, chain),
           lambda: kk.finish(chain, last, n_sel, P, out_k)]
    fns.append(fns[0])
    ts = timed(fns, reps)
    for k, tm in zip(names, ts):
        res[k] = entry(tm, None if k == "fa_reduce_weighted" else ts[0][0])
    res["fa_reduce_spread"] = round(abs(ts[-1][0] / ts[0][0] - 1.0), 4)
    res["n_selected"] = int(n_sel.cpu()[0])
    part_s = max(ts[1][0] - ts[2][0], 1e-6) * 1e-3
    flop = plan["tiles"] * 64 * 64 * P * 2
    fetch = tile_rows(K) * P * 4 + plan["tiles"] * P * 4  # the rows, and the slice of L every tile reads
    res["gram_partials"] = {"ms": round(part_s * 1e3, 4), "flop": flop, "TFLOPs": round(flop / part_s / 1e12, 3),
                            "share_of_fp64_matrix_peak": round(flop / part_s / FP64_MATRIX_PEAK, 4),
                            "fetch_bytes": fetch, "fetch_TBps": round(fetch / part_s / 1e12, 3),
                            "share_of_read_ceiling": round(fetch / part_s / READ_CEILING, 4)}
    for k in names + ["gram_partials"]:
        print(f"[{name}] {k} {res[k]}", flush=True)
    del out_a, out_k, G2
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

    def krum_round():
        r = KrumRound(L, dev, K, KrumSpec(f), staging=st, last_f32=last, capacity=K)
        r.adopt_resident(K)
        return lambda: r.finalize_mean(den, float(K), out=out, cur_side=side)

    makers = [plain_round, krum_round]
    ms = [[] for _ in makers]
    for rep in range(2 + round_reps):  # two warm-up rounds of each
        for i, make in enumerate(makers):
            fin = make()
            torch.cuda.synchronize()
            t = _once(fin)
            if rep >= 2:
                ms[i].append(t)
    tm = [(float(np.median(v)), float(min(v)), float(max(v)), len(v)) for v in ms]
    res["device_round_finish"] = entry(tm[0])
    res["krum_round_finish"] = entry(tm[1])
    res["krum_round_finish"]["ratio_to_device_round_finish"] = round(tm[1][0] / tm[0][0], 4)
    for k in ("device_round_finish", "krum_round_finish"):
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
        raise SystemExit("krum_measure: --reps must be at least 20")
    for c in a.configs.split(","):
        if c not in SHAPES:
            raise SystemExit(f"krum_measure: unknown config {c!r} (known: {', '.join(SHAPES)})")
    if not torch.cuda.is_available():
        raise SystemExit("krum_measure: needs a GPU (a CPU run gives no time)")
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "read_ceiling_Bps": READ_CEILING, "fp64_matrix_peak_FLOPs": FP64_MATRIX_PEAK, "shapes": []}
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
