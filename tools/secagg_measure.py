"""Time the stages of a secure-aggregation round (include/fedsecagg.h) beside fa_reduce over the same bytes, in one
process ("Secure aggregation").

    python -u tools/secagg_measure.py [--configs c1,c2,k100,head] [--reps 20] [--out profiles/secagg_measure.json]

Per shape (c1: 10 x 24,492, the FEMNIST CNN, a bucket of six mask workgroups; c2: 100 x 1 M; k100: 100 x 25 M; head:
1000 x 25 M) the rows are device-resident: fp32 x_k = L + noise for fa_reduce and the SAME memory read as uint32 words
for fsa_reduce (a modular sum does not care what the bits mean), so both kernels stream the same K x P x 4 bytes.
Three warm-up calls, then ``--reps`` timed calls each (fewer, at least 5, of a call that takes more than 200 ms) of
    fa_reduce        unweighted, no finalize
    fsa_reduce       the modular sum
    fsa_mask_sum     at M = 10, 100 and 1000 keys (half added, half subtracted), in place on the sum
    fsa_finish       with its range count
alternating in that order; device events around each wrapper call; medians.  The mask sum is also reported as ns per
key x column, as key x columns per second and as a fraction of fsa_reduce; the op-count estimate it stands beside is
about 62 integer ops per word (20 rounds x 4 quarter rounds x 12 ops, 16 adds of the input and 16 of the sum, per 16
words).  Then the whole finish of a device-resident round (``adopt_resident``): ``SecAggRound.finalize_mean`` with K
self-mask keys to remove (every client arrived, nobody dropped; ``verify=False``: the rows are noise, not masked
updates) against ``DeviceRound.finalize_mean``, alternating, ``--round-reps`` each.
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
from fedscale_amd import kernels_secagg as ks  # noqa: E402

SHAPES = {"c1": (10, 24_492), "c2": (100, 1_000_000), "k100": (100, 25_000_000), "head": (1000, 25_000_000)}
BLOCK = 50  # rows filled at a time: no second K x ld temporary
MASK_KEYS = (10, 100, 1000)
OPS_PER_WORD = (20 * 4 * 12 + 16 + 16) / 16.0  # the op-count estimate: 62 integer ops per keystream word


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


def entry(ms, base=None, base_name="fsa_reduce") -> dict:
    med, lo, hi, n = ms
    r = {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "calls": n}
    if base is not None:
        r["ratio_to_" + base_name] = round(med / base, 4)
    return r


def measure(name: str, K: int, P: int, reps: int, round_reps: int) -> dict:
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.round import DeviceRound
    from fedscale_amd.secagg_round import MaskedStaging, SecAggRound, SecAggSpec

    dev = torch.device("cuda:0")
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    st = ClientStaging(L, dev, K, bulk=False)
    x, ld = st.x, L.ld
    y = x.view(torch.int32)  # the same rows as uint32 words
    last = torch.empty(ld, device=dev).normal_(0.0, 1.0)
    fill(x, last)
    out_a, out_f = (torch.empty(ld, device=dev) for _ in range(2))
    total = torch.empty(ld, dtype=torch.int32, device=dev)
    oor = torch.zeros(1, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(0)
    keys = torch.from_numpy(rng.integers(0, 1 << 32, (max(MASK_KEYS + (K,)), 8), dtype=np.uint64)
                            .astype(np.uint32).view(np.int32)).to(dev)
    spec = SecAggSpec(16, 20, verify=False)
    spec.check_clients(K)
    res = {"config": name, "K": K, "P": P, "ld": ld, "reps": reps, "bytes_reduced": K * P * 4,
           "ops_per_word_estimate": OPS_PER_WORD, "reduce_plan": ks.reduce32_plan(
               torch.cuda.get_device_properties(0).multi_processor_count, K, P),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count,
           "mask_workgroups": -(-P // 4096)}
    names = ["fa_reduce", "fsa_reduce"] + [f"fsa_mask_sum_M{m}" for m in MASK_KEYS] + ["fsa_finish", "fa_reduce_again"]
    fns = [lambda: kx.reduce(x, K, P, out_a), lambda: ks.reduce32(y, K, P, total)]
    fns += [(lambda m=m: ks.mask_sum(keys, m // 2, m - m // 2, (1, 2, 3), P, total, total)) for m in MASK_KEYS]
    fns.append(lambda: ks.finish(total, last, P, spec.frac_bits, spec.mag_bits, K, out_f, oor))
    fns.append(fns[0])
    ts = timed(fns, reps)
    for k, tm in zip(names, ts):
        res[k] = entry(tm, None if k == "fsa_reduce" else ts[1][0])
    res["fa_reduce_spread"] = round(abs(ts[-1][0] / ts[0][0] - 1.0), 4)
    res["fa_reduce_GBps"] = round(K * P * 4 / (ts[0][0] * 1e-3) / 1e9, 1)
    res["fsa_reduce_GBps"] = round(K * P * 4 / (ts[1][0] * 1e-3) / 1e9, 1)
    for m in MASK_KEYS:
        e = res[f"fsa_mask_sum_M{m}"]
        e["ns_per_key_column"] = round(e["ms_median"] * 1e6 / (m * P), 6)
        e["G_key_columns_per_s"] = round(m * P / (e["ms_median"] * 1e-3) / 1e9, 2)
        e["T_int_ops_per_s_at_estimate"] = round(OPS_PER_WORD * m * P / (e["ms_median"] * 1e-3) / 1e12, 2)
    for k in names + ["fa_reduce_GBps", "fsa_reduce_GBps"]:
        print(f"[{name}] {k} {res[k]}", flush=True)
    del out_a, out_f, total
    torch.cuda.empty_cache()
    if round_reps <= 0:
        return res
    # the whole finish of a device-resident round; the masked staging adopts the rows that are already there
    mst = MaskedStaging(L, dev, 1)
    mst.y, mst.capacity = y, K
    mst.xi = torch.zeros(K, L.ldq, dtype=torch.int64, device=dev)
    den = float(np.float32(K))
    out = torch.empty(ld, device=dev)
    side = torch.zeros(L.ldq, dtype=torch.float64, device=dev)
    self_keys = keys[:K].cpu().numpy().view(np.uint32)

    def plain_round():
        r = DeviceRound(L, dev, K, "fedavg", capacity=K, staging=st)
        r.adopt_resident(K)
        return lambda: r.finalize_mean(den, float(K), out=out, cur_side=side)

    def secagg_round():
        r = SecAggRound(L, dev, K, "fedavg", spec, staging=mst, last_f32=last, capacity=K)
        r.adopt_resident(K)
        r.unmask(self_keys, [], (1, 2, 3))
        return lambda: r.finalize_mean(den, float(K), out=out, cur_side=side)

    makers = [plain_round, secagg_round]
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
    res["secagg_round_finish"] = entry(tm[1], tm[0][0], "device_round_finish")
    res["secagg_round_keys"] = K
    for k in ("device_round_finish", "secagg_round_finish"):
        print(f"[{name}] {k} {res[k]}", flush=True)
    res["round_reps"] = round_reps
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="c1,c2,k100,head")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--round-reps", type=int, default=5)
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("secagg_measure: --reps must be at least 20")
    for c in a.configs.split(","):
        if c not in SHAPES:
            raise SystemExit(f"secagg_measure: unknown config {c!r} (known: {', '.join(SHAPES)})")
    if not torch.cuda.is_available():
        raise SystemExit("secagg_measure: needs a GPU (a CPU run gives no time)")
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
