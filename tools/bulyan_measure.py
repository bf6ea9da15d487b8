"""Time Bulyan (include/fedbulyan.h) beside the rules it is built from, over the same device-resident rows, in one
process ("Bulyan").

    python -u tools/bulyan_measure.py [--configs c2,wide,head] [--reps 20] [--out profiles/bulyan_measure.json]

Per shape (c2: 100 x 1 M; wide: 100 x 25 M; head: 1000 x 25 M) the rows are x_k = L + noise, staged through
``adopt_resident``; f is 10 % of K and the largest f that K allows ((K - 3) // 4).  Two warm-up rounds, then ``--reps``
(>= 20) timed repeats each of
    fbl_reduce                       over the theta rows fbl_select picked          4 theta P + 4 P bytes
    fbl_reduce with the kept counts  the same launch as BulyanRound makes it
    fdt_reduce at the median         over the same theta rows, gathered contiguous  (the parent's kernel)
    fbl_select                       theta + 2 launches, from the round's Gram matrix
    BulyanRound.finalize_mean        fk_gram, fbl_select, fbl_reduce
    KrumRound.finalize_mean          Multi-Krum at the same f
    DeviceRound.finalize_mean        one finalising fa_reduce
alternating in that order, so that drift of the machine falls on all of them; device events around each; medians.
Reported: ms, and for fbl_reduce the verdicts on its two predictions — "one read of the theta rows at the 7.23 TB/s
stream-read ceiling" (profiles/r01_hbm_stream_read_ceiling.json) and the operation count of DESIGN.md (128 vector
instructions of 4 cycles per 64 padded elements at 2.4 GHz on 4 SIMDs of every CU, plus 15 % for the chain) — each met
within 1.15 x, else "missed, n x"; for fbl_select "theta + 2 launches of 10 us"; and the ratio fdt_reduce / fbl_reduce
that decides whether the barrier-free selection paid.
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
from fedscale_amd import kernels_bulyan as kb  # noqa: E402
from fedscale_amd import kernels_deeptrim as kd  # noqa: E402

READ_CEILING = 7.23e12  # B/s
CLOCK = 2.4e9           # Hz
LAUNCH_S = 10e-6        # what one small dependent launch is predicted to cost
SHAPES = {"c2": (100, 1_000_000), "wide": (100, 25_000_000), "head": (1000, 25_000_000)}
BLOCK = 50  # rows filled at a time: no second K x ld temporary


def fill(x: torch.Tensor, last: torch.Tensor):
    """x_k = last + N(0, 0.01^2)."""
    for k0 in range(0, x.shape[0], BLOCK):
        b = x[k0:k0 + BLOCK]
        b.normal_(0.0, 0.01)
        b.add_(last)


def verdict(ms: float, predicted_ms: float) -> str:
    n = ms / predicted_ms
    return "met" if n <= 1.15 else f"missed, {n:.2f} x"


def measure(name: str, K: int, P: int, f: int, reps: int) -> dict:
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.bulyan_round import BulyanRound, BulyanSpec
    from fedscale_amd.krum_round import KrumRound, KrumSpec
    from fedscale_amd.round import DeviceRound

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    st = ClientStaging(L, dev, K, bulk=False)
    last = torch.empty(L.ld, device=dev).normal_(0.0, 1.0)
    fill(st.x, last)
    den = float(np.float32(K))
    out = torch.empty(L.ld, device=dev)
    side = torch.zeros(L.ldq, dtype=torch.float64, device=dev)
    theta, beta = kb.counts(K, f)

    def maker(cls, *spec, **kw):
        def make():
            r = cls(L, dev, K, *spec, staging=st, capacity=K, **kw)
            r.adopt_resident(K)
            return lambda: r.finalize_mean(den, float(K), out=out, cur_side=side)
        return make

    # one Bulyan round up front: its Gram matrix and selection feed the kernel timings
    first = BulyanRound(L, dev, K, BulyanSpec(f), staging=st, capacity=K, last_f32=last)
    first.adopt_resident(K)
    first.finalize_mean(den, float(K), out=out, cur_side=side)
    torch.cuda.synchronize()
    assert first.n_selected == theta
    gram, sel, n_sel = first._gram, first._sel.clone(), first._n_sel.clone()
    picks, sel2, n2 = torch.empty_like(sel), torch.empty_like(sel), torch.empty_like(n_sel)
    sws = kb.select_workspace(K, dev)
    rows = st.x[sel.long()].contiguous()  # the same theta rows, contiguous, for the parent's kernel
    t_med = (theta - 1) // 2

    kept = torch.zeros(K, dtype=torch.int64, device=dev)
    names = ["fbl_reduce", "fbl_reduce_counted", "fbl_select", "bulyan_round_finish", "krum_round_finish",
             "device_round_finish"]
    makers = [lambda: lambda: kb.reduce_bulyan(st.x, K, P, sel, n_sel, theta, beta, last, out),
              lambda: lambda: kb.reduce_bulyan(st.x, K, P, sel, n_sel, theta, beta, last, out, kept=kept),
              lambda: lambda: kb.select(gram, K, f, picks, sel2, n2, sws),
              maker(BulyanRound, BulyanSpec(f), last_f32=last), maker(KrumRound, KrumSpec(f), last_f32=last),
              maker(DeviceRound, "fedavg")]
    if t_med >= 1:
        names.insert(1, "fdt_reduce_median_same_rows")
        makers.insert(1, lambda: lambda: kd.reduce_deep(rows, theta, P, t_med, out))
    ms = [[] for _ in makers]
    for rep in range(2 + reps):  # two warm-up rounds of each
        for i, make in enumerate(makers):
            fin = make()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fin()
            b.record()
            b.synchronize()
            if rep >= 2:
                ms[i].append(a.elapsed_time(b))
    plan = kb.plan(cus, theta, P)
    bytes_ms = 4 * theta * P / READ_CEILING * 1e3
    # two bisections of 32 steps, a compare and an add per register key: 128 instructions of 4 cycles per 64 padded
    # elements, on the 4 SIMDs of every CU
    padded = plan["lanes"] * plan["rows"] * P
    ops_ms = 1.15 * padded / 64 * 128 * 4 / (cus * 4 * CLOCK) * 1e3  # (15 %: the chain's theta dependent adds)
    sel_ms = (theta + 2) * LAUNCH_S * 1e3
    res = {"config": name, "K": K, "P": P, "f": f, "theta": theta, "beta": beta, "reps": reps, "cus": cus,
           "fbl_plan": plan, "predicted_ms_fbl_reduce_bytes": round(bytes_ms, 4),
           "predicted_ms_fbl_reduce_ops": round(ops_ms, 4), "predicted_ms_fbl_select": round(sel_ms, 4)}
    med = {}
    for k, m in zip(names, ms):
        med[k] = float(np.median(m))
        res[k] = {"ms_median": round(med[k], 4), "ms_min": round(min(m), 4), "ms_max": round(max(m), 4)}
    res["fbl_reduce"]["one_read_at_ceiling"] = verdict(med["fbl_reduce"], bytes_ms)
    res["fbl_reduce"]["operation_count"] = verdict(med["fbl_reduce"], ops_ms)
    res["fbl_select"]["launches"] = verdict(med["fbl_select"], sel_ms)
    if "fdt_reduce_median_same_rows" in med:
        res["fdt_over_fbl"] = round(med["fdt_reduce_median_same_rows"] / med["fbl_reduce"], 3)
    for k in names:
        print(f"[{name} f={f}] {k} {res[k]}", flush=True)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--configs", default="c2,wide,head")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("bulyan_measure: --reps must be at least 20")
    for c in a.configs.split(","):
        if c not in SHAPES:
            raise SystemExit(f"bulyan_measure: unknown config {c!r} (known: {', '.join(SHAPES)})")
    if not torch.cuda.is_available():
        raise SystemExit("bulyan_measure: needs a GPU (a CPU run gives no time)")
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "read_ceiling_Bps": READ_CEILING, "shapes": []}
    for c in a.configs.split(","):
        K, P = SHAPES[c]
        for f in (K // 10, (K - 3) // 4):
            res["shapes"].append(measure(c, K, P, f, a.reps))
            torch.cuda.empty_cache()
            if a.out:  # after every shape: a later shape that runs out of time loses nothing
                with open(a.out, "w") as fh:
                    fh.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
