"""Time frt_rotate and frt_unrotate (include/fedrotate.h) beside fsg_sign_row, and the device-resident rotated sign
round beside the plain sign1 round, in one process; recompute the kept-energy table on the host.

    python -u tools/rotate_measure.py [--reps 30] [--out profiles/rotate_measure.json]

Kernels, at 1 M and 25 M columns: device events around each wrapper call, three warm-up calls, then ``--reps`` (>= 20)
timed calls per kernel, the kernels alternating back to back so that drift of the machine falls on all of them;
medians.  Per kernel the algorithmic bytes — frt_rotate with a base reads 8 B and writes 4 B per column, frt_unrotate
reads 4 B and writes 4 B — against the 7.23 TB/s stream-read ceiling (profiles/r01_hbm_stream_read_ceiling.json).

Rounds, at 100 x 1 M, 100 x 25 M and 1000 x 25 M, rows resident in HBM: the plain round is fsg_reduce over P columns
and fcl_finish; the rotated round is fsg_reduce over P' columns, frt_unrotate in place and fcl_finish.  The
prediction made before the kernel existed: by bytes the rotated round exceeds the plain one by one frt_unrotate
(8 B / column at the read ceiling, 0.03 ms at 25 M).  ``meets_prediction`` is extra <= 1.5 x that.

Kept energy: the share of ||e||^2 the scaled sign keeps, with and without the rotation, for six update shapes at
P = 2^20 on the host (``encode_host``, ``rotate_host``), one seed per case.
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
from fedscale_amd import kernels_clip as kc  # noqa: E402
from fedscale_amd import kernels_rotate as kr  # noqa: E402
from fedscale_amd import kernels_sign as kg  # noqa: E402
from fedscale_amd.cloud.execution.rotate_upload import rotate_host  # noqa: E402
from fedscale_amd.cloud.execution.sign_upload import encode_host  # noqa: E402

READ_CEILING = 7.23e12  # B/s
KERNEL_P = (1_000_000, 25_000_000)
ROUNDS = ((100, 1_000_000), (100, 25_000_000), (1000, 25_000_000))
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


def entry(ms, nbytes) -> dict:
    med, lo, hi = ms
    floor_ms = nbytes / READ_CEILING * 1e3
    return {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "bytes": int(nbytes),
            "TBps": round(nbytes / (med * 1e-3) / 1e12, 3), "byte_floor_ms": round(floor_ms, 4),
            "share_of_read_ceiling": round(floor_ms / med, 4)}


def kernels(P: int, reps: int) -> dict:
    dev = torch.device("cuda:0")
    Pp = kr.padded(P)
    x = torch.empty(P, device=dev).normal_(0.0, 0.01)
    base = torch.empty(P, device=dev).normal_(0.0, 1.0)
    y = torch.empty(Pp, device=dev)
    out = torch.empty(P, device=dev)
    NB = kg.blocks(Pp)
    bits = torch.empty(NB * 32, dtype=torch.uint8, device=dev)
    scales = torch.empty(NB, device=dev)
    kr.rotate(x, base, P, 1, y)
    tr, tu, ts = timed([lambda: kr.rotate(x, base, P, 1, y), lambda: kr.unrotate(y, P, 1, out),
                        lambda: kg.sign_row(y, None, None, Pp, bits, scales, None)], reps)
    res = {"P": P, "P_padded": Pp, "frt_rotate": entry(tr, 8 * P + 4 * Pp), "frt_unrotate": entry(tu, 4 * Pp + 4 * P),
           "fsg_sign_row": entry(ts, 4 * Pp + Pp // 8 + 4 * NB)}
    for k in ("frt_rotate", "frt_unrotate", "fsg_sign_row"):
        print(f"[P={P}] {k} {res[k]}", flush=True)
    return res


def rounds(K: int, P: int, reps: int) -> dict:
    dev = torch.device("cuda:0")
    Pp = kr.padded(P)
    den = float(np.float32(K))
    bits = torch.empty(K, kg.bit_stride(Pp), dtype=torch.uint8, device=dev)
    scales = torch.empty(K, kg.scale_stride(Pp), device=dev).uniform_(0.005, 0.015)
    for k0 in range(0, K, BLOCK):
        bits[k0:k0 + BLOCK].random_(0, 256)
    # the plain round's rows are the first ceil(P / 8) bytes and ceil(P / 256) scales of the same rows
    pbits = bits[:, :kg.bit_stride(P)].contiguous()
    pscales = scales[:, :kg.scale_stride(P)].contiguous()
    last = torch.empty((P + 63) // 64 * 64, device=dev).normal_()
    chain_p = torch.empty((P + 63) // 64 * 64, device=dev)
    chain_r = torch.empty(Pp, device=dev)
    out = torch.empty((P + 63) // 64 * 64, device=dev)

    def plain():
        kg.reduce_sign(pbits, pscales, K, P, chain_p)
        kc.finish(chain_p, last, P, den, out)

    def rotated():
        kg.reduce_sign(bits, scales, K, Pp, chain_r)
        kr.unrotate(chain_r, P, 1, chain_r)
        kc.finish(chain_r, last, P, den, out)

    tp, tr = timed([plain, rotated], reps)
    predicted = (4 * Pp + 4 * P) / READ_CEILING * 1e3
    extra = round(tr[0], 4) - round(tp[0], 4)
    res = {"K": K, "P": P, "P_padded": Pp, "reps": reps, "plain_round_ms": round(tp[0], 4),
           "rotated_round_ms": round(tr[0], 4), "extra_ms": round(extra, 4),
           "predicted_extra_ms": round(predicted, 4), "extra_over_predicted": round(extra / predicted, 2),
           "meets_prediction": bool(extra <= 1.5 * predicted)}
    print(f"[round {K} x {P}] {res}", flush=True)
    return res


def kept_energy(P: int = 1 << 20) -> list:
    rng = np.random.default_rng(2026)
    g = lambda: rng.standard_normal(P)  # noqa: E731
    cases = {"gaussian": g(), "laplace": rng.laplace(size=P), "student_t_3": rng.standard_t(3, P),
             "sparse_1pct_gaussian": np.where(rng.random(P) < 0.01, g(), 0.0),
             "gaussian_lognormal_scales": g() * np.exp(2.0 * g()), "student_t_1.5": rng.standard_t(1.5, P)}

    def kept(v):
        v = np.ascontiguousarray(v, dtype=np.float32)
        _, _, r = encode_host(v)
        return 1.0 - float((r.astype(np.float64) ** 2).sum() / (v.astype(np.float64) ** 2).sum())

    out = []
    for name, e in cases.items():
        e = e.astype(np.float32)
        out.append({"update": name, "P": P, "sign1": round(kept(e), 4),
                    "sign1_rht4096": round(kept(rotate_host(e, None, 2026)), 4)})
        print(f"[kept energy] {out[-1]}", flush=True)
    return out


def main(argv=None) -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--out", default=None, help="write the JSON result here too")
    a = p.parse_args(argv)
    if a.reps < 20:
        raise SystemExit("rotate_measure: --reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("rotate_measure: needs a GPU (a CPU run gives no time)")
    res = {"device": torch.cuda.get_device_name(0), "build_id": _native.build_info()["build_id"],
           "build_defs": _native.build_info().get("defs", ""), "read_ceiling_Bps": READ_CEILING,
           "calls_per_median": a.reps, "kernels": [kernels(P, a.reps) for P in KERNEL_P], "rounds": []}
    for K, P in ROUNDS:
        res["rounds"].append(rounds(K, P, a.reps))
        torch.cuda.empty_cache()
    res["kept_energy"] = kept_energy()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
