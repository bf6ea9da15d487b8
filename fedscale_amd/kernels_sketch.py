"""Typed torch-tensor wrappers over the Count-Sketch upload path's C ABI (include/fedsketch.h), with the same
host-side checks as ``kernels_sparse``: device / dtype / contiguity / size, launched on the current HIP stream of the
output's device.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native_sketch as NK
from ._native import ptr
from .kernels import _dev, _stream

TILE = NK.TILE  #: the largest bucket tile of an fcs_sketch_row workgroup (a compile-time constant of the library)
U = NK.U        #: blocks whose loads a lane of fcs_sketch_row keeps in flight
_M64 = (1 << 64) - 1


def table_floats(R: int, C: int) -> int:
    """R * C, refused unless (R, C) is a shape of the contract (fcs_table_floats; no GPU needed)."""
    return int(NK.call("fcs_table_floats", int(R), int(C)))


def sketch_plan(cus: int, P: int, R: int, C: int) -> dict:
    """The launch fcs_sketch_row makes at (P, R, C) on a GPU of ``cus`` compute units (fcs_sketch_plan; no GPU
    needed): tile, U, blocks, grid."""
    buf = np.zeros(NK.PLAN_FIELDS, dtype=np.int64)
    NK.call("fcs_sketch_plan", int(cus), int(P), int(R), int(C), buf.ctypes.data)
    return dict(zip(("tile", "U", "blocks", "grid"), buf.tolist()))


def _same(dev, **ts):
    for name, t in ts.items():
        if t is not None and t.device != dev:
            raise ValueError(f"{name}: on {t.device}, the output on {dev}")


def sketch_row(x: torch.Tensor, base: Optional[torch.Tensor], r_in: Optional[torch.Tensor], P: int, R: int, C: int,
               seed: int, table: torch.Tensor, *, subtract: bool = False, tile: int = 0) -> torch.Tensor:
    """table[:R * C] <- the blocked Count Sketch of x[:P] - base[:P] (+ r_in[:P]); with ``subtract`` the table minus
    that sketch, in place (fcs_sketch_row).  ``tile``: 0 for the plan's, or 256 / 512 / 1024 (the same bits)."""
    P, n = int(P), table_floats(R, C)
    _dev(table, torch.float32, "table", n)
    for t, name in ((x, "x"), (base, "base"), (r_in, "r_in")):
        if t is not None:
            _dev(t, torch.float32, name, P)
    _same(table.device, x=x, base=base, r_in=r_in)
    NK.call("fcs_sketch_row", ptr(x), ptr(base), ptr(r_in), P, int(R), int(C), int(seed) & _M64, ptr(table),
            int(tile), NK.SUBTRACT_FROM if subtract else 0, _stream(table))
    return table


def estimate(table: torch.Tensor, P: int, R: int, C: int, seed: int, est: torch.Tensor) -> torch.Tensor:
    """est[:P] <- the median-of-R estimate of every column out of ``table`` (fcs_estimate)."""
    P = int(P)
    _dev(table, torch.float32, "table", table_floats(R, C))
    _dev(est, torch.float32, "est", P)
    _same(est.device, table=table)
    NK.call("fcs_estimate", ptr(table), P, int(R), int(C), int(seed) & _M64, ptr(est), _stream(est))
    return est


def state_step(s: torch.Tensor, su_in: torch.Tensor, se_in: torch.Tensor, rho: float, n: int, su_out: torch.Tensor,
               se_out: torch.Tensor, nonfinite: torch.Tensor):
    """su_out <- rho * su_in + s, se_out <- se_in + su_out over n floats; nonfinite (int32 [1], the bits of a
    uint32) += the non-finite entries of s (fcs_state_step)."""
    n = int(n)
    for t, name in ((s, "s"), (su_in, "su_in"), (se_in, "se_in"), (su_out, "su_out"), (se_out, "se_out")):
        _dev(t, torch.float32, name, n)
    _dev(nonfinite, torch.int32, "nonfinite", 1, align=4)
    _same(su_out.device, s=s, su_in=su_in, se_in=se_in, se_out=se_out, nonfinite=nonfinite)
    NK.call("fcs_state_step", ptr(s), ptr(su_in), ptr(se_in), float(np.float32(rho)), n, ptr(su_out), ptr(se_out),
            ptr(nonfinite), _stream(su_out))


def apply_pairs(idx: torch.Tensor, val: torch.Tensor, k: int, P: int, dense: torch.Tensor, l_in: torch.Tensor,
                l_out: torch.Tensor):
    """dense[:P] <- the k pairs densified over +0.0; l_out[:P] <- l_in[:P] with l_in[idx] + val at the named columns
    (fcs_apply).  idx: int32 tensor holding uint32 bits, unique values."""
    k, P = int(k), int(P)
    _dev(idx, torch.int32, "idx", k, align=4)
    _dev(val, torch.float32, "val", k, align=4)
    for t, name in ((dense, "dense"), (l_in, "l_in"), (l_out, "l_out")):
        _dev(t, torch.float32, name, P)
    _same(l_out.device, idx=idx, val=val, dense=dense, l_in=l_in)
    NK.call("fcs_apply", ptr(idx), ptr(val), k, P, ptr(dense), ptr(l_in), ptr(l_out), _stream(l_out))
