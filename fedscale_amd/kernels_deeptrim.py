"""Typed torch-tensor wrappers over the deep trimmed mean's C ABI (include/feddeeptrim.h), with the same host-side
checks as ``kernels.reduce``: device / dtype / contiguity / size, launched on the current HIP stream of the output's
device.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native_deeptrim as ND
from ._native import ptr
from .kernels import _check_x, _dev, _pinned, _stream


def max_rows() -> int:
    """The largest round the kernel takes (fdt_max_rows)."""
    return int(ND.call("fdt_max_rows"))


def _check_t(K: int, t: int):
    if t < 1 or 2 * t >= K or K > ND.MAX_ROWS:
        raise ValueError(f"t={t} must satisfy 1 <= t and 2t < K={K}, and K <= {ND.MAX_ROWS} (fdt_max_rows)")


def reduce_deep(x: torch.Tensor, K: int, P: int, t: int, out: torch.Tensor, *, mirror: Optional[torch.Tensor] = None,
                dropped: Optional[torch.Tensor] = None, cus: int = 0) -> torch.Tensor:
    """out[:P] <- the trimmed mean of x[:K, :P] with t rows dropped per side and column (fdt_reduce).
    ``mirror``: a second copy of out, device or pinned host memory; ``dropped``: an int64 [K, 2] device table the
    per-row (low, high) drop counts are added to; ``cus``: plan the launch for this many compute units instead of the
    device's (the result's bits do not depend on it)."""
    ld = _check_x(x, K, P)
    _check_t(K, t)
    _dev(out, torch.float32, "out", P)
    if mirror is not None:
        if mirror.device.type == "cpu":
            _pinned(mirror, torch.float32, "mirror", P)
        else:
            _dev(mirror, torch.float32, "mirror", P)
    if dropped is not None:
        _dev(dropped, torch.int64, "dropped", 2 * K, align=8)
    ND.call("fdt_reduce", ptr(x), ld, int(K), int(P), int(t), ptr(out), ptr(mirror), ptr(dropped), int(cus),
            _stream(out))
    return out


def plan(cus: int, K: int, P: int, t: int) -> dict:
    """The launch fdt_reduce makes at (K, P, t) on a GPU of ``cus`` compute units (fdt_plan; no GPU needed): C (the
    columns of a tile, a function of K alone), lanes (per column), rows (per lane), lds (bytes), tiles, grid, wgs
    (workgroups per CU)."""
    buf = np.zeros(ND.PLAN_FIELDS, dtype=np.int64)
    ND.call("fdt_plan", int(cus), int(K), int(P), int(t), buf.ctypes.data)
    return dict(zip(("C", "lanes", "rows", "lds", "tiles", "grid", "wgs"), buf.tolist()))
