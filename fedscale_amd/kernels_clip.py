"""Typed torch-tensor wrappers over norm-clipped FedAvg's C ABI (include/fedclip.h), with the same host-side checks
as ``kernels.reduce``: device / dtype / contiguity / size, launched on the current HIP stream of the output's device.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native_clip as NC
from ._native import FA_ACCUMULATE, ptr
from .kernels import _check_x, _cols, _dev, _pinned, _stream, _strip_plan


def workspace_bytes(n: int, P: int) -> int:
    """Bytes of the workspace ``row_sqnorms`` needs for n rows of P columns (fcl_workspace_bytes)."""
    return int(NC.call("fcl_workspace_bytes", int(n), int(P)))


def workspace(n: int, P: int, device) -> torch.Tensor:
    """A float64 workspace for ``row_sqnorms`` over up to n rows of P columns."""
    return torch.empty(workspace_bytes(n, P) // 8, dtype=torch.float64, device=device)


def row_sqnorms(x: torch.Tensor, n: int, P: int, last: torch.Tensor, sq: torch.Tensor,
                ws: torch.Tensor) -> torch.Tensor:
    """sq[k] <- the fp64 squared norm of x[k, :P] - last[:P], k < n (fcl_row_sqnorms); ``ws``: ``workspace``."""
    ld = _check_x(x, n, P)
    _dev(last, torch.float32, "last", _cols(P))
    _dev(sq, torch.float64, "sq", n, align=8)
    _dev(ws, torch.float64, "workspace", 1, align=8)
    NC.call("fcl_row_sqnorms", ptr(x), ld, int(n), int(P), ptr(last), ptr(sq), ptr(ws), ws.numel() * 8, _stream(sq))
    return sq


def norm_plan(cus: int, P: int) -> dict:
    """The launches fcl_row_sqnorms makes at P columns on ``cus`` compute units (fcl_norm_plan; no GPU needed)."""
    buf = np.zeros(4, dtype=np.int64)
    n = int(NC.call("fcl_norm_plan", int(cus), int(P), buf.ctypes.data))
    return dict(launches=n, tiles=int(buf[0]), grid=int(buf[1]), waves=int(buf[2]), tile_cols=int(buf[3]))


def clip_coefs(sq: torch.Tensor, n: int, max_norm: float, c: torch.Tensor, rejected: torch.Tensor) -> torch.Tensor:
    """c[k] <- the clip coefficient of sq[k] against max_norm, k < n; rejected[0] += rows whose sq is not finite
    (fcl_clip_coefs)."""
    _dev(sq, torch.float64, "sq", n, align=8)
    _dev(c, torch.float32, "c", n, align=4)
    _dev(rejected, torch.int32, "rejected", 1, align=4)
    NC.call("fcl_clip_coefs", ptr(sq), int(n), float(max_norm), ptr(c), ptr(rejected), _stream(c))
    return c


def reduce_clip(x: torch.Tensor, n: int, P: int, last: torch.Tensor, c: torch.Tensor, out: torch.Tensor, *,
                acc_in: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[:P] <- the clipped chain over x[:n, :P] against ``last`` with coefficients ``c``, continuing ``acc_in``
    when given (fcl_reduce); out may be acc_in."""
    ld = _check_x(x, n, P) if n > 0 else (x.shape[1] if x is not None else _cols(P))
    _dev(last, torch.float32, "last", _cols(P))
    _dev(out, torch.float32, "out", P)
    if n > 0:
        _dev(c, torch.float32, "c", n, align=4)
    if acc_in is not None:
        _dev(acc_in, torch.float32, "acc_in", _cols(P))
    NC.call("fcl_reduce", ptr(x) if n > 0 else None, ld, int(n), int(P), ptr(last), ptr(c) if n > 0 else None,
            ptr(acc_in), ptr(out), FA_ACCUMULATE if acc_in is not None else 0, _stream(out))
    return out


def reduce_clip_plan(cus: int, K: int, P: int) -> list:
    """The launches fcl_reduce makes at (K, P) on a GPU of ``cus`` compute units (fcl_reduce_plan; no GPU needed):
    a list of dicts V, U, col0, tiles, sw, grid."""
    return _strip_plan(lambda out, cap: NC.call("fcl_reduce_plan", int(cus), int(K), int(P), out, cap),
                       NC.PLAN_FIELDS)


def finish(chain: torch.Tensor, last: torch.Tensor, P: int, denom: float, out: torch.Tensor, *,
           z: Optional[torch.Tensor] = None, sigma: float = 0.0, mean_delta_out: Optional[torch.Tensor] = None,
           mirror: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[:P] <- last + (chain / denom [+ sigma * z]) (fcl_finish); ``mean_delta_out``: the bracket; ``mirror``:
    a second copy of out, device or pinned host memory."""
    _dev(chain, torch.float32, "chain", _cols(P))
    _dev(last, torch.float32, "last", _cols(P))
    _dev(out, torch.float32, "out", P)
    if sigma > 0:
        if z is None:
            raise ValueError("finish: sigma > 0 needs z")
        _dev(z, torch.float32, "z", _cols(P))
    if mean_delta_out is not None:
        _dev(mean_delta_out, torch.float32, "mean_delta_out", P)
    if mirror is not None:
        if mirror.device.type == "cpu":
            _pinned(mirror, torch.float32, "mirror", P)
        else:
            _dev(mirror, torch.float32, "mirror", P)
    NC.call("fcl_finish", ptr(chain), ptr(last), ptr(z) if sigma > 0 else None, float(sigma), float(denom), int(P),
            ptr(out), ptr(mean_delta_out), ptr(mirror), _stream(out))
    return out
