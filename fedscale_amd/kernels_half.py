"""Typed torch-tensor wrappers over the 16-bit upload path's C ABI (include/fedhalf.h), with the same host-side
checks as ``kernels.reduce``: device / dtype / contiguity / size, launched on the current HIP stream of the
output's device.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _native_half as NH
from ._native import FA_ACCUMULATE, FA_FINALIZE, ptr
from .kernels import _cols, _dev, _pinned, _stream, _strip_plan

#: the 16-bit row element types: name -> (torch dtype, FH_* code)
ROW_DTYPES = {"float16": (torch.float16, NH.FH_F16), "bfloat16": (torch.bfloat16, NH.FH_BF16)}
_CODE_OF = {t: c for t, c in ROW_DTYPES.values()}


def row_dtype(dtype):
    """(torch dtype, FH_* code) of an upload dtype given by name or as a torch dtype; ValueError otherwise."""
    if isinstance(dtype, torch.dtype) and dtype in _CODE_OF:
        return dtype, _CODE_OF[dtype]
    if isinstance(dtype, str) and dtype in ROW_DTYPES:
        return ROW_DTYPES[dtype]
    raise ValueError(f"upload dtype {dtype!r}: expected 'float16' or 'bfloat16'")


def _check_x16(x: torch.Tensor, K: int, P: int) -> int:
    if not isinstance(x, torch.Tensor) or x.dtype not in _CODE_OF:
        raise TypeError(f"x16: expected a torch.float16 / torch.bfloat16 tensor, got "
                        f"{getattr(x, 'dtype', type(x).__name__)}")
    _dev(x, x.dtype, "x16")
    if x.dim() != 2:
        raise ValueError("x16: expected a [K, ld] client-major buffer")
    if K > x.shape[0]:
        raise ValueError(f"x16: K={K} > rows {x.shape[0]}")
    ld = x.shape[1]
    if ld < P or ld % 64:
        raise ValueError(f"x16: ld={ld} must be >= P={P} and a multiple of 64")
    return ld


def reduce16(x16: torch.Tensor, K: int, P: int, out: torch.Tensor, *, a: Optional[torch.Tensor] = None,
             acc_in: Optional[torch.Tensor] = None, denom: float = 1.0, finalize: bool = False,
             mirror: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fa_reduce's in-order fp32 chain over the 16-bit rows x16[:K, :P] (fh_reduce); ``mirror`` (with
    ``finalize``): a second copy of the mean, device or pinned host memory."""
    if K > 0:
        ld = _check_x16(x16, K, P)
        code = _CODE_OF[x16.dtype]
    else:
        ld, code = (x16.shape[1], _CODE_OF[x16.dtype]) if x16 is not None else ((P + 63) // 64 * 64, NH.FH_F16)
    _dev(out, torch.float32, "out", _cols(P))
    if a is not None:
        _dev(a, torch.float32, "a", K, align=4)
    if acc_in is not None:
        _dev(acc_in, torch.float32, "acc_in", _cols(P))
    if mirror is not None:
        if not finalize:
            raise ValueError("mirror: needs finalize=True")
        if mirror.device.type == "cpu":
            _pinned(mirror, torch.float32, "mirror", _cols(P))
        else:
            _dev(mirror, torch.float32, "mirror", _cols(P))
    flags = (FA_ACCUMULATE if acc_in is not None else 0) | (FA_FINALIZE if finalize else 0)
    NH.call("fh_reduce", ptr(x16) if K > 0 else None, code, ld, K, P, ptr(a), ptr(acc_in), ptr(out), ptr(mirror),
            float(denom), flags, _stream(out))
    return out


def reduce16_plan(cus: int, K: int, P: int, weighted: bool = False) -> list:
    """The launches fh_reduce makes at (K, P) on a GPU of ``cus`` compute units (fh_reduce_plan; no GPU needed):
    a list of dicts V, U, col0, tiles, sw, grid."""
    return _strip_plan(lambda out, cap: NH.call("fh_reduce_plan", int(cus), int(K), int(P), 1 if weighted else 0,
                                                out, cap), NH.PLAN_FIELDS)


def reduce16_launches(K: int, P: int, weighted: bool = False) -> int:
    """Kernel launches one fh_reduce call makes at (K, P) on the current device (fh_reduce_launches)."""
    return int(NH.call("fh_reduce_launches", int(K), int(P), 1 if weighted else 0))


def pack_row16(tensors: Sequence[torch.Tensor], offsets: Sequence[int], row16: torch.Tensor) -> torch.Tensor:
    """Round the fp32 device tensors into the 16-bit device row at element offsets ``offsets`` (fh_pack_row: one
    multi-tensor launch per 64 tensors; elements of the row outside every tensor are left untouched)."""
    if not isinstance(row16, torch.Tensor) or row16.dtype not in _CODE_OF:
        raise TypeError("row16: expected a torch.float16 / torch.bfloat16 tensor")
    _dev(row16, row16.dtype, "row16", align=2)
    if len(tensors) != len(offsets):
        raise ValueError("pack_row16: one offset per tensor")
    n = row16.numel()
    for i, (t, o) in enumerate(zip(tensors, offsets)):
        _dev(t, torch.float32, f"tensors[{i}]", align=4)
        if t.device != row16.device:
            raise ValueError(f"tensors[{i}]: on {t.device}, the row on {row16.device}")
        if o < 0 or o + t.numel() > n:
            raise ValueError(f"tensors[{i}]: elements [{o}, {o + t.numel()}) outside the row of {n}")
    T = len(tensors)
    src = np.asarray([t.data_ptr() for t in tensors], dtype=np.uint64)
    numel = np.asarray([t.numel() for t in tensors], dtype=np.int64)
    off = np.asarray(list(offsets), dtype=np.int64)
    NH.call("fh_pack_row", src.ctypes.data, numel.ctypes.data, off.ctypes.data, T, ptr(row16), _CODE_OF[row16.dtype],
            _stream(row16))
    return row16
