"""Typed torch-tensor wrappers over the MXFP4 delta-upload path's C ABI (include/fedquant4.h), with the same host-side
checks as ``kernels_quant``: device / dtype / contiguity / size, launched on the current HIP stream of the output's
device.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _native_quant4 as NQ4
from ._native import FA_ACCUMULATE, ptr
from .kernels import _cols, _dev, _stream, _strip_plan

BLOCK = NQ4.BLOCK  #: columns that share one scale byte (16 code bytes)


def blocks(P: int) -> int:
    """Scale bytes of a row of P columns: ceil(P / 32)."""
    return (int(P) + BLOCK - 1) // BLOCK


def code_bytes(P: int) -> int:
    """Code bytes of a row of P columns on the wire: 16 per block, the padding codes of the last block included."""
    return blocks(P) * (BLOCK // 2)


def _check_rows(q4: torch.Tensor, scales: torch.Tensor, n: int, P: int):
    for t, name in ((q4, "q4"), (scales, "scales")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise TypeError(f"{name}: expected a torch.uint8 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        _dev(t, torch.uint8, name)
        if t.dim() != 2:
            raise ValueError(f"{name}: expected a [n, stride] client-major buffer")
        if n > t.shape[0]:
            raise ValueError(f"{name}: n={n} > rows {t.shape[0]}")
    ld, lds = 2 * q4.shape[1], scales.shape[1]
    if ld < P or ld % 64:
        raise ValueError(f"q4: rows of {q4.shape[1]} bytes hold ld={ld} columns; ld must be >= P={P} and a multiple "
                         f"of 64")
    if lds < blocks(P):
        raise ValueError(f"scales: lds={lds} must be >= ceil(P / 32)={blocks(P)}")
    if scales.device != q4.device:
        raise ValueError(f"scales: on {scales.device}, q4 on {q4.device}")
    return ld, lds


def reduce4(q4: torch.Tensor, scales: torch.Tensor, n: int, P: int, out: torch.Tensor, *,
            acc_in: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[:P] <- the in-order fp32 chain over the dequantised rows (q4 [n, ld / 2], scales [n, lds])[:n, :P],
    continuing ``acc_in`` when given (fq4_reduce); out may be acc_in, and is written in [0, P) only."""
    if n > 0:
        ld, lds = _check_rows(q4, scales, n, P)
    else:
        ld, lds = (P + 63) // 64 * 64, blocks(P)
    _dev(out, torch.float32, "out", P)
    if acc_in is not None:
        _dev(acc_in, torch.float32, "acc_in", _cols(P))
    NQ4.call("fq4_reduce", ptr(q4) if n > 0 else None, ptr(scales) if n > 0 else None, ld, lds, int(n), int(P),
             ptr(acc_in), ptr(out), FA_ACCUMULATE if acc_in is not None else 0, _stream(out))
    return out


def reduce4_plan(cus: int, K: int, P: int) -> list:
    """The launches fq4_reduce makes at (K, P) on a GPU of ``cus`` compute units (fq4_reduce_plan; no GPU needed):
    a list of dicts V, U, col0, tiles, sw, grid."""
    return _strip_plan(lambda out, cap: NQ4.call("fq4_reduce_plan", int(cus), int(K), int(P), out, cap),
                       NQ4.PLAN_FIELDS)


def quantize_row4(x: torch.Tensor, base: Optional[torch.Tensor], residual: Optional[torch.Tensor], P: int,
                  q4: torch.Tensor, scales: torch.Tensor, residual_out: Optional[torch.Tensor] = None) -> None:
    """(q4, scales[, residual_out]) <- MXFP4 of the fp32 device row x[:P] - base[:P] + residual[:P]
    (fq4_quantize_row; ``base`` and ``residual`` may be None): 16 * ceil(P / 32) code bytes, the padding codes 0,
    ceil(P / 32) scale bytes and, when given, the P floats this encoding leaves behind.  ``residual_out`` may be
    ``residual``."""
    _dev(x, torch.float32, "x", P)
    for t, name in ((base, "base"), (residual, "residual"), (residual_out, "residual_out")):
        if t is not None:
            _dev(t, torch.float32, name, P)
            if t.device != x.device:
                raise ValueError(f"{name}: on {t.device}, x on {x.device}")
    _dev(q4, torch.uint8, "q4", code_bytes(P))
    _dev(scales, torch.uint8, "scales", blocks(P), align=1)
    if q4.device != x.device or scales.device != x.device:
        raise ValueError(f"q4 / scales: on {q4.device} / {scales.device}, x on {x.device}")
    NQ4.call("fq4_quantize_row", ptr(x), ptr(base), ptr(residual), int(P), ptr(q4), ptr(scales), ptr(residual_out),
             _stream(q4))
