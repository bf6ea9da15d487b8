"""Typed torch-tensor wrappers over the MXFP8 delta-upload path's C ABI (include/fedquant.h), with the same host-side
checks as ``kernels_half``: device / dtype / contiguity / size, launched on the current HIP stream of the output's
device.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _native_quant as NQ
from ._native import FA_ACCUMULATE, ptr
from .kernels import _cols, _dev, _stream, _strip_plan

BLOCK = NQ.BLOCK  #: columns that share one scale byte


def blocks(P: int) -> int:
    """Scale bytes of a row of P columns: ceil(P / 32)."""
    return (int(P) + BLOCK - 1) // BLOCK


def _check_rows(q8: torch.Tensor, scales: torch.Tensor, n: int, P: int):
    for t, name in ((q8, "q8"), (scales, "scales")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise TypeError(f"{name}: expected a torch.uint8 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        _dev(t, torch.uint8, name)
        if t.dim() != 2:
            raise ValueError(f"{name}: expected a [n, stride] client-major buffer")
        if n > t.shape[0]:
            raise ValueError(f"{name}: n={n} > rows {t.shape[0]}")
    ld, lds = q8.shape[1], scales.shape[1]
    if ld < P or ld % 64:
        raise ValueError(f"q8: ld={ld} must be >= P={P} and a multiple of 64")
    if lds < blocks(P):
        raise ValueError(f"scales: lds={lds} must be >= ceil(P / 32)={blocks(P)}")
    if scales.device != q8.device:
        raise ValueError(f"scales: on {scales.device}, q8 on {q8.device}")
    return ld, lds


def reduce8(q8: torch.Tensor, scales: torch.Tensor, n: int, P: int, out: torch.Tensor, *,
            acc_in: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[:P] <- the in-order fp32 chain over the dequantised rows (q8, scales)[:n, :P], continuing ``acc_in`` when
    given (fq_reduce); out may be acc_in, and is written in [0, P) only."""
    if n > 0:
        ld, lds = _check_rows(q8, scales, n, P)
    else:
        ld, lds = (P + 63) // 64 * 64, blocks(P)
    _dev(out, torch.float32, "out", P)
    if acc_in is not None:
        _dev(acc_in, torch.float32, "acc_in", _cols(P))
    NQ.call("fq_reduce", ptr(q8) if n > 0 else None, ptr(scales) if n > 0 else None, ld, lds, int(n), int(P),
            ptr(acc_in), ptr(out), FA_ACCUMULATE if acc_in is not None else 0, _stream(out))
    return out


def reduce8_plan(cus: int, K: int, P: int) -> list:
    """The launches fq_reduce makes at (K, P) on a GPU of ``cus`` compute units (fq_reduce_plan; no GPU needed):
    a list of dicts V, U, col0, tiles, sw, grid."""
    return _strip_plan(lambda out, cap: NQ.call("fq_reduce_plan", int(cus), int(K), int(P), out, cap),
                       NQ.PLAN_FIELDS)


def quantize_row(x: torch.Tensor, base: Optional[torch.Tensor], P: int, q8: torch.Tensor,
                 scales: torch.Tensor) -> None:
    """(q8, scales) <- MXFP8 of the fp32 device row x[:P] - base[:P] (of x[:P] when ``base`` is None)
    (fq_quantize_row): round_up(P, 32) codes, the padding codes 0, and ceil(P / 32) scale bytes."""
    _dev(x, torch.float32, "x", P)
    if base is not None:
        _dev(base, torch.float32, "base", P)
        if base.device != x.device:
            raise ValueError(f"base: on {base.device}, x on {x.device}")
    _dev(q8, torch.uint8, "q8", blocks(P) * BLOCK)
    _dev(scales, torch.uint8, "scales", blocks(P), align=1)
    if q8.device != x.device or scales.device != x.device:
        raise ValueError(f"q8 / scales: on {q8.device} / {scales.device}, x on {x.device}")
    NQ.call("fq_quantize_row", ptr(x), ptr(base), int(P), ptr(q8), ptr(scales), _stream(q8))
