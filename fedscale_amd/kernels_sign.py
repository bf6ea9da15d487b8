"""Typed torch-tensor wrappers over the 1-bit sign delta-upload path's C ABI (include/fedsign.h), with the same
host-side checks as ``kernels_quant``: device / dtype / contiguity / size, launched on the current HIP stream of the
output's device.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _native_sign as NS
from ._native import FA_ACCUMULATE, ptr
from .kernels import _cols, _dev, _stream, _strip_plan

BLOCK = NS.BLOCK  #: columns that share one fp32 scale


def blocks(P: int) -> int:
    """Scales of a row of P columns: ceil(P / 256)."""
    return (int(P) + BLOCK - 1) // BLOCK


def bit_bytes(P: int) -> int:
    """Bytes of a row's sign bits on the wire: ceil(P / 8)."""
    return (int(P) + 7) // 8


def bit_stride(P: int) -> int:
    """ldb of a staging for P columns: round_up(ceil(P / 8), 16) bytes."""
    return (bit_bytes(P) + 15) // 16 * 16


def scale_stride(P: int) -> int:
    """lds of a staging for P columns: round_up(ceil(P / 256), 4) floats."""
    return (blocks(P) + 3) // 4 * 4


def _check_rows(bits: torch.Tensor, scales: torch.Tensor, n: int, P: int):
    for t, name, dt in ((bits, "bits", torch.uint8), (scales, "scales", torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise TypeError(f"{name}: expected a {dt} tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        _dev(t, dt, name)
        if t.dim() != 2:
            raise ValueError(f"{name}: expected a [n, stride] client-major buffer")
        if n > t.shape[0]:
            raise ValueError(f"{name}: n={n} > rows {t.shape[0]}")
    ldb, lds = bits.shape[1], scales.shape[1]
    if ldb < bit_bytes(P) or ldb % 16:
        raise ValueError(f"bits: ldb={ldb} must be >= ceil(P / 8)={bit_bytes(P)} and a multiple of 16")
    if lds < blocks(P):
        raise ValueError(f"scales: lds={lds} must be >= ceil(P / 256)={blocks(P)}")
    if scales.device != bits.device:
        raise ValueError(f"scales: on {scales.device}, bits on {bits.device}")
    return ldb, lds


def reduce_sign(bits: torch.Tensor, scales: torch.Tensor, n: int, P: int, out: torch.Tensor, *,
                acc_in: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[:P] <- the in-order fp32 chain over the dequantised rows (bits, scales)[:n, :P], continuing ``acc_in`` when
    given (fsg_reduce); out may be acc_in, and is written in [0, P) only."""
    if n > 0:
        ldb, lds = _check_rows(bits, scales, n, P)
    else:
        ldb, lds = bit_stride(P), scale_stride(P)
    _dev(out, torch.float32, "out", P)
    if acc_in is not None:
        _dev(acc_in, torch.float32, "acc_in", _cols(P))
    NS.call("fsg_reduce", ptr(bits) if n > 0 else None, ptr(scales) if n > 0 else None, ldb, lds, int(n), int(P),
            ptr(acc_in), ptr(out), FA_ACCUMULATE if acc_in is not None else 0, _stream(out))
    return out


def reduce_sign_plan(cus: int, K: int, P: int) -> list:
    """The launches fsg_reduce makes at (K, P) on a GPU of ``cus`` compute units (fsg_reduce_plan; no GPU needed):
    a list of dicts V, U, col0, tiles, sw, grid."""
    return _strip_plan(lambda out, cap: NS.call("fsg_reduce_plan", int(cus), int(K), int(P), out, cap),
                       NS.PLAN_FIELDS)


def sign_row(x: torch.Tensor, base: Optional[torch.Tensor], residual: Optional[torch.Tensor], P: int,
             bits: torch.Tensor, scales: torch.Tensor, residual_out: Optional[torch.Tensor] = None) -> None:
    """(bits, scales[, residual_out]) <- the scaled sign of the fp32 device row x[:P] - base[:P] + residual[:P]
    (fsg_sign_row; ``base`` and ``residual`` may be None): 32 * ceil(P / 256) bytes of bits, the padding bits 0,
    ceil(P / 256) scales and, when given, the P floats of what this encoding leaves behind.  ``residual_out`` may be
    ``residual``."""
    _dev(x, torch.float32, "x", P, align=4)
    for t, name in ((base, "base"), (residual, "residual"), (residual_out, "residual_out")):
        if t is not None:
            _dev(t, torch.float32, name, P, align=4)
            if t.device != x.device:
                raise ValueError(f"{name}: on {t.device}, x on {x.device}")
    _dev(bits, torch.uint8, "bits", blocks(P) * (BLOCK // 8))
    _dev(scales, torch.float32, "scales", blocks(P), align=4)
    if bits.device != x.device or scales.device != x.device:
        raise ValueError(f"bits / scales: on {bits.device} / {scales.device}, x on {x.device}")
    NS.call("fsg_sign_row", ptr(x), ptr(base), ptr(residual), int(P), ptr(bits), ptr(scales), ptr(residual_out),
            _stream(bits))
