"""Typed torch-tensor wrappers over the trimmed mean's C ABI (include/fedtrim.h), with the same host-side checks as
``kernels.reduce``: device / dtype / contiguity / size, launched on the current HIP stream of the output's device.
The order keys are unsigned 32-bit words; torch carries them as ``int32`` tensors (the same bits).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native_trim as NT
from ._native import ptr
from .kernels import _check_x, _cols, _dev, _pinned, _stream


def max_trim() -> int:
    """The largest trim count per side the kernels take (ft_max_trim)."""
    return int(NT.call("ft_max_trim"))


def _check_t(K: int, t: int, least: int = 0):
    if t < least or 2 * t >= K or t > NT.MAX_TRIM:
        raise ValueError(f"t={t} must satisfy {least} <= t, 2t < K={K} and t <= {NT.MAX_TRIM} (ft_max_trim)")


def thresholds(P: int, device) -> tuple:
    """(lo, hi, ties): three int32 device vectors of round_up(P, 4) words for ``select`` / ``reduce_trim``."""
    return tuple(torch.empty(_cols(P), dtype=torch.int32, device=device) for _ in range(3))


def select(x: torch.Tensor, K: int, P: int, t: int, lo: torch.Tensor, hi: torch.Tensor,
           ties: torch.Tensor) -> tuple:
    """lo[:P], hi[:P], ties[:P] <- the t-th smallest and largest order key of every column of x[:K, :P] and the
    dropped ties at each (ft_select)."""
    ld = _check_x(x, K, P)
    _check_t(K, t, 1)
    for name, v in (("lo", lo), ("hi", hi), ("ties", ties)):
        _dev(v, torch.int32, name, P)
    NT.call("ft_select", ptr(x), ld, int(K), int(P), int(t), ptr(lo), ptr(hi), ptr(ties), _stream(lo))
    return lo, hi, ties


def reduce_trim(x: torch.Tensor, K: int, P: int, t: int, out: torch.Tensor, *, lo: Optional[torch.Tensor] = None,
                hi: Optional[torch.Tensor] = None, ties: Optional[torch.Tensor] = None,
                mirror: Optional[torch.Tensor] = None, dropped: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[:P] <- the trimmed mean of x[:K, :P] under ``select``'s thresholds (ft_reduce); t == 0 takes none.
    ``mirror``: a second copy of out, device or pinned host memory; ``dropped``: an int64 [K, 2] device table the
    per-row (low, high) drop counts are added to."""
    ld = _check_x(x, K, P)
    _check_t(K, t)
    _dev(out, torch.float32, "out", P)
    given = [v is not None for v in (lo, hi, ties)]
    if t == 0 and any(given):
        raise ValueError("reduce_trim: t=0 takes no thresholds")
    if t > 0:
        if not all(given):
            raise ValueError("reduce_trim: t > 0 needs lo, hi and ties (select)")
        for name, v in (("lo", lo), ("hi", hi), ("ties", ties)):
            _dev(v, torch.int32, name, _cols(P))
    if mirror is not None:
        if mirror.device.type == "cpu":
            _pinned(mirror, torch.float32, "mirror", P)
        else:
            _dev(mirror, torch.float32, "mirror", P)
    if dropped is not None:
        _dev(dropped, torch.int64, "dropped", 2 * K, align=8)
    NT.call("ft_reduce", ptr(x), ld, int(K), int(P), int(t), ptr(lo), ptr(hi), ptr(ties), ptr(out), ptr(mirror),
            ptr(dropped), _stream(out))
    return out


def plan(cus: int, K: int, P: int, t: int) -> list:
    """The launches ft_select and then ft_reduce make at (K, P, t) on a GPU of ``cus`` compute units (ft_plan; no GPU
    needed): a list of dicts kernel ("select" / "reduce"), T, V, U, col0, tiles, grid."""
    buf = np.zeros(8 * NT.PLAN_FIELDS, dtype=np.int64)
    n = int(NT.call("ft_plan", int(cus), int(K), int(P), int(t), buf.ctypes.data, 8))
    rows = buf[:n * NT.PLAN_FIELDS].reshape(n, NT.PLAN_FIELDS).tolist()
    names = {NT.KERNEL_SELECT: "select", NT.KERNEL_REDUCE: "reduce"}
    return [dict(kernel=names[r[0]], T=r[1], V=r[2], U=r[3], col0=r[4], tiles=r[5], grid=r[6]) for r in rows]
