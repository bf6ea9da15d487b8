"""Typed torch-tensor wrappers over the block Hadamard rotation's C ABI (include/fedrotate.h), with the same host-side
checks as ``kernels_sign``: device / dtype / contiguity / size, launched on the current HIP stream of the output's
device.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _native_rotate as NR
from ._native import ptr
from .kernels import _dev, _stream

BLOCK = NR.BLOCK  #: columns of one Hadamard block
_MASK64 = (1 << 64) - 1


def padded(P: int) -> int:
    """P' = round_up(P, 4096): the columns of a rotated row (frt_padded)."""
    return int(NR.call("frt_padded", int(P)))


def check_seed(seed) -> int:
    """``seed`` as an int in [0, 2^64); TypeError / ValueError otherwise."""
    if isinstance(seed, bool) or not hasattr(seed, "__index__"):
        raise TypeError(f"seed: expected an integer in [0, 2^64), got {type(seed).__name__}")
    s = int(seed)
    if not 0 <= s <= _MASK64:
        raise ValueError(f"seed: {s} is not in [0, 2^64)")
    return s


def rotate(x: torch.Tensor, base: Optional[torch.Tensor], P: int, seed: int, y: torch.Tensor) -> torch.Tensor:
    """y[:P'] <- H D (x[:P] - base[:P]) / 64 per block of 4096 columns, the padding +0.0 before the diagonal
    (frt_rotate; ``base`` may be None).  y must not overlap x or base."""
    _dev(x, torch.float32, "x", P, align=4)
    if base is not None:
        _dev(base, torch.float32, "base", P, align=4)
        if base.device != x.device:
            raise ValueError(f"base: on {base.device}, x on {x.device}")
    _dev(y, torch.float32, "y", padded(P))
    if y.device != x.device:
        raise ValueError(f"y: on {y.device}, x on {x.device}")
    NR.call("frt_rotate", ptr(x), ptr(base), int(P), check_seed(seed), ptr(y), _stream(y))
    return y


def unrotate(y: torch.Tensor, P: int, seed: int, out: torch.Tensor) -> torch.Tensor:
    """out[:P] <- D H y[:P'] / 64 per block of 4096 columns (frt_unrotate); out may be y, and is written in [0, P)
    only."""
    _dev(y, torch.float32, "y", padded(P))
    _dev(out, torch.float32, "out", P)
    if out.device != y.device:
        raise ValueError(f"out: on {out.device}, y on {y.device}")
    NR.call("frt_unrotate", ptr(y), int(P), check_seed(seed), ptr(out), _stream(out))
    return out
