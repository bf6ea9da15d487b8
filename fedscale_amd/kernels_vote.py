"""Typed torch-tensor wrappers over the majority-vote sign path's C ABI (include/fedvote.h), with the same host-side
checks as ``kernels_sign``: device / dtype / contiguity / size, launched on the current HIP stream of the output's
device.  Counts are uint32 on the device and ``torch.int32`` tensors here (a count is at most 2^24).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native_vote as NV
from ._native import FA_ACCUMULATE, ptr
from .kernels import _dev, _pinned, _stream

MODES = tuple(NV.MODES)  #: "majority": the sign of the vote margin; "mean": the mean of the signs
MAX_ROWS = NV.MAX_ROWS   #: rows one count_votes call takes


def bit_bytes(P: int) -> int:
    """Bytes of a row's sign bits on the wire: ceil(P / 8)."""
    return (int(P) + 7) // 8


def bit_stride(P: int) -> int:
    """ldb of a staging for P columns: round_up(ceil(P / 8), 16) bytes."""
    return (bit_bytes(P) + 15) // 16 * 16


def count_votes(bits: torch.Tensor, n: int, P: int, cnt: torch.Tensor, *, accumulate: bool = False) -> torch.Tensor:
    """cnt[:P] <- (``accumulate``: cnt[:P] +) the number of rows of bits[:n] whose bit p is set (fvt_count); exact,
    and written in [0, P) only."""
    _dev(cnt, torch.int32, "cnt", P)
    if n > 0:
        _dev(bits, torch.uint8, "bits")
        if bits.dim() != 2 or n > bits.shape[0]:
            raise ValueError(f"bits: expected a [rows >= {n}, ldb] client-major buffer, got {tuple(bits.shape)}")
        ldb = bits.shape[1]
        if ldb < bit_bytes(P) or ldb % 16:
            raise ValueError(f"bits: ldb={ldb} must be >= ceil(P / 8)={bit_bytes(P)} and a multiple of 16")
        if bits.device != cnt.device:
            raise ValueError(f"bits: on {bits.device}, cnt on {cnt.device}")
    else:
        ldb = bit_stride(P)
    NV.call("fvt_count", ptr(bits) if n > 0 else None, ldb, int(n), int(P), ptr(cnt),
            FA_ACCUMULATE if accumulate else 0, _stream(cnt))
    return cnt


def count_votes_plan(cus: int, n: int, P: int) -> list:
    """The launches fvt_count makes at (n, P) on a GPU of ``cus`` compute units (fvt_count_plan; no GPU needed): a
    list of dicts V, U, col0, tiles, sw, grid, S — S workgroups share the rows of every tile."""
    buf = np.zeros(8 * NV.PLAN_FIELDS, dtype=np.int64)
    k = int(NV.call("fvt_count_plan", int(cus), int(n), int(P), buf.ctypes.data, 8))
    rows = buf[:k * NV.PLAN_FIELDS].reshape(k, NV.PLAN_FIELDS).tolist()
    return [dict(zip(("V", "U", "col0", "tiles", "sw", "grid", "S"), r)) for r in rows]


def finish_vote(cnt: torch.Tensor, L: torch.Tensor, P: int, K: int, eta: float, out: torch.Tensor, *,
                mode: str = "majority", mirror: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[:P] (and mirror[:P]) <- L + the step of the vote margin K - 2 cnt (fvt_finish): ``eta`` times its sign
    ("majority", +0.0 on a tie) or times its mean over K ("mean")."""
    if mode not in NV.MODES:
        raise ValueError(f"mode {mode!r}: expected one of {MODES}")
    _dev(cnt, torch.int32, "cnt", P)
    _dev(L, torch.float32, "L", P)
    _dev(out, torch.float32, "out", P)
    if mirror is not None:
        if mirror.device.type == "cpu":
            _pinned(mirror, torch.float32, "mirror", P)
        else:
            _dev(mirror, torch.float32, "mirror", P)
    NV.call("fvt_finish", ptr(cnt), ptr(L), int(P), int(K), float(eta), NV.MODES[mode], ptr(out), ptr(mirror),
            _stream(out))
    return out


def vote_row(x: torch.Tensor, base: Optional[torch.Tensor], P: int, bits: torch.Tensor) -> torch.Tensor:
    """bits[:ceil(P / 8)] <- the sign bits of the fp32 device row x[:P] - base[:P] (fvt_sign_row; ``base`` may be
    None), the padding bits 0."""
    _dev(x, torch.float32, "x", P, align=4)
    if base is not None:
        _dev(base, torch.float32, "base", P, align=4)
        if base.device != x.device:
            raise ValueError(f"base: on {base.device}, x on {x.device}")
    _dev(bits, torch.uint8, "bits", bit_bytes(P), align=1)
    if bits.device != x.device:
        raise ValueError(f"bits: on {bits.device}, x on {x.device}")
    NV.call("fvt_sign_row", ptr(x), ptr(base), int(P), ptr(bits), _stream(bits))
    return bits
