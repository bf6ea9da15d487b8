"""Typed torch-tensor wrappers over the top-k sparse delta-upload path's C ABI (include/fedsparse.h), with the same
host-side checks as ``kernels_quant``: device / dtype / contiguity / size, launched on the current HIP stream of the
output's device.

Index arrays hold uint32 values; on the device they are ``torch.int32`` tensors with the same bits (every index is
below P <= 2^31 - 1, so the two readings agree).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native_sparse as NS
from ._native import FA_ACCUMULATE, ptr
from .kernels import _cols, _dev, _stream

TILE = NS.TILE  #: columns of one tile of fs_reduce (a compile-time constant of the library)
IDX_T = torch.int32
CHECK_ROWS_MAX = 65535  #: rows one fs_check_rows call takes (a row is a workgroup row of its grid)


def boundaries(P: int) -> int:
    """Tile boundaries of a row of P columns: ceil(P / TILE) + 1."""
    return (int(P) + TILE - 1) // TILE + 1


def row_stride(kmax: int) -> int:
    """``ldk`` of a staging whose rows hold up to ``kmax`` pairs: a multiple of 4 (16-byte rows), at least 4."""
    return max(4, (int(kmax) + 3) // 4 * 4)


def _rows(idx: torch.Tensor, nnz: torch.Tensor, n: int, val: Optional[torch.Tensor] = None) -> int:
    _dev(idx, IDX_T, "idx")
    if idx.dim() != 2:
        raise ValueError("idx: expected a [n, ldk] client-major buffer")
    ldk = idx.shape[1]
    if ldk % 4:
        raise ValueError(f"idx: ldk={ldk} must be a multiple of 4")
    if n > idx.shape[0]:
        raise ValueError(f"idx: n={n} > rows {idx.shape[0]}")
    _dev(nnz, torch.int32, "nnz", n, align=4)
    if nnz.device != idx.device:
        raise ValueError(f"nnz: on {nnz.device}, idx on {idx.device}")
    if val is not None:
        _dev(val, torch.float32, "val")
        if val.dim() != 2 or val.shape[1] != ldk or n > val.shape[0]:
            raise ValueError(f"val: expected a [>= {n}, {ldk}] buffer like idx, got {tuple(val.shape)}")
        if val.device != idx.device:
            raise ValueError(f"val: on {val.device}, idx on {idx.device}")
    return ldk


def _offsets(offsets: torch.Tensor, n: int, P: int, device) -> int:
    _dev(offsets, torch.int32, "offsets", align=4)
    if offsets.dim() != 2 or offsets.shape[0] < boundaries(P) or offsets.shape[1] < n:
        raise ValueError(f"offsets: expected a [>= {boundaries(P)}, >= {n}] buffer, got {tuple(offsets.shape)}")
    if offsets.device != device:
        raise ValueError(f"offsets: on {offsets.device}, the rows on {device}")
    return offsets.shape[1]


def row_offsets(idx: torch.Tensor, nnz: torch.Tensor, n: int, P: int, offsets: torch.Tensor,
                row0: int = 0) -> torch.Tensor:
    """offsets[b, k] <- the position in row k of the first index >= b * TILE, for every boundary b and the rows
    row0 <= k < row0 + n (fs_row_offsets); ``offsets`` is an int32 [>= boundaries(P), >= row0 + n] buffer."""
    row0 = int(row0)
    if row0 < 0:
        raise ValueError(f"row0={row0}")
    ldk = _rows(idx, nnz, row0 + n)
    ldo = _offsets(offsets, row0 + n, P, idx.device)
    NS.call("fs_row_offsets", ptr(idx) + row0 * ldk * 4, ldk, ptr(nnz) + row0 * 4, int(n), int(P),
            ptr(offsets) + row0 * 4, ldo, _stream(offsets))
    return offsets


def check_rows(idx: torch.Tensor, nnz: torch.Tensor, n: int, P: int, flags: torch.Tensor,
               row0: int = 0) -> torch.Tensor:
    """flags[k] <- non-zero when row k (row0 <= k < row0 + n) is not strictly increasing, names a column >= P or has
    a count outside [0, ldk]; 0 otherwise (fs_check_rows)."""
    row0 = int(row0)
    if row0 < 0:
        raise ValueError(f"row0={row0}")
    ldk = _rows(idx, nnz, row0 + n)
    _dev(flags, torch.int32, "flags", row0 + n, align=4)
    if flags.device != idx.device:
        raise ValueError(f"flags: on {flags.device}, idx on {idx.device}")
    NS.call("fs_check_rows", ptr(idx) + row0 * ldk * 4, ldk, ptr(nnz) + row0 * 4, int(n), int(P),
            ptr(flags) + row0 * 4, _stream(flags))
    return flags


def reduce_sparse(idx: torch.Tensor, val: torch.Tensor, nnz: torch.Tensor, offsets: torch.Tensor,
                  flags: torch.Tensor, n: int, P: int, out: torch.Tensor, *,
                  acc_in: Optional[torch.Tensor] = None, row0: int = 0) -> torch.Tensor:
    """out[:P] <- the in-order fp32 chain over the staged sparse rows [row0, row0 + n), continuing ``acc_in`` when
    given (fs_reduce); rows whose flag is non-zero are skipped; out may be acc_in, and is written in [0, P) only."""
    _dev(out, torch.float32, "out", P)
    if acc_in is not None:
        _dev(acc_in, torch.float32, "acc_in", _cols(P))
    row0 = int(row0)
    if row0 < 0:
        raise ValueError(f"row0={row0}")
    if n > 0:
        ldk = _rows(idx, nnz, row0 + n, val)
        ldo = _offsets(offsets, row0 + n, P, idx.device)
        _dev(flags, torch.int32, "flags", row0 + n, align=4)
        if flags.device != idx.device or out.device != idx.device:
            raise ValueError(f"flags / out: on {flags.device} / {out.device}, idx on {idx.device}")
        NS.call("fs_reduce", ptr(idx) + row0 * ldk * 4, ptr(val) + row0 * ldk * 4, ldk, ptr(nnz) + row0 * 4,
                ptr(offsets) + row0 * 4, ldo, ptr(flags) + row0 * 4, int(n), int(P), ptr(acc_in), ptr(out),
                FA_ACCUMULATE if acc_in is not None else 0, _stream(out))
    else:
        NS.call("fs_reduce", None, None, 0, None, None, 0, None, 0, int(P), ptr(acc_in), ptr(out),
                FA_ACCUMULATE if acc_in is not None else 0, _stream(out))
    return out


def reduce_sparse_plan(cus: int, K: int, P: int) -> list:
    """The launches fs_reduce makes at (K, P) on a GPU of ``cus`` compute units (fs_reduce_plan; no GPU needed):
    a list of dicts tile, U, col0, tiles, per, grid."""
    buf = np.zeros(8 * NS.PLAN_FIELDS, dtype=np.int64)
    n = int(NS.call("fs_reduce_plan", int(cus), int(K), int(P), buf.ctypes.data, 8))
    rows = buf[:n * NS.PLAN_FIELDS].reshape(n, NS.PLAN_FIELDS).tolist()
    return [dict(zip(("tile", "U", "col0", "tiles", "per", "grid"), r)) for r in rows]


def topk_workspace(P: int) -> int:
    """Bytes of fs_topk_row's workspace at P columns (fs_topk_workspace; no GPU needed)."""
    return int(NS.call("fs_topk_workspace", int(P)))


def topk_row(x: torch.Tensor, base: Optional[torch.Tensor], r_in: Optional[torch.Tensor], P: int, k: int,
             workspace: torch.Tensor, idx_out: torch.Tensor, val_out: torch.Tensor,
             r_out: Optional[torch.Tensor] = None) -> int:
    """(idx_out, val_out)[:min(k, P)] <- the top-k selection of the fp32 device row x[:P] - base[:P] (+ r_in[:P]),
    in increasing index order; r_out[:P] <- what was dropped (fs_topk_row).  Returns min(k, P)."""
    P, k = int(P), int(k)
    if k < 1:
        raise ValueError(f"k={k}: a selection keeps at least one column")
    kk = min(k, P)
    _dev(x, torch.float32, "x", P)
    for t, name in ((base, "base"), (r_in, "r_in"), (r_out, "r_out")):
        if t is not None:
            _dev(t, torch.float32, name, P)
            if t.device != x.device:
                raise ValueError(f"{name}: on {t.device}, x on {x.device}")
    _dev(workspace, torch.uint8, "workspace", topk_workspace(P))
    _dev(idx_out, IDX_T, "idx_out", kk)
    _dev(val_out, torch.float32, "val_out", kk)
    if workspace.device != x.device or idx_out.device != x.device or val_out.device != x.device:
        raise ValueError(f"workspace / idx_out / val_out: not all on {x.device}")
    NS.call("fs_topk_row", ptr(x), ptr(base), ptr(r_in), P, k, ptr(workspace), ptr(idx_out), ptr(val_out),
            ptr(r_out), _stream(idx_out))
    return kk
