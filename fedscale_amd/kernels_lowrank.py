"""Typed torch-tensor wrappers over the low-rank delta-upload path's C ABI (include/fedlowrank.h), with the same
host-side checks as ``kernels_quant``: device / dtype / contiguity / size, launched on the current HIP stream of the
output's device.

Entries are described to the library by an int64 ``dims`` array [E, 2]: (O, I) for a factored entry, (numel, 0) for
a dense one (``entry_dims``, from ``lowrank_upload.factored``).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native_lowrank as NL
from ._native import FA_ACCUMULATE, ptr
from .cloud.execution.lowrank_upload import check_rank, factored, matrix_dims
from .kernels import _dev, _stream

DEPTH = NL.DEPTH  #: staged inner rows of one LDS stage of flr_reduce (a compile-time constant of the library)
HEAD_T = np.dtype([("magic", "<i4"), ("rank", "<i4"), ("r2", "<i4"), ("n_entries", "<i4"), ("n_tiles", "<i8"),
                   ("ldf", "<i8"), ("P", "<i8"), ("row_floats", "<i8"), ("reserved", "<i8", (2,))])
ENTRY_T = np.dtype([("chain_off", "<i8"), ("ut_off", "<i8"), ("v_off", "<i8"), ("O", "<i4"), ("I", "<i4"),
                    ("O4", "<i4"), ("I4", "<i4"), ("kind", "<i4"), ("tile", "<i4"), ("ntr", "<i4"), ("ntc", "<i4"),
                    ("first_tile", "<i8")])
TILE_T = np.dtype([("entry", "<i4"), ("tr", "<i4"), ("tc", "<i4"), ("kind", "<i4")])


def entry_dims(shapes, rank: int) -> np.ndarray:
    """The [E, 2] int64 ``dims`` of float32 entries of ``shapes`` at ``rank``: (O, I) when ``factored``, else
    (numel, 0)."""
    rank = check_rank(rank)
    out = np.zeros((len(shapes), 2), dtype=np.int64)
    for i, s in enumerate(shapes):
        O, I = matrix_dims(s)
        out[i] = (O, I) if factored(tuple(s), rank) else (O * I if len(s) else 1, 0)
    return out


def _dims(dims) -> np.ndarray:
    d = np.ascontiguousarray(dims, dtype=np.int64)
    if d.ndim != 2 or d.shape[1] != 2:
        raise ValueError(f"dims: expected an [E, 2] array, got {d.shape}")
    return d


def row_layout(rank: int, dims):
    """(ldf, offsets [E, 2]) of a staged row (flr_row_layout; no GPU needed): the row stride in floats and, per
    entry, where its Ut (or its dense values) and its V start."""
    d = _dims(dims)
    off = np.zeros((d.shape[0], 2), dtype=np.int64)
    ldf = int(NL.call("flr_row_layout", int(rank), d.shape[0], d.ctypes.data, off.ctypes.data))
    return ldf, off


def reduce_plan(cus: int, rank: int, dims, force_tile: int = 0):
    """(tiles, per-entry list of dicts kind, tile, tiles, first) of flr_reduce at ``cus`` compute units
    (flr_reduce_plan; no GPU needed)."""
    d = _dims(dims)
    buf = np.zeros((d.shape[0], NL.PLAN_FIELDS), dtype=np.int64)
    n = int(NL.call("flr_reduce_plan", int(cus), int(rank), d.shape[0], d.ctypes.data, int(force_tile),
                    buf.ctypes.data))
    return n, [dict(zip(("kind", "tile", "tiles", "first"), r)) for r in buf.tolist()]


def reduce_table(cus: int, rank: int, dims, force_tile: int = 0) -> np.ndarray:
    """The tile table of flr_reduce as the bytes the kernel reads (flr_reduce_table; no GPU needed)."""
    d = _dims(dims)
    need = int(NL.call("flr_reduce_table", int(cus), int(rank), d.shape[0], d.ctypes.data, int(force_tile), None, 0))
    buf = np.zeros(need, dtype=np.uint8)
    NL.call("flr_reduce_table", int(cus), int(rank), d.shape[0], d.ctypes.data, int(force_tile), buf.ctypes.data, need)
    return buf


def parse_table(buf: np.ndarray):
    """(head, entries, tiles) of a table: numpy records over ``buf``."""
    head = buf[:HEAD_T.itemsize].view(HEAD_T)[0]
    e1 = HEAD_T.itemsize + int(head["n_entries"]) * ENTRY_T.itemsize
    return head, buf[HEAD_T.itemsize:e1].view(ENTRY_T), buf[e1:].view(TILE_T)


class TileTable:
    """The tile table of one (shapes, rank, device): its host bytes, and their copy on the device."""

    _cache = {}

    def __init__(self, dims, rank: int, device, force_tile: int = 0):
        self.dims, self.rank, self.force_tile = _dims(dims), check_rank(rank), int(force_tile)
        self.device = torch.device(device)
        self.cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        self.host = reduce_table(self.cus, self.rank, self.dims, self.force_tile)
        head = parse_table(self.host)[0]
        self.ldf, self.P, self.tiles = int(head["ldf"]), int(head["P"]), int(head["n_tiles"])
        self.dev = torch.from_numpy(self.host).to(self.device)

    @classmethod
    def of(cls, dims, rank: int, device, force_tile: int = 0) -> "TileTable":
        """The cached table of (shapes, rank, CU count of the device) — built once, as heterofl's chunk lists."""
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        key = (_dims(dims).tobytes(), int(rank), idx, int(force_tile))
        t = cls._cache.get(key)
        if t is None:
            if len(cls._cache) > 32:
                cls._cache.clear()
            t = cls._cache[key] = cls(dims, rank, torch.device("cuda", idx), force_tile)
        return t


def reduce_lowrank(staged: torch.Tensor, n: int, table: TileTable, out: torch.Tensor, *,
                   acc_in: Optional[torch.Tensor] = None, row0: int = 0) -> torch.Tensor:
    """out[:P] <- the factors of the staged rows [row0, row0 + n) multiplied out and chained, dense entries added, in
    arrival order, continuing ``acc_in`` when given (flr_reduce); out may be acc_in and is written in [0, P) only."""
    _dev(out, torch.float32, "out", table.P)
    if acc_in is not None:
        _dev(acc_in, torch.float32, "acc_in", table.P)
    n, row0 = int(n), int(row0)
    if row0 < 0 or n < 0:
        raise ValueError(f"row0={row0}, n={n}")
    _dev(staged, torch.float32, "staged")
    if staged.dim() != 2 or staged.shape[1] != table.ldf or row0 + n > staged.shape[0]:
        raise ValueError(f"staged: expected a [>= {row0 + n}, {table.ldf}] buffer, got {tuple(staged.shape)}")
    if staged.device != out.device or table.dev.device != out.device:
        raise ValueError(f"staged / table: on {staged.device} / {table.dev.device}, out on {out.device}")
    NL.call("flr_reduce", ptr(staged) + row0 * table.ldf * 4, table.ldf, n, table.rank, table.dims.shape[0],
            table.dims.ctypes.data, table.force_tile, ptr(table.dev), table.host.ctypes.data, table.host.size,
            ptr(acc_in), ptr(out), FA_ACCUMULATE if acc_in is not None else 0, _stream(out))
    return out
