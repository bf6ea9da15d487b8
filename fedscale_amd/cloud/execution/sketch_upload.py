"""Executor side of the Count-Sketch upload path (FetchSGD): ``compress_sketch(state, base, spec)``.

With ``TorchModelAdapter(upload_sketch=SketchSpec(...))`` on the aggregator, the executor sends a Count Sketch of its
UPDATE ``e = x - L`` — against ``L``, the weights it was sent for this round — instead of its state: ``rows x cols``
float32 whatever the model's size, 5.2 MB instead of 100 MB for a 25 M model at 5 x 2^18::

    from fedscale_amd.cloud.execution.sketch_upload import SketchSpec, compress_sketch
    results["update_weight"] = compress_sketch(model.state_dict(), weights_received_for_this_round, spec)

The executor keeps NO state between rounds: momentum and error feedback live on the server, in sketch space.  That is
what this rung is for — clients that take part once in a thousand rounds; an executor that can keep a residual
recovers more per byte with ``compress_topk``.  include/fedsketch.h states the contract (a blocked Count Sketch: a
bucket takes exactly one column of each block of ``cols`` columns and adds them in block order, so the table is a
pure function of the update and the seed); this module restates it in numpy for a state on the host and goes through
``fcs_sketch_row`` for a state on a GPU.  Both give the same bytes.

Wire format: a plain dict in the state's order holding the entries that are NOT float32 (int64 counters) unchanged,
plus ``SKETCH_KEY`` (float32 [rows, cols]).  float32 entries do not appear.  (A list upload carries the non-float32
entries in order, then the table.)
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Union

import numpy as np
import torch

from .quant_upload import _base_values, _host, _is_f32

SKETCH_KEY = "__sketch_table__"
ROWS = (1, 3, 5, 7)
LOG2_COLS = (10, 24)
_G = 0xD1B54A32D192ED03
_M64 = (1 << 64) - 1


@dataclasses.dataclass(frozen=True)
class SketchSpec:
    """What the executors and the aggregator of a sketched round agree on.  ``rows`` in {1, 3, 5, 7}; ``cols`` a power
    of two in [2^10, 2^24], or None for the largest one with ``rows * cols <= P / compression`` (at least 1024);
    ``k``: the columns a round applies, a density in (0, 1] (a float) or a count (an int >= 1); ``momentum``: the
    server's rho in [0, 1); ``seed``: 64 bits, shared by every client and every round."""

    rows: int = 5
    cols: Optional[int] = None
    compression: float = 20
    k: Union[float, int] = 0.01
    momentum: float = 0.9
    seed: int = 0

    def __post_init__(self):
        if isinstance(self.rows, bool) or self.rows not in ROWS:
            raise ValueError(f"upload_sketch rows={self.rows!r}: expected one of {ROWS}")
        c = self.cols
        if c is not None and (isinstance(c, bool) or not isinstance(c, int) or c & (c - 1) or
                              not 1 << LOG2_COLS[0] <= c <= 1 << LOG2_COLS[1]):
            raise ValueError(f"upload_sketch cols={c!r}: expected a power of two in [2^{LOG2_COLS[0]}, "
                             f"2^{LOG2_COLS[1]}], or None")
        if isinstance(self.compression, bool) or not float(self.compression) >= 1.0:
            raise ValueError(f"upload_sketch compression={self.compression!r}: expected a ratio >= 1")
        k = self.k
        if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)):
            raise ValueError(f"upload_sketch k={k!r}: expected a density in (0, 1] or a count >= 1")
        if isinstance(k, (int, np.integer)):
            if k < 1:
                raise ValueError(f"upload_sketch k={k!r}: expected a density in (0, 1] or a count >= 1")
        elif not 0.0 < float(k) <= 1.0:
            raise ValueError(f"upload_sketch k={k!r}: expected a density in (0, 1] or a count >= 1")
        if isinstance(self.momentum, bool) or not 0.0 <= float(self.momentum) < 1.0:
            raise ValueError(f"upload_sketch momentum={self.momentum!r}: expected rho in [0, 1)")
        if isinstance(self.seed, bool) or not isinstance(self.seed, (int, np.integer)) or not 0 <= self.seed <= _M64:
            raise ValueError(f"upload_sketch seed={self.seed!r}: expected an integer of 64 bits")

    @classmethod
    def of(cls, spec) -> "SketchSpec":
        if spec is True:
            return cls()
        if not isinstance(spec, cls):
            raise TypeError(f"upload_sketch: expected a SketchSpec (or True for its defaults), got "
                            f"{type(spec).__name__}")
        return spec

    def cols_for(self, P: int) -> int:
        """C at a bucket of P columns."""
        if self.cols is not None:
            return self.cols
        c = LOG2_COLS[0]
        while c < LOG2_COLS[1] and self.rows * (2 << c) * float(self.compression) <= int(P):
            c += 1
        return 1 << c

    def count(self, P: int) -> int:
        """The columns a round applies at a bucket of P columns: at most P."""
        P = int(P)
        if isinstance(self.k, (int, np.integer)):
            return min(P, int(self.k))
        return min(P, max(1, int(math.ceil(float(self.k) * P))))


def mix(s, w):
    """The splitmix64 of include/fedrotate.h over uint64 arrays (or ints), mod 2^64."""
    with np.errstate(over="ignore"):
        z = np.uint64(s) + (np.asarray(w, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sign_words(seed: int, j: int, n_words: int) -> np.ndarray:
    """The sign words of row j for the columns [0, 64 * n_words)."""
    return mix((int(seed) + (2 * j + 1) * _G) & _M64, np.arange(n_words, dtype=np.uint64))


def block_masks(seed: int, j: int, n_blocks: int, C: int) -> np.ndarray:
    """The bucket masks of row j for the blocks [0, n_blocks), int64."""
    m = mix((int(seed) + (2 * j + 2) * _G) & _M64, np.arange(n_blocks, dtype=np.uint64))
    return (m & np.uint64(C - 1)).astype(np.int64)


def _signed(e: np.ndarray, seed: int, j: int) -> np.ndarray:
    """e with row j's sign bits xored in."""
    P = e.size
    w = sign_words(seed, j, (P + 63) // 64)
    p = np.arange(P, dtype=np.uint64)
    bit = ((w[(p >> np.uint64(6)).astype(np.int64)] >> (p & np.uint64(63))) & np.uint64(1)).astype(np.uint32)
    return (e.view(np.uint32) ^ (bit << np.uint32(31))).view(np.float32)


def sketch_host(e: np.ndarray, R: int, C: int, seed: int) -> np.ndarray:
    """The float32 [R, C] table of the float32 vector ``e`` (include/fedsketch.h): per row, the blocks added in
    ascending order — a vector add per block, every bucket taking that block's one column."""
    e = np.ascontiguousarray(e, dtype=np.float32)
    P = e.size
    NB = (P + C - 1) // C
    T = np.zeros((R, C), dtype=np.float32)
    u = np.arange(C, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(R):
            t = _signed(e, seed, j)
            m = block_masks(seed, j, NB, C)
            for b in range(NB):
                n = min(C, P - b * C)
                q = u[:n] ^ m[b]
                T[j, q] = T[j, q] + t[b * C:b * C + n]
    return T


def compress_sketch(state, base, spec: SketchSpec) -> dict:
    """name -> array, in ``state``'s order, plus ``SKETCH_KEY``: the Count Sketch of ``state - base`` over the float32
    entries, the rest as they are (numpy arrays).  ``base``: the weights this round started from, a dict with the
    state's keys or a list in its order.  A state whose float32 tensors are on a GPU is sketched there
    (fcs_sketch_row) and the table crosses to the host in one copy.  Both paths give the same bytes."""
    spec = SketchSpec.of(spec)
    items = list(state.items())
    bvals = _base_values(items, base)
    f_idx = [i for i, (_, v) in enumerate(items) if _is_f32(v)]
    for i in f_idx:
        name, v = items[i]
        b = bvals[i]
        if tuple(b.shape) != tuple(v.shape):
            raise ValueError(f"{name}: base shape {tuple(b.shape)} != state shape {tuple(v.shape)}")
        if not _is_f32(b):
            raise TypeError(f"{name}: base dtype {b.dtype}, the state's entry is float32")
    sizes = [int(np.prod(items[i][1].shape)) if len(items[i][1].shape) else 1 for i in f_idx]
    P = int(sum(sizes))
    if P > 0x7FFFFFFF:
        raise ValueError(f"a bucket of {P} columns: a sketch takes at most 2^31 - 1")
    R, C = spec.rows, spec.cols_for(P)
    on_gpu = [i for i in f_idx if isinstance(items[i][1], torch.Tensor) and items[i][1].is_cuda]
    if not on_gpu or P == 0:
        x = np.empty(P, dtype=np.float32)
        L = np.empty(P, dtype=np.float32)
        o = 0
        for i, n in zip(f_idx, sizes):
            x[o:o + n] = np.asarray(_host(items[i][1])).reshape(-1)
            L[o:o + n] = np.asarray(_host(bvals[i])).reshape(-1)
            o += n
        with np.errstate(invalid="ignore", over="ignore"):
            table = sketch_host(x - L, R, C, spec.seed)
    else:
        from ... import kernels_sketch as kk

        dev = items[on_gpu[0]][1].device
        with torch.cuda.device(dev):
            x = torch.cat([torch.as_tensor(items[i][1]).detach().to(dev).reshape(-1) for i in f_idx])
            L = torch.cat([torch.as_tensor(bvals[i]).detach().to(dev).reshape(-1) for i in f_idx])
            t = torch.empty(R * C, dtype=torch.float32, device=dev)
            kk.sketch_row(x, L, None, P, R, C, spec.seed, t)
            table = t.cpu().numpy().reshape(R, C)  # one D2H (synchronises with the launch)
    out = {}  # a plain dict, in the state's order
    f_set = set(f_idx)
    for i, (name, v) in enumerate(items):
        if i not in f_set:
            out[name] = _host(v)
    if SKETCH_KEY in out:
        raise ValueError(f"the state has an entry named {SKETCH_KEY!r}")
    out[SKETCH_KEY] = table
    return out
