"""Typed torch-tensor wrappers over Krum / Multi-Krum's C ABI (include/fedkrum.h), with the same host-side checks as
``kernels.reduce``: device / dtype / contiguity / size, launched on the current HIP stream of the output's device.
The chain over the kept rows is ``kernels_clip.reduce_clip`` (fcl_reduce) with the 0 / 1 coefficients of ``select``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native_krum as NK
from ._native import ptr
from .kernels import _check_x, _cols, _dev, _pinned, _stream


def _check_k(K: int):
    if not 1 <= K <= NK.MAX_K:
        raise ValueError(f"K={K} must satisfy 1 <= K <= {NK.MAX_K} (FK_MAX_K)")


def gram_plan(K: int, P: int) -> dict:
    """The plan of ``gram`` at (K, P) (fk_gram_plan; no GPU needed): row_tile, tiles, nsplit, split_cols, step_cols,
    last_steps.  A function of (K, P) alone."""
    buf = np.zeros(NK.PLAN_FIELDS, dtype=np.int64)
    NK.call("fk_gram_plan", int(K), int(P), buf.ctypes.data)
    names = ("row_tile", "tiles", "nsplit", "split_cols", "step_cols", "last_steps")
    return dict(zip(names, buf.tolist()))


def gram_workspace_bytes(K: int, P: int) -> int:
    """Bytes of the workspace ``gram`` needs at (K, P) (fk_gram_workspace_bytes)."""
    return int(NK.call("fk_gram_workspace_bytes", int(K), int(P)))


def gram_workspace(K: int, P: int, device) -> torch.Tensor:
    """A float64 workspace for ``gram`` at (K, P)."""
    return torch.empty(max(1, gram_workspace_bytes(K, P) // 8), dtype=torch.float64, device=device)


def gram(x: torch.Tensor, K: int, P: int, last: torch.Tensor, out: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """out[:K*K] <- the fp64 Gram matrix of x[:K, :P] - last[:P] (fk_gram); ``ws``: ``gram_workspace``."""
    _check_k(K)
    ld = _check_x(x, K, P)
    _dev(last, torch.float32, "last", _cols(P))
    _dev(out, torch.float64, "gram", K * K, align=8)
    _dev(ws, torch.float64, "workspace", 1, align=8)
    NK.call("fk_gram", ptr(x), ld, int(K), int(P), ptr(last), ptr(out), ptr(ws), ws.numel() * 8, _stream(out))
    return out


def scores(g: torch.Tensor, K: int, f: int, out: torch.Tensor) -> torch.Tensor:
    """out[:K] <- every row's Krum score from the Gram matrix ``g`` (fk_scores); 2f + 3 <= K."""
    _check_k(K)
    if f < 0 or 2 * f + 3 > K:
        raise ValueError(f"f={f} must satisfy 0 <= f and 2f + 3 <= K={K}")
    _dev(g, torch.float64, "gram", K * K, align=8)
    _dev(out, torch.float64, "score", K, align=8)
    NK.call("fk_scores", ptr(g), int(K), int(f), ptr(out), _stream(out))
    return out


def select(score: torch.Tensor, K: int, m: int, c: torch.Tensor, n_sel: torch.Tensor) -> tuple:
    """c[:K] <- 1.0 for the m best-scored rows with a finite score (ties to the earlier arrival), 0.0 for the rest;
    n_sel[0] <- how many were kept (fk_select)."""
    _check_k(K)
    if not 1 <= m <= K:
        raise ValueError(f"m={m} must satisfy 1 <= m <= K={K}")
    _dev(score, torch.float64, "score", K, align=8)
    _dev(c, torch.float32, "c", K, align=4)
    _dev(n_sel, torch.int32, "n_sel", 1, align=4)
    NK.call("fk_select", ptr(score), int(K), int(m), ptr(c), ptr(n_sel), _stream(c))
    return c, n_sel


def finish(chain: torch.Tensor, last: torch.Tensor, n_sel: torch.Tensor, P: int, out: torch.Tensor, *,
           mirror: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[:P] <- last + chain / float(n_sel[0]), or last when n_sel[0] == 0 (fk_finish; the count is read on the
    device); ``mirror``: a second copy of out, device or pinned host memory."""
    _dev(chain, torch.float32, "chain", _cols(P))
    _dev(last, torch.float32, "last", _cols(P))
    _dev(n_sel, torch.int32, "n_sel", 1, align=4)
    _dev(out, torch.float32, "out", P)
    if mirror is not None:
        if mirror.device.type == "cpu":
            _pinned(mirror, torch.float32, "mirror", P)
        else:
            _dev(mirror, torch.float32, "mirror", P)
    NK.call("fk_finish", ptr(chain), ptr(last), ptr(n_sel), int(P), ptr(out), ptr(mirror), _stream(out))
    return out
