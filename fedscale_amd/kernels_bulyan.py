"""Typed torch-tensor wrappers over Bulyan's C ABI (include/fedbulyan.h), with the same host-side checks as
``kernels.reduce``: device / dtype / contiguity / size, launched on the current HIP stream of the output's device.
The Gram matrix the selection reads is ``kernels_krum.gram`` (fk_gram), unchanged.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native_bulyan as NB
from . import _native_krum as NK
from ._native import ptr
from .kernels import _check_x, _cols, _dev, _pinned, _stream


def counts(K: int, f: int) -> tuple:
    """(theta, beta) = (K - 2f - 2, K - 4f - 2) of a round of K uploads with f assumed bad; ValueError outside
    0 <= f, 4f + 3 <= K <= FK_MAX_K."""
    if f < 0 or 4 * f + 3 > K:
        raise ValueError(f"f={f} bad uploads need 0 <= f and 4f + 3 <= K, K={K} is too few")
    if K > NK.MAX_K:
        raise ValueError(f"K={K} exceeds the limit FK_MAX_K = {NK.MAX_K}")
    return K - 2 * f - 2, K - 4 * f - 2


def select_workspace_bytes(K: int) -> int:
    """Bytes of the workspace ``select`` needs at K (fbl_select_workspace_bytes)."""
    return int(NB.call("fbl_select_workspace_bytes", int(K)))


def select_workspace(K: int, device) -> torch.Tensor:
    """A float64 workspace for ``select`` at K."""
    return torch.empty((select_workspace_bytes(K) + 7) // 8, dtype=torch.float64, device=device)


def select(g: torch.Tensor, K: int, f: int, picks: torch.Tensor, sel: torch.Tensor, n_sel: torch.Tensor,
           ws: torch.Tensor) -> tuple:
    """picks[:theta] <- the rows Krum picks in theta = K - 2f - 2 iterations, each winner removed, in selection
    order; sel[:theta] <- the same rows in arrival order; n_sel[0] <- how many were picked (-1 fills both from there
    on when the finite scores run out) (fbl_select, from the Gram matrix ``g``); ``ws``: ``select_workspace``."""
    theta, _ = counts(K, f)
    _dev(g, torch.float64, "gram", K * K, align=8)
    _dev(picks, torch.int32, "picks", theta, align=4)
    _dev(sel, torch.int32, "sel", theta, align=4)
    _dev(n_sel, torch.int32, "n_sel", 1, align=4)
    _dev(ws, torch.float64, "workspace", 1, align=8)
    NB.call("fbl_select", ptr(g), int(K), int(f), ptr(picks), ptr(sel), ptr(n_sel), ptr(ws), ws.numel() * 8,
            _stream(picks))
    return picks, sel, n_sel


def reduce_bulyan(x: torch.Tensor, K: int, P: int, sel: torch.Tensor, n_sel: torch.Tensor, theta: int, beta: int,
                  last: torch.Tensor, out: torch.Tensor, *, mirror: Optional[torch.Tensor] = None,
                  kept: Optional[torch.Tensor] = None, cus: int = 0) -> torch.Tensor:
    """out[:P] <- per column the mean of the beta values of the rows x[sel[:theta], :P] closest to their (lower)
    median, or last[:P] when n_sel[0] != theta (fbl_reduce; the count is read on the device).  ``mirror``: a second
    copy of out, device or pinned host memory; ``kept``: an int64 [K] device table the per-row kept counts are added
    to; ``cus``: plan the launch for this many compute units instead of the device's (the result's bits do not depend
    on it)."""
    ld = _check_x(x, K, P)
    if not 1 <= beta <= theta <= K <= NK.MAX_K:
        raise ValueError(f"beta={beta}, theta={theta} must satisfy 1 <= beta <= theta <= K={K} <= {NK.MAX_K}")
    _dev(sel, torch.int32, "sel", theta, align=4)
    _dev(n_sel, torch.int32, "n_sel", 1, align=4)
    _dev(last, torch.float32, "last", _cols(P))
    _dev(out, torch.float32, "out", P)
    if mirror is not None:
        if mirror.device.type == "cpu":
            _pinned(mirror, torch.float32, "mirror", P)
        else:
            _dev(mirror, torch.float32, "mirror", P)
    if kept is not None:
        _dev(kept, torch.int64, "kept", K, align=8)
    NB.call("fbl_reduce", ptr(x), ld, int(K), int(P), ptr(sel), ptr(n_sel), int(theta), int(beta), ptr(last),
            ptr(out), ptr(mirror), ptr(kept), int(cus), _stream(out))
    return out


def plan(cus: int, theta: int, P: int) -> dict:
    """The launch fbl_reduce makes at (theta, P) on a GPU of ``cus`` compute units (fbl_plan; no GPU needed): lanes
    (per column), rows (per lane), W (the columns of a tile), passes (over a tile), lds (bytes), tiles, grid."""
    buf = np.zeros(NB.PLAN_FIELDS, dtype=np.int64)
    NB.call("fbl_plan", int(cus), int(theta), int(P), buf.ctypes.data)
    return dict(zip(("lanes", "rows", "W", "passes", "lds", "tiles", "grid"), buf.tolist()))
