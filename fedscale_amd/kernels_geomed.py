"""Typed torch-tensor wrappers over geometric-median aggregation's C ABI (include/fedgeomed.h), with the same host-side
checks as ``kernels.reduce``: device / dtype / contiguity / size, launched on the current HIP stream of the output's
device.  The Gram is ``kernels_krum.gram`` (fk_gram), the streamed distances ``kernels_clip.row_sqnorms``
(fcl_row_sqnorms) and the chain ``kernels_clip.reduce_clip`` (fcl_reduce) with the fp32 weights of ``start`` /
``weights``.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _native_geomed as NG
from ._native import ptr
from .kernels import _cols, _dev, _pinned, _stream


def _check_k(K: int):
    if not 1 <= K <= NG.MAX_K:
        raise ValueError(f"K={K} must satisfy 1 <= K <= {NG.MAX_K} (FGM_MAX_K)")


def _check_wcn(K: int, w: torch.Tensor, c: torch.Tensor, n_valid: torch.Tensor):
    _dev(w, torch.float64, "w", K, align=8)
    _dev(c, torch.float32, "c", K, align=4)
    _dev(n_valid, torch.int32, "n_valid", 1, align=4)


def start(q0: torch.Tensor, K: int, w: torch.Tensor, c: torch.Tensor, n_valid: torch.Tensor, *,
          stride: int = 1) -> tuple:
    """w[:K], c[:K], n_valid[0] <- the start weights of the squared update norms q0[k * stride] (fgm_start): the mean
    of the updates clipped to the median norm.  ``stride`` K + 1 reads the diagonal of a K x K Gram."""
    _check_k(K)
    if stride < 1:
        raise ValueError(f"stride={stride} must be >= 1")
    _dev(q0, torch.float64, "q0", (K - 1) * stride + 1, align=8)
    _check_wcn(K, w, c, n_valid)
    NG.call("fgm_start", ptr(q0), int(stride), int(K), ptr(w), ptr(c), ptr(n_valid), _stream(w))
    return w, c, n_valid


def weights(q: torch.Tensor, K: int, nu: float, w: torch.Tensor, c: torch.Tensor, obj: torch.Tensor,
            n_valid: torch.Tensor) -> tuple:
    """w[:K], c[:K] <- the normalised inverse distances 1 / max(sqrt(q), nu); obj[0] <- the sum of the distances;
    n_valid[0] <- the rows with a finite q (fgm_weights)."""
    _check_k(K)
    nu = float(nu)
    if not (math.isfinite(nu) and nu > 0):
        raise ValueError(f"nu={nu!r} must be finite and > 0")
    _dev(q, torch.float64, "q", K, align=8)
    _check_wcn(K, w, c, n_valid)
    _dev(obj, torch.float64, "obj", 1, align=8)
    NG.call("fgm_weights", ptr(q), int(K), nu, ptr(w), ptr(c), ptr(obj), ptr(n_valid), _stream(w))
    return w, c, n_valid


def dist2_workspace_bytes(K: int) -> int:
    """Bytes of the workspace ``gram_dist2`` needs at K (fgm_dist2_workspace_bytes)."""
    return int(NG.call("fgm_dist2_workspace_bytes", int(K)))


def dist2_workspace(K: int, device) -> torch.Tensor:
    """A float64 workspace for ``gram_dist2`` at K."""
    return torch.empty(dist2_workspace_bytes(K) // 8, dtype=torch.float64, device=device)


def gram_dist2(g: torch.Tensor, K: int, w: torch.Tensor, q: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """q[:K] <- the squared distance of every update to sum_k w[k] d_k, from the Gram matrix ``g`` of the updates
    (fgm_gram_dist2); ``ws``: ``dist2_workspace``."""
    _check_k(K)
    _dev(g, torch.float64, "gram", K * K, align=8)
    _dev(w, torch.float64, "w", K, align=8)
    _dev(q, torch.float64, "q", K, align=8)
    _dev(ws, torch.float64, "workspace", 1, align=8)
    NG.call("fgm_gram_dist2", ptr(g), int(K), ptr(w), ptr(q), ptr(ws), ws.numel() * 8, _stream(q))
    return q


def finish(chain: torch.Tensor, last: torch.Tensor, n_valid: torch.Tensor, P: int, out: torch.Tensor, *,
           mirror: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[:P] <- last + chain, or last when n_valid[0] == 0 (fgm_finish; the count is read on the device);
    ``mirror``: a second copy of out, device or pinned host memory."""
    _dev(chain, torch.float32, "chain", _cols(P))
    _dev(last, torch.float32, "last", _cols(P))
    _dev(n_valid, torch.int32, "n_valid", 1, align=4)
    _dev(out, torch.float32, "out", P)
    if mirror is not None:
        if mirror.device.type == "cpu":
            _pinned(mirror, torch.float32, "mirror", P)
        else:
            _dev(mirror, torch.float32, "mirror", P)
    NG.call("fgm_finish", ptr(chain), ptr(last), ptr(n_valid), int(P), ptr(out), ptr(mirror), _stream(out))
    return out
