"""Executor side of the low-rank delta-upload path: ``LowRankCompressor(rank, seed).compress(state, base)``.

The reference's executor uploads its trained state_dict as float32 numpy arrays.  With
``TorchModelAdapter(upload_lowrank=rank)`` on the aggregator, the executor sends, for every weight matrix that is
worth factoring, two thin factors of its UPDATE ``d = x - L`` — against ``L``, the weights it was sent for this round —
instead of the matrix: ``r * (O + I)`` floats for ``O * I`` (PowerSGD, Vogels et al. 2019)::

    from fedscale_amd.cloud.execution.lowrank_upload import LowRankCompressor
    self.compressor = LowRankCompressor(rank=4, seed=client_id)      # once: it keeps Q and the residual
    results["update_weight"] = self.compressor.compress(model.state_dict(), weights_received_for_this_round)

Which entries are factored is ``factored(shape, rank)``, a function of the shape and the rank alone that both sides
use.  Wire format: a plain dict in the state's order; a factored entry holds one float32 array ``[r, O + I]`` whose
row j is ``Ut[j, 0:O]`` followed by ``V[j, 0:I]`` (the entry's delta is ``d[o, i] = sum_j Ut[j, o] * V[j, i]``); every
other float32 entry holds its delta ``x - L`` in the entry's shape; non-float32 entries (int64 counters) travel
unchanged.

An existing LoRA pair ``(B [O, r], A [r, I])`` of a layer is already an upload: ``Ut = B.T``, ``V = A``
(``pack_factors(B.T, A)``); the aggregator's sum over clients of ``B_k A_k`` is the stacked aggregation of FLoRA.

One PowerSGD step per factored entry and round, on ``M = (x - L) + residual`` viewed as ``[O, I]``:
``P = M Q``; ``P`` orthonormalised (torch.linalg.qr); ``Q = M^T P``; upload ``Ut = P^T``, ``V = Q^T``;
``residual = M - P Q^T`` (error feedback; ``error_feedback=False`` drops it).  ``Q`` is warm-started from the
previous round and drawn per entry from ``seed`` on the first.  torch only: it runs wherever the tensors live.
"""
from __future__ import annotations

import zlib

import numpy as np
import torch

from .quant_upload import _base_values, _host, _is_f32

MAX_RANK = 64


def check_rank(rank) -> int:
    """``rank`` as an int when it is one in 1..64; ValueError otherwise."""
    if isinstance(rank, bool) or not isinstance(rank, (int, np.integer)) or not 1 <= int(rank) <= MAX_RANK:
        raise ValueError(f"upload_lowrank {rank!r}: expected an integer rank in 1..{MAX_RANK}")
    return int(rank)


def matrix_dims(shape) -> tuple:
    """(O, I) of an entry of shape (O, *rest): I = prod(rest); a scalar or 1-D entry has I = 1."""
    shape = tuple(int(s) for s in shape)
    if not shape:
        return 1, 1
    return shape[0], int(np.prod(shape[1:], dtype=np.int64)) if len(shape) > 1 else 1


def factored(shape, rank: int) -> bool:
    """Whether a float32 entry of ``shape`` travels as rank-``rank`` factors: at least 2-D, both sides of its
    [O, I] view longer than the rank, and the factors smaller than the matrix."""
    if len(shape) < 2:
        return False
    O, I = matrix_dims(shape)
    return min(O, I) > rank and rank * (O + I) < O * I


def pack_factors(Ut, V):
    """The wire array [r, O + I] of the factors ``Ut [r, O]`` and ``V [r, I]`` (numpy float32)."""
    Ut, V = np.asarray(_host(Ut), dtype=np.float32), np.asarray(_host(V), dtype=np.float32)
    if Ut.ndim != 2 or V.ndim != 2 or Ut.shape[0] != V.shape[0]:
        raise ValueError(f"pack_factors: Ut {Ut.shape} and V {V.shape} must be [r, O] and [r, I]")
    return np.ascontiguousarray(np.concatenate([Ut, V], axis=1))


def expand(upload, layout) -> list:
    """The dense float32 deltas of an upload (dict, or list in layout order), one array per float32 entry of
    ``layout`` (a ``BucketLayout``) in the entry's shape: factors multiplied out in float32 by numpy, dense entries as
    they are.  An array [r, O + I] never has its entry's shape (O, *rest), so the arrays tell which entries are
    factored."""
    values = layout.values_of(upload)
    out = []
    for e in layout.f_entries:
        v = np.asarray(_host(values[e.index]))
        O, I = matrix_dims(e.shape)
        if tuple(v.shape) == e.shape:
            out.append(v.astype(np.float32))
        elif v.ndim == 2 and v.shape[1] == O + I and len(e.shape) >= 2:
            out.append((v[:, :O].T.astype(np.float32) @ v[:, O:].astype(np.float32)).reshape(e.shape))
        else:
            raise TypeError(f"{e.name}: shape {tuple(v.shape)} is neither the entry's {e.shape} nor factors "
                            f"[r, {O + I}]")
    return out


class LowRankCompressor:
    """One client's PowerSGD state: per factored entry the warm-start ``Q [I, r]`` and, with error feedback, the
    residual ``[O, I]``; both live where the entry's tensors live."""

    def __init__(self, rank: int, seed: int = 0, error_feedback: bool = True):
        self.rank = check_rank(rank)
        self.seed = int(seed)
        self.error_feedback = bool(error_feedback)
        self.Q = {}         # name -> [I, r]
        self.residual = {}  # name -> [O, I]

    def _first_q(self, name: str, I: int, like: torch.Tensor) -> torch.Tensor:
        g = torch.Generator()  # a CPU generator: the same draws wherever the tensors live
        g.manual_seed((self.seed * 0x9E3779B1 + zlib.crc32(name.encode())) % (1 << 63))
        return torch.randn(I, self.rank, generator=g, dtype=torch.float32).to(like.device)

    def compress(self, state, base) -> dict:
        """name -> array, in ``state``'s order: the upload of ``state - base`` (+ the residuals kept from earlier
        rounds).  ``base``: the weights this round started from, a dict with the state's keys or a list in its
        order."""
        items = list(state.items())
        bvals = _base_values(items, base)
        out = {}
        for (name, v), b in zip(items, bvals):
            if not _is_f32(v):
                out[name] = _host(v)
                continue
            if tuple(b.shape) != tuple(v.shape):
                raise ValueError(f"{name}: base shape {tuple(b.shape)} != state shape {tuple(v.shape)}")
            if not _is_f32(b):
                raise TypeError(f"{name}: base dtype {b.dtype}, the state's entry is float32")
            x = torch.as_tensor(v).detach()
            d = x - torch.as_tensor(b).detach().to(x.device)
            if not factored(tuple(x.shape), self.rank):
                out[name] = d.cpu().numpy()
                continue
            O, I = matrix_dims(x.shape)
            M = d.reshape(O, I)
            if self.error_feedback and name in self.residual:
                M = M + self.residual[name]
            Q = self.Q.get(name)
            if Q is None:
                Q = self._first_q(name, I, M)
            P, _ = torch.linalg.qr(M @ Q)  # [O, r], orthonormal columns
            Q = M.t() @ P                  # [I, r]
            self.Q[name] = Q
            if self.error_feedback:
                self.residual[name] = M - P @ Q.t()
            out[name] = torch.cat([P.t(), Q.t()], dim=1).contiguous().cpu().numpy()
        return out
