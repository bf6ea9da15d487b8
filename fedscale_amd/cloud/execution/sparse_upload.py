"""Executor side of the top-k sparse delta-upload path: ``compress_topk(state, base, density=...)``.

The reference's executor uploads its trained state_dict as float32 numpy arrays (torch_client.py:79-91).  With
``TorchModelAdapter(upload_topk=density)`` on the aggregator, the executor sends the k largest-magnitude entries of
its UPDATE ``e = x - L`` instead — against ``L``, the weights it was sent for this round — as (index, value) pairs:
8 bytes per kept entry on the wire and in the aggregator's staging area, 2 MB instead of 100 MB for a 25 M model at
1 % density::

    from fedscale_amd.cloud.execution.sparse_upload import compress_topk
    upload, self.residual = compress_topk(model.state_dict(), weights_received_for_this_round, density=0.01,
                                          residual=self.residual, residual_out=True)
    results["update_weight"] = upload

Dropping entries is lossy; error feedback ("sparsified SGD with memory") keeps what was dropped: ``residual`` is added
to this round's update before the selection and ``residual_out`` is what this round drops.  It is the executor's
state to keep between rounds.  Everything after the selection is exact: kept values are not rounded, and the
aggregator runs an fp32 chain (include/fedsparse.h states the rule; this module and ``fs_topk_row`` give the same
bytes).

Wire format: a plain dict in the state's order holding the entries that are NOT float32 (int64 counters) unchanged,
plus ``IDX_KEY`` (uint32 [nnz], strictly increasing positions in the float32 entries concatenated in the state's
order) and ``VAL_KEY`` (float32 [nnz]).  float32 entries do not appear.  (A list upload carries the non-float32
entries in order, then the index array, then the value array.)
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from .quant_upload import _base_values, _host, _is_f32

IDX_KEY = "__topk_idx__"
VAL_KEY = "__topk_val__"


def count_of(density: float, P: int) -> int:
    """Pairs a row of P columns keeps at ``density``: max(1, ceil(density * P)), at most P."""
    density = float(density)
    if not 0.0 < density <= 1.0:
        raise ValueError(f"density {density!r}: expected a fraction in (0, 1]")
    return min(int(P), max(1, int(math.ceil(density * int(P)))))


def select_host(e: np.ndarray, k: int):
    """(idx uint32 [min(k, P)], kept mask) of the float32 vector ``e`` by the threshold rule of include/fedsparse.h:
    every column whose key (|e| as its bits) exceeds the k-th largest key, and the lowest-indexed columns of that key
    until k are kept."""
    P = e.size
    k = min(int(k), P)
    keep = np.zeros(P, dtype=bool)
    if k == 0:
        return np.zeros(0, dtype=np.uint32), keep
    key = np.ascontiguousarray(e, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    tau = np.partition(key, P - k)[P - k]
    keep = key > tau
    need = k - int(keep.sum())
    keep[np.flatnonzero(key == tau)[:need]] = True
    return np.flatnonzero(keep).astype(np.uint32), keep


def compress_topk(state, base, density: Optional[float] = None, k: Optional[int] = None, residual=None,
                  residual_out: Optional[bool] = None):
    """``(upload, residual_out)``: the top-k sparsified ``state - base`` (+ ``residual``) over the float32 entries.

    ``base``: the weights this round started from, a dict with the state's keys or a list in its order.  Exactly one
    of ``density`` (k = max(1, ceil(density * P))) and ``k``.  ``residual``: one flat float32 vector of P on the
    same side as the state (numpy for a host state, a device tensor for a state on a GPU), or None.  The second
    result is the flat float32 vector of what this round dropped when ``residual_out`` is true (default: when a
    ``residual`` was given), else None.  A state whose float32 tensors are on a GPU is selected there
    (fs_topk_row) and the pairs cross to the host in one copy.  Both paths give the same bytes."""
    if (density is None) == (k is None):
        raise ValueError("compress_topk: give exactly one of density and k")
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
    if k is None:
        k = count_of(density, P) if P else 0
    elif int(k) < 1:
        raise ValueError(f"k={k}: a selection keeps at least one column")
    k = min(int(k), P)
    want_out = (residual is not None) if residual_out is None else bool(residual_out)
    if residual is not None and (tuple(residual.shape) != (P,) or not _is_f32(residual)):
        raise ValueError(f"residual: expected a flat float32 vector of {P}, got "
                         f"{getattr(residual, 'dtype', type(residual).__name__)} "
                         f"{tuple(getattr(residual, 'shape', ()))}")
    on_gpu = [i for i in f_idx if isinstance(items[i][1], torch.Tensor) and items[i][1].is_cuda]
    r_out = None
    if not on_gpu or P == 0:
        x = np.empty(P, dtype=np.float32)
        L = np.empty(P, dtype=np.float32)
        o = 0
        for i, n in zip(f_idx, sizes):
            x[o:o + n] = np.asarray(_host(items[i][1])).reshape(-1)
            L[o:o + n] = np.asarray(_host(bvals[i])).reshape(-1)
            o += n
        with np.errstate(invalid="ignore", over="ignore"):
            e = x - L
            if residual is not None:
                e = e + np.asarray(_host(residual), dtype=np.float32)
        idx, keep = select_host(e, k)
        val = e[idx.astype(np.int64)]
        if want_out:
            r_out = np.where(keep, np.float32(0.0), e).astype(np.float32)
    else:
        from ... import kernels_sparse as ks

        dev = items[on_gpu[0]][1].device
        with torch.cuda.device(dev):
            xs = [torch.as_tensor(items[i][1]).detach().to(dev).reshape(-1) for i in f_idx]
            Ls = [torch.as_tensor(bvals[i]).detach().to(dev).reshape(-1) for i in f_idx]
            x, L = torch.cat(xs), torch.cat(Ls)
            r_in = None
            if residual is not None:
                r_in = torch.as_tensor(residual).detach().to(dev).contiguous()
            if want_out:
                r_out = torch.empty(P, dtype=torch.float32, device=dev)
            kp = (k + 3) // 4 * 4
            buf = torch.empty(2 * kp, dtype=torch.int32, device=dev)
            ws = torch.empty(ks.topk_workspace(P), dtype=torch.uint8, device=dev)
            ks.topk_row(x, L, r_in, P, k, ws, buf[:kp], buf[kp:].view(torch.float32), r_out)
            host = buf.cpu().numpy()  # one D2H (synchronises with the launches)
        idx, val = host[:k].view(np.uint32), host[kp:kp + k].view(np.float32)
    out = {}  # a plain dict, in the state's order: what the aggregator and ingress.loads take without a copy
    f_set = set(f_idx)
    for i, (name, v) in enumerate(items):
        if i not in f_set:
            out[name] = _host(v)
    if IDX_KEY in out or VAL_KEY in out:
        raise ValueError(f"the state has an entry named {IDX_KEY!r} or {VAL_KEY!r}")
    out[IDX_KEY] = idx
    out[VAL_KEY] = val
    return out, r_out

