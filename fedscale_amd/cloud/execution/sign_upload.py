"""Executor side of the 1-bit sign delta-upload path: ``compress_sign(state, base, residual=...)``.

The reference's executor uploads its trained state_dict as float32 numpy arrays (torch_client.py:79-91).  With
``TorchModelAdapter(upload_sign="sign1")`` on the aggregator, the executor sends the scaled sign of its UPDATE
``e = x - L`` instead — against ``L``, the weights it was sent for this round — one bit per parameter plus one float32
scale (the mean magnitude) per block of 256 parameters: 9/64 byte per parameter on the wire and in the aggregator's
staging area, 3.5 MB instead of 100 MB for a 25 M model::

    from fedscale_amd.cloud.execution.sign_upload import compress_sign
    upload, self.residual = compress_sign(model.state_dict(), weights_received_for_this_round,
                                          residual=self.residual, residual_out=True)
    results["update_weight"] = upload

Keeping only the sign is lossy; error feedback (EF-signSGD, 1-bit SGD) keeps what was lost: ``residual`` is added to
this round's update before it is encoded and ``residual_out`` is what this round's encoding leaves behind.  It is the
executor's state to keep between rounds.  Everything after the encoding is exact: the aggregator dequantises by a sign
flip of the scale and runs an fp32 chain (include/fedsign.h states the contract; this module and ``fsg_sign_row`` give
the same bytes).

Wire format: a plain dict in the state's order holding the entries that are NOT float32 (int64 counters) unchanged,
plus ``BITS_KEY`` (uint8 [ceil(P / 8)]: column p of the float32 entries concatenated in the state's order is bit p % 8
of byte p / 8) and ``SCALES_KEY`` (float32 [ceil(P / 256)]).  float32 entries do not appear.  (A list upload carries
the non-float32 entries in order, then the bits, then the scales.)
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .quant_upload import _base_values, _host, _is_f32

BITS_KEY = "__sign_bits__"
SCALES_KEY = "__sign_scales__"
BLOCK = 256
_NAN_SCALE = np.uint32(0x7FC00000)
_LANE = np.arange(64)


def encode_host(e: np.ndarray):
    """(bits uint8 [ceil(P / 8)], scales float32 [ceil(P / 256)], residual float32 [P]) of the float32 vector ``e``
    (include/fedsign.h): the block scale is the fp64 sum of |e| in the contract's fixed order over the block's
    existing column count, rounded once to fp32."""
    e = np.ascontiguousarray(e, dtype=np.float32)
    P = e.size
    NB = (P + BLOCK - 1) // BLOCK
    if P == 0:
        return np.zeros(0, np.uint8), np.zeros(0, np.float32), np.zeros(0, np.float32)
    pad = np.zeros(NB * BLOCK, dtype=np.float32)
    pad[:P] = e
    u = pad.view(np.uint32)
    bit = (u >> np.uint32(31)).astype(np.uint8).reshape(NB, BLOCK)
    bad = ((u & np.uint32(0x7FFFFFFF)) >= np.uint32(0x7F800000)).reshape(NB, BLOCK).any(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(pad).astype(np.float64).reshape(NB, 4, 64)
        t = ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]
        for m in (32, 16, 8, 4, 2, 1):  # wave_sum's xor butterfly: every lane adds its partner's value
            t = t + t[:, _LANE ^ m]
        n_b = np.full(NB, float(BLOCK))
        n_b[-1] = float(P - BLOCK * (NB - 1))
        scales = (t[:, 0] / n_b).astype(np.float32)
    scales.view(np.uint32)[bad] = _NAN_SCALE
    bit[bad] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        deq = np.where(bit.reshape(-1)[:P] != 0, -np.repeat(scales, BLOCK)[:P], np.repeat(scales, BLOCK)[:P])
        residual = (e - deq).astype(np.float32)
    residual[np.repeat(bad, BLOCK)[:P]] = np.float32(0.0)
    bits = np.packbits(bit.reshape(-1), bitorder="little")[:(P + 7) // 8]
    return bits, scales, residual


def compress_sign(state, base, residual=None, residual_out: Optional[bool] = None):
    """``(upload, residual_out)``: the scaled sign of ``state - base`` (+ ``residual``) over the float32 entries.

    ``base``: the weights this round started from, a dict with the state's keys or a list in its order.
    ``residual``: one flat float32 vector of P on the same side as the state (numpy for a host state, a device tensor
    for a state on a GPU), or None.  The second result is the flat float32 vector of what this round's encoding leaves
    behind when ``residual_out`` is true (default: when a ``residual`` was given), else None.  A state whose float32
    tensors are on a GPU is encoded there by one launch (fsg_sign_row) and the bits and scales cross to the host in
    one copy.  Both paths give the same bytes."""
    items = list(state.items())
    for name, _ in items:
        if name in (BITS_KEY, SCALES_KEY):
            raise ValueError(f"the state has an entry named {name!r}")
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
    NB = (P + BLOCK - 1) // BLOCK
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
        bits, scales, r = encode_host(e)
        if want_out:
            r_out = r
    else:
        from ... import kernels_sign as kg

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
            nbits = NB * (BLOCK // 8)
            buf = torch.empty(nbits + 4 * NB, dtype=torch.uint8, device=dev)
            kg.sign_row(x, L, r_in, P, buf[:nbits], buf[nbits:].view(torch.float32), r_out)
            host = buf.cpu().numpy()  # one D2H (synchronises with the launch)
        bits, scales = host[:(P + 7) // 8], host[nbits:].view(np.float32)
    out = {}  # a plain dict, in the state's order: what the aggregator and ingress.loads take without a copy
    f_set = set(f_idx)
    for i, (name, v) in enumerate(items):
        if i not in f_set:
            out[name] = _host(v)
    out[BITS_KEY] = bits
    out[SCALES_KEY] = scales
    return out, r_out
