"""Executor side of the MXFP4 delta-upload path: ``compress_delta4(state, base, residual=...)``.

The reference's executor uploads its trained state_dict as float32 numpy arrays (torch_client.py:79-91).  With
``TorchModelAdapter(upload_fp4="mxfp4")`` on the aggregator, the executor sends the UPDATE ``d = x - L`` of its
float32 entries instead — against ``L``, the weights it was sent for this round — quantised to the OCP Microscaling
format MXFP4: 17/32 byte per parameter on the wire and in the aggregator's staging area, 13.3 MB instead of 100 MB for
a 25 M model::

    from fedscale_amd.cloud.execution.quant4_upload import compress_delta4
    upload, self.residual = compress_delta4(model.state_dict(), weights_received_for_this_round,
                                            residual=self.residual, residual_out=True)
    results["update_weight"] = upload

This step is lossy (one rounding per element to the eight e2m1 magnitudes, relative to the largest delta of its block
of 32); error feedback keeps what was lost: ``residual`` is added to this round's update before it is quantised and
``residual_out`` is what this round's encoding leaves behind.  It is the executor's state to keep between rounds, and
optional.  Everything after the encoding is exact: the aggregator dequantises each code exactly and runs an fp32 chain
(include/fedquant4.h states the contract; this module and ``fq4_quantize_row`` give the same bytes).

Wire format: a plain dict in the state's order holding the entries that are NOT float32 (int64 counters) unchanged,
plus ``CODES_KEY`` (uint8 [16 * ceil(P / 32)]: column p of the float32 entries concatenated in the state's order is
the low nibble of byte p / 2 when p is even and its high nibble when p is odd; the padding codes of the last block are
0) and ``SCALES_KEY`` (uint8 [ceil(P / 32)] E8M0 scale bytes).  float32 entries do not appear.  (A list upload
carries the non-float32 entries in order, then the codes, then the scales.)
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .quant_upload import _base_values, _host, _is_f32

CODES_KEY = "__mxfp4_codes__"
SCALES_KEY = "__mxfp4_scales__"
BLOCK = 32
#: value(code) of the 16 e2m1 codes: s eem
VALUES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0],
                  dtype=np.float32)


def block_scales(d: np.ndarray) -> np.ndarray:
    """The E8M0 scale byte of every row of the float32 [NB, 32] array ``d``, on its bit fields alone:
    clamp(E - 2 + (M > 0x400000), 2, 252) of the row's largest |d|; 255 for a row holding a NaN or an infinity."""
    am = (d.view(np.uint32) & np.uint32(0x7FFFFFFF)).max(axis=1).astype(np.int64)
    s = (am >> 23) - 2 + ((am & 0x7FFFFF) > 0x400000)
    s = np.clip(s, 2, 252)
    s[am >= 0x7F800000] = 255
    return s.astype(np.uint8)


def round_e2m1(v: np.ndarray) -> np.ndarray:
    """The e2m1 code of every element of the float32 array ``v`` in [-6, 6]: the nearest magnitude, a tie to the code
    whose low bit is 0, the sign bit kept."""
    m = np.abs(v)
    c = ((m > 0.25).astype(np.uint8) + (m >= 0.75) + (m > 1.25) + (m >= 1.75) + (m > 2.5) + (m >= 3.5) + (m > 5.0))
    return (c | ((v.view(np.uint32) >> np.uint32(31)) << np.uint32(3))).astype(np.uint8)


def quantize_host(d: np.ndarray):
    """(codes uint8 [16 * ceil(P / 32)], scales uint8 [ceil(P / 32)], residual float32 [P]) of the float32 vector
    ``d`` (include/fedquant4.h), in numpy integer and float32 arithmetic."""
    d = np.ascontiguousarray(d, dtype=np.float32)
    P = d.size
    NB = (P + BLOCK - 1) // BLOCK
    blk = np.zeros(NB * BLOCK, dtype=np.float32)
    blk[:P] = d
    blk = blk.reshape(NB, BLOCK)
    s = block_scales(blk)
    bad = s == 255
    fin = np.where(bad, 252, s).astype(np.uint32)
    mul = ((np.uint32(254) - fin) << np.uint32(23)).view(np.float32)  # 2^(127 - s)
    sc = (fin << np.uint32(23)).view(np.float32)                      # 2^(s - 127)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = np.clip(blk * mul[:, None], np.float32(-6.0), np.float32(6.0))
        v[bad] = 0.0
        code = round_e2m1(v)
        residual = (blk - VALUES[code] * sc[:, None]).astype(np.float32)
    residual[bad] = 0.0
    code = code.reshape(-1)
    return (code[0::2] | (code[1::2] << 4)).astype(np.uint8), s, residual.reshape(-1)[:P]


def compress_delta4(state, base, residual=None, residual_out: Optional[bool] = None):
    """``(upload, residual_out)``: the MXFP4 codes of ``state - base`` (+ ``residual``) over the float32 entries.

    ``base``: the weights this round started from, a dict with the state's keys or a list in its order.
    ``residual``: one flat float32 vector of P on the same side as the state (numpy for a host state, a device tensor
    for a state on a GPU), or None.  The second result is the flat float32 vector of what this round's encoding leaves
    behind when ``residual_out`` is true (default: when a ``residual`` was given), else None.  A state whose float32
    tensors are on a GPU is quantised there by one launch (fq4_quantize_row) and the codes and scale bytes cross to
    the host in one copy.  Both paths give the same bytes."""
    items = list(state.items())
    for name, _ in items:
        if name in (CODES_KEY, SCALES_KEY):
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
            d = x - L
            if residual is not None:
                d = d + np.asarray(_host(residual), dtype=np.float32)
        codes, scales, r = quantize_host(d)
        if want_out:
            r_out = r
    else:
        from ... import kernels_quant4 as kq4

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
            nc = NB * (BLOCK // 2)
            buf = torch.empty(nc + NB, dtype=torch.uint8, device=dev)
            kq4.quantize_row4(x, L, r_in, P, buf[:nc], buf[nc:], r_out)
            host = buf.cpu().numpy()  # one D2H (synchronises with the launch)
        codes, scales = host[:nc], host[nc:]
    out = {}  # a plain dict, in the state's order: what the aggregator and ingress.loads take without a copy
    f_set = set(f_idx)
    for i, (name, v) in enumerate(items):
        if i not in f_set:
            out[name] = _host(v)
    out[CODES_KEY] = codes
    out[SCALES_KEY] = scales
    return out, r_out
