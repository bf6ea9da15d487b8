"""Executor side of the MXFP8 delta-upload path: ``compress_delta(state, base)``.

The reference's executor uploads its trained state_dict as float32 numpy arrays (torch_client.py:79-91).  With
``TorchModelAdapter(upload_quant="mxfp8")`` on the aggregator, the executor sends the UPDATE ``d = x - L`` of its
float32 entries instead — against ``L``, the weights it was sent for this round — quantised to the OCP Microscaling
format MXFP8: 1 + 1/32 bytes per parameter on the wire and in the aggregator's staging area::

    from fedscale_amd.cloud.execution.quant_upload import compress_delta
    results["update_weight"] = compress_delta(model.state_dict(), weights_received_for_this_round)

This step is lossy (one rounding to nearest even per element, relative to the largest delta of its block of 32);
everything after it is exact: the aggregator dequantises each code exactly and runs an fp32 chain
(include/fedquant.h states the arithmetic; this module and ``fq_quantize_row`` give the same bytes).

Wire format: a plain dict in the state's order; every float32 entry is a uint8 array of that entry's shape holding
``e4m3fn`` codes; entries of any other dtype (int64 counters) are passed through unchanged; one extra key,
``SCALES_KEY``, holds the uint8 [ceil(P / 32)] array of E8M0 scale bytes — blocks run over the float32 entries
concatenated in the state's order and do not restart at entry boundaries.  (A list upload carries the scale array
last.)
"""
from __future__ import annotations

import numpy as np
import torch

SCALES_KEY = "__mxfp8_scales__"
BLOCK = 32
_F32 = np.dtype(np.float32)


def _is_f32(v) -> bool:
    if isinstance(v, torch.Tensor):
        return v.dtype == torch.float32
    return isinstance(v, np.ndarray) and v.dtype == _F32


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v


def block_scales(d: np.ndarray) -> np.ndarray:
    """The E8M0 scale byte of every row of the float32 [NB, 32] array ``d``, on its bit fields alone:
    clamp(E - 8 + (M > 0x600000), 10, 246) of the row's largest |d|; 255 for a row holding a NaN or an infinity."""
    am = (d.view(np.uint32) & np.uint32(0x7FFFFFFF)).max(axis=1).astype(np.int64)
    s = (am >> 23) - 8 + ((am & 0x7FFFFF) > 0x600000)
    s = np.clip(s, 10, 246)
    s[am >= 0x7F800000] = 255
    return s.astype(np.uint8)


def quantize_host(d: np.ndarray):
    """(codes uint8 [round_up(P, 32)], scales uint8 [ceil(P / 32)]) of the float32 vector ``d`` (include/fedquant.h):
    numpy integer arithmetic for the scale, torch's CPU float8_e4m3fn cast for the rounding."""
    P = d.size
    NB = (P + BLOCK - 1) // BLOCK
    blk = np.zeros(NB * BLOCK, dtype=np.float32)
    blk[:P] = d
    blk = blk.reshape(NB, BLOCK)
    s = block_scales(blk)
    bad = s == 255
    mul = ((254 - np.where(bad, 246, s).astype(np.uint32)) << np.uint32(23)).view(np.float32)  # 2^(127 - s)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = np.clip(blk * mul[:, None], np.float32(-448.0), np.float32(448.0))
    v[bad] = 0.0  # codes of such a block are unspecified; both paths write 0
    codes = torch.from_numpy(v.reshape(-1)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return codes, s


def _base_values(state_items, base) -> list:
    if type(base) is dict or hasattr(base, "keys"):
        try:
            return [base[k] for k, _ in state_items]
        except KeyError as e:
            raise ValueError(f"base has no entry {e.args[0]!r} of the state") from None
    base = list(base)
    if len(base) != len(state_items):
        raise ValueError(f"base has {len(base)} entries, the state has {len(state_items)}")
    return base


def compress_delta(state, base) -> dict:
    """name -> array, in ``state``'s order, plus ``SCALES_KEY``: the MXFP8 codes of ``state - base`` over the float32
    entries, the rest as they are (numpy arrays).  ``base``: the weights this round started from, a dict with the
    state's keys or a list in its order (what the executor received).  A state whose float32 tensors are on a GPU is
    quantised there by one launch (fq_quantize_row) and copied to the host once; the dict's arrays are then views of
    that one host buffer.  Both paths give the same bytes."""
    items = list(state.items())
    bvals = _base_values(items, base)
    f_idx = [i for i, (_, v) in enumerate(items) if _is_f32(v)]
    for i in f_idx:
        k, v = items[i]
        b = bvals[i]
        if tuple(b.shape) != tuple(v.shape):
            raise ValueError(f"{k}: base shape {tuple(b.shape)} != state shape {tuple(v.shape)}")
        if not _is_f32(b):
            raise TypeError(f"{k}: base dtype {b.dtype}, the state's entry is float32")
    sizes = [int(np.prod(items[i][1].shape)) if len(items[i][1].shape) else 1 for i in f_idx]
    P = int(sum(sizes))
    NB = (P + BLOCK - 1) // BLOCK
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
            codes, scales = quantize_host(x - L)
    else:
        from ... import kernels_quant as kq

        dev = items[on_gpu[0]][1].device
        with torch.cuda.device(dev):
            xs = [torch.as_tensor(items[i][1]).detach().to(dev).reshape(-1) for i in f_idx]
            Ls = [torch.as_tensor(bvals[i]).detach().to(dev).reshape(-1) for i in f_idx]
            x, L = torch.cat(xs), torch.cat(Ls)
            buf = torch.empty(max(16, NB * BLOCK + NB), dtype=torch.uint8, device=dev)
            kq.quantize_row(x, L, P, buf[:NB * BLOCK], buf[NB * BLOCK:NB * BLOCK + NB])
            host = buf.cpu().numpy()  # one D2H (synchronises with the launch)
        codes, scales = host[:NB * BLOCK], host[NB * BLOCK:NB * BLOCK + NB]
    out = {}  # a plain dict, in the state's order: what the aggregator and ingress.loads take without a copy
    where, o = {}, 0
    for i, n in zip(f_idx, sizes):
        where[i] = (o, n)
        o += n
    for i, (k, v) in enumerate(items):
        if i in where:
            o, n = where[i]
            out[k] = codes[o:o + n].reshape(tuple(v.shape))
        else:
            out[k] = _host(v)
    if SCALES_KEY in out:
        raise ValueError(f"the state has an entry named {SCALES_KEY!r}")
    out[SCALES_KEY] = scales
    return out
