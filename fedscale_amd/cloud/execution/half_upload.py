"""Executor side of the 16-bit upload path: ``compress_update(state, dtype)``.

The reference's executor uploads its trained state_dict as float32 numpy arrays (torch_client.py:79-91).  With
``TorchModelAdapter(upload_dtype=...)`` on the aggregator, the executor sends every float32 entry in 16 bits
instead — half the bytes on the wire and in the aggregator's staging area::

    from fedscale_amd.cloud.execution.half_upload import compress_update
    results["update_weight"] = compress_update(model.state_dict(), "bfloat16")

This step is lossy (one rounding to nearest even per element); everything after it is exact: the aggregator
widens each element back to fp32 and runs the fp32 reduction of the float32 path (include/fedhalf.h).

float16 entries are numpy ``float16`` arrays; bfloat16 entries are numpy ``uint16`` arrays holding the bfloat16
bits (numpy has no bfloat16).  Entries of any other dtype (int64 counters) are passed through unchanged.
"""
from __future__ import annotations

import numpy as np
import torch

_F32 = np.dtype(np.float32)


def _check_dtype(dtype) -> str:
    name = {torch.float16: "float16", torch.bfloat16: "bfloat16"}.get(dtype, dtype)
    if name not in ("float16", "bfloat16"):
        raise ValueError(f"upload dtype {dtype!r}: expected 'float16' or 'bfloat16'")
    return name


def _round_host(a, name: str) -> np.ndarray:
    """One float32 entry (CPU tensor or array) in 16 bits: numpy's astype(float16), torch's to(bfloat16)."""
    if isinstance(a, torch.Tensor):
        a = a.detach().numpy()
    if name == "float16":
        with np.errstate(over="ignore"):  # beyond the float16 range: +-inf, as specified
            return a.astype(np.float16)
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16)


def _is_f32(v) -> bool:
    if isinstance(v, torch.Tensor):
        return v.dtype == torch.float32
    return isinstance(v, np.ndarray) and v.dtype == _F32


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v


def compress_update(state, dtype="float16") -> dict:
    """name -> array, in ``state``'s order: float32 entries as float16 (or uint16 bfloat16 bits), the rest as
    they are (numpy arrays).  A state whose float32 tensors are on a GPU is rounded there into one 16-bit row by
    one multi-tensor launch (fh_pack_row) and copied to the host once; the dict's arrays are then views of that
    one host buffer.  Both paths give the same bits."""
    name = _check_dtype(dtype)
    items = list(state.items())
    on_gpu = [k for k, v in items if isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32]
    out = {}  # a plain dict, in the state's order: what the aggregator and ingress.loads take without a copy
    if not on_gpu:
        for k, v in items:
            out[k] = _round_host(v, name) if _is_f32(v) else _host(v)
        return out

    from ... import kernels_half as kh

    tdt = kh.row_dtype(name)[0]
    dev = state[on_gpu[0]].device
    srcs, offs, total = [], [], 0
    for k in on_gpu:
        t = state[k].detach()
        if t.device != dev:
            raise ValueError(f"{k}: on {t.device}, the state's other tensors on {dev}")
        srcs.append(t if t.is_contiguous() else t.contiguous())
        offs.append(total)
        total += (t.numel() + 7) // 8 * 8  # every entry starts 16-byte aligned in the row
    with torch.cuda.device(dev):
        row = torch.empty(max(8, total), dtype=tdt, device=dev)
        kh.pack_row16(srcs, offs, row)
        host = row.view(torch.int16).cpu().numpy()  # one D2H (synchronises with the launch)
    host = host.view(np.float16 if name == "float16" else np.uint16)
    where = dict(zip(on_gpu, offs))
    for k, v in items:
        if k in where:
            o = where[k]
            out[k] = host[o:o + v.numel()].reshape(tuple(v.shape))
        else:
            out[k] = _round_host(v, name) if _is_f32(v) else _host(v)
    return out
