"""Typed torch-tensor wrappers over the secure-aggregation path's C ABI (include/fedsecagg.h), with the same host-side
checks as ``kernels_quant``: device / dtype / contiguity / size, launched on the current HIP stream of the output's
device.

The words of this path are uint32 mod 2^32.  On the device they live in ``torch.int32`` tensors — the same bits; this
torch build copies, slices and allocates int32 everywhere, which it does not do for its uint32 dtype.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native_secagg as NS
from ._native import FA_ACCUMULATE, ptr
from .kernels import _cols, _dev, _pinned, _stream, _strip_plan

WORD = torch.int32  #: the device dtype of a uint32 word (same bits)
MAX_COLS = 1 << 36  #: col0 + P of one mask stream: the 32-bit block counter times 16 columns


def check_nonce(nonce) -> tuple:
    """``nonce`` as three uint32 words; ValueError otherwise."""
    try:
        n = tuple(int(v) for v in nonce)
    except TypeError:
        raise ValueError(f"nonce={nonce!r}: expected three uint32 words") from None
    if len(n) != 3 or any(not 0 <= v <= 0xFFFFFFFF for v in n):
        raise ValueError(f"nonce={nonce!r}: expected three uint32 words")
    return n


def keys_array(keys) -> np.ndarray:
    """``keys`` (a list of 256-bit keys, each eight uint32 words or 32 bytes — little-endian words, as RFC 8439 reads
    a key — or a uint32 [M, 8] array) as a C-contiguous uint32 [M, 8] array; ValueError names what does not fit."""
    if isinstance(keys, np.ndarray) and keys.dtype == np.uint32 and keys.ndim == 2 and keys.shape[1] == 8:
        return np.ascontiguousarray(keys)
    out = np.empty((len(keys), 8), dtype=np.uint32)
    for i, k in enumerate(keys):
        if isinstance(k, (bytes, bytearray, memoryview)):
            if len(k) != 32:
                raise ValueError(f"key {i}: {len(k)} bytes, a key has 32")
            out[i] = np.frombuffer(bytes(k), dtype="<u4")
            continue
        w = [int(v) for v in k]
        if len(w) != 8 or any(not 0 <= v <= 0xFFFFFFFF for v in w):
            raise ValueError(f"key {i}: expected eight uint32 words or 32 bytes")
        out[i] = w
    return out


def encode_row(x: torch.Tensor, base: Optional[torch.Tensor], P: int, frac_bits: int, mag_bits: int,
               out: torch.Tensor, stats: torch.Tensor) -> None:
    """out[:P] <- the fixed-point words of the fp32 device row x[:P] - base[:P] (of x[:P] when ``base`` is None);
    stats[:2] <- (n_clamped, n_nan) (fsa_encode_row)."""
    _dev(x, torch.float32, "x", P)
    if base is not None:
        _dev(base, torch.float32, "base", P)
        if base.device != x.device:
            raise ValueError(f"base: on {base.device}, x on {x.device}")
    _dev(out, WORD, "out", P)
    _dev(stats, torch.int64, "stats", 2, align=8)
    if out.device != x.device or stats.device != x.device:
        raise ValueError(f"out / stats: on {out.device} / {stats.device}, x on {x.device}")
    NS.call("fsa_encode_row", ptr(x), ptr(base), int(P), int(frac_bits), int(mag_bits), ptr(out), ptr(stats),
            _stream(out))


def mask_sum(keys: Optional[torch.Tensor], n_add: int, n_sub: int, nonce, P: int, acc_in: torch.Tensor,
             out: torch.Tensor, *, col0: int = 0) -> torch.Tensor:
    """out[:P] <- acc_in[:P] + the keystreams of keys[:n_add] - those of keys[n_add:n_add + n_sub], mod 2^32, over
    stream columns [col0, col0 + P) (fsa_mask_sum); ``keys`` an int32 [M, 8] device tensor (None with no key at all);
    out may be acc_in."""
    n_add, n_sub = int(n_add), int(n_sub)
    M = n_add + n_sub
    n0, n1, n2 = check_nonce(nonce)
    if n_add < 0 or n_sub < 0 or M > NS.MAX_KEYS:
        raise ValueError(f"mask_sum: n_add={n_add}, n_sub={n_sub}: negative, or more than FSA_MAX_KEYS={NS.MAX_KEYS}")
    if col0 < 0 or col0 % 16 or col0 + P > MAX_COLS:
        raise ValueError(f"mask_sum: col0={col0} must be a multiple of 16 with col0 + P <= 2^36")
    _dev(out, WORD, "out", P)
    _dev(acc_in, WORD, "acc_in", P)
    if acc_in.device != out.device:
        raise ValueError(f"acc_in: on {acc_in.device}, out on {out.device}")
    if M > 0:
        _dev(keys, WORD, "keys", 8 * M, align=4)
        if keys.device != out.device:
            raise ValueError(f"keys: on {keys.device}, out on {out.device}")
    NS.call("fsa_mask_sum", ptr(keys) if M > 0 else None, n_add, n_sub, n0, n1, n2, int(col0), int(P), ptr(acc_in),
            ptr(out), _stream(out))
    return out


def reduce32(y: torch.Tensor, n: int, P: int, out: torch.Tensor, *,
             acc_in: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[:P] <- the sum mod 2^32 of the rows y[:n, :P], continuing ``acc_in`` when given (fsa_reduce); out may be
    acc_in, and is written in [0, P) only."""
    if n > 0:
        _dev(y, WORD, "y")
        if y.dim() != 2:
            raise ValueError("y: expected a [n, ld] client-major buffer")
        if n > y.shape[0]:
            raise ValueError(f"y: n={n} > rows {y.shape[0]}")
        ld = y.shape[1]
        if ld < P or ld % 64:
            raise ValueError(f"y: ld={ld} must be >= P={P} and a multiple of 64")
    else:
        ld = (P + 63) // 64 * 64
    _dev(out, WORD, "out", P)
    if acc_in is not None:
        _dev(acc_in, WORD, "acc_in", _cols(P))
    NS.call("fsa_reduce", ptr(y) if n > 0 else None, ld, int(n), int(P), ptr(acc_in), ptr(out),
            FA_ACCUMULATE if acc_in is not None else 0, _stream(out))
    return out


def reduce32_plan(cus: int, K: int, P: int) -> list:
    """The launches fsa_reduce makes at (K, P) on a GPU of ``cus`` compute units (fsa_reduce_plan; no GPU needed):
    a list of dicts V, U, col0, tiles, sw, grid."""
    return _strip_plan(lambda out, cap: NS.call("fsa_reduce_plan", int(cus), int(K), int(P), out, cap),
                       NS.PLAN_FIELDS)


def finish(total: torch.Tensor, last: torch.Tensor, P: int, frac_bits: int, mag_bits: int, n: int,
           out: torch.Tensor, out_of_range: torch.Tensor, *, mirror: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[:P] <- last + float((int32(total) * 2^-frac_bits) / n); out_of_range[0] <- the columns with
    |int32(total)| > n * (2^mag_bits - 1) (fsa_finish); ``mirror``: a second copy of out, device or pinned host
    memory."""
    _dev(total, WORD, "sum", _cols(P))
    _dev(last, torch.float32, "last", _cols(P))
    _dev(out, torch.float32, "out", P)
    _dev(out_of_range, torch.int64, "out_of_range", 1, align=8)
    if mirror is not None:
        if mirror.device.type == "cpu":
            _pinned(mirror, torch.float32, "mirror", P)
        else:
            _dev(mirror, torch.float32, "mirror", P)
    NS.call("fsa_finish", ptr(total), ptr(last), int(P), int(frac_bits), int(mag_bits), int(n), ptr(out),
            ptr(mirror), ptr(out_of_range), _stream(out))
    return out
