"""Executor side of the rotated 1-bit sign delta-upload path: ``compress_sign_rotated(state, base, seed, ...)``.

``compress_sign`` (sign_upload.py) keeps, of a block's energy, the share (sum |e|)^2 / (n sum e^2): 2/pi for a
Gaussian block, and next to nothing for the updates federated clients really send — embedding rows touched by a few
tokens, dead channels, heavy tails.  A random rotation before the encoder makes 1-bit quantisation distribution-free
(Suresh et al., ICML 2017; DRIVE, Vargaftik et al., NeurIPS 2021): the update is multiplied by a seed's +-1 diagonal
and by the orthonormal 4096-point Hadamard matrix, block by block, and the SIGN ENCODER SEES THE ROTATED VECTOR.
With ``TorchModelAdapter(upload_sign="sign1", upload_rotate="rht4096")`` on the aggregator::

    from fedscale_amd.cloud.execution.rotate_upload import compress_sign_rotated
    upload, self.residual = compress_sign_rotated(model.state_dict(), weights_received_for_this_round, JOB_SEED,
                                                  residual=self.residual, residual_out=True)
    results["update_weight"] = upload

The rotation is linear, so the aggregator chains the rotated rows as they are and rotates the chain back once per
round; it is orthonormal, so the encoder's error in rotated space is its error in parameter space.  include/fedrotate.h
states the transform (the diagonal, the stage order, the padding); this module's numpy path and ``frt_rotate`` give the
same bits.

Wire format: ``compress_sign``'s over the rotated vector of P' = round_up(P, 4096) columns — ``BITS_KEY`` (uint8
[P' / 8]) and ``SCALES_KEY`` (float32 [P' / 256]) beside the entries that are not float32 — plus ``ROTATE_KEY``, a
uint64 array of shape (1,) holding the seed.  (A list upload carries the non-float32 entries in order, then the bits,
the scales and the seed.)  All uploads of a round carry the same seed; the aggregator refuses a second one.

Error feedback lives in rotated space: ``residual`` is a flat float32 vector of P', added to the rotated update before
it is encoded.  A residual is valid under its seed only; ``rerotate(residual, old_seed, new_seed)`` converts it (one
more rounding per element).  Use ONE SEED PER JOB when residuals are carried.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .quant_upload import _base_values, _host, _is_f32
from .sign_upload import BITS_KEY, BLOCK, SCALES_KEY, encode_host

ROTATE_KEY = "__rot_seed__"
ROT_BLOCK = 4096  # FRT_BLOCK
_M64 = (1 << 64) - 1
_F32 = np.float32


def padded(P: int) -> int:
    """P' = round_up(P, 4096)."""
    return (int(P) + ROT_BLOCK - 1) // ROT_BLOCK * ROT_BLOCK


def _seed(seed) -> int:
    if isinstance(seed, bool) or not hasattr(seed, "__index__"):
        raise TypeError(f"seed: expected an integer in [0, 2^64), got {type(seed).__name__}")
    s = int(seed)
    if not 0 <= s <= _M64:
        raise ValueError(f"seed: {s} is not in [0, 2^64)")
    return s


def diag_bits(seed: int, n: int) -> np.ndarray:
    """uint8 [n]: d[p] for p < n — bit p % 64 of splitmix64's output for the word p / 64 (include/fedrotate.h)."""
    seed, n = _seed(seed), int(n)
    w = np.arange((n + 63) // 64, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (w + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return np.unpackbits(z.astype("<u8").view(np.uint8), bitorder="little")[:n]


def _fwht(v: np.ndarray) -> np.ndarray:
    """The twelve butterfly stages h = 1 ... 2048 and the scale 2^-6 over float32 [NB, 4096], in place."""
    nb = v.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        h = 1
        while h < ROT_BLOCK:
            w = v.reshape(nb, ROT_BLOCK // (2 * h), 2, h)
            a, b = w[:, :, 0, :].copy(), w[:, :, 1, :]
            w[:, :, 0, :] = a + b
            w[:, :, 1, :] = a - b  # lower minus upper
            h *= 2
        v *= _F32(0.015625)
    return v


def _flip(v: np.ndarray, seed: int) -> None:
    """The diagonal: d[p] xored into the fp32 sign bit, in place."""
    u = v.reshape(-1).view(np.uint32)
    u ^= diag_bits(seed, u.size).astype(np.uint32) << np.uint32(31)


def rotate_host(x, base, seed: int) -> np.ndarray:
    """float32 [P']: frt_rotate on the host — e = x - base (``base`` may be None), the padding +0.0, the diagonal, the
    transform."""
    x = np.ascontiguousarray(x, dtype=_F32).reshape(-1)
    P = x.size
    v = np.zeros(padded(P), dtype=_F32)
    with np.errstate(invalid="ignore", over="ignore"):
        v[:P] = x if base is None else x - np.ascontiguousarray(base, dtype=_F32).reshape(-1)
    if P == 0:
        return v
    _flip(v, seed)
    return _fwht(v.reshape(-1, ROT_BLOCK)).reshape(-1)


def unrotate_host(y, P: int, seed: int) -> np.ndarray:
    """float32 [P]: frt_unrotate on the host — the transform over the P' columns, then the diagonal."""
    P = int(P)
    y = np.ascontiguousarray(y, dtype=_F32).reshape(-1)
    if y.size != padded(P):
        raise ValueError(f"y: {y.size} columns, a rotated row of P={P} has {padded(P)}")
    if P == 0:
        return np.zeros(0, dtype=_F32)
    v = _fwht(y.copy().reshape(-1, ROT_BLOCK)).reshape(-1)
    _flip(v, seed)
    return v[:P].copy()


def rerotate(residual, old_seed: int, new_seed: int):
    """A rotated-space residual of P' columns carried under ``old_seed``, as the residual under ``new_seed``:
    unrotate, then rotate, on the side the residual is on (numpy, or a device tensor).  Both sides give the same
    bits."""
    old_seed, new_seed = _seed(old_seed), _seed(new_seed)
    n = int(residual.shape[0]) if len(residual.shape) == 1 else -1
    if n < 0 or n % ROT_BLOCK or not _is_f32(residual):
        raise ValueError(f"residual: expected a flat float32 vector of a multiple of {ROT_BLOCK} columns, got "
                         f"{getattr(residual, 'dtype', type(residual).__name__)} "
                         f"{tuple(getattr(residual, 'shape', ()))}")
    if isinstance(residual, torch.Tensor) and residual.is_cuda:
        from ... import kernels_rotate as kr

        with torch.cuda.device(residual.device):
            mid = torch.empty(n, dtype=torch.float32, device=residual.device)
            out = torch.empty(n, dtype=torch.float32, device=residual.device)
            if n:
                kr.unrotate(residual.detach().contiguous(), n, old_seed, mid)
                kr.rotate(mid, None, n, new_seed, out)
        return out
    return rotate_host(unrotate_host(np.asarray(_host(residual)), n, old_seed), None, new_seed)


def compress_sign_rotated(state, base, seed: int, residual=None, residual_out: Optional[bool] = None):
    """``(upload, residual_out)``: the scaled sign of the rotation of ``state - base`` (+ ``residual``) over the
    float32 entries.

    ``base``: the weights this round started from, a dict with the state's keys or a list in its order.
    ``seed``: the rotation's 64-bit seed, the same for every executor of a round.
    ``residual``: one flat float32 vector of P' = round_up(P, 4096) in rotated space, on the same side as the state
    (numpy for a host state, a device tensor for a state on a GPU), or None; valid under ``seed`` only (``rerotate``).
    The second result is the flat float32 vector of P' of what this round's encoding leaves behind when
    ``residual_out`` is true (default: when a ``residual`` was given), else None.  A state whose float32 tensors are on
    a GPU is rotated and encoded there (frt_rotate, then fsg_sign_row) and the bits and scales cross to the host in
    one copy.  Both paths give the same bytes."""
    seed = _seed(seed)
    items = list(state.items())
    for name, _ in items:
        if name in (BITS_KEY, SCALES_KEY, ROTATE_KEY):
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
    Pp = padded(P)
    NB = Pp // BLOCK
    want_out = (residual is not None) if residual_out is None else bool(residual_out)
    if residual is not None and (tuple(residual.shape) != (Pp,) or not _is_f32(residual)):
        raise ValueError(f"residual: expected a flat float32 vector of P'={Pp} (rotated space), got "
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
        y = rotate_host(x, L, seed)
        if residual is not None:
            with np.errstate(invalid="ignore", over="ignore"):
                y = y + np.asarray(_host(residual), dtype=np.float32)
        bits, scales, r = encode_host(y)
        if want_out:
            r_out = r
    else:
        from ... import kernels_rotate as kr
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
                r_out = torch.empty(Pp, dtype=torch.float32, device=dev)
            y = torch.empty(Pp, dtype=torch.float32, device=dev)
            kr.rotate(x, L, P, seed, y)
            nbits = NB * (BLOCK // 8)
            buf = torch.empty(nbits + 4 * NB, dtype=torch.uint8, device=dev)
            kg.sign_row(y, None, r_in, Pp, buf[:nbits], buf[nbits:].view(torch.float32), r_out)
            host = buf.cpu().numpy()  # one D2H (synchronises with the launches)
        bits, scales = host[:nbits], host[nbits:].view(np.float32)
    out = {}  # a plain dict, in the state's order: what the aggregator and ingress.loads take without a copy
    f_set = set(f_idx)
    for i, (name, v) in enumerate(items):
        if i not in f_set:
            out[name] = _host(v)
    out[BITS_KEY] = bits
    out[SCALES_KEY] = scales
    out[ROTATE_KEY] = np.array([seed], dtype=np.uint64)
    return out, r_out
