"""Auxo's cohort-clustering features on the device: per-client gradient signatures, their centred and
normalised forms, and the K x K Gram matrix (include/fedcohort.h, fedscale_amd/csrc/cohort_sig.hip).

Reference (examples/auxo): ``AuxoClientMetadata.register_gradient`` (client_metadata.py:10-17) subtracts the
upload from the cohort's model per tensor, concatenates every tensor in state_dict order, keeps the last
``len // 10`` elements and casts them to float16; ``cohort_clustering`` (client_manager.py:208-210) takes the
column mean over the round's K signatures, centres them and L2-normalises the rows for k-means / kNN.

``signature_plan`` maps that concatenation onto the flat layout of ``fedscale_amd.bucket`` (pure Python);
``CohortSignatures`` holds a finished round's [K, D] float16 signatures in HBM and derives the rest lazily.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from .bucket import BucketLayout, round_up

#: the reference's AuxoClientMetadata.grad_ratio (client_metadata.py:8)
GRAD_RATIO = 10


class SignaturePlan:
    """Where the signature's D elements live in a layout's device buffers.

    ``segs``: int64 [nseg, 3] rows (offset in the fp32 bucket, offset in the signature, length) of contiguous
    runs of fp32 elements; ``isegs``: int64 [niseg, 2] rows (side-table index, offset in the signature) of the
    int64 elements inside the tail.  ``N``: elements of the reference's concatenation; ``D``: signature length;
    ``ldd``: row stride of the device matrices (a multiple of 64 float16, so rows start 128-byte aligned)."""

    __slots__ = ("N", "D", "ldd", "segs", "isegs")

    def __init__(self, N: int, D: int, segs: List[Tuple[int, int, int]], isegs: List[Tuple[int, int]]):
        self.N, self.D = int(N), int(D)
        self.ldd = round_up(max(self.D, 1), 64)
        self.segs = np.asarray(segs, dtype=np.int64).reshape(-1, 3)
        self.isegs = np.asarray(isegs, dtype=np.int64).reshape(-1, 2)

    def gather(self, f32: np.ndarray, side: np.ndarray) -> np.ndarray:
        """The D tail elements of a (fp32 bucket, int64 side table) pair as float64, in signature order — the
        host restatement of what the segments select (tests, tools)."""
        out = np.zeros(self.D, dtype=np.float64)
        for src, dst, n in self.segs.tolist():
            out[dst:dst + n] = f32[src:src + n]
        for q, dst in self.isegs.tolist():
            out[dst] = side[q]
        return out


def signature_plan(layout: BucketLayout) -> SignaturePlan:
    """The reference's ``np.concatenate([...])[-val_len:]`` (client_metadata.py:14-16) on ``layout``: the
    concatenation holds all T tensors in state_dict order, N = P_full + Q elements; ``val_len = N // 10``.  When
    N < 10, ``val_len`` is 0 and ``gradient[-0:]`` is the WHOLE vector, so D = N there (kept as the reference
    has it).  The fp32 bucket has no padding between entries, so consecutive fp32 entries merge into one
    segment; each int64 entry inside the tail splits the run."""
    if layout.world != 1:
        raise NotImplementedError(
            f"signature_plan: the layout is shard {layout.rank} of {layout.world}; cohort signatures of a "
            f"parameter-sharded model are not supported (use a whole-model layout)")
    N = layout.P_full + layout.Q
    D = N // GRAD_RATIO
    if D == 0:
        D = N
    t0 = N - D  # first concatenation index inside the signature
    segs: List[Tuple[int, int, int]] = []
    isegs: List[Tuple[int, int]] = []
    c = 0
    for e in layout.entries:
        lo, hi = max(c, t0), c + e.numel
        if lo < hi:
            if e.kind == "f":
                src, dst, n = e.offset + (lo - c), lo - t0, hi - lo
                if segs and segs[-1][0] + segs[-1][2] == src and segs[-1][1] + segs[-1][2] == dst:
                    segs[-1] = (segs[-1][0], segs[-1][1], segs[-1][2] + n)
                else:
                    segs.append((src, dst, n))
            else:
                isegs.extend((e.offset + (i - c), i - t0) for i in range(lo, hi))
        c += e.numel
    return SignaturePlan(N, D, segs, isegs)


# ---- kernel wrappers -----------------------------------------------------------------------------
def _half_matrix(t, name: str, K: int, D: int) -> int:
    import torch

    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.float16:
        raise TypeError(f"{name}: expected a float16 device tensor (the HIP path has no CPU fallback)")
    if t.dim() != 2 or t.shape[0] < K or t.shape[1] < D or t.stride(1) != 1 and t.shape[1] > 1:
        raise ValueError(f"{name}: expected a row-major [>= {K}, >= {D}] matrix, got {tuple(t.shape)}")
    return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]), 1)


def _handle(t) -> int:
    from .state import raw_stream

    return raw_stream(t.device.index)


def signature(x, xi, n: int, last_f32, last_i64, plan: SignaturePlan, sig_out, row0: int = 0):
    """fc_signature: rows [row0, row0 + n) of ``sig_out`` from the first n rows of the staging area (x, xi; device
    tensors or the staging's pinned mirror).  Asynchronous on the current stream of sig_out's device."""
    from . import _native_cohort as nc

    if n <= 0:
        return
    ldd = _half_matrix(sig_out, "sig_out", row0 + n, plan.D)
    if x.shape[0] < n or (plan.isegs.size and xi.shape[0] < n):
        raise ValueError(f"signature: {n} rows, the staging area holds {x.shape[0]}")
    segs, isegs = np.ascontiguousarray(plan.segs), np.ascontiguousarray(plan.isegs)
    nc.call("fc_signature", x.data_ptr(), int(x.stride(0)), int(n), last_f32.data_ptr(),
            xi.data_ptr() if isegs.size else None, int(xi.stride(0)) if isegs.size else 1,
            last_i64.data_ptr() if isegs.size else None, segs.ctypes.data, len(segs), isegs.ctypes.data, len(isegs),
            sig_out.data_ptr() + row0 * ldd * 2, ldd, _handle(sig_out))


def center(sig, K: int, D: int):
    """fc_center -> (avg16 [D], centered [K, ldd], sumsq [K] fp64) of sig[:K, :D]."""
    import torch

    from . import _native_cohort as nc

    ldd = _half_matrix(sig, "sig", K, D)
    dev = sig.device
    avg = torch.empty(round_up(max(D, 1), 8), dtype=torch.float16, device=dev)
    cen = torch.empty(K, ldd, dtype=torch.float16, device=dev)
    sumsq = torch.empty(K, dtype=torch.float64, device=dev)
    ws = torch.empty(max(1, nc.load().fc_center_workspace_bytes(K, D) // 8), dtype=torch.float64, device=dev)
    nc.call("fc_center", sig.data_ptr(), ldd, K, D, avg.data_ptr(), cen.data_ptr(), sumsq.data_ptr(), ws.data_ptr(),
            _handle(sig))
    return avg[:D], cen, sumsq


def normalize(cen, K: int, D: int, norms):
    """fc_normalize -> normalized [K, ldd] float16."""
    import torch

    from . import _native_cohort as nc

    ldd = _half_matrix(cen, "centered", K, D)
    if norms.dtype != torch.float64 or norms.device != cen.device or norms.numel() < K or not norms.is_contiguous():
        raise TypeError("norms: expected K contiguous float64 values on the matrix's device")
    out = torch.empty_like(cen)
    nc.call("fc_normalize", cen.data_ptr(), ldd, K, D, norms.data_ptr(), out.data_ptr(), _handle(cen))
    return out


def gram(c, K: Optional[int] = None, D: Optional[int] = None):
    """fc_gram: the K x K fp32 matrix C * C^T of a float16 device matrix (its first K rows and D columns)."""
    import torch

    from . import _native_cohort as nc

    K = c.shape[0] if K is None else K
    D = c.shape[1] if D is None else D
    ldd = _half_matrix(c, "c", K, D)
    if K > nc.GRAM_MAX_K:
        raise ValueError(f"gram: K={K} rows, the kernel takes at most {nc.GRAM_MAX_K}")
    out = torch.empty(K, K, dtype=torch.float32, device=c.device)
    ws = torch.empty(max(4, nc.load().fc_gram_workspace_bytes(K, D) // 4), dtype=torch.float32, device=c.device)
    nc.call("fc_gram", c.data_ptr(), ldd, K, D, out.data_ptr(), ws.data_ptr(), _handle(c))
    return out


class CohortSignatures:
    """The K signatures of one cohort round, device-resident ([K, ldd] float16 in arrival order), with what
    client_manager.py:208-216 derives from them.  Every result is computed once, on first use, on the owning
    adapter's stream; the accessors return device tensors the caller's current stream is ordered after.

    Lifetime: the tensors belong to this object (they are views of its buffers, not copies) and were allocated on
    the adapter's stream.  Each accessor records the caller's current stream on what it returns
    (``Tensor.record_stream``), so the blocks are not reused while work queued on that stream up to the moment the
    object is dropped may still read them; a caller that hands them to yet another stream records that stream itself.

        sigs = aggregator.cohort_signatures[cohort_id]
        centered_grad, norm_grad = sigs.features()      # numpy float16 [K, D], as client_manager.py:214-216 uses
        cos = sigs.cosine()                             # K x K, from the Gram: 4 MB instead of K x D
    """

    def __init__(self, sig, K: int, D: int, client_ids=(), dstream=None):
        self._sig, self.K, self.D = sig, int(K), int(D)
        self.client_ids = list(client_ids)
        self.dstream = dstream
        self._center = self._norms = self._normalized = self._gram = None

    def _on(self):
        from .bucket import _NULL_CTX

        return _NULL_CTX if self.dstream is None else self.dstream.joined()

    def _give(self, t):
        """``t`` for the caller: its current stream is recorded as a user of t's memory (see the class docstring)."""
        import torch

        if self.dstream is not None:
            cur = torch.cuda.current_stream(t.device)
            if cur != self.dstream.stream:
                t.record_stream(cur)
        return t

    def raw(self):
        """[K, D] float16: register_gradient's output per client (client_metadata.py:16)."""
        with self._on():  # (the join: the caller's stream waits for the round's signature launches)
            t = self._sig[:self.K, :self.D]
        return self._give(t)

    def _centered(self):
        if self._center is None:
            self._center = center(self._sig, self.K, self.D)
        return self._center

    def mean(self):
        """[D] float16: np.mean(gradient_list, axis=0) (client_manager.py:208)."""
        with self._on():
            t = self._centered()[0]
        return self._give(t)

    def centered(self):
        """[K, D] float16: gradient_list - avg_grad (client_manager.py:209)."""
        with self._on():
            t = self._centered()[1][:self.K, :self.D]
        return self._give(t)

    def sumsq(self):
        """[K] float64: per-row sums of squares of ``centered()``."""
        with self._on():
            t = self._centered()[2]
        return self._give(t)

    def norms(self):
        """[K] float64: L2 norms of the rows of ``centered()``."""
        import torch

        with self._on():
            if self._norms is None:
                self._norms = torch.sqrt(self._centered()[2])
        return self._give(self._norms)

    def normalized(self):
        """[K, D] float16: the rows of ``centered()`` divided by their norms (client_manager.py:210; an all-zero
        row stays zero)."""
        with self._on():
            if self._normalized is None:
                self.norms()
                self._normalized = normalize(self._centered()[1], self.K, self.D, self._norms)
        return self._give(self._normalized[:self.K, :self.D])

    def gram(self):
        """[K, K] fp32: centered * centered^T (f16 matrix unit, fp32 accumulation)."""
        with self._on():
            if self._gram is None:
                self._gram = gram(self._centered()[1], self.K, self.D)
        return self._give(self._gram)

    # ---- host helpers --------------------------------------------------------------------------
    @staticmethod
    def _host(t) -> np.ndarray:
        return t.cpu().numpy()  # (the accessors have ordered the caller's stream after the adapter's)

    def cosine(self) -> np.ndarray:
        """K x K float64 cosine similarities of the centred signatures (Gram / norms; a zero row has norm 1)."""
        g = self._host(self.gram()).astype(np.float64)
        n = self._host(self.norms()).copy()
        n[n == 0.0] = 1.0
        return g / np.outer(n, n)

    def pairwise_sqdist(self) -> np.ndarray:
        """K x K float64 squared Euclidean distances of the centred signatures: |c_i|^2 + |c_j|^2 - 2 G_ij
        (clipped at 0; the diagonal is 0)."""
        g = self._host(self.gram()).astype(np.float64)
        s = self._host(self.sumsq())
        d = np.maximum(s[:, None] + s[None, :] - 2.0 * g, 0.0)
        np.fill_diagonal(d, 0.0)
        return d

    def features(self):
        """(centered_grad, norm_grad) as numpy float16 [K, D]: what ``cohort_clustering`` hands to
        ``update_mainR`` and ``knn_update_subR`` (client_manager.py:214-216)."""
        return self._host(self.centered()), self._host(self.normalized())
