"""A round whose client uploads arrive and are staged as top-k sparse deltas and are chained in fp32.

What an executor uploads is the k largest-magnitude entries of its update ``e = x - L`` against the model ``L`` it
was sent for this round (plus, with error feedback, what its earlier rounds dropped), as (index, value) pairs over
the concatenated fp32 bucket (fedscale_amd/cloud/execution/sparse_upload.py; include/fedsparse.h states the rule).
``SparseStaging`` holds [capacity, ldk] rows of indices and of values — 8 bytes per kept entry on the wire, per
staged client and per reduction pass — with each row's tile offsets and validity flag computed when it is staged,
and ``SparseRound`` is what ``TorchModelAdapter._apply_round`` and the aggregator mixins use of ``DeviceRound``:
``fs_reduce`` chains the pairs in arrival order, a column a row does not name is not touched by it, and the round is
closed by ``fcl_finish`` (include/fedclip.h) against the round's snapshot of ``L``: new model = L + chain / K.  The
int64 side table travels and reduces as in ``DeviceRound``.

A malformed row (indices not strictly increasing, or one >= P) raises at ``put`` when it arrives in host memory.  A
row of device tensors is checked on the device without a synchronisation (``fs_check_rows``): a flagged row
contributes nothing to the chain, the mean still divides by K, and ``SparseRound.rejected()`` counts such rows.

Opt-in (``TorchModelAdapter(upload_topk=density)``); FedAvg and — as the mean followed by the existing YoGi step —
fed-yogi, fed-adam, fed-adagrad or fed-avgm (the mean, then the server step).  FedBuff (a stale client's base is not this round's ``L``), q-FedAvg, 16-bit uploads, MXFP8 uploads,
sharded models, client-sharded ranks, cohort signatures, clip and trim are refused.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import kernels as kx
from . import kernels_clip as kc
from . import kernels_sparse as ks
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout
from .cloud.execution.sparse_upload import IDX_KEY, VAL_KEY, count_of
from .round import on_stream
from .state import DeviceStream

_I64, _U32, _F32 = np.dtype(np.int64), np.dtype(np.uint32), np.dtype(np.float32)
_IDX_TORCH = tuple(t for t in (torch.int32, getattr(torch, "uint32", None)) if t is not None)


def check_density(density) -> float:
    """``density`` as a float when it is a fraction in (0, 1]; ValueError otherwise."""
    try:
        d = float(density)
    except (TypeError, ValueError):
        raise ValueError(f"upload_topk {density!r}: expected a density in (0, 1]") from None
    if isinstance(density, bool) or not 0.0 < d <= 1.0:
        raise ValueError(f"upload_topk {density!r}: expected a density in (0, 1]")
    return d


def refuse(what: str, density=None) -> NotImplementedError:
    """The error of a combination the sparse-delta upload path does not take."""
    return NotImplementedError(f"upload_topk={density!r} combined with {what} is not supported: top-k sparse delta "
                               f"uploads take FedAvg and fed-yogi rounds of one whole model on one device")


def default_capacity_topk(layout: BucketLayout, K: int, kmax: int, device, budget_fraction: float = 0.5) -> int:
    """Clients per chunk, from rows of 8 bytes per pair plus their tile offsets: all K when they fit in
    ``budget_fraction`` of the free HBM."""
    free, _ = torch.cuda.mem_get_info(device)
    per_client = ks.row_stride(kmax) * 8 + ks.boundaries(layout.P) * 4 + layout.ldq * 8 + 8
    return min(max(1, int(free * budget_fraction) // max(1, per_client)), max(1, K))


def upload_plan_topk(layout: BucketLayout, update, kmax: int, device=None):
    """Validate one sparse upload against the layout (no GPU needed for host entries): ``(side, idx, val)`` with
    side a list of (entry, value) for the int64 entries in layout order, and idx / val either C-contiguous host arrays
    (uint32 / float32 [nnz]) or tensors on ``device``.  Host arrays are checked in full — dtype, strictly increasing,
    below P, nnz <= kmax — and TypeError / ValueError name the problem; device tensors are checked for dtype and
    size here and for their contents by fs_check_rows."""
    n_side = len(layout.i_entries)
    if type(update) is dict:
        if IDX_KEY not in update or VAL_KEY not in update:
            raise TypeError(f"{IDX_KEY} / {VAL_KEY}: the upload carries no index or value array (upload_topk; a dense "
                            f"float32 upload is not a sparse one: see sparse_upload.compress_topk)")
        idx, val = update[IDX_KEY], update[VAL_KEY]
        names = [k for k in update if k not in (IDX_KEY, VAL_KEY)]
        want = [e.name for e in layout.i_entries]
        if names != want:
            raise ValueError(f"update names the entries {names}, a sparse upload carries the non-float32 entries "
                             f"{want} beside {IDX_KEY} and {VAL_KEY}")
        values = [update[k] for k in names]
    else:
        values = list(update)
        if len(values) != n_side + 2:
            raise ValueError(f"update has {len(values)} arrays, a sparse upload has the model's {n_side} non-float32 "
                             f"entries, then the index array, then the value array (upload_topk)")
        idx, val = values[-2], values[-1]
        values = values[:-2]

    side = []
    for e, v in zip(layout.i_entries, values):
        if isinstance(v, torch.Tensor):
            if v.dtype != torch.int64:
                raise TypeError(f"{e.name}: dtype {v.dtype}, the entry is int64")
            v = v.detach()
            v = v if device is not None and v.device == device else v.cpu().numpy()
        else:
            v = v if type(v) is np.ndarray else np.asarray(v)
            if v.dtype != _I64:
                raise TypeError(f"{e.name}: dtype {v.dtype}, the entry is int64")
        if tuple(v.shape) != e.shape:
            raise TypeError(f"{e.name}: shape {tuple(v.shape)} != model shape {e.shape}")
        side.append((e, v))

    if isinstance(idx, torch.Tensor) or isinstance(val, torch.Tensor):
        if not (isinstance(idx, torch.Tensor) and isinstance(val, torch.Tensor)):
            raise TypeError(f"{IDX_KEY} / {VAL_KEY}: one is a tensor and the other is not")
        if idx.dtype not in _IDX_TORCH:
            raise TypeError(f"{IDX_KEY}: dtype {idx.dtype}, this staging takes uint32 (or int32) indices")
        if val.dtype != torch.float32:
            raise TypeError(f"{VAL_KEY}: dtype {val.dtype}, this staging takes float32 values")
        if idx.dim() != 1 or val.dim() != 1 or idx.shape != val.shape:
            raise ValueError(f"{IDX_KEY} / {VAL_KEY}: shapes {tuple(idx.shape)} / {tuple(val.shape)}, expected two "
                             f"flat arrays of one length")
        if idx.shape[0] > kmax:
            raise ValueError(f"{IDX_KEY}: nnz={idx.shape[0]} > kmax={kmax}, the most pairs the declared density keeps")
        idx, val = idx.detach(), val.detach()
        if device is not None and idx.device == device and val.device == device:
            return side, idx.contiguous().view(torch.int32), val.contiguous()
        idx, val = idx.cpu().contiguous().view(torch.int32).numpy().view(np.uint32), val.cpu().contiguous().numpy()
    idx = idx if type(idx) is np.ndarray else np.asarray(idx)
    val = val if type(val) is np.ndarray else np.asarray(val)
    if idx.dtype != _U32:
        raise TypeError(f"{IDX_KEY}: dtype {idx.dtype}, this staging takes uint32 indices (see "
                        f"sparse_upload.compress_topk)")
    if val.dtype != _F32:
        raise TypeError(f"{VAL_KEY}: dtype {val.dtype}, this staging takes float32 values")
    if idx.ndim != 1 or val.ndim != 1 or idx.shape != val.shape:
        raise ValueError(f"{IDX_KEY} / {VAL_KEY}: shapes {idx.shape} / {val.shape}, expected two flat arrays of one "
                         f"length")
    n = idx.shape[0]
    if n > kmax:
        raise ValueError(f"{IDX_KEY}: nnz={n} > kmax={kmax}, the most pairs the declared density keeps")
    if n:
        if n > 1:
            step = idx[1:] <= idx[:-1]
            if step.any():
                j = int(np.argmax(step))
                what = "a duplicate index" if idx[j + 1] == idx[j] else "indices not sorted"
                raise ValueError(f"{IDX_KEY}: {what} at position {j + 1} ({idx[j]} then {idx[j + 1]}): indices must "
                                 f"be strictly increasing")
        if int(idx[-1]) >= layout.P:
            raise ValueError(f"{IDX_KEY}: index {int(idx[-1])} >= P={layout.P} columns")
    return (side, idx if idx.flags.c_contiguous else np.ascontiguousarray(idx),
            val if val.flags.c_contiguous else np.ascontiguousarray(val))


class SparseStaging:
    """Device staging area for up to ``capacity`` sparse client uploads of at most ``kmax`` pairs: ``idx``
    [capacity, ldk] (uint32 bits in an int32 tensor), ``val`` [capacity, ldk] float32, ``nnz`` [capacity] int32,
    ``offsets`` [boundaries, capacity] int32 and ``flags`` [capacity] int32 (both written at ``put`` on the staging's
    stream), ``xi`` [capacity, ldq] int64.  Host uploads cross PCIe from one pinned row per array (a ring of two);
    an event per pinned row guards its reuse."""

    def __init__(self, layout: BucketLayout, device, capacity: int, density: float,
                 dstream: Optional[DeviceStream] = None, ring: int = 2):
        self.density = check_density(density)
        if layout.world != 1:
            raise refuse("a parameter-sharded layout", self.density)
        if layout.P > 0x7FFFFFFF:
            raise refuse(f"a bucket of {layout.P} columns (indices are below 2^31)", self.density)
        self.layout, self.device, self.dstream = layout, torch.device(device), dstream
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.capacity = int(capacity)
        self.side_scratch = None  # (int64, float64) side-table sums of a round, reused
        self.kmax = count_of(self.density, layout.P) if layout.P else 0
        self.ldk = ks.row_stride(self.kmax)
        self.nb = ks.boundaries(layout.P)
        with self._on():
            self.idx = torch.zeros(self.capacity, self.ldk, dtype=torch.int32, device=self.device)
            self.val = torch.zeros(self.capacity, self.ldk, dtype=torch.float32, device=self.device)
            self.nnz = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
            self.offsets = torch.zeros(self.nb, self.capacity, dtype=torch.int32, device=self.device)
            self.flags = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
            self.xi = torch.zeros(self.capacity, layout.ldq, dtype=torch.int64, device=self.device)
        self._ring, self._ring_n, self._next = [], ring, 0

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def _stream(self):
        return self.dstream.stream if self.dstream is not None else torch.cuda.current_stream(self._dev_index)

    def index_rows(self, slot: int, n: int = 1):
        """Tile offsets and validity flags of the staged rows [slot, slot + n), on the current stream."""
        if n > 0 and self.layout.P > 0:
            ks.row_offsets(self.idx, self.nnz, n, self.layout.P, self.offsets, row0=slot)
            for k0 in range(0, n, ks.CHECK_ROWS_MAX):  # fs_check_rows takes that many rows per call
                ks.check_rows(self.idx, self.nnz, min(ks.CHECK_ROWS_MAX, n - k0), self.layout.P, self.flags,
                              row0=slot + k0)

    def put(self, slot: int, update):
        """Stage one upload (dict, or list of the non-float32 entries, then indices, then values) into ``slot``;
        errors surface here, synchronously."""
        lay = self.layout
        side, idx, val = upload_plan_topk(lay, update, self.kmax, self.device)
        if not 0 <= slot < self.capacity:
            raise IndexError(f"slot {slot} of {self.capacity}")
        n = int(idx.shape[0])
        if isinstance(idx, torch.Tensor) and all(isinstance(v, torch.Tensor) for _, v in side):
            with self._on():
                if self.dstream is not None:
                    self.dstream.wait_caller()  # the caller's device tensors
                with torch.cuda.stream(self._stream()):
                    for e, v in side:
                        self.xi[slot, e.offset:e.offset + e.numel].copy_(v.reshape(-1), non_blocking=True)
                    if n:
                        self.idx[slot, :n].copy_(idx, non_blocking=True)
                        self.val[slot, :n].copy_(val, non_blocking=True)
                    self.nnz[slot:slot + 1].fill_(n)
                    self.index_rows(slot)
            return
        if isinstance(idx, torch.Tensor):  # device pairs beside host side entries: everything through the host
            idx, val = idx.cpu().numpy().view(np.uint32), val.cpu().numpy()
        if not self._ring:
            for _ in range(self._ring_n):
                hx = torch.zeros(self.ldk, dtype=torch.int32).pin_memory()
                hv = torch.zeros(self.ldk, dtype=torch.float32).pin_memory()
                hi = torch.zeros(lay.ldq, dtype=torch.int64).pin_memory()
                self._ring.append([hx, hv, hi, hx.numpy().view(np.uint32), hv.numpy(), hi.numpy(), None])
        r = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        if r[6] is not None:
            r[6].synchronize()  # the previous H2Ds out of these pinned rows have completed
        for e, v in side:
            if isinstance(v, torch.Tensor):  # a device entry among host ones
                v = v.cpu().numpy()
            r[5][e.offset:e.offset + e.numel] = v.reshape(-1)
        r[3][:n] = idx
        r[4][:n] = val
        with self._on():
            st = self._stream()
            with torch.cuda.stream(st):
                if n:
                    self.idx[slot, :n].copy_(r[0][:n], non_blocking=True)
                    self.val[slot, :n].copy_(r[1][:n], non_blocking=True)
                if lay.Q:
                    self.xi[slot, :lay.Q].copy_(r[2][:lay.Q], non_blocking=True)
                self.nnz[slot:slot + 1].fill_(n)
                self.index_rows(slot)
            if r[6] is None:
                r[6] = torch.cuda.Event()
            r[6].record(st)


class SparseRound:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, over a ``SparseStaging``."""

    policy = "fedavg"
    cg = None        # never client-sharded
    head = 0         # no head launch, no small-round mirror path
    sig_plan = None  # no cohort signatures

    def __init__(self, layout: BucketLayout, device, K: int, policy: str, *, staging: SparseStaging,
                 last_f32: torch.Tensor, capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None):
        if policy != "fedavg":
            raise refuse(f"a {policy} round", staging.density)
        if K < 1:
            raise ValueError("a round needs K >= 1 client results")
        self.layout, self.device, self.K = layout, torch.device(device), int(K)
        self.dstream, self.staging, self.last_f32 = dstream, staging, last_f32
        self.upload_topk = staging.density
        self.cap = min(staging.capacity, capacity or staging.capacity)
        self.n = self.slot = self.chunks_done = 0
        with self._on():
            if staging.side_scratch is None:
                staging.side_scratch = (torch.empty(layout.ldq, dtype=torch.int64, device=self.device),
                                        torch.empty(layout.ldq, dtype=torch.float64, device=self.device))
            self.chain = torch.zeros(layout.ld, dtype=torch.float32, device=self.device)
            self._rejected = torch.zeros((), dtype=torch.int64, device=self.device)
        self.acc_i, self.acc_d = staging.side_scratch

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def add(self, update, *, weight: Optional[float] = None, loss=None, learning_rate=None, q=None):
        """Stage one arriving sparse upload (in arrival order)."""
        if self.n >= self.K:
            raise RuntimeError(f"round already has its K={self.K} results")
        if self.slot == self.cap:
            self._fold_chunk()
        self.staging.put(self.slot, update)
        self.slot += 1
        self.n += 1

    @on_stream
    def adopt_resident(self, n: int):
        """Measurement hook, as ``DeviceRound.adopt_resident``: take ``n`` arrivals whose pairs and counts are ALREADY
        in the staging slots [slot, slot + n), written there on the device; their offsets and flags are computed
        here (tools/sparse_reduce_measure.py)."""
        if n < 0 or self.slot + n > self.cap or self.n + n > self.K:
            raise ValueError(f"adopt_resident: {n} arrivals do not fit (slot {self.slot} of {self.cap}, "
                             f"{self.n} of K={self.K})")
        self.staging.index_rows(self.slot, n)
        self.slot += n
        self.n += n

    def _reduce_chunk(self):
        """The staged chunk's pairs onto the chain (the same chain across chunks), and its side-table sums."""
        L, st, n = self.layout, self.staging, self.slot
        first = self.chunks_done == 0
        if n > 0 and L.P > 0:
            ks.reduce_sparse(st.idx, st.val, st.nnz, st.offsets, st.flags, n, L.P, self.chain,
                             acc_in=None if first else self.chain)
            self._rejected += (st.flags[:n] != 0).sum()
        kx.side_accumulate(st.xi, n, L.Q, 0, acc_i=self.acc_i, acc_d=self.acc_d, accumulate=not first)
        self.chunks_done += 1
        self.slot = 0

    @on_stream
    def _fold_chunk(self):
        """Fold the staged chunk into the running chain (not the last chunk of the round)."""
        self._reduce_chunk()

    def _check_complete(self):
        if self.n != self.K:
            raise RuntimeError(f"finalize with {self.n} of K={self.K} results")

    def rejected(self) -> int:
        """Rows of the chunks reduced so far that fs_check_rows flagged, read from the device now on the round's own
        stream — the one the counter is cleared and added to on — which it synchronises with.  A flagged row
        contributed nothing; the mean still divides by K."""
        with self._on():
            return int(self._rejected.item())

    @on_stream
    def finalize_mean(self, denom32: float, denom64: float, *, out: torch.Tensor, cur_side: torch.Tensor,
                      model_side: Optional[torch.Tensor] = None, yogi: Optional[dict] = None,
                      mirror: Optional[torch.Tensor] = None):
        """Reduce the last chunk, then ``out`` <- the round's starting model plus the mean delta (fcl_finish, no
        noise); the side table as ``DeviceRound.finalize_mean`` (fed-yogi rounds take ``out`` as the mean, then the
        existing fa_yogi_step)."""
        if yogi is not None:
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)", self.upload_topk)
        self._check_complete()
        den = float(np.float32(self.K))
        if float(denom32) != den:
            raise ValueError(f"a sparse-delta round divides by its client count K={self.K}, not {denom32}")
        L = self.layout
        self._reduce_chunk()
        kc.finish(self.chain, self.last_f32, L.P, den, out, mirror=mirror)
        kx.side_close(L.Q, 0, denom64, acc_i=self.acc_i, acc_d=self.acc_d, cur=cur_side, model=model_side)
