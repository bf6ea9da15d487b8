"""A round whose client uploads arrive and are staged in 16 bits (float16 or bfloat16) and are reduced in fp32.

``HalfStaging`` is ``ClientStaging`` with [capacity, ld] rows of 2-byte elements — half the PCIe bytes per upload,
half the HBM per staged client — and ``HalfRound`` is what ``TorchModelAdapter._apply_round`` and the aggregator
mixins use of ``DeviceRound``, reduced by ``fh_reduce`` (include/fedhalf.h): every element is widened exactly to
fp32 and takes the adds of ``fa_reduce`` in arrival order, so the result is the float32 path's on the widened
uploads, bit for bit.  This is NOT what the reference's numpy lines would do with float16 arrays
(aggregator.py:500-507 would chain in float16).  The int64 side table travels and reduces as in ``DeviceRound``.

Opt-in (``TorchModelAdapter(upload_dtype=...)``); FedAvg, FedBuff and — as the mean followed by the existing YoGi
step — fed-yogi, fed-adam, fed-adagrad or fed-avgm (the mean, then the server step).  q-FedAvg, sharded models, client-sharded ranks and cohort signatures are refused.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import kernels as kx
from . import kernels_half as kh
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout, default_pack_workers
from .round import on_stream
from .state import DeviceStream

_I64 = np.dtype(np.int64)
_F16, _U16, _I16 = np.dtype(np.float16), np.dtype(np.uint16), np.dtype(np.int16)


def refuse(what: str, dtype) -> NotImplementedError:
    """The error of a combination the 16-bit upload path does not take."""
    return NotImplementedError(f"upload_dtype={dtype!r} combined with {what} is not supported: 16-bit uploads "
                               f"take FedAvg, FedBuff and fed-yogi rounds of one whole model on one device")


def default_capacity16(layout: BucketLayout, K: int, device, budget_fraction: float = 0.5) -> int:
    """Clients per chunk, from 2-byte rows: all K when they fit in ``budget_fraction`` of the free HBM."""
    free, _ = torch.cuda.mem_get_info(device)
    per_client = layout.ld * 2 + layout.ldq * 8
    return min(max(1, int(free * budget_fraction) // max(1, per_client)), max(1, K))


def upload_plan16(layout: BucketLayout, update, dtype_name: str, device=None):
    """Validate one 16-bit upload against the layout (no GPU needed for host entries): a list, in layout order, of
    (entry, value) with value a C-contiguous host array (float16 / 16-bit integers holding bfloat16 bits / int64)
    or a tensor on ``device``.  TypeError names the entry whose dtype or shape does not fit — a float32 array
    included: the staging holds 16-bit rows, and a silent cast would hide a misconfigured executor."""
    tdt = kh.row_dtype(dtype_name)[0]
    values = layout.values_of(update)
    plan = []
    for e in layout.entries:
        v = values[e.index]
        if isinstance(v, torch.Tensor):
            want = tdt if e.kind == "f" else torch.int64
            if v.dtype != want:
                raise TypeError(f"{e.name}: dtype {v.dtype}, this staging takes {want} for the entry "
                                f"(upload_dtype={dtype_name})")
            if tuple(v.shape) != e.shape:
                raise TypeError(f"{e.name}: shape {tuple(v.shape)} != model shape {e.shape}")
            v = v.detach()
            if device is not None and v.device == device:
                plan.append((e, v if v.is_contiguous() else v.contiguous()))
                continue
            v = v.cpu().contiguous()
            v = (v.view(torch.int16) if e.kind == "f" else v).numpy()
        else:
            v = v if type(v) is np.ndarray else np.asarray(v)
            if e.kind == "i":
                ok, takes = v.dtype == _I64, "int64"
            elif dtype_name == "float16":
                ok, takes = v.dtype == _F16, "float16"
            else:
                ok, takes = v.dtype in (_U16, _I16), "uint16 / int16 arrays of bfloat16 bits"
            if not ok:
                raise TypeError(f"{e.name}: dtype {v.dtype}, this staging takes {takes} for the entry "
                                f"(upload_dtype={dtype_name}; see half_upload.compress_update)")
            if v.shape != e.shape:
                raise TypeError(f"{e.name}: shape {tuple(v.shape)} != model shape {e.shape}")
            if not v.flags.c_contiguous:
                v = np.ascontiguousarray(v)
        plan.append((e, v))
    return plan


class HalfStaging:
    """Device staging area for up to ``capacity`` 16-bit client uploads: ``x16`` [capacity, ld] float16 or bfloat16,
    ``xi`` [capacity, ldq] int64.  Host uploads are gathered into one pinned 16-bit row (a ring of two) by
    ``fa_host_gather`` and cross PCIe in one H2D on the staging's stream; an event per pinned row guards its reuse.
    (ClientStaging's bulk mirror, zero-copy small rounds, HostRow and RegisteredUpload have no 16-bit form.)"""

    def __init__(self, layout: BucketLayout, device, capacity: int, dtype, dstream: Optional[DeviceStream] = None,
                 ring: int = 2, pack_workers: Optional[int] = None):
        self.torch_dtype, self.code = kh.row_dtype(dtype)
        self.dtype = "float16" if self.torch_dtype == torch.float16 else "bfloat16"
        if layout.world != 1:
            raise refuse("a parameter-sharded layout", self.dtype)
        self.layout, self.device, self.dstream = layout, torch.device(device), dstream
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.capacity = int(capacity)
        self.pack_workers = pack_workers or default_pack_workers()
        self.side_scratch = None  # (int64, float64) side-table sums of a round, reused
        with self._on():
            self.x16 = torch.zeros(self.capacity, layout.ld, dtype=self.torch_dtype, device=self.device)
            self.xi = torch.zeros(self.capacity, layout.ldq, dtype=torch.int64, device=self.device)
        self._x16_bits = self.x16.view(torch.int16)  # the H2D's destination (pinned rows are int16)
        self._ring, self._ring_n, self._next = [], ring, 0
        # fp32 entries' places in a row, in bytes (static half of the gather)
        self._f_offs = np.asarray([2 * e.offset for e in layout.f_entries if e.numel], dtype=np.int64)
        self._f_sizes = np.asarray([2 * e.numel for e in layout.f_entries if e.numel], dtype=np.int64)

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def _stream(self):
        return self.dstream.stream if self.dstream is not None else torch.cuda.current_stream(self._dev_index)

    def put(self, slot: int, update):
        """Stage one upload (dict or list in layout order) into ``slot``; errors surface here, synchronously."""
        lay = self.layout
        plan = upload_plan16(lay, update, self.dtype, self.device)
        if not 0 <= slot < self.capacity:
            raise IndexError(f"slot {slot} of {self.capacity}")
        if plan and all(isinstance(v, torch.Tensor) for _, v in plan):
            with self._on():
                if self.dstream is not None:
                    self.dstream.wait_caller()  # the caller's device tensors
                for e, v in plan:
                    dst = self.x16[slot] if e.kind == "f" else self.xi[slot]
                    dst[e.offset:e.offset + e.numel].copy_(v.reshape(-1), non_blocking=True)
            return
        if not self._ring:
            for _ in range(self._ring_n):
                h16 = torch.zeros(lay.ld, dtype=torch.int16).pin_memory()
                hi = torch.zeros(lay.ldq, dtype=torch.int64).pin_memory()
                self._ring.append([h16, hi, h16.numpy(), hi.numpy(), None])
        r = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        if r[4] is not None:
            r[4].synchronize()  # the previous H2D out of this pinned row has completed
        ptrs, keep = [], []
        for e, v in plan:
            if isinstance(v, torch.Tensor):  # a device entry among host ones
                v = v.cpu()
                v = (v.view(torch.int16) if e.kind == "f" else v).numpy()
            if e.kind == "i":
                r[3][e.offset:e.offset + e.numel] = v.reshape(-1)
            elif e.numel:
                keep.append(v)
                ptrs.append(v.__array_interface__["data"][0])
        if ptrs:
            from . import _native

            ps = np.asarray(ptrs, dtype=np.uint64)
            _native.call("fa_host_gather", r[2].__array_interface__["data"][0], ps.ctypes.data,
                         self._f_offs.ctypes.data, self._f_sizes.ctypes.data, len(ptrs), int(self.pack_workers))
        del keep
        with self._on():
            st = self._stream()
            with torch.cuda.stream(st):
                if lay.P:
                    self._x16_bits[slot, :lay.P].copy_(r[0][:lay.P], non_blocking=True)
                if lay.Q:
                    self.xi[slot, :lay.Q].copy_(r[1][:lay.Q], non_blocking=True)
            if r[4] is None:
                r[4] = torch.cuda.Event()
            r[4].record(st)


class HalfRound:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, over a ``HalfStaging``."""

    def __init__(self, layout: BucketLayout, device, K: int, policy: str, *, staging: HalfStaging,
                 capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None):
        if policy not in ("fedavg", "fedbuff"):
            raise refuse(f"a {policy} round", staging.dtype)
        if K < 1:
            raise ValueError("a round needs K >= 1 client results")
        self.layout, self.device, self.K, self.policy = layout, torch.device(device), int(K), policy
        self.dstream, self.staging = dstream, staging
        self.upload_dtype = staging.dtype
        self.cap = min(staging.capacity, capacity or staging.capacity)
        self.n = self.slot = self.chunks_done = 0
        self.acc = None
        if staging.side_scratch is None:
            with self._on():
                staging.side_scratch = (torch.empty(layout.ldq, dtype=torch.int64, device=self.device),
                                        torch.empty(layout.ldq, dtype=torch.float64, device=self.device))
        self.acc_i, self.acc_d = staging.side_scratch
        self._w32 = np.zeros(self.cap, dtype=np.float32)
        self._w64 = np.zeros(self.cap, dtype=np.float64)

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def add(self, update, *, weight: Optional[float] = None, loss=None, learning_rate=None, q=None):
        """Stage one arriving 16-bit upload (in arrival order)."""
        if self.n >= self.K:
            raise RuntimeError(f"round already has its K={self.K} results")
        if self.slot == self.cap:
            self._fold_chunk()
        self.staging.put(self.slot, update)
        if self.policy == "fedbuff":
            self._w32[self.slot] = np.float32(weight)  # fp32 array * Python float: scalar rounds to fp32
            self._w64[self.slot] = float(weight)       # int64 array * Python float: float64
        self.slot += 1
        self.n += 1

    def _chunk_weights(self):
        if self.policy != "fedbuff":
            return None, None
        n = self.slot
        a32 = torch.from_numpy(self._w32[:n].copy()).to(self.device, non_blocking=True)
        a64 = torch.from_numpy(self._w64[:n].copy()).to(self.device, non_blocking=True)
        return a32, a64

    @on_stream
    def _fold_chunk(self):
        """Fold the staged chunk into the running fp32 chain (not the last chunk of the round)."""
        L, st, n = self.layout, self.staging, self.slot
        first = self.chunks_done == 0
        if self.acc is None:
            self.acc = torch.zeros(L.ld, dtype=torch.float32, device=self.device)
        a32, a64 = self._chunk_weights()
        kh.reduce16(st.x16, n, L.P, self.acc, a=a32, acc_in=None if first else self.acc)
        kx.side_accumulate(st.xi, n, L.Q, 0 if self.policy == "fedavg" else 1, w=a64, acc_i=self.acc_i,
                           acc_d=self.acc_d, accumulate=not first)
        self.chunks_done += 1
        self.slot = 0

    def _check_complete(self):
        if self.n != self.K:
            raise RuntimeError(f"finalize with {self.n} of K={self.K} results")

    @on_stream
    def finalize_mean(self, denom32: float, denom64: float, *, out: torch.Tensor, cur_side: torch.Tensor,
                      model_side: Optional[torch.Tensor] = None, yogi: Optional[dict] = None,
                      mirror: Optional[torch.Tensor] = None):
        """Reduce the last chunk with the division fused (``DeviceRound.finalize_mean`` without the fused YoGi
        epilogue: fed-yogi rounds take the mean, then the existing fa_yogi_step)."""
        if yogi is not None:
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)", self.upload_dtype)
        self._check_complete()
        L, st, n = self.layout, self.staging, self.slot
        first = self.chunks_done == 0
        a32, a64 = self._chunk_weights()
        mode = 0 if self.policy == "fedavg" else 1
        kh.reduce16(st.x16, n, L.P, out, a=a32, acc_in=None if first else self.acc, denom=denom32, finalize=True,
                    mirror=mirror)
        kx.side_accumulate(st.xi, n, L.Q, mode, w=a64, acc_i=self.acc_i, acc_d=self.acc_d, accumulate=not first)
        kx.side_close(L.Q, mode, denom64, acc_i=self.acc_i, acc_d=self.acc_d, cur=cur_side, model=model_side)
