"""A round whose client uploads arrive and are staged as MXFP8 deltas and are reduced in fp32.

What an executor uploads is its update ``d = x - L`` against the model ``L`` it was sent for this round, quantised
once to the OCP Microscaling format MXFP8: blocks of 32 ``e4m3fn`` codes over the concatenated fp32 bucket share one
E8M0 scale byte (fedscale_amd/cloud/execution/quant_upload.py; include/fedquant.h states the arithmetic).
``QuantStaging`` is ``HalfStaging`` with [capacity, ld] rows of codes and [capacity, ld / 32] rows of scale bytes —
1 + 1/32 bytes per parameter on the wire, per staged client and per reduction pass — and ``QuantRound`` is what
``TorchModelAdapter._apply_round`` and the aggregator mixins use of ``DeviceRound``: ``fq_reduce`` dequantises every
code exactly and chains the deltas in arrival order, and the round is closed by ``fcl_finish`` (include/fedclip.h)
against the round's snapshot of ``L``: new model = L + chain / K.  The int64 side table travels and reduces as in
``DeviceRound``.

Opt-in (``TorchModelAdapter(upload_quant="mxfp8")``); FedAvg and — as the mean followed by the existing YoGi step —
fed-yogi, fed-adam, fed-adagrad or fed-avgm (the mean, then the server step).  FedBuff (a stale client's base is not this round's ``L``), q-FedAvg, 16-bit uploads, sharded models,
client-sharded ranks, cohort signatures, clip and trim are refused.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import kernels as kx
from . import kernels_clip as kc
from . import kernels_quant as kq
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout, default_pack_workers
from .cloud.execution.quant_upload import SCALES_KEY  # (dict uploads; list uploads carry the scale array last)
from .round import on_stream
from .state import DeviceStream

FORMATS = ("mxfp8",)
_I64, _U8 = np.dtype(np.int64), np.dtype(np.uint8)


def check_format(fmt) -> str:
    """``fmt`` when it names a quantised upload format; ValueError otherwise."""
    if fmt not in FORMATS:
        raise ValueError(f"upload_quant {fmt!r}: expected 'mxfp8'")
    return fmt


def refuse(what: str, fmt: str = "mxfp8") -> NotImplementedError:
    """The error of a combination the quantised-delta upload path does not take."""
    return NotImplementedError(f"upload_quant={fmt!r} combined with {what} is not supported: MXFP8 delta uploads "
                               f"take FedAvg and fed-yogi rounds of one whole model on one device")


def default_capacity8(layout: BucketLayout, K: int, device, budget_fraction: float = 0.5) -> int:
    """Clients per chunk, from rows of ld * (1 + 1/32) bytes: all K when they fit in ``budget_fraction`` of the free
    HBM."""
    free, _ = torch.cuda.mem_get_info(device)
    per_client = layout.ld + layout.ld // kq.BLOCK + layout.ldq * 8
    return min(max(1, int(free * budget_fraction) // max(1, per_client)), max(1, K))


def upload_plan8(layout: BucketLayout, update, device=None):
    """Validate one MXFP8 upload against the layout (no GPU needed for host entries): ``(plan, scales)`` with plan
    a list, in layout order, of (entry, value) — value a C-contiguous host array (uint8 codes / int64) or a tensor on
    ``device`` — and scales the uint8 [ceil(P / 32)] scale array (host array or tensor on ``device``).  TypeError
    names the entry whose dtype or shape does not fit — a float32 array included: the staging holds codes, and a silent
    cast would hide a misconfigured executor."""
    if type(update) is dict:
        if SCALES_KEY not in update:
            raise TypeError(f"{SCALES_KEY}: the upload carries no scale array (upload_quant='mxfp8'; see "
                            f"quant_upload.compress_delta)")
        scales = update[SCALES_KEY]
        values = [v for k, v in update.items() if k != SCALES_KEY]
    else:
        values = list(update)
        if len(values) != layout.T + 1:
            raise ValueError(f"update has {len(values)} tensors, the model has {layout.T} and the scale array goes "
                             f"last (upload_quant='mxfp8')")
        scales = values.pop()
    values = layout.values_of(values)
    NB = kq.blocks(layout.P)

    def fit(name, v, want_t, want_n, takes, shape):
        if isinstance(v, torch.Tensor):
            if v.dtype != want_t:
                raise TypeError(f"{name}: dtype {v.dtype}, this staging takes {want_t} for the entry "
                                f"(upload_quant='mxfp8')")
            if tuple(v.shape) != shape:
                raise TypeError(f"{name}: shape {tuple(v.shape)} != {'model ' if name != SCALES_KEY else ''}shape "
                                f"{shape}")
            v = v.detach()
            if device is not None and v.device == device:
                return v if v.is_contiguous() else v.contiguous()
            return v.cpu().contiguous().numpy()
        v = v if type(v) is np.ndarray else np.asarray(v)
        if v.dtype != want_n:
            raise TypeError(f"{name}: dtype {v.dtype}, this staging takes {takes} for the entry "
                            f"(upload_quant='mxfp8'; see quant_upload.compress_delta)")
        if v.shape != shape:
            raise TypeError(f"{name}: shape {tuple(v.shape)} != {'model ' if name != SCALES_KEY else ''}shape {shape}")
        return v if v.flags.c_contiguous else np.ascontiguousarray(v)

    plan = []
    for e in layout.entries:
        if e.kind == "f":
            plan.append((e, fit(e.name, values[e.index], torch.uint8, _U8, "uint8 arrays of e4m3 codes", e.shape)))
        else:
            plan.append((e, fit(e.name, values[e.index], torch.int64, _I64, "int64", e.shape)))
    scales = fit(SCALES_KEY, scales, torch.uint8, _U8, "a uint8 array of E8M0 scale bytes", (NB,))
    return plan, scales


class QuantStaging:
    """Device staging area for up to ``capacity`` MXFP8 client uploads: ``q8`` [capacity, ld] uint8 codes, ``scales``
    [capacity, ld / 32] uint8 scale bytes, ``xi`` [capacity, ldq] int64.  Host uploads are gathered into one pinned
    row per array (a ring of two) by ``fa_host_gather`` and cross PCIe in one H2D per array on the staging's stream;
    an event per pinned row guards its reuse."""

    fmt = "mxfp8"

    def __init__(self, layout: BucketLayout, device, capacity: int, dstream: Optional[DeviceStream] = None,
                 ring: int = 2, pack_workers: Optional[int] = None):
        if layout.world != 1:
            raise refuse("a parameter-sharded layout")
        self.layout, self.device, self.dstream = layout, torch.device(device), dstream
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.capacity = int(capacity)
        self.pack_workers = pack_workers or default_pack_workers()
        self.side_scratch = None  # (int64, float64) side-table sums of a round, reused
        self.lds = layout.ld // kq.BLOCK
        self.NB = kq.blocks(layout.P)
        with self._on():
            self.q8 = torch.zeros(self.capacity, layout.ld, dtype=torch.uint8, device=self.device)
            self.scales = torch.zeros(self.capacity, self.lds, dtype=torch.uint8, device=self.device)
            self.xi = torch.zeros(self.capacity, layout.ldq, dtype=torch.int64, device=self.device)
        self._ring, self._ring_n, self._next = [], ring, 0
        # fp32 entries' places in a row of codes, in bytes (static half of the gather)
        self._f_offs = np.asarray([e.offset for e in layout.f_entries if e.numel], dtype=np.int64)
        self._f_sizes = np.asarray([e.numel for e in layout.f_entries if e.numel], dtype=np.int64)

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def _stream(self):
        return self.dstream.stream if self.dstream is not None else torch.cuda.current_stream(self._dev_index)

    def put(self, slot: int, update):
        """Stage one upload (dict, or list in layout order with the scale array last) into ``slot``; errors surface
        here, synchronously."""
        lay = self.layout
        plan, scales = upload_plan8(lay, update, self.device)
        if not 0 <= slot < self.capacity:
            raise IndexError(f"slot {slot} of {self.capacity}")
        if isinstance(scales, torch.Tensor) and all(isinstance(v, torch.Tensor) for _, v in plan):
            with self._on():
                if self.dstream is not None:
                    self.dstream.wait_caller()  # the caller's device tensors
                for e, v in plan:
                    dst = self.q8[slot] if e.kind == "f" else self.xi[slot]
                    dst[e.offset:e.offset + e.numel].copy_(v.reshape(-1), non_blocking=True)
                self.scales[slot, :self.NB].copy_(scales, non_blocking=True)
            return
        if not self._ring:
            for _ in range(self._ring_n):
                h8 = torch.zeros(lay.ld, dtype=torch.uint8).pin_memory()
                hs = torch.zeros(max(1, self.lds), dtype=torch.uint8).pin_memory()
                hi = torch.zeros(lay.ldq, dtype=torch.int64).pin_memory()
                self._ring.append([h8, hs, hi, h8.numpy(), hs.numpy(), hi.numpy(), None])
        r = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        if r[6] is not None:
            r[6].synchronize()  # the previous H2Ds out of these pinned rows have completed
        ptrs, keep = [], []
        for e, v in plan:
            if isinstance(v, torch.Tensor):  # a device entry among host ones
                v = v.cpu().numpy()
            if e.kind == "i":
                r[5][e.offset:e.offset + e.numel] = v.reshape(-1)
            elif e.numel:
                keep.append(v)
                ptrs.append(v.__array_interface__["data"][0])
        if ptrs:
            from . import _native

            ps = np.asarray(ptrs, dtype=np.uint64)
            _native.call("fa_host_gather", r[3].__array_interface__["data"][0], ps.ctypes.data,
                         self._f_offs.ctypes.data, self._f_sizes.ctypes.data, len(ptrs), int(self.pack_workers))
        del keep
        r[4][:self.NB] = scales.cpu().numpy() if isinstance(scales, torch.Tensor) else scales
        with self._on():
            st = self._stream()
            with torch.cuda.stream(st):
                if lay.P:
                    self.q8[slot, :lay.P].copy_(r[0][:lay.P], non_blocking=True)
                    self.scales[slot, :self.NB].copy_(r[1][:self.NB], non_blocking=True)
                if lay.Q:
                    self.xi[slot, :lay.Q].copy_(r[2][:lay.Q], non_blocking=True)
            if r[6] is None:
                r[6] = torch.cuda.Event()
            r[6].record(st)


class QuantRound:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, over a ``QuantStaging``."""

    policy = "fedavg"
    cg = None        # never client-sharded
    head = 0         # no head launch, no small-round mirror path
    sig_plan = None  # no cohort signatures

    def __init__(self, layout: BucketLayout, device, K: int, policy: str, *, staging: QuantStaging,
                 last_f32: torch.Tensor, capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None):
        if policy != "fedavg":
            raise refuse(f"a {policy} round", staging.fmt)
        if K < 1:
            raise ValueError("a round needs K >= 1 client results")
        self.layout, self.device, self.K = layout, torch.device(device), int(K)
        self.dstream, self.staging, self.last_f32 = dstream, staging, last_f32
        self.upload_quant = staging.fmt
        self.cap = min(staging.capacity, capacity or staging.capacity)
        self.n = self.slot = self.chunks_done = 0
        with self._on():
            if staging.side_scratch is None:
                staging.side_scratch = (torch.empty(layout.ldq, dtype=torch.int64, device=self.device),
                                        torch.empty(layout.ldq, dtype=torch.float64, device=self.device))
            self.chain = torch.zeros(layout.ld, dtype=torch.float32, device=self.device)
        self.acc_i, self.acc_d = staging.side_scratch

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def add(self, update, *, weight: Optional[float] = None, loss=None, learning_rate=None, q=None):
        """Stage one arriving MXFP8 upload (in arrival order)."""
        if self.n >= self.K:
            raise RuntimeError(f"round already has its K={self.K} results")
        if self.slot == self.cap:
            self._fold_chunk()
        self.staging.put(self.slot, update)
        self.slot += 1
        self.n += 1

    def adopt_resident(self, n: int):
        """Measurement hook, as ``DeviceRound.adopt_resident``: take ``n`` arrivals whose uploads are ALREADY in the
        staging slots [slot, slot + n), written there on the device (tools/quant_reduce_measure.py)."""
        if n < 0 or self.slot + n > self.cap or self.n + n > self.K:
            raise ValueError(f"adopt_resident: {n} arrivals do not fit (slot {self.slot} of {self.cap}, "
                             f"{self.n} of K={self.K})")
        self.slot += n
        self.n += n

    def _reduce_chunk(self):
        """The staged chunk's deltas onto the chain (the same chain across chunks), and its side-table sums."""
        L, st, n = self.layout, self.staging, self.slot
        first = self.chunks_done == 0
        if n > 0 and L.P > 0:
            kq.reduce8(st.q8, st.scales, n, L.P, self.chain, acc_in=None if first else self.chain)
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

    @on_stream
    def finalize_mean(self, denom32: float, denom64: float, *, out: torch.Tensor, cur_side: torch.Tensor,
                      model_side: Optional[torch.Tensor] = None, yogi: Optional[dict] = None,
                      mirror: Optional[torch.Tensor] = None):
        """Reduce the last chunk, then ``out`` <- the round's starting model plus the mean delta (fcl_finish, no
        noise); the side table as ``DeviceRound.finalize_mean`` (fed-yogi rounds take ``out`` as the mean, then the
        existing fa_yogi_step)."""
        if yogi is not None:
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)", self.upload_quant)
        self._check_complete()
        den = float(np.float32(self.K))
        if float(denom32) != den:
            raise ValueError(f"a quantised-delta round divides by its client count K={self.K}, not {denom32}")
        L = self.layout
        self._reduce_chunk()
        kc.finish(self.chain, self.last_f32, L.P, den, out, mirror=mirror)
        kx.side_close(L.Q, 0, denom64, acc_i=self.acc_i, acc_d=self.acc_d, cur=cur_side, model=model_side)
