"""A round whose client uploads arrive and are staged as MXFP4 deltas and are reduced in fp32.

What an executor uploads is its update ``d = x - L`` against the model ``L`` it was sent for this round (plus, with
error feedback, what its earlier rounds' encodings left behind), quantised once to the OCP Microscaling format MXFP4:
blocks of 32 ``e2m1`` codes, two to a byte, over the concatenated fp32 bucket share one E8M0 scale byte
(fedscale_amd/cloud/execution/quant4_upload.py; include/fedquant4.h states the contract).  ``Quant4Staging`` holds
[capacity, ld / 2] rows of code bytes and [capacity, ld / 32] rows of scale bytes — 17/32 byte per parameter on the
wire, per staged client and per reduction pass — and ``Quant4Round`` is what ``TorchModelAdapter._apply_round`` and
the aggregator mixins use of ``DeviceRound``: ``fq4_reduce`` dequantises every code exactly and chains the deltas in
arrival order, and the round is closed by ``fcl_finish`` (include/fedclip.h) against the round's snapshot of ``L``:
new model = L + chain / K.  The int64 side table travels and reduces as in ``DeviceRound``.

Opt-in (``TorchModelAdapter(upload_fp4="mxfp4")``); FedAvg and — as the mean followed by the server step — fed-yogi,
fed-adam, fed-adagrad or fed-avgm.  FedBuff (a stale client's base is not this round's ``L``), q-FedAvg, the other
upload formats, sharded models, client-sharded ranks, cohort signatures, clip, trim, Krum, geometric-median and
secure-aggregation rounds are refused.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import kernels as kx
from . import kernels_clip as kc
from . import kernels_quant4 as kq4
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout, default_pack_workers
from .cloud.execution.quant4_upload import CODES_KEY, SCALES_KEY
from .round import on_stream
from .state import DeviceStream

FORMATS4 = ("mxfp4",)
_I64, _U8 = np.dtype(np.int64), np.dtype(np.uint8)


def check_format4(fmt) -> str:
    """``fmt`` when it names a 4-bit upload format; ValueError otherwise."""
    if fmt not in FORMATS4:
        raise ValueError(f"upload_fp4 {fmt!r}: expected 'mxfp4'")
    return fmt


def refuse(what: str, fmt: str = "mxfp4") -> NotImplementedError:
    """The error of a combination the 4-bit delta upload path does not take."""
    return NotImplementedError(f"upload_fp4={fmt!r} combined with {what} is not supported: MXFP4 delta uploads take "
                               f"FedAvg and server-optimizer rounds of one whole model on one device")


def default_capacity4(layout: BucketLayout, K: int, device, budget_fraction: float = 0.5) -> int:
    """Clients per chunk, from rows of ld * 17/32 bytes: all K when they fit in ``budget_fraction`` of the free
    HBM."""
    free, _ = torch.cuda.mem_get_info(device)
    per_client = layout.ld // 2 + layout.ld // kq4.BLOCK + layout.ldq * 8
    return min(max(1, int(free * budget_fraction) // max(1, per_client)), max(1, K))


def upload_plan4(layout: BucketLayout, update, device=None):
    """Validate one MXFP4 upload against the layout (no GPU needed for host entries): ``(side, codes, scales)`` with
    side a list of (entry, value) for the int64 entries in layout order, codes the uint8 [16 * ceil(P / 32)] array and
    scales the uint8 [ceil(P / 32)] array — each a C-contiguous host array or a tensor on ``device``.  TypeError names
    the entry whose dtype or shape does not fit — a float32 model entry included: the staging holds codes, and a
    silent cast would hide a misconfigured executor."""
    n_side = len(layout.i_entries)
    if type(update) is dict:
        for e in layout.f_entries:
            if e.name in update:
                v = update[e.name]
                raise TypeError(f"{e.name}: dtype {getattr(v, 'dtype', type(v).__name__)}, this staging takes the "
                                f"float32 entries as e2m1 codes under {CODES_KEY} (upload_fp4='mxfp4'; see "
                                f"quant4_upload.compress_delta4)")
        for key in (CODES_KEY, SCALES_KEY):
            if key not in update:
                raise TypeError(f"{key}: the upload carries no such array (upload_fp4='mxfp4'; a dense float32 "
                                f"upload is not an MXFP4 upload: see quant4_upload.compress_delta4)")
        codes, scales = update[CODES_KEY], update[SCALES_KEY]
        names = [k for k in update if k not in (CODES_KEY, SCALES_KEY)]
        want = [e.name for e in layout.i_entries]
        if names != want:
            raise ValueError(f"update names the entries {names}, an MXFP4 upload carries the non-float32 entries "
                             f"{want} beside {CODES_KEY} and {SCALES_KEY}")
        values = [update[k] for k in names]
    else:
        values = list(update)
        if len(values) != n_side + 2:
            raise ValueError(f"update has {len(values)} arrays, an MXFP4 upload has the model's {n_side} non-float32 "
                             f"entries, then the codes, then the scales (upload_fp4='mxfp4')")
        codes, scales = values[-2], values[-1]
        values = values[:-2]

    def fit(name, v, want_t, want_n, takes, shape, what="model "):
        if isinstance(v, torch.Tensor):
            if v.dtype != want_t:
                raise TypeError(f"{name}: dtype {v.dtype}, this staging takes {takes} for the entry "
                                f"(upload_fp4='mxfp4')")
            if tuple(v.shape) != shape:
                raise TypeError(f"{name}: shape {tuple(v.shape)} != {what}shape {shape}")
            v = v.detach()
            if device is not None and v.device == device:
                return v if v.is_contiguous() else v.contiguous()
            return v.cpu().contiguous().numpy()
        v = v if type(v) is np.ndarray else np.asarray(v)
        if v.dtype != want_n:
            raise TypeError(f"{name}: dtype {v.dtype}, this staging takes {takes} for the entry "
                            f"(upload_fp4='mxfp4'; see quant4_upload.compress_delta4)")
        if v.shape != shape:
            raise TypeError(f"{name}: shape {tuple(v.shape)} != {what}shape {shape}")
        return v if v.flags.c_contiguous else np.ascontiguousarray(v)

    side = [(e, fit(e.name, v, torch.int64, _I64, "int64", e.shape)) for e, v in zip(layout.i_entries, values)]
    codes = fit(CODES_KEY, codes, torch.uint8, _U8, "a uint8 array of packed e2m1 codes",
                (kq4.code_bytes(layout.P),), "")
    scales = fit(SCALES_KEY, scales, torch.uint8, _U8, "a uint8 array of E8M0 scale bytes", (kq4.blocks(layout.P),),
                 "")
    return side, codes, scales


class Quant4Staging:
    """Device staging area for up to ``capacity`` MXFP4 client uploads: ``q4`` [capacity, ld / 2] uint8 code bytes,
    ``scales`` [capacity, ld / 32] uint8 scale bytes, ``xi`` [capacity, ldq] int64.  A host upload's code array is
    copied into one pinned row (a ring of two) by ``fa_host_gather``'s worker pool and crosses PCIe in one H2D per
    array on the staging's stream; an event per pinned row guards its reuse."""

    fmt = "mxfp4"

    def __init__(self, layout: BucketLayout, device, capacity: int, dstream: Optional[DeviceStream] = None,
                 ring: int = 2, pack_workers: Optional[int] = None):
        if layout.world != 1:
            raise refuse("a parameter-sharded layout")
        self.layout, self.device, self.dstream = layout, torch.device(device), dstream
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.capacity = int(capacity)
        self.pack_workers = pack_workers or default_pack_workers()
        self.side_scratch = None  # (int64, float64) side-table sums of a round, reused
        self.ldc, self.lds = layout.ld // 2, layout.ld // kq4.BLOCK
        self.NC, self.NB = kq4.code_bytes(layout.P), kq4.blocks(layout.P)
        with self._on():
            self.q4 = torch.zeros(self.capacity, self.ldc, dtype=torch.uint8, device=self.device)
            self.scales = torch.zeros(self.capacity, self.lds, dtype=torch.uint8, device=self.device)
            self.xi = torch.zeros(self.capacity, layout.ldq, dtype=torch.int64, device=self.device)
        self._ring, self._ring_n, self._next = [], ring, 0
        # the chunks of the code array the gather's workers copy side by side (1 MiB each)
        step = 1 << 20
        self._g_offs = np.arange(0, max(1, self.NC), step, dtype=np.int64)
        self._g_sizes = np.minimum(step, self.NC - self._g_offs).astype(np.int64)

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def _stream(self):
        return self.dstream.stream if self.dstream is not None else torch.cuda.current_stream(self._dev_index)

    def put(self, slot: int, update):
        """Stage one upload (dict, or list of the non-float32 entries, then the codes, then the scales) into
        ``slot``; errors surface here, synchronously."""
        lay = self.layout
        side, codes, scales = upload_plan4(lay, update, self.device)
        if not 0 <= slot < self.capacity:
            raise IndexError(f"slot {slot} of {self.capacity}")
        if (isinstance(codes, torch.Tensor) and isinstance(scales, torch.Tensor)
                and all(isinstance(v, torch.Tensor) for _, v in side)):
            with self._on():
                if self.dstream is not None:
                    self.dstream.wait_caller()  # the caller's device tensors
                with torch.cuda.stream(self._stream()):
                    for e, v in side:
                        self.xi[slot, e.offset:e.offset + e.numel].copy_(v.reshape(-1), non_blocking=True)
                    self.q4[slot, :self.NC].copy_(codes, non_blocking=True)
                    self.scales[slot, :self.NB].copy_(scales, non_blocking=True)
            return
        if not self._ring:
            for _ in range(self._ring_n):
                h4 = torch.zeros(max(16, self.ldc), dtype=torch.uint8).pin_memory()
                hs = torch.zeros(max(1, self.lds), dtype=torch.uint8).pin_memory()
                hi = torch.zeros(lay.ldq, dtype=torch.int64).pin_memory()
                self._ring.append([h4, hs, hi, h4.numpy(), hs.numpy(), hi.numpy(), None])
        r = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        if r[6] is not None:
            r[6].synchronize()  # the previous H2Ds out of these pinned rows have completed
        for e, v in side:
            if isinstance(v, torch.Tensor):  # a device entry among host ones
                v = v.cpu().numpy()
            r[5][e.offset:e.offset + e.numel] = v.reshape(-1)
        if isinstance(codes, torch.Tensor):
            codes = codes.cpu().numpy()
        if self.NC:
            from . import _native

            src = codes.__array_interface__["data"][0]
            ps = (np.uint64(src) + self._g_offs.astype(np.uint64)).astype(np.uint64)
            _native.call("fa_host_gather", r[3].__array_interface__["data"][0], ps.ctypes.data,
                         self._g_offs.ctypes.data, self._g_sizes.ctypes.data, len(ps), int(self.pack_workers))
        r[4][:self.NB] = scales.cpu().numpy() if isinstance(scales, torch.Tensor) else scales
        with self._on():
            st = self._stream()
            with torch.cuda.stream(st):
                if lay.P:
                    self.q4[slot, :self.NC].copy_(r[0][:self.NC], non_blocking=True)
                    self.scales[slot, :self.NB].copy_(r[1][:self.NB], non_blocking=True)
                if lay.Q:
                    self.xi[slot, :lay.Q].copy_(r[2][:lay.Q], non_blocking=True)
            if r[6] is None:
                r[6] = torch.cuda.Event()
            r[6].record(st)


class Quant4Round:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, over a ``Quant4Staging``."""

    policy = "fedavg"
    cg = None        # never client-sharded
    head = 0         # no head launch, no small-round mirror path
    sig_plan = None  # no cohort signatures

    def __init__(self, layout: BucketLayout, device, K: int, policy: str, *, staging: Quant4Staging,
                 last_f32: torch.Tensor, capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None):
        if policy != "fedavg":
            raise refuse(f"a {policy} round", staging.fmt)
        if K < 1:
            raise ValueError("a round needs K >= 1 client results")
        self.layout, self.device, self.K = layout, torch.device(device), int(K)
        self.dstream, self.staging, self.last_f32 = dstream, staging, last_f32
        self.upload_fp4 = staging.fmt
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
        """Stage one arriving MXFP4 upload (in arrival order)."""
        if self.n >= self.K:
            raise RuntimeError(f"round already has its K={self.K} results")
        if self.slot == self.cap:
            self._fold_chunk()
        self.staging.put(self.slot, update)
        self.slot += 1
        self.n += 1

    def adopt_resident(self, n: int):
        """Measurement hook, as ``DeviceRound.adopt_resident``: take ``n`` arrivals whose uploads are ALREADY in the
        staging slots [slot, slot + n), written there on the device (tools/quant4_reduce_measure.py)."""
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
            kq4.reduce4(st.q4, st.scales, n, L.P, self.chain, acc_in=None if first else self.chain)
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
        noise); the side table as ``DeviceRound.finalize_mean`` (server-optimizer rounds take ``out`` as the mean,
        then their own step)."""
        if yogi is not None:
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)", self.upload_fp4)
        self._check_complete()
        den = float(np.float32(self.K))
        if float(denom32) != den:
            raise ValueError(f"a 4-bit delta round divides by its client count K={self.K}, not {denom32}")
        L = self.layout
        self._reduce_chunk()
        kc.finish(self.chain, self.last_f32, L.P, den, out, mirror=mirror)
        kx.side_close(L.Q, 0, denom64, acc_i=self.acc_i, acc_d=self.acc_d, cur=cur_side, model=model_side)
