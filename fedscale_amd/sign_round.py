"""A round whose client uploads arrive and are staged as 1-bit sign deltas and are reduced in fp32.

What an executor uploads is its update ``e = x - L`` against the model ``L`` it was sent for this round (plus, with
error feedback, what its earlier rounds' encodings left behind), compressed once to the scaled sign: one bit per
column of the concatenated fp32 bucket and one float32 scale — the mean magnitude — per block of 256 columns
(fedscale_amd/cloud/execution/sign_upload.py; include/fedsign.h states the contract).  ``SignStaging`` holds
[capacity, ldb] rows of bit bytes and [capacity, lds] rows of scales — 9/64 byte per parameter on the wire, per
staged client and per reduction pass — and ``SignRound`` is what ``TorchModelAdapter._apply_round`` and the
aggregator mixins use of ``DeviceRound``: ``fsg_reduce`` dequantises every column exactly (a sign flip of its block's
scale) and chains the deltas in arrival order, and the round is closed by ``fcl_finish`` (include/fedclip.h) against
the round's snapshot of ``L``: new model = L + chain / K.  The int64 side table travels and reduces as in
``DeviceRound``.

Opt-in (``TorchModelAdapter(upload_sign="sign1")``); FedAvg and — as the mean followed by the existing YoGi step —
fed-yogi, fed-adam, fed-adagrad or fed-avgm (the mean, then the server step).  FedBuff (a stale client's base is not this round's ``L``), q-FedAvg, the other upload formats, sharded
models, client-sharded ranks, cohort signatures, clip, trim, Krum, geometric-median and secure-aggregation rounds are
refused.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import kernels as kx
from . import kernels_clip as kc
from . import kernels_sign as kg
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout
from .cloud.execution.sign_upload import BITS_KEY, SCALES_KEY
from .round import on_stream
from .state import DeviceStream

FORMATS = ("sign1",)
_I64, _U8, _F32 = np.dtype(np.int64), np.dtype(np.uint8), np.dtype(np.float32)


def check_format(fmt) -> str:
    """``fmt`` when it names a sign upload format; ValueError otherwise."""
    if fmt not in FORMATS:
        raise ValueError(f"upload_sign {fmt!r}: expected 'sign1'")
    return fmt


def refuse(what: str, fmt: str = "sign1") -> NotImplementedError:
    """The error of a combination the sign-delta upload path does not take."""
    return NotImplementedError(f"upload_sign={fmt!r} combined with {what} is not supported: 1-bit sign delta uploads "
                               f"take FedAvg and fed-yogi rounds of one whole model on one device")


def default_capacity_sign(layout: BucketLayout, K: int, device, budget_fraction: float = 0.5) -> int:
    """Clients per chunk, from rows of ldb bytes and lds scales: all K when they fit in ``budget_fraction`` of the free
    HBM."""
    free, _ = torch.cuda.mem_get_info(device)
    per_client = kg.bit_stride(layout.P) + 4 * kg.scale_stride(layout.P) + layout.ldq * 8
    return min(max(1, int(free * budget_fraction) // max(1, per_client)), max(1, K))


def upload_plan_sign(layout: BucketLayout, update, device=None):
    """Validate one sign upload against the layout (no GPU needed for host entries): ``(side, bits, scales)`` with
    side a list of (entry, value) for the int64 entries in layout order, bits the uint8 [ceil(P / 8)] array and scales
    the float32 [ceil(P / 256)] array — each a C-contiguous host array or a tensor on ``device``.  TypeError names the
    entry whose dtype or shape does not fit — a float32 model entry included: the staging holds bits, and a silent
    cast would hide a misconfigured executor."""
    n_side = len(layout.i_entries)
    if type(update) is dict:
        for e in layout.f_entries:
            if e.name in update:
                v = update[e.name]
                raise TypeError(f"{e.name}: dtype {getattr(v, 'dtype', type(v).__name__)}, this staging takes the "
                                f"float32 entries as sign bits under {BITS_KEY} (upload_sign='sign1'; see "
                                f"sign_upload.compress_sign)")
        for key in (BITS_KEY, SCALES_KEY):
            if key not in update:
                raise TypeError(f"{key}: the upload carries no such array (upload_sign='sign1'; a dense float32 "
                                f"upload is not a sign upload: see sign_upload.compress_sign)")
        bits, scales = update[BITS_KEY], update[SCALES_KEY]
        names = [k for k in update if k not in (BITS_KEY, SCALES_KEY)]
        want = [e.name for e in layout.i_entries]
        if names != want:
            raise ValueError(f"update names the entries {names}, a sign upload carries the non-float32 entries "
                             f"{want} beside {BITS_KEY} and {SCALES_KEY}")
        values = [update[k] for k in names]
    else:
        values = list(update)
        if len(values) != n_side + 2:
            raise ValueError(f"update has {len(values)} arrays, a sign upload has the model's {n_side} non-float32 "
                             f"entries, then the bits, then the scales (upload_sign='sign1')")
        bits, scales = values[-2], values[-1]
        values = values[:-2]

    def fit(name, v, want_t, want_n, takes, shape, what="model "):
        if isinstance(v, torch.Tensor):
            if v.dtype != want_t:
                raise TypeError(f"{name}: dtype {v.dtype}, this staging takes {takes} for the entry "
                                f"(upload_sign='sign1')")
            if tuple(v.shape) != shape:
                raise TypeError(f"{name}: shape {tuple(v.shape)} != {what}shape {shape}")
            v = v.detach()
            if device is not None and v.device == device:
                return v if v.is_contiguous() else v.contiguous()
            return v.cpu().contiguous().numpy()
        v = v if type(v) is np.ndarray else np.asarray(v)
        if v.dtype != want_n:
            raise TypeError(f"{name}: dtype {v.dtype}, this staging takes {takes} for the entry "
                            f"(upload_sign='sign1'; see sign_upload.compress_sign)")
        if v.shape != shape:
            raise TypeError(f"{name}: shape {tuple(v.shape)} != {what}shape {shape}")
        return v if v.flags.c_contiguous else np.ascontiguousarray(v)

    side = [(e, fit(e.name, v, torch.int64, _I64, "int64", e.shape)) for e, v in zip(layout.i_entries, values)]
    bits = fit(BITS_KEY, bits, torch.uint8, _U8, "a uint8 array of sign bits", (kg.bit_bytes(layout.P),), "")
    scales = fit(SCALES_KEY, scales, torch.float32, _F32, "a float32 array of block scales", (kg.blocks(layout.P),),
                 "")
    return side, bits, scales


class SignStaging:
    """Device staging area for up to ``capacity`` sign client uploads: ``bits`` [capacity, ldb] uint8 with
    ldb = round_up(ceil(P / 8), 16), ``scales`` [capacity, lds] float32 with lds = round_up(ceil(P / 256), 4) (the
    layout's ld is only 64-aligned, so the staging computes its own strides), ``xi`` [capacity, ldq] int64.  Host
    uploads cross PCIe from one pinned row per array (a ring of two) in one H2D per array on the staging's stream; an
    event per pinned row guards its reuse."""

    fmt = "sign1"

    def __init__(self, layout: BucketLayout, device, capacity: int, dstream: Optional[DeviceStream] = None,
                 ring: int = 2):
        if layout.world != 1:
            raise refuse("a parameter-sharded layout")
        self.layout, self.device, self.dstream = layout, torch.device(device), dstream
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.capacity = int(capacity)
        self.side_scratch = None  # (int64, float64) side-table sums of a round, reused
        self.PB, self.NB = kg.bit_bytes(layout.P), kg.blocks(layout.P)
        self.ldb, self.lds = kg.bit_stride(layout.P), kg.scale_stride(layout.P)
        with self._on():
            self.bits = torch.zeros(self.capacity, max(16, self.ldb), dtype=torch.uint8, device=self.device)
            self.scales = torch.zeros(self.capacity, max(4, self.lds), dtype=torch.float32, device=self.device)
            self.xi = torch.zeros(self.capacity, layout.ldq, dtype=torch.int64, device=self.device)
        self._ring, self._ring_n, self._next = [], ring, 0

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def _stream(self):
        return self.dstream.stream if self.dstream is not None else torch.cuda.current_stream(self._dev_index)

    def put(self, slot: int, update):
        """Stage one upload (dict, or list of the non-float32 entries, then the bits, then the scales) into ``slot``;
        errors surface here, synchronously."""
        lay = self.layout
        side, bits, scales = upload_plan_sign(lay, update, self.device)
        if not 0 <= slot < self.capacity:
            raise IndexError(f"slot {slot} of {self.capacity}")
        if (isinstance(bits, torch.Tensor) and isinstance(scales, torch.Tensor)
                and all(isinstance(v, torch.Tensor) for _, v in side)):
            with self._on():
                if self.dstream is not None:
                    self.dstream.wait_caller()  # the caller's device tensors
                with torch.cuda.stream(self._stream()):
                    for e, v in side:
                        self.xi[slot, e.offset:e.offset + e.numel].copy_(v.reshape(-1), non_blocking=True)
                    self.bits[slot, :self.PB].copy_(bits, non_blocking=True)
                    self.scales[slot, :self.NB].copy_(scales, non_blocking=True)
            return
        if not self._ring:
            for _ in range(self._ring_n):
                hb = torch.zeros(max(16, self.ldb), dtype=torch.uint8).pin_memory()
                hs = torch.zeros(max(4, self.lds), dtype=torch.float32).pin_memory()
                hi = torch.zeros(lay.ldq, dtype=torch.int64).pin_memory()
                self._ring.append([hb, hs, hi, hb.numpy(), hs.numpy(), hi.numpy(), None])
        r = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        if r[6] is not None:
            r[6].synchronize()  # the previous H2Ds out of these pinned rows have completed
        for e, v in side:
            if isinstance(v, torch.Tensor):  # a device entry among host ones
                v = v.cpu().numpy()
            r[5][e.offset:e.offset + e.numel] = v.reshape(-1)
        r[3][:self.PB] = bits.cpu().numpy() if isinstance(bits, torch.Tensor) else bits
        r[4][:self.NB] = scales.cpu().numpy() if isinstance(scales, torch.Tensor) else scales
        with self._on():
            st = self._stream()
            with torch.cuda.stream(st):
                if lay.P:
                    self.bits[slot, :self.PB].copy_(r[0][:self.PB], non_blocking=True)
                    self.scales[slot, :self.NB].copy_(r[1][:self.NB], non_blocking=True)
                if lay.Q:
                    self.xi[slot, :lay.Q].copy_(r[2][:lay.Q], non_blocking=True)
            if r[6] is None:
                r[6] = torch.cuda.Event()
            r[6].record(st)


class SignRound:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, over a ``SignStaging``."""

    policy = "fedavg"
    cg = None        # never client-sharded
    head = 0         # no head launch, no small-round mirror path
    sig_plan = None  # no cohort signatures

    def __init__(self, layout: BucketLayout, device, K: int, policy: str, *, staging: SignStaging,
                 last_f32: torch.Tensor, capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None):
        if policy != "fedavg":
            raise refuse(f"a {policy} round", staging.fmt)
        if K < 1:
            raise ValueError("a round needs K >= 1 client results")
        self.layout, self.device, self.K = layout, torch.device(device), int(K)
        self.dstream, self.staging, self.last_f32 = dstream, staging, last_f32
        self.upload_sign = staging.fmt
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
        """Stage one arriving sign upload (in arrival order)."""
        if self.n >= self.K:
            raise RuntimeError(f"round already has its K={self.K} results")
        if self.slot == self.cap:
            self._fold_chunk()
        self.staging.put(self.slot, update)
        self.slot += 1
        self.n += 1

    def adopt_resident(self, n: int):
        """Measurement hook, as ``DeviceRound.adopt_resident``: take ``n`` arrivals whose uploads are ALREADY in the
        staging slots [slot, slot + n), written there on the device (tools/sign_reduce_measure.py)."""
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
            kg.reduce_sign(st.bits, st.scales, n, L.P, self.chain, acc_in=None if first else self.chain)
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
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)", self.upload_sign)
        self._check_complete()
        den = float(np.float32(self.K))
        if float(denom32) != den:
            raise ValueError(f"a sign-delta round divides by its client count K={self.K}, not {denom32}")
        L = self.layout
        self._reduce_chunk()
        kc.finish(self.chain, self.last_f32, L.P, den, out, mirror=mirror)
        kx.side_close(L.Q, 0, denom64, acc_i=self.acc_i, acc_d=self.acc_d, cur=cur_side, model=model_side)
