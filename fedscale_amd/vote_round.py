"""A round whose client uploads are bare sign bits and whose new model is their majority vote.

What an executor uploads is the sign of its update ``e = x - L`` against the model ``L`` it was sent for this round,
one bit per column of the concatenated fp32 bucket and nothing else (fedscale_amd/cloud/execution/vote_upload.py;
include/fedvote.h states the contract).  ``VoteStaging`` holds [capacity, ldb] rows of bit bytes — 1/8 byte per
parameter on the wire, per staged client and per counting pass — and ``VoteRound`` is what
``TorchModelAdapter._apply_round`` and the aggregator mixins use of ``DeviceRound``: ``fvt_count`` tallies every
column's set bits exactly into a persistent ``counts`` buffer (chunk after chunk: integer sums do not depend on the
chunking), and the round is closed by ``fvt_finish`` against the round's snapshot of ``L``: new model = L + lr * the
sign (or the mean) of the vote margin K - 2 counts.  The int64 side table travels and reduces as in ``DeviceRound``.

Opt-in (``TorchModelAdapter(upload_vote=VoteSpec(lr))``); FedAvg and — as that result followed by the existing server
step — fed-yogi, fed-adam, fed-adagrad or fed-avgm.  FedBuff (a stale client's base is not this round's ``L``),
q-FedAvg, the other upload formats, sharded models, client-sharded ranks, cohort signatures, clip, trim, Krum,
geometric-median and secure-aggregation rounds are refused.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import kernels as kx
from . import kernels_vote as kv
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout
from .cloud.execution.vote_upload import VOTE_BITS_KEY, VoteSpec
from .round import on_stream
from .state import DeviceStream

_I64, _U8 = np.dtype(np.int64), np.dtype(np.uint8)


def refuse(what: str, spec=None) -> NotImplementedError:
    """The error of a combination the majority-vote upload path does not take."""
    return NotImplementedError(f"upload_vote={spec!r} combined with {what} is not supported: majority-vote sign "
                               f"uploads take FedAvg and server-step rounds of one whole model on one device")


def default_capacity_vote(layout: BucketLayout, K: int, device, budget_fraction: float = 0.5) -> int:
    """Clients per chunk, from rows of ldb bytes: all K when they fit in ``budget_fraction`` of the free HBM (and in
    one fvt_count call)."""
    free, _ = torch.cuda.mem_get_info(device)
    per_client = kv.bit_stride(layout.P) + layout.ldq * 8
    return min(max(1, int(free * budget_fraction) // max(1, per_client)), max(1, K), kv.MAX_ROWS)


def upload_plan_vote(layout: BucketLayout, update, device=None):
    """Validate one vote upload against the layout (no GPU needed for host entries): ``(side, bits)`` with side a
    list of (entry, value) for the int64 entries in layout order and bits the uint8 [ceil(P / 8)] array — each a
    C-contiguous host array or a tensor on ``device``.  TypeError names the entry whose dtype or shape does not fit —
    a float32 model entry included: the staging holds bits, and a silent cast would hide a misconfigured executor."""
    n_side = len(layout.i_entries)
    if type(update) is dict:
        for e in layout.f_entries:
            if e.name in update:
                v = update[e.name]
                raise TypeError(f"{e.name}: dtype {getattr(v, 'dtype', type(v).__name__)}, this staging takes the "
                                f"float32 entries as sign bits under {VOTE_BITS_KEY} (upload_vote; see "
                                f"vote_upload.compress_vote)")
        if VOTE_BITS_KEY not in update:
            raise TypeError(f"{VOTE_BITS_KEY}: the upload carries no such array (upload_vote; a dense float32 upload "
                            f"is not a vote upload: see vote_upload.compress_vote)")
        bits = update[VOTE_BITS_KEY]
        names = [k for k in update if k != VOTE_BITS_KEY]
        want = [e.name for e in layout.i_entries]
        if names != want:
            raise ValueError(f"update names the entries {names}, a vote upload carries the non-float32 entries "
                             f"{want} beside {VOTE_BITS_KEY}")
        values = [update[k] for k in names]
    else:
        values = list(update)
        if len(values) != n_side + 1:
            raise ValueError(f"update has {len(values)} arrays, a vote upload has the model's {n_side} non-float32 "
                             f"entries, then the bits (upload_vote)")
        bits = values[-1]
        values = values[:-1]

    def fit(name, v, want_t, want_n, takes, shape, what="model "):
        if isinstance(v, torch.Tensor):
            if v.dtype != want_t:
                raise TypeError(f"{name}: dtype {v.dtype}, this staging takes {takes} for the entry (upload_vote)")
            if tuple(v.shape) != shape:
                raise TypeError(f"{name}: shape {tuple(v.shape)} != {what}shape {shape}")
            v = v.detach()
            if device is not None and v.device == device:
                return v if v.is_contiguous() else v.contiguous()
            return v.cpu().contiguous().numpy()
        v = v if type(v) is np.ndarray else np.asarray(v)
        if v.dtype != want_n:
            raise TypeError(f"{name}: dtype {v.dtype}, this staging takes {takes} for the entry (upload_vote; see "
                            f"vote_upload.compress_vote)")
        if v.shape != shape:
            raise TypeError(f"{name}: shape {tuple(v.shape)} != {what}shape {shape}")
        return v if v.flags.c_contiguous else np.ascontiguousarray(v)

    side = [(e, fit(e.name, v, torch.int64, _I64, "int64", e.shape)) for e, v in zip(layout.i_entries, values)]
    bits = fit(VOTE_BITS_KEY, bits, torch.uint8, _U8, "a uint8 array of sign bits", (kv.bit_bytes(layout.P),), "")
    return side, bits


class VoteStaging:
    """Device staging area for up to ``capacity`` vote uploads: ``bits`` [capacity, ldb] uint8 with
    ldb = round_up(ceil(P / 8), 16), ``xi`` [capacity, ldq] int64.  Host uploads cross PCIe from one pinned row per
    array (a ring of two) in one H2D per array on the staging's stream; an event per pinned row guards its reuse."""

    def __init__(self, layout: BucketLayout, device, capacity: int, dstream: Optional[DeviceStream] = None,
                 ring: int = 2):
        if layout.world != 1:
            raise refuse("a parameter-sharded layout")
        if not 1 <= int(capacity) <= kv.MAX_ROWS:
            raise ValueError(f"a vote staging holds 1..{kv.MAX_ROWS} uploads, not {capacity}")
        self.layout, self.device, self.dstream = layout, torch.device(device), dstream
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.capacity = int(capacity)
        self.side_scratch = None  # (int64, float64) side-table sums of a round, reused
        self.PB, self.ldb = kv.bit_bytes(layout.P), kv.bit_stride(layout.P)
        with self._on():
            self.bits = torch.zeros(self.capacity, max(16, self.ldb), dtype=torch.uint8, device=self.device)
            self.xi = torch.zeros(self.capacity, layout.ldq, dtype=torch.int64, device=self.device)
        self._ring, self._ring_n, self._next = [], ring, 0

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def _stream(self):
        return self.dstream.stream if self.dstream is not None else torch.cuda.current_stream(self._dev_index)

    def put(self, slot: int, update):
        """Stage one upload (dict, or list of the non-float32 entries, then the bits) into ``slot``; errors surface
        here, synchronously."""
        lay = self.layout
        side, bits = upload_plan_vote(lay, update, self.device)
        if not 0 <= slot < self.capacity:
            raise IndexError(f"slot {slot} of {self.capacity}")
        if isinstance(bits, torch.Tensor) and all(isinstance(v, torch.Tensor) for _, v in side):
            with self._on():
                if self.dstream is not None:
                    self.dstream.wait_caller()  # the caller's device tensors
                with torch.cuda.stream(self._stream()):
                    for e, v in side:
                        self.xi[slot, e.offset:e.offset + e.numel].copy_(v.reshape(-1), non_blocking=True)
                    self.bits[slot, :self.PB].copy_(bits, non_blocking=True)
            return
        if not self._ring:
            for _ in range(self._ring_n):
                hb = torch.zeros(max(16, self.ldb), dtype=torch.uint8).pin_memory()
                hi = torch.zeros(lay.ldq, dtype=torch.int64).pin_memory()
                self._ring.append([hb, hi, hb.numpy(), hi.numpy(), None])
        r = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        if r[4] is not None:
            r[4].synchronize()  # the previous H2Ds out of these pinned rows have completed
        for e, v in side:
            if isinstance(v, torch.Tensor):  # a device entry among host ones
                v = v.cpu().numpy()
            r[3][e.offset:e.offset + e.numel] = v.reshape(-1)
        r[2][:self.PB] = bits.cpu().numpy() if isinstance(bits, torch.Tensor) else bits
        with self._on():
            st = self._stream()
            with torch.cuda.stream(st):
                if lay.P:
                    self.bits[slot, :self.PB].copy_(r[0][:self.PB], non_blocking=True)
                if lay.Q:
                    self.xi[slot, :lay.Q].copy_(r[1][:lay.Q], non_blocking=True)
            if r[4] is None:
                r[4] = torch.cuda.Event()
            r[4].record(st)


class VoteRound:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, over a ``VoteStaging``."""

    policy = "fedavg"
    cg = None        # never client-sharded
    head = 0         # no head launch, no small-round mirror path
    sig_plan = None  # no cohort signatures

    def __init__(self, layout: BucketLayout, device, K: int, policy: str, spec, *, staging: VoteStaging,
                 last_f32: torch.Tensor, capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None):
        self.upload_vote = spec = VoteSpec.of(spec)
        if policy != "fedavg":
            raise refuse(f"a {policy} round", spec)
        if not 1 <= K <= (1 << 24):
            raise ValueError("a majority-vote round needs 1 <= K <= 2^24 client results")
        self.layout, self.device, self.K = layout, torch.device(device), int(K)
        self.dstream, self.staging, self.last_f32 = dstream, staging, last_f32
        self.cap = min(staging.capacity, capacity or staging.capacity)
        self.n = self.slot = self.chunks_done = 0
        with self._on():
            if staging.side_scratch is None:
                staging.side_scratch = (torch.empty(layout.ldq, dtype=torch.int64, device=self.device),
                                        torch.empty(layout.ldq, dtype=torch.float64, device=self.device))
            self._counts = torch.zeros(max(4, layout.ld), dtype=torch.int32, device=self.device)
        self.acc_i, self.acc_d = staging.side_scratch

    @property
    def counts(self) -> torch.Tensor:
        """The tally so far, int32 [P]: for every column the staged-and-folded uploads that voted "down" (their sign
        bit set).  Complete, and still readable, after ``finalize_mean``."""
        return self._counts[:self.layout.P]

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def add(self, update, *, weight: Optional[float] = None, loss=None, learning_rate=None, q=None):
        """Stage one arriving vote upload (every client has one vote: ``weight`` is not used)."""
        if self.n >= self.K:
            raise RuntimeError(f"round already has its K={self.K} results")
        if self.slot == self.cap:
            self._fold_chunk()
        self.staging.put(self.slot, update)
        self.slot += 1
        self.n += 1

    def adopt_resident(self, n: int):
        """Measurement hook, as ``DeviceRound.adopt_resident``: take ``n`` arrivals whose uploads are ALREADY in the
        staging slots [slot, slot + n), written there on the device (tools/vote_reduce_measure.py)."""
        if n < 0 or self.slot + n > self.cap or self.n + n > self.K:
            raise ValueError(f"adopt_resident: {n} arrivals do not fit (slot {self.slot} of {self.cap}, "
                             f"{self.n} of K={self.K})")
        self.slot += n
        self.n += n

    def _reduce_chunk(self):
        """The staged chunk's votes onto the tally (the same tally across chunks), and its side-table sums."""
        L, st, n = self.layout, self.staging, self.slot
        first = self.chunks_done == 0
        if n > 0 and L.P > 0:
            kv.count_votes(st.bits, n, L.P, self._counts, accumulate=True)  # _counts starts a round at zero
        kx.side_accumulate(st.xi, n, L.Q, 0, acc_i=self.acc_i, acc_d=self.acc_d, accumulate=not first)
        self.chunks_done += 1
        self.slot = 0

    @on_stream
    def _fold_chunk(self):
        """Fold the staged chunk into the running tally (not the last chunk of the round)."""
        self._reduce_chunk()

    def _check_complete(self):
        if self.n != self.K:
            raise RuntimeError(f"finalize with {self.n} of K={self.K} results")

    @on_stream
    def finalize_mean(self, denom32: float, denom64: float, *, out: torch.Tensor, cur_side: torch.Tensor,
                      model_side: Optional[torch.Tensor] = None, yogi: Optional[dict] = None,
                      mirror: Optional[torch.Tensor] = None):
        """Count the last chunk, then ``out`` <- the round's starting model plus the vote's step (fvt_finish); the
        side table as ``DeviceRound.finalize_mean`` (server-step rounds take ``out`` as the mean, then their step)."""
        if yogi is not None:
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)", self.upload_vote)
        self._check_complete()
        if float(denom32) != float(np.float32(self.K)):
            raise ValueError(f"a majority-vote round divides by its client count K={self.K}, not {denom32}")
        L, spec = self.layout, self.upload_vote
        self._reduce_chunk()
        if L.P > 0:
            kv.finish_vote(self._counts, self.last_f32, L.P, self.K, spec.lr, out, mode=spec.mode, mirror=mirror)
        kx.side_close(L.Q, 0, denom64, acc_i=self.acc_i, acc_d=self.acc_d, cur=cur_side, model=model_side)
