"""A round whose client uploads arrive and are staged as low-rank factors and are multiplied out on the matrix unit.

What an executor uploads is, for every weight matrix worth factoring, two thin factors ``Ut [r, O]``, ``V [r, I]`` of
its update ``d = x - L`` against the model ``L`` it was sent for this round, and the dense delta of every other
float32 entry (fedscale_amd/cloud/execution/lowrank_upload.py; include/fedlowrank.h states the formats and the
arithmetic).  ``LowRankStaging`` is [capacity, ldf] float32 rows of factors — ``r (O + I)`` floats for ``O I`` on the
wire, per staged client and per reduction pass — and ``LowRankRound`` is what ``TorchModelAdapter._apply_round`` and
the aggregator mixins use of ``DeviceRound``: ``flr_reduce`` forms the sum over clients of ``Ut^T V`` per entry in one
launch per staged chunk, in arrival order, and the round is closed by ``fcl_finish`` (include/fedclip.h) against the
round's snapshot of ``L``: new model = L + chain / K.  The int64 side table travels and reduces as in ``DeviceRound``.

Opt-in (``TorchModelAdapter(upload_lowrank=rank)``); FedAvg and — as the mean followed by the server step — fed-yogi,
fed-adam, fed-adagrad or fed-avgm.  FedBuff (a stale client's base is not this round's ``L``), q-FedAvg, every other
upload format, sharded models, client-sharded ranks, cohort signatures, clip, trim, krum, geomed and secagg are
refused.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import kernels as kx
from . import kernels_clip as kc
from . import kernels_lowrank as kl
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout, default_pack_workers
from .cloud.execution.lowrank_upload import check_rank
from .round import on_stream
from .state import DeviceStream

_I64, _F32 = np.dtype(np.int64), np.dtype(np.float32)


def refuse(what: str, rank=None) -> NotImplementedError:
    """The error of a combination the low-rank delta-upload path does not take."""
    return NotImplementedError(f"upload_lowrank={rank!r} combined with {what} is not supported: low-rank delta uploads "
                               f"take FedAvg, fed-yogi, fed-adam, fed-adagrad and fed-avgm rounds of one whole model "
                               f"on one device")


def layout_dims(layout: BucketLayout, rank: int) -> np.ndarray:
    """``kernels_lowrank.entry_dims`` of the layout's float32 entries."""
    return kl.entry_dims([e.shape for e in layout.f_entries], rank)


def default_capacity_lowrank(layout: BucketLayout, K: int, ldf: int, device, budget_fraction: float = 0.5) -> int:
    """Clients per chunk, from rows of ldf floats: all K when they fit in ``budget_fraction`` of the free HBM."""
    free, _ = torch.cuda.mem_get_info(device)
    per_client = ldf * 4 + layout.ldq * 8
    return min(max(1, int(free * budget_fraction) // max(1, per_client)), max(1, K))


def upload_plan_lowrank(layout: BucketLayout, update, rank: int, dims: np.ndarray, device=None) -> list:
    """Validate one low-rank upload against the layout (no GPU needed for host entries): a list, in layout order, of
    (entry, value) — value a C-contiguous host array or a tensor on ``device``.  A factored entry takes a float32
    [rank, O + I] array, a dense one float32 in the entry's shape, the rest int64; TypeError names the entry whose
    dtype or shape does not fit."""
    values = layout.values_of(update)
    want = {}
    for e, (O, I) in zip(layout.f_entries, dims.tolist()):
        want[e.index] = (rank, O + I) if I else e.shape
    plan = []
    for e in layout.entries:
        v = values[e.index]
        shape = want.get(e.index, e.shape)
        t_want, n_want = (torch.float32, _F32) if e.kind == "f" else (torch.int64, _I64)
        what = "the factors [rank, O + I] of the entry" if shape != e.shape else "the entry's shape"
        if isinstance(v, torch.Tensor):
            if v.dtype != t_want:
                raise TypeError(f"{e.name}: dtype {v.dtype}, this staging takes {t_want} for the entry "
                                f"(upload_lowrank={rank})")
            if tuple(v.shape) != shape:
                raise TypeError(f"{e.name}: shape {tuple(v.shape)} != {shape}, {what} (upload_lowrank={rank}; see "
                                f"lowrank_upload.LowRankCompressor)")
            v = v.detach()
            v = (v if v.is_contiguous() else v.contiguous()) if device is not None and v.device == device \
                else v.cpu().contiguous().numpy()
        else:
            v = v if type(v) is np.ndarray else np.asarray(v)
            if v.dtype != n_want:
                raise TypeError(f"{e.name}: dtype {v.dtype}, this staging takes {n_want} for the entry "
                                f"(upload_lowrank={rank})")
            if v.shape != shape:
                raise TypeError(f"{e.name}: shape {tuple(v.shape)} != {shape}, {what} (upload_lowrank={rank}; see "
                                f"lowrank_upload.LowRankCompressor)")
            v = v if v.flags.c_contiguous else np.ascontiguousarray(v)
        plan.append((e, v))
    return plan


class LowRankStaging:
    """Device staging area for up to ``capacity`` low-rank client uploads: ``rows`` [capacity, ldf] float32 (the
    staged format of include/fedlowrank.h, zero-filled once: padding is never written), ``xi`` [capacity, ldq] int64.
    Host uploads are gathered into one pinned row (a ring of two) by ``fa_host_gather``, one piece per staged factor
    row, and cross PCIe in one H2D on the staging's stream; an event per pinned row guards its reuse."""

    def __init__(self, layout: BucketLayout, device, capacity: int, rank: int, dstream: Optional[DeviceStream] = None,
                 ring: int = 2, pack_workers: Optional[int] = None):
        self.rank = check_rank(rank)
        if layout.world != 1:
            raise refuse("a parameter-sharded layout", self.rank)
        self.layout, self.device, self.dstream = layout, torch.device(device), dstream
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.capacity = int(capacity)
        self.pack_workers = pack_workers or default_pack_workers()
        self.side_scratch = None  # (int64, float64) side-table sums of a round, reused
        self.dims = layout_dims(layout, self.rank)
        self.table = kl.TileTable.of(self.dims, self.rank, self.device)
        self.ldf = self.table.ldf
        _, self.offsets = kl.row_layout(self.rank, self.dims)
        self.used = int(kl.parse_table(self.table.host)[0]["row_floats"])
        with self._on():
            self.rows = torch.zeros(self.capacity, self.ldf, dtype=torch.float32, device=self.device)
            self.xi = torch.zeros(self.capacity, layout.ldq, dtype=torch.int64, device=self.device)
        self._ring, self._ring_n, self._next = [], ring, 0
        # the static half of the gather: per float32 entry the pieces (source byte offset, destination byte offset,
        # bytes) of its array — one per staged factor row
        self._pieces = []
        r = self.rank
        for (O, I), (uo, vo) in zip(self.dims.tolist(), self.offsets.tolist()):
            if I:
                O4, I4 = (O + 3) // 4 * 4, (I + 3) // 4 * 4
                p = [(4 * j * (O + I), 4 * (uo + j * O4), 4 * O) for j in range(r)]
                p += [(4 * (j * (O + I) + O), 4 * (vo + j * I4), 4 * I) for j in range(r)]
            else:
                p = [(0, 4 * uo, 4 * O)] if O else []
            self._pieces.append(np.asarray(p, dtype=np.int64).reshape(-1, 3))
        cat = np.concatenate(self._pieces) if self._pieces else np.zeros((0, 3), dtype=np.int64)
        self._src_rel = np.ascontiguousarray(cat[:, 0]).astype(np.uint64)
        self._dst_offs, self._sizes = np.ascontiguousarray(cat[:, 1]), np.ascontiguousarray(cat[:, 2])
        self._counts = [len(p) for p in self._pieces]

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def _stream(self):
        return self.dstream.stream if self.dstream is not None else torch.cuda.current_stream(self._dev_index)

    def put(self, slot: int, update):
        """Stage one upload (dict, or list in layout order) into ``slot``; errors surface here, synchronously."""
        lay, r = self.layout, self.rank
        plan = upload_plan_lowrank(lay, update, r, self.dims, self.device)
        if not 0 <= slot < self.capacity:
            raise IndexError(f"slot {slot} of {self.capacity}")
        f_rank = {e.index: i for i, e in enumerate(lay.f_entries)}
        if plan and all(isinstance(v, torch.Tensor) for _, v in plan):
            with self._on():
                if self.dstream is not None:
                    self.dstream.wait_caller()  # the caller's device tensors
                row = self.rows[slot]
                for e, v in plan:
                    if e.kind == "i":
                        self.xi[slot, e.offset:e.offset + e.numel].copy_(v.reshape(-1), non_blocking=True)
                        continue
                    (O, I), (uo, vo) = self.dims[f_rank[e.index]].tolist(), self.offsets[f_rank[e.index]].tolist()
                    if I:
                        O4, I4, r2 = (O + 3) // 4 * 4, (I + 3) // 4 * 4, (r + 1) // 2 * 2
                        row[uo:uo + r2 * O4].view(r2, O4)[:r, :O].copy_(v[:, :O], non_blocking=True)
                        row[vo:vo + r2 * I4].view(r2, I4)[:r, :I].copy_(v[:, O:], non_blocking=True)
                    elif O:
                        row[uo:uo + O].copy_(v.reshape(-1), non_blocking=True)
            return
        if not self._ring:
            for _ in range(self._ring_n):
                hf = torch.zeros(self.ldf, dtype=torch.float32).pin_memory()
                hi = torch.zeros(lay.ldq, dtype=torch.int64).pin_memory()
                self._ring.append([hf, hi, hf.numpy(), hi.numpy(), None])
        ring = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        if ring[4] is not None:
            ring[4].synchronize()  # the previous H2Ds out of these pinned rows have completed
        bases, keep = [], []
        for e, v in plan:
            if isinstance(v, torch.Tensor):  # a device entry among host ones
                v = v.cpu().numpy()
            if e.kind == "i":
                ring[3][e.offset:e.offset + e.numel] = v.reshape(-1)
            else:
                keep.append(v)
                bases.append(v.__array_interface__["data"][0])
        if len(self._sizes):
            from . import _native

            ps = np.repeat(np.asarray(bases, dtype=np.uint64), self._counts) + self._src_rel
            _native.call("fa_host_gather", ring[2].__array_interface__["data"][0], ps.ctypes.data,
                         self._dst_offs.ctypes.data, self._sizes.ctypes.data, len(ps), int(self.pack_workers))
        del keep
        with self._on():
            st = self._stream()
            with torch.cuda.stream(st):
                if self.used:
                    self.rows[slot, :self.used].copy_(ring[0][:self.used], non_blocking=True)
                if lay.Q:
                    self.xi[slot, :lay.Q].copy_(ring[1][:lay.Q], non_blocking=True)
            if ring[4] is None:
                ring[4] = torch.cuda.Event()
            ring[4].record(st)


class LowRankRound:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, over a ``LowRankStaging``."""

    policy = "fedavg"
    cg = None        # never client-sharded
    head = 0         # no head launch, no small-round mirror path
    sig_plan = None  # no cohort signatures

    def __init__(self, layout: BucketLayout, device, K: int, policy: str, *, staging: LowRankStaging,
                 last_f32: torch.Tensor, capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None):
        if policy != "fedavg":
            raise refuse(f"a {policy} round", staging.rank)
        if K < 1:
            raise ValueError("a round needs K >= 1 client results")
        self.layout, self.device, self.K = layout, torch.device(device), int(K)
        self.dstream, self.staging, self.last_f32 = dstream, staging, last_f32
        self.upload_lowrank = staging.rank
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
        """Stage one arriving low-rank upload (in arrival order)."""
        if self.n >= self.K:
            raise RuntimeError(f"round already has its K={self.K} results")
        if self.slot == self.cap:
            self._fold_chunk()
        self.staging.put(self.slot, update)
        self.slot += 1
        self.n += 1

    def adopt_resident(self, n: int):
        """Measurement hook, as ``DeviceRound.adopt_resident``: take ``n`` arrivals whose uploads are ALREADY in the
        staging slots [slot, slot + n), written there on the device (tools/lowrank_measure.py)."""
        if n < 0 or self.slot + n > self.cap or self.n + n > self.K:
            raise ValueError(f"adopt_resident: {n} arrivals do not fit (slot {self.slot} of {self.cap}, "
                             f"{self.n} of K={self.K})")
        self.slot += n
        self.n += n

    def _reduce_chunk(self):
        """The staged chunk's factors multiplied out onto the chain (the same chain across chunks), and its
        side-table sums."""
        L, st, n = self.layout, self.staging, self.slot
        first = self.chunks_done == 0
        if n > 0 and L.P > 0:
            kl.reduce_lowrank(st.rows, n, st.table, self.chain, acc_in=None if first else self.chain)
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
        noise); the side table as ``DeviceRound.finalize_mean`` (rounds with a server step take ``out`` as the mean,
        then the step)."""
        if yogi is not None:
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)", self.upload_lowrank)
        self._check_complete()
        den = float(np.float32(self.K))
        if float(denom32) != den:
            raise ValueError(f"a low-rank delta round divides by its client count K={self.K}, not {denom32}")
        L = self.layout
        self._reduce_chunk()
        kc.finish(self.chain, self.last_f32, L.P, den, out, mirror=mirror)
        kx.side_close(L.Q, 0, denom64, acc_i=self.acc_i, acc_d=self.acc_d, cur=cur_side, model=model_side)
