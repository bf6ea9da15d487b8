"""A secure-aggregation round: client uploads arrive as masked integers mod 2^32 and are unmasked on the device.

Secure aggregation after Bonawitz et al. (CCS 2017) and Bell et al. (CCS 2020): an executor uploads its update
``d = x - L`` against the model ``L`` it was sent for this round as fixed-point integers mod 2^32, hidden under
pseudorandom masks (fedscale_amd/cloud/execution/secagg_upload.py; include/fedsecagg.h states the arithmetic).  The
pairwise masks cancel in the sum, the self masks are removed once by the server from keys the protocol reconstructs,
and the server's data path handles the sum and nothing else.  ``MaskedStaging`` is ``QuantStaging`` with
[capacity, ld] rows of 32-bit words — 4 bytes per parameter on the wire, per staged client and per reduction pass —
and ``SecAggRound`` is what ``TorchModelAdapter._apply_round`` and the aggregator mixins use of ``DeviceRound``:
``fsa_reduce`` sums the rows mod 2^32 (no order changes a bit), ``fsa_mask_sum`` removes the masks the caller names,
and ``fsa_finish`` turns the sum into new model = L + sum / (2^f K), counting the columns that left [-K B, K B] — which
a correct unmask never does and a wrong or missing key does in nearly every column.  The int64 side table travels and
reduces as in ``DeviceRound``, unmasked.

What is here is the arithmetic.  Key agreement, secret sharing, dropout recovery and authenticated channels are the
deployment's protocol: the caller supplies 256-bit keys and says which are added and which subtracted, so any mask
graph (complete, k-regular, ring) works ("Secure aggregation").

Opt-in (``TorchModelAdapter(upload_secagg=SecAggSpec(...))``); FedAvg and — as the mean followed by the existing YoGi
step — fed-yogi, fed-adam, fed-adagrad or fed-avgm (the mean, then the server step).  FedBuff, q-FedAvg, clip, trim, Krum, geometric median, 16-bit, MXFP8 and top-k uploads, cohort
signatures, sharded layouts and client-sharded ranks are refused: each of them needs individual uploads, which is what
secure aggregation hides.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native_secagg as NS
from . import kernels as kx
from . import kernels_secagg as ks
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout, default_pack_workers
from .round import on_stream
from .state import DeviceStream

_I64, _U32 = np.dtype(np.int64), np.dtype(np.uint32)
_INT32_MAX = (1 << 31) - 1
# the torch dtypes an upload's words may arrive in: int32 (what this path allocates and copies) and, where this torch
# build has it, uint32 — the same bits, staged through an int32 view
_WORD_DTYPES = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)


class SecAggUnmaskError(RuntimeError):
    """The unmasked sum left [-K B, K B] in ``count`` of ``P`` columns: a key handed to ``SecAggRound.unmask`` is wrong
    or missing (or an executor's masks were).  The round was not applied; the model is what it was."""

    def __init__(self, count: int, P: int, K: int, spec: "SecAggSpec"):
        self.count, self.P = int(count), int(P)
        super().__init__(f"secure aggregation: {count} of {P} columns of the unmasked sum are outside "
                         f"[-K B, K B] (K={K}, {spec!r}): a mask key is wrong or missing; the round was not applied")


def refuse(what: str) -> NotImplementedError:
    """The error of a combination the secure-aggregation path does not take."""
    return NotImplementedError(f"upload_secagg (SecAggSpec / device_upload_secagg) combined with {what} is not "
                               f"supported: secure aggregation takes FedAvg and fed-yogi rounds of one whole model on "
                               f"one device — selectors, clipping and other per-client steps need individual uploads, "
                               f"which is what secure aggregation hides")


class SecAggSpec:
    """``frac_bits`` f: the fixed-point fraction bits, an int in [0, 30] — an update is rounded to a multiple of
    2^-f.  ``mag_bits`` b: an int in [1, 30] — an encoded element is clamped to [-B, B], B = 2^b - 1, so updates up
    to about 2^(b - f) in magnitude pass unclamped.  ``verify``: ``finalize_mean`` reads the range check's counter
    (one host synchronisation per round) and raises ``SecAggUnmaskError`` when it is not zero.  A round of K uploads
    needs K * B <= 2^31 - 1: the defaults (16, 20) allow K <= 2048."""

    __slots__ = ("frac_bits", "mag_bits", "verify")

    def __init__(self, frac_bits=16, mag_bits=20, verify=True):
        if isinstance(frac_bits, SecAggSpec):
            frac_bits, mag_bits, verify = frac_bits.frac_bits, frac_bits.mag_bits, frac_bits.verify
        for name, v, lo, hi in (("frac_bits", frac_bits, 0, NS.MAX_FRAC_BITS), ("mag_bits", mag_bits, 1, NS.MAX_MAG_BITS)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"SecAggSpec: {name}={v!r} must be an int in [{lo}, {hi}]")
        if not isinstance(verify, (bool, np.bool_)):
            raise ValueError(f"SecAggSpec: verify={verify!r} must be a bool")
        object.__setattr__(self, "frac_bits", int(frac_bits))
        object.__setattr__(self, "mag_bits", int(mag_bits))
        object.__setattr__(self, "verify", bool(verify))

    @classmethod
    def of(cls, what) -> "SecAggSpec":
        """The spec of what ``upload_secagg`` and ``device_upload_secagg`` take: a spec, or True (the defaults)."""
        if isinstance(what, SecAggSpec):
            return what
        if what is True:
            return cls()
        raise TypeError(f"upload_secagg: expected a fedscale_amd.secagg_round.SecAggSpec (or True), got {what!r}")

    @property
    def bound(self) -> int:
        """B = 2^mag_bits - 1, the largest magnitude of an encoded element."""
        return (1 << self.mag_bits) - 1

    def max_clients(self) -> int:
        """The largest K with K * B <= 2^31 - 1."""
        return _INT32_MAX // self.bound

    def check_clients(self, K: int) -> int:
        """K when a round of K uploads cannot wrap (K * B <= 2^31 - 1); ValueError otherwise."""
        K = int(K)
        if K < 1:
            raise ValueError("a round needs K >= 1 client results")
        if K * self.bound > _INT32_MAX:
            raise ValueError(f"{self!r}: a round of K={K} uploads can wrap mod 2^32 (K * (2^{self.mag_bits} - 1) > "
                             f"2^31 - 1); this spec allows K <= {self.max_clients()} (lower mag_bits, or K)")
        return K

    def __setattr__(self, name, value):
        raise AttributeError("SecAggSpec is immutable")

    def __reduce__(self):
        return (SecAggSpec, (self.frac_bits, self.mag_bits, self.verify))

    def __repr__(self):
        return f"SecAggSpec(frac_bits={self.frac_bits!r}, mag_bits={self.mag_bits!r}, verify={self.verify!r})"

    def __eq__(self, other):
        return (isinstance(other, SecAggSpec) and other.frac_bits == self.frac_bits
                and other.mag_bits == self.mag_bits and other.verify == self.verify)

    def __hash__(self):
        return hash((self.frac_bits, self.mag_bits, self.verify))


def default_capacity_secagg(layout: BucketLayout, K: int, device, budget_fraction: float = 0.5) -> int:
    """Clients per chunk, from rows of 4 * ld bytes: all K when they fit in ``budget_fraction`` of the free HBM."""
    free, _ = torch.cuda.mem_get_info(device)
    per_client = layout.ld * 4 + layout.ldq * 8
    return min(max(1, int(free * budget_fraction) // max(1, per_client)), max(1, K))


def upload_plan_secagg(layout: BucketLayout, update, device=None):
    """Validate one masked upload against the layout (no GPU needed for host entries): a list, in layout order, of
    (entry, value) — value a C-contiguous host array (uint32 words / int64) or a tensor on ``device`` (int32 words /
    int64).  TypeError names the entry whose dtype or shape does not fit — a float32 array included: the staging holds
    masked words, and a silent cast would hide a misconfigured executor."""
    values = layout.values_of(update)

    def fit(name, v, kind, shape):
        takes = "uint32 arrays of masked words" if kind == "f" else "int64"
        if isinstance(v, torch.Tensor):
            ok = v.dtype in _WORD_DTYPES if kind == "f" else v.dtype == torch.int64
            if not ok:
                raise TypeError(f"{name}: dtype {v.dtype}, this staging takes "
                                f"{'torch.int32 (or uint32) words' if kind == 'f' else 'torch.int64'} for the entry "
                                f"(upload_secagg; see secagg_upload.compress_secagg)")
            if tuple(v.shape) != shape:
                raise TypeError(f"{name}: shape {tuple(v.shape)} != model shape {shape}")
            v = v.detach()
            if kind == "f" and v.dtype != torch.int32:
                v = v.view(torch.int32)
            if device is not None and v.device == device:
                return v if v.is_contiguous() else v.contiguous()
            v = v.cpu().contiguous().numpy()
            return v.view(np.uint32) if kind == "f" else v
        v = v if type(v) is np.ndarray else np.asarray(v)
        if v.dtype != (_U32 if kind == "f" else _I64):
            raise TypeError(f"{name}: dtype {v.dtype}, this staging takes {takes} for the entry (upload_secagg; see "
                            f"secagg_upload.compress_secagg)")
        if v.shape != shape:
            raise TypeError(f"{name}: shape {tuple(v.shape)} != model shape {shape}")
        return v if v.flags.c_contiguous else np.ascontiguousarray(v)

    return [(e, fit(e.name, values[e.index], e.kind, e.shape)) for e in layout.entries]


class MaskedStaging:
    """Device staging area for up to ``capacity`` masked client uploads: ``y`` [capacity, ld] int32 (uint32 words, the
    same bits), ``xi`` [capacity, ldq] int64.  Host uploads are gathered into one pinned row per array (a ring of two)
    by ``fa_host_gather`` and cross PCIe in one H2D per array on the staging's stream; an event per pinned row guards
    its reuse."""

    def __init__(self, layout: BucketLayout, device, capacity: int, dstream: Optional[DeviceStream] = None,
                 ring: int = 2, pack_workers: Optional[int] = None):
        if layout.world != 1:
            raise refuse("a parameter-sharded layout")
        self.layout, self.device, self.dstream = layout, torch.device(device), dstream
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.capacity = int(capacity)
        self.pack_workers = pack_workers or default_pack_workers()
        self.side_scratch = None  # (int64, float64) side-table sums of a round, reused
        with self._on():
            self.y = torch.zeros(self.capacity, layout.ld, dtype=ks.WORD, device=self.device)
            self.xi = torch.zeros(self.capacity, layout.ldq, dtype=torch.int64, device=self.device)
        self._ring, self._ring_n, self._next = [], ring, 0
        # fp32 entries' places in a row of words, in bytes (static half of the gather)
        self._f_offs = np.asarray([4 * e.offset for e in layout.f_entries if e.numel], dtype=np.int64)
        self._f_sizes = np.asarray([4 * e.numel for e in layout.f_entries if e.numel], dtype=np.int64)

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def _stream(self):
        return self.dstream.stream if self.dstream is not None else torch.cuda.current_stream(self._dev_index)

    def put(self, slot: int, update):
        """Stage one upload (dict, or list in layout order) into ``slot``; errors surface here, synchronously."""
        lay = self.layout
        plan = upload_plan_secagg(lay, update, self.device)
        if not 0 <= slot < self.capacity:
            raise IndexError(f"slot {slot} of {self.capacity}")
        if plan and all(isinstance(v, torch.Tensor) for _, v in plan):
            with self._on():
                if self.dstream is not None:
                    self.dstream.wait_caller()  # the caller's device tensors
                for e, v in plan:
                    dst = self.y[slot] if e.kind == "f" else self.xi[slot]
                    dst[e.offset:e.offset + e.numel].copy_(v.reshape(-1), non_blocking=True)
            return
        if not self._ring:
            for _ in range(self._ring_n):
                hy = torch.zeros(lay.ld, dtype=ks.WORD).pin_memory()
                hi = torch.zeros(lay.ldq, dtype=torch.int64).pin_memory()
                self._ring.append([hy, hi, hy.numpy(), hi.numpy(), None])
        r = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        if r[4] is not None:
            r[4].synchronize()  # the previous H2Ds out of these pinned rows have completed
        ptrs, keep = [], []
        for e, v in plan:
            if isinstance(v, torch.Tensor):  # a device entry among host ones
                v = v.cpu().numpy()
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
                    self.y[slot, :lay.P].copy_(r[0][:lay.P], non_blocking=True)
                if lay.Q:
                    self.xi[slot, :lay.Q].copy_(r[1][:lay.Q], non_blocking=True)
            if r[4] is None:
                r[4] = torch.cuda.Event()
            r[4].record(st)


class SecAggRound:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, over a ``MaskedStaging``."""

    policy = "fedavg"
    cg = None        # never client-sharded
    head = 0         # no head launch, no small-round mirror path
    sig_plan = None  # no cohort signatures

    def __init__(self, layout: BucketLayout, device, K: int, policy: str, spec: SecAggSpec, *,
                 staging: MaskedStaging, last_f32: torch.Tensor, capacity: Optional[int] = None,
                 dstream: Optional[DeviceStream] = None):
        if policy != "fedavg":
            raise refuse(f"a {policy} round")
        spec = SecAggSpec.of(spec)
        spec.check_clients(K)
        self.layout, self.device, self.K = layout, torch.device(device), int(K)
        self.dstream, self.staging, self.last_f32 = dstream, staging, last_f32
        self.upload_secagg = spec
        self.cap = min(staging.capacity, capacity or staging.capacity)
        self.n = self.slot = self.chunks_done = 0
        self._keys = None  # (uint32 [M, 8] host array, n_add, nonce) once unmask() was called
        self._finished = False
        with self._on():
            if staging.side_scratch is None:
                staging.side_scratch = (torch.empty(layout.ldq, dtype=torch.int64, device=self.device),
                                        torch.empty(layout.ldq, dtype=torch.float64, device=self.device))
            self.total = torch.zeros(layout.ld, dtype=ks.WORD, device=self.device)
            self._oor = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.acc_i, self.acc_d = staging.side_scratch

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    @property
    def n_keys(self) -> int:
        """Keys handed to ``unmask`` (0 before it was called)."""
        return 0 if self._keys is None else len(self._keys[0])

    def add(self, update, *, weight: Optional[float] = None, loss=None, learning_rate=None, q=None):
        """Stage one arriving masked upload (in arrival order; the sum does not depend on it)."""
        if self.n >= self.K:
            raise RuntimeError(f"round already has its K={self.K} results")
        if self.slot == self.cap:
            self._fold_chunk()
        self.staging.put(self.slot, update)
        self.slot += 1
        self.n += 1

    def adopt_resident(self, n: int):
        """Measurement hook, as ``DeviceRound.adopt_resident``: take ``n`` arrivals whose uploads are ALREADY in the
        staging slots [slot, slot + n), written there on the device (tools/secagg_measure.py)."""
        if n < 0 or self.slot + n > self.cap or self.n + n > self.K:
            raise ValueError(f"adopt_resident: {n} arrivals do not fit (slot {self.slot} of {self.cap}, "
                             f"{self.n} of K={self.K})")
        self.slot += n
        self.n += n

    def unmask(self, sub_keys, add_keys, nonce=(0, 0, 0)):
        """Name the masks the finish removes from the sum, exactly once per round and before it is finished:
        ``sub_keys`` are subtracted — the self-mask keys of the clients that arrived, and the pairwise keys an arrived
        client ADDED towards a neighbour that dropped; ``add_keys`` are added — the pairwise keys an arrived client
        SUBTRACTED towards a neighbour that dropped.  Empty lists for a round with no masks.  ``nonce``: the round's,
        as the executors used it."""
        if self._keys is not None:
            raise RuntimeError("unmask() was already called for this round")
        nonce = ks.check_nonce(nonce)
        add, sub = ks.keys_array(list(add_keys)), ks.keys_array(list(sub_keys))
        if len(add) + len(sub) > NS.MAX_KEYS:
            raise ValueError(f"unmask: {len(add) + len(sub)} keys exceed the limit FSA_MAX_KEYS = {NS.MAX_KEYS}")
        self._keys = (np.concatenate([add, sub]), len(add), nonce)

    def _reduce_chunk(self):
        """The staged chunk's rows onto the running sum (the same sum across chunks), and its side-table sums."""
        L, st, n = self.layout, self.staging, self.slot
        first = self.chunks_done == 0
        if n > 0 and L.P > 0:
            ks.reduce32(st.y, n, L.P, self.total, acc_in=None if first else self.total)
        kx.side_accumulate(st.xi, n, L.Q, 0, acc_i=self.acc_i, acc_d=self.acc_d, accumulate=not first)
        self.chunks_done += 1
        self.slot = 0

    @on_stream
    def _fold_chunk(self):
        """Fold the staged chunk into the running sum (not the last chunk of the round)."""
        self._reduce_chunk()

    def _check_complete(self):
        if self.n != self.K:
            raise RuntimeError(f"finalize with {self.n} of K={self.K} results")

    def out_of_range(self) -> int:
        """Columns of the unmasked sum outside [-K B, K B], read from the device (synchronises); 0 for a correct
        unmask.  Only after the round was finished."""
        if not self._finished:
            raise RuntimeError("out_of_range() before the round was finished")
        return int(self._oor.item())

    @on_stream
    def finalize_mean(self, denom32: float, denom64: float, *, out: torch.Tensor, cur_side: torch.Tensor,
                      model_side: Optional[torch.Tensor] = None, yogi: Optional[dict] = None,
                      mirror: Optional[torch.Tensor] = None):
        """Reduce the last chunk, remove the masks ``unmask`` named, then ``out`` <- the round's starting model plus
        the mean update (fsa_finish); with ``verify`` the range check's counter is read and a non-zero count raises
        ``SecAggUnmaskError`` before the side table is closed.  The side table as ``DeviceRound.finalize_mean``
        (fed-yogi rounds take ``out`` as the mean, then the existing fa_yogi_step)."""
        spec = self.upload_secagg
        if yogi is not None:
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)")
        self._check_complete()
        if self._keys is None:
            raise RuntimeError("a secure-aggregation round is finished only after unmask(sub_keys, add_keys, nonce) "
                               "(empty lists for a round with no masks)")
        if self._finished:
            raise RuntimeError("the round was already finished")
        if float(denom32) != float(np.float32(self.K)):
            raise ValueError(f"a secure-aggregation round divides by its client count K={self.K}, not {denom32}")
        L = self.layout
        self._reduce_chunk()
        keys, n_add, nonce = self._keys
        if len(keys) and L.P > 0:
            dkeys = torch.from_numpy(keys.view(np.int32)).to(self.device, non_blocking=False)
            ks.mask_sum(dkeys, n_add, len(keys) - n_add, nonce, L.P, self.total, self.total)
        ks.finish(self.total, self.last_f32, L.P, spec.frac_bits, spec.mag_bits, self.K, out, self._oor,
                  mirror=mirror)
        self._finished = True
        if spec.verify:
            bad = int(self._oor.item())  # one host synchronisation per round
            if bad:
                raise SecAggUnmaskError(bad, L.P, self.K, spec)
        kx.side_close(L.Q, 0, denom64, acc_i=self.acc_i, acc_d=self.acc_d, cur=cur_side, model=model_side)
