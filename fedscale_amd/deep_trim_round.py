"""A FedAvg round that averages, for every parameter, only the middle of the K uploaded values at ANY depth: the t
smallest and the t largest are dropped on the device, 1 <= t, 2t < K — 10-20 % per side at K = 1000, the median at
any K, the inner trimmed mean of Bulyan.

The arithmetic is ``trim_round``'s (include/fedtrim.h, restated in include/feddeeptrim.h: order key, lo / hi and
their tie counts, the kept rule walked in arrival order, the chain from the first kept value, IEEE division by
float(K - 2t), int64 per-row drop counts), and where both run — t <= 16 — the bits are the same.  What differs is the
kernel: ``trim`` keeps 2t keys per column in registers and reads the rows twice; ``deep_trim`` holds tiles of all K
rows in LDS, selects there by radix, and reads the rows once (fedscale_amd/csrc/deep_trim.hip).  Rounds of up to
``fdt_max_rows()`` = 4096 uploads.

``DeepTrimmedRound`` is what ``TorchModelAdapter._apply_round`` and the aggregator mixins use of ``DeviceRound``, over
the ordinary fp32 ``ClientStaging``.  All K rows are resident: a round larger than the staging capacity is refused
when it begins (there is no chunk folding).  With t = 0 the round is plain unweighted FedAvg through ``ft_reduce``,
bit for bit.  Opt-in (``TorchModelAdapter.begin_round(deep_trim=...)``, ``DeviceAggregatorMixin.device_deep_trim``);
FedAvg and — as the mean followed by the existing server step — fed-yogi, fed-adam, fed-adagrad or fed-avgm.
``trim`` itself, norm clipping, Krum, the geometric median, every upload format, cohort signatures, sharded layouts,
FedBuff and q-FedAvg are refused.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _native_deeptrim as ND
from . import kernels as kx
from . import kernels_deeptrim as kd
from . import kernels_trim as kt
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout, ClientStaging
from .round import on_stream
from .state import DeviceStream


def refuse(what: str) -> NotImplementedError:
    """The error of a combination deep trimmed-mean aggregation does not take."""
    return NotImplementedError(f"deep_trim (DeepTrimSpec / device_deep_trim) combined with {what} is not supported: "
                               f"deep trimmed-mean aggregation takes FedAvg and server-optimizer rounds of float32 "
                               f"uploads to one whole model on one device")


class DeepTrimSpec:
    """``deep_trim``: a non-negative int — the count t dropped per side; a float in [0, 0.5) — the fraction per side,
    t = floor(f * K); or ``"median"`` — t = (K - 1) // 2.  The forms of ``TrimSpec``, without its depth limit."""

    __slots__ = ("trim",)

    def __init__(self, trim):
        if isinstance(trim, DeepTrimSpec):
            trim = trim.trim
        if isinstance(trim, str):
            if trim != "median":
                raise ValueError(f"DeepTrimSpec: trim={trim!r}: the only string form is 'median'")
        elif isinstance(trim, (int, np.integer)) and not isinstance(trim, (bool, np.bool_)):
            trim = int(trim)
            if trim < 0:
                raise ValueError(f"DeepTrimSpec: the count trim={trim!r} must be >= 0")
        elif isinstance(trim, (float, np.floating)):
            trim = float(trim)
            if not (math.isfinite(trim) and 0.0 <= trim < 0.5):
                raise ValueError(f"DeepTrimSpec: the fraction trim={trim!r} must lie in [0, 0.5)")
        else:
            raise ValueError(f"DeepTrimSpec: trim={trim!r} must be an int, a float in [0, 0.5) or 'median'")
        object.__setattr__(self, "trim", trim)

    def __setattr__(self, name, value):
        raise AttributeError("DeepTrimSpec is immutable")

    def __repr__(self):
        return f"DeepTrimSpec({self.trim!r})"

    def __eq__(self, other):
        return isinstance(other, DeepTrimSpec) and type(other.trim) is type(self.trim) and other.trim == self.trim

    def __hash__(self):
        return hash(("deep", type(self.trim).__name__, self.trim))

    def count(self, K: int) -> int:
        """The rows dropped per side of a round of K uploads; ValueError when the round cannot take it."""
        K = int(K)
        if K < 1:
            raise ValueError("a round needs K >= 1 client results")
        if isinstance(self.trim, str):  # "median"
            t = (K - 1) // 2
        elif isinstance(self.trim, float):
            t = int(math.floor(self.trim * K))
        else:
            t = self.trim
        if 2 * t >= K:
            raise ValueError(f"{self!r}: dropping t={t} per side leaves nothing of K={K} uploads (needs 2t < K)")
        if K > ND.MAX_ROWS:
            raise ValueError(f"{self!r}: K={K} uploads exceed the limit fdt_max_rows() = {ND.MAX_ROWS}")
        return t


class DeepTrimmedRound:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, averaging the kept rows only."""

    policy = "fedavg"
    cg = None        # never client-sharded
    head = 0         # no head launch, no small-round mirror path
    sig_plan = None  # no cohort signatures

    def __init__(self, layout: BucketLayout, device, K: int, deep_trim: DeepTrimSpec, *, staging: ClientStaging,
                 capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None, policy: str = "fedavg"):
        if not isinstance(deep_trim, DeepTrimSpec):
            raise TypeError(f"deep_trim: expected a DeepTrimSpec, got {type(deep_trim).__name__}")
        if policy != "fedavg":
            raise refuse(f"a {policy} round")
        if layout.world != 1:
            raise refuse("a parameter-sharded layout")
        self.t = deep_trim.count(K)  # (refuses K < 1)
        self.layout, self.device, self.K, self.deep_trim = layout, torch.device(device), int(K), deep_trim
        cap = min(staging.capacity, capacity or staging.capacity)
        if self.K > cap:
            raise ValueError(f"a deep trimmed round needs all K={self.K} uploads resident, the staging capacity is "
                             f"{cap}: there is no chunk folding (raise capacity=, or lower K)")
        self.dstream, self.staging, self.cap = dstream, staging, cap
        staging.generation += 1  # a new round takes the staging slots over
        self.generation = staging.generation
        self.n = self.slot = self.chunks_done = 0
        L = layout
        with self._on():
            if staging.side_scratch is None:
                staging.side_scratch = (torch.empty(L.ldq, dtype=torch.int64, device=self.device),
                                        torch.empty(L.ldq, dtype=torch.float64, device=self.device))
            self._dropped = torch.zeros((self.K, 2), dtype=torch.int64, device=self.device)
        self.acc_i, self.acc_d = staging.side_scratch
        self._host = None  # the drop counts once fetched

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def add(self, update, *, weight: Optional[float] = None, loss=None, learning_rate=None, q=None):
        """Stage one arriving upload (in arrival order)."""
        if self.n >= self.K:
            raise RuntimeError(f"round already has its K={self.K} results")
        self.staging.put(self.slot, update)
        self.slot += 1
        self.n += 1

    def adopt_resident(self, n: int):
        """Measurement hook, as ``DeviceRound.adopt_resident``: take ``n`` arrivals whose updates are ALREADY in the
        staging slots [slot, slot + n), written there on the device (tools/deep_trim_measure.py)."""
        if n < 0 or self.slot + n > self.cap or self.n + n > self.K:
            raise ValueError(f"adopt_resident: {n} arrivals do not fit (slot {self.slot} of {self.cap}, "
                             f"{self.n} of K={self.K})")
        self.slot += n
        self.n += n

    def _check_complete(self):
        if self.n != self.K:
            raise RuntimeError(f"finalize with {self.n} of K={self.K} results")

    @on_stream
    def finalize_mean(self, denom32: float, denom64: float, *, out: torch.Tensor, cur_side: torch.Tensor,
                      model_side: Optional[torch.Tensor] = None, yogi: Optional[dict] = None,
                      mirror: Optional[torch.Tensor] = None):
        """``out`` <- the trimmed mean of the staged rows in one launch (fdt_reduce; t = 0: ft_reduce, plain FedAvg);
        the side table as ``DeviceRound.finalize_mean`` (server-optimizer rounds take ``out`` as the mean, then the
        existing step)."""
        if yogi is not None:
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)")
        self._check_complete()
        if self.chunks_done:
            raise RuntimeError("the round is already finalized")
        if float(denom32) != float(np.float32(self.K)):
            raise ValueError(f"a deep trimmed round of K={self.K} uploads divides its kept rows by K - 2t itself; the "
                             f"caller's denominator must be float32(K), not {denom32}")
        self.staging.drain()
        L, st, K, t = self.layout, self.staging, self.K, self.t
        if L.P > 0:
            if t > 0:
                kd.reduce_deep(st.x, K, L.P, t, out, mirror=mirror, dropped=self._dropped)
            else:
                kt.reduce_trim(st.x, K, L.P, 0, out, mirror=mirror)
        kx.side_accumulate(st.xi, K, L.Q, 0, acc_i=self.acc_i, acc_d=self.acc_d, accumulate=False)
        kx.side_close(L.Q, 0, denom64, acc_i=self.acc_i, acc_d=self.acc_d, cur=cur_side, model=model_side)
        self.chunks_done = 1
        self.slot = 0

    # ---- what the round did, for operators (a host copy; the first call waits for the round's kernels) ----------
    def dropped(self) -> np.ndarray:
        """int64[K, 2]: in how many of the P columns each upload, in arrival order, was dropped as one of the t
        smallest ([:, 0]) and as one of the t largest ([:, 1])."""
        if self._host is None:
            self._check_complete()
            if not self.chunks_done:
                raise RuntimeError("the round is not finalized yet")
            with self._on():
                self._host = self._dropped.cpu().numpy()
        return self._host.copy()
