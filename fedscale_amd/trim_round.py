"""A FedAvg round that averages, for every parameter, only the middle of the K uploaded values: the t smallest and the
t largest are dropped on the device (the coordinate-wise trimmed mean; ``"median"`` is its limit case).

Server-side robust aggregation after Yin et al. (ICML 2018).  Unlike the norm clip of ``clip_round`` it needs no
bound that fits honest updates: an upload scaled by 1e15, or one full of NaNs, is simply among the values dropped.
For K uploads ``x_k`` in arrival order (include/fedtrim.h has the contract; fp32, rounded to nearest, never fused):

    key(v) = the total order -inf < ... < -0 < +0 < ... < +inf < NaN on fp32 bit patterns
    lo, hi = the t-th smallest / largest key of the column; ties at lo / hi are dropped first come, first dropped
    chain  = the first kept x_k, then + every later kept x_k in arrival order;  new value = chain / float(K - 2t)

What is trimmed is the whole fp32 bucket — parameters and fp32 buffers (BatchNorm statistics) alike; the int64 side
table takes plain FedAvg's path with denominator K.  With t = 0 the round is plain unweighted FedAvg, bit for bit.

``TrimmedRound`` is what ``TorchModelAdapter._apply_round`` and the aggregator mixins use of ``DeviceRound``, over the
ordinary fp32 ``ClientStaging``.  The selection needs all K rows resident: a round larger than the staging capacity
is refused when it begins (there is no chunk folding).  Opt-in (``TorchModelAdapter.begin_round(trim=...)``,
``DeviceAggregatorMixin.device_trim``); FedAvg and — as the trimmed mean followed by the existing YoGi step —
fed-yogi, fed-adam, fed-adagrad or fed-avgm (the mean, then the server step).  Norm clipping, 16-bit uploads, cohort signatures, sharded layouts, FedBuff and q-FedAvg are refused.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _native_trim as NT
from . import kernels as kx
from . import kernels_trim as kt
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout, ClientStaging
from .round import on_stream
from .state import DeviceStream


def refuse(what: str) -> NotImplementedError:
    """The error of a combination trimmed-mean aggregation does not take."""
    return NotImplementedError(f"trim (TrimSpec / device_trim) combined with {what} is not supported: trimmed-mean "
                               f"aggregation takes FedAvg and fed-yogi rounds of float32 uploads to one whole model "
                               f"on one device")


class TrimSpec:
    """``trim``: a non-negative int — the count t dropped per side; a float in [0, 0.5) — the fraction per side,
    t = floor(f * K); or ``"median"`` — t = (K - 1) // 2."""

    __slots__ = ("trim",)

    def __init__(self, trim):
        if isinstance(trim, TrimSpec):
            trim = trim.trim
        if isinstance(trim, (bool, np.bool_)):
            raise ValueError(f"TrimSpec: trim={trim!r} must be an int, a float in [0, 0.5) or 'median', not a bool")
        if isinstance(trim, str):
            if trim != "median":
                raise ValueError(f"TrimSpec: trim={trim!r}: the only string form is 'median'")
        elif isinstance(trim, (int, np.integer)):
            trim = int(trim)
            if trim < 0:
                raise ValueError(f"TrimSpec: the count trim={trim!r} must be >= 0")
        elif isinstance(trim, (float, np.floating)):
            trim = float(trim)
            if not (math.isfinite(trim) and 0.0 <= trim < 0.5):
                raise ValueError(f"TrimSpec: the fraction trim={trim!r} must lie in [0, 0.5)")
        else:
            raise ValueError(f"TrimSpec: trim={trim!r} must be an int, a float in [0, 0.5) or 'median'")
        object.__setattr__(self, "trim", trim)

    def __setattr__(self, name, value):
        raise AttributeError("TrimSpec is immutable")

    def __repr__(self):
        return f"TrimSpec({self.trim!r})"

    def __eq__(self, other):
        return isinstance(other, TrimSpec) and type(other.trim) is type(self.trim) and other.trim == self.trim

    def __hash__(self):
        return hash((type(self.trim).__name__, self.trim))

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
        if t > NT.MAX_TRIM:
            raise ValueError(f"{self!r}: t={t} per side at K={K} exceeds the limit ft_max_trim() = {NT.MAX_TRIM}")
        return t


class TrimmedRound:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, averaging the kept rows only."""

    policy = "fedavg"
    cg = None        # never client-sharded
    head = 0         # no head launch, no small-round mirror path
    sig_plan = None  # no cohort signatures

    def __init__(self, layout: BucketLayout, device, K: int, trim: TrimSpec, *, staging: ClientStaging,
                 capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None, policy: str = "fedavg"):
        if not isinstance(trim, TrimSpec):
            raise TypeError(f"trim: expected a TrimSpec, got {type(trim).__name__}")
        if policy != "fedavg":
            raise refuse(f"a {policy} round")
        if layout.world != 1:
            raise refuse("a parameter-sharded layout")
        self.t = trim.count(K)  # (refuses K < 1)
        self.layout, self.device, self.K, self.trim = layout, torch.device(device), int(K), trim
        cap = min(staging.capacity, capacity or staging.capacity)
        if self.K > cap:
            raise ValueError(f"a trimmed round needs all K={self.K} uploads resident, the staging capacity is {cap}: "
                             f"there is no chunk folding (raise capacity=, or lower K)")
        self.dstream, self.staging, self.cap = dstream, staging, cap
        staging.generation += 1  # a new round takes the staging slots over
        self.generation = staging.generation
        self.n = self.slot = self.chunks_done = 0
        L = layout
        with self._on():
            if staging.side_scratch is None:
                staging.side_scratch = (torch.empty(L.ldq, dtype=torch.int64, device=self.device),
                                        torch.empty(L.ldq, dtype=torch.float64, device=self.device))
            self._thr = kt.thresholds(L.P, self.device) if self.t > 0 else (None, None, None)
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
        staging slots [slot, slot + n), written there on the device (tools/trim_reduce_measure.py)."""
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
        """Select, then ``out`` <- the trimmed mean of the staged rows (ft_select, ft_reduce); the side table as
        ``DeviceRound.finalize_mean`` (fed-yogi rounds take ``out`` as the mean, then the existing fa_yogi_step)."""
        if yogi is not None:
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)")
        self._check_complete()
        if self.chunks_done:
            raise RuntimeError("the round is already finalized")
        if float(denom32) != float(np.float32(self.K)):
            raise ValueError(f"a trimmed round of K={self.K} uploads divides its kept rows by K - 2t itself; the "
                             f"caller's denominator must be float32(K), not {denom32}")
        self.staging.drain()
        L, st, K, t = self.layout, self.staging, self.K, self.t
        lo, hi, ties = self._thr
        if L.P > 0:
            if t > 0:
                kt.select(st.x, K, L.P, t, lo, hi, ties)
            kt.reduce_trim(st.x, K, L.P, t, out, lo=lo, hi=hi, ties=ties, mirror=mirror,
                           dropped=self._dropped if t > 0 else None)
        kx.side_accumulate(st.xi, K, L.Q, 0, acc_i=self.acc_i, acc_d=self.acc_d, accumulate=False)
        kx.side_close(L.Q, 0, denom64, acc_i=self.acc_i, acc_d=self.acc_d, cur=cur_side, model=model_side)
        self.chunks_done = 1
        self.slot = 0

    # ---- what the round did, for operators (a host copy; the first call waits for the round's kernels) ----------
    def dropped(self) -> np.ndarray:
        """int64[K, 2]: in how many of the P columns each upload, in arrival order, was dropped as one of the t
        smallest ([:, 0]) and as one of the t largest ([:, 1]).  An honest upload is dropped in about t / K of the
        columns on each side; one dropped in nearly all of them on one side is an outlier worth a look."""
        if self._host is None:
            self._check_complete()
            if not self.chunks_done:
                raise RuntimeError("the round is not finalized yet")
            with self._on():
                self._host = self._dropped.cpu().numpy()
        return self._host.copy()
