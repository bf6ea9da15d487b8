"""A FedAvg round that keeps whole uploads by their distance to the others and averages only those (Krum / Multi-Krum).

Server-side robust aggregation after Blanchard et al. (NeurIPS 2017).  The norm clip of ``clip_round`` needs a bound
tuned to honest updates and the trimmed mean of ``trim_round`` judges every parameter on its own; a colluding minority
that stays inside the honest range in every coordinate passes both.  Krum scores each upload by its squared distance
to its K - f - 2 nearest other uploads and keeps the m best-scored uploads whole.  For a round that starts from model
``L`` with K uploads ``x_k`` in arrival order (include/fedkrum.h has the contract):

    d_k   = x_k - L (fp32)                 G[i][j] = sum double(d_i) * double(d_j)   (fp64, on the matrix unit)
    dist2 = clamp((G[i][i] + G[j][j]) - 2 G[i][j]) to [+0, +inf], NaN -> +inf
    score = the K - f - 2 smallest dist2 of the row, added in ascending order
    kept  = the m smallest (score, arrival) with a finite score;  new model = L + (sum of kept d_k) / n_kept

What is selected is the whole fp32 bucket — parameters and fp32 buffers (BatchNorm statistics) alike; the int64 side
table takes plain FedAvg's path with denominator K.  An upload with an inf or NaN anywhere has an infinite score and
is never kept; when no upload has a finite score the model is left as it was.

``KrumRound`` is what ``TorchModelAdapter._apply_round`` and the aggregator mixins use of ``DeviceRound``, over the
ordinary fp32 ``ClientStaging``.  The distances need all K rows resident: a round larger than the staging capacity is
refused when it begins (there is no chunk folding).  Opt-in (``TorchModelAdapter.begin_round(krum=...)``,
``DeviceAggregatorMixin.device_krum``); FedAvg and — as the selected mean followed by the existing YoGi step —
fed-yogi, fed-adam, fed-adagrad or fed-avgm (the mean, then the server step).  Norm clipping, trimming, 16-bit, MXFP8 and top-k uploads, cohort signatures, sharded layouts, FedBuff and
q-FedAvg are refused.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _native_krum as NK
from . import kernels as kx
from . import kernels_clip as kc
from . import kernels_krum as kk
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout, ClientStaging
from .round import on_stream
from .state import DeviceStream


def refuse(what: str) -> NotImplementedError:
    """The error of a combination Krum aggregation does not take."""
    return NotImplementedError(f"krum (KrumSpec / device_krum) combined with {what} is not supported: Multi-Krum "
                               f"aggregation takes FedAvg and fed-yogi rounds of float32 uploads to one whole model "
                               f"on one device")


class KrumSpec:
    """``f``: a non-negative int — the uploads assumed bad; or a float in [0, 0.5) — their fraction, f = floor(frac *
    K).  ``m``: the uploads kept, an int >= 1; None keeps K - f (Multi-Krum); 1 is Krum."""

    __slots__ = ("f", "m")

    def __init__(self, f, m=None):
        if isinstance(f, KrumSpec):
            if m is None:
                m = f.m
            f = f.f
        if isinstance(f, (bool, np.bool_)):
            raise ValueError(f"KrumSpec: f={f!r} must be an int or a float in [0, 0.5), not a bool")
        if isinstance(f, (int, np.integer)):
            f = int(f)
            if f < 0:
                raise ValueError(f"KrumSpec: the count f={f!r} must be >= 0")
        elif isinstance(f, (float, np.floating)):
            f = float(f)
            if not (math.isfinite(f) and 0.0 <= f < 0.5):
                raise ValueError(f"KrumSpec: the fraction f={f!r} must lie in [0, 0.5)")
        else:
            raise ValueError(f"KrumSpec: f={f!r} must be an int or a float in [0, 0.5)")
        if m is not None:
            if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)):
                raise ValueError(f"KrumSpec: m={m!r} must be None or an int >= 1")
            m = int(m)
            if m < 1:
                raise ValueError(f"KrumSpec: m={m!r} must be None or an int >= 1")
        object.__setattr__(self, "f", f)
        object.__setattr__(self, "m", m)

    def __setattr__(self, name, value):
        raise AttributeError("KrumSpec is immutable")

    def __repr__(self):
        return f"KrumSpec({self.f!r}, m={self.m!r})"

    def __eq__(self, other):
        return (isinstance(other, KrumSpec) and type(other.f) is type(self.f) and other.f == self.f
                and other.m == self.m)

    def __hash__(self):
        return hash((type(self.f).__name__, self.f, self.m))

    def counts(self, K: int) -> tuple:
        """(f, m) of a round of K uploads; ValueError when the round cannot take them."""
        K = int(K)
        if K < 1:
            raise ValueError("a round needs K >= 1 client results")
        f = int(math.floor(self.f * K)) if isinstance(self.f, float) else self.f
        if 2 * f + 3 > K:
            raise ValueError(f"{self!r}: f={f} bad uploads need 2f + 3 <= K, K={K} is too few")
        if K > NK.MAX_K:
            raise ValueError(f"{self!r}: K={K} exceeds the limit FK_MAX_K = {NK.MAX_K}")
        m = K - f if self.m is None else self.m
        if m > K - f:
            raise ValueError(f"{self!r}: m={m} kept uploads need m <= K - f = {K - f}")
        return f, m


class KrumRound:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, averaging the selected rows only."""

    policy = "fedavg"
    cg = None        # never client-sharded
    head = 0         # no head launch, no small-round mirror path
    sig_plan = None  # no cohort signatures

    def __init__(self, layout: BucketLayout, device, K: int, krum: KrumSpec, *, staging: ClientStaging,
                 last_f32: torch.Tensor, capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None,
                 policy: str = "fedavg"):
        if not isinstance(krum, KrumSpec):
            raise TypeError(f"krum: expected a KrumSpec, got {type(krum).__name__}")
        if policy != "fedavg":
            raise refuse(f"a {policy} round")
        if layout.world != 1:
            raise refuse("a parameter-sharded layout")
        self.f, self.m = krum.counts(K)  # (refuses K < 1)
        self.layout, self.device, self.K, self.krum = layout, torch.device(device), int(K), krum
        cap = min(staging.capacity, capacity or staging.capacity)
        if self.K > cap:
            raise ValueError(f"a Krum round needs all K={self.K} uploads resident, the staging capacity is {cap}: "
                             f"there is no chunk folding (raise capacity=, or lower K)")
        self.dstream, self.staging, self.cap, self.last_f32 = dstream, staging, cap, last_f32
        staging.generation += 1  # a new round takes the staging slots over
        self.generation = staging.generation
        self.n = self.slot = self.chunks_done = 0
        L = layout
        with self._on():
            if staging.side_scratch is None:
                staging.side_scratch = (torch.empty(L.ldq, dtype=torch.int64, device=self.device),
                                        torch.empty(L.ldq, dtype=torch.float64, device=self.device))
            self.chain = torch.zeros(L.ld, dtype=torch.float32, device=self.device)
            self._gram = torch.zeros(self.K * self.K, dtype=torch.float64, device=self.device)
            self._score = torch.zeros(self.K, dtype=torch.float64, device=self.device)
            self.coef = torch.zeros(self.K, dtype=torch.float32, device=self.device)
            self._n_sel = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._ws = kk.gram_workspace(self.K, L.P, self.device)
        self.acc_i, self.acc_d = staging.side_scratch
        self._host = None  # (scores, coefficients, n_sel) once fetched

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
        staging slots [slot, slot + n), written there on the device (tools/krum_measure.py)."""
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
        """Gram, scores, selection, the chain over the kept rows, then ``out`` <- the round's starting model plus
        their mean (fk_gram, fk_scores, fk_select, fcl_reduce, fk_finish — no host synchronisation in between); the
        side table as ``DeviceRound.finalize_mean`` (fed-yogi rounds take ``out`` as the mean, then the existing
        fa_yogi_step)."""
        if yogi is not None:
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)")
        self._check_complete()
        if self.chunks_done:
            raise RuntimeError("the round is already finalized")
        if float(denom32) != float(np.float32(self.K)):
            raise ValueError(f"a Krum round of K={self.K} uploads divides its kept rows by their number itself; the "
                             f"caller's denominator must be float32(K), not {denom32}")
        self.staging.drain()
        L, st, K = self.layout, self.staging, self.K
        kk.gram(st.x, K, L.P, self.last_f32, self._gram, self._ws)
        kk.scores(self._gram, K, self.f, self._score)
        kk.select(self._score, K, self.m, self.coef, self._n_sel)
        if L.P > 0:
            kc.reduce_clip(st.x, K, L.P, self.last_f32, self.coef, self.chain)
            kk.finish(self.chain, self.last_f32, self._n_sel, L.P, out, mirror=mirror)
        kx.side_accumulate(st.xi, K, L.Q, 0, acc_i=self.acc_i, acc_d=self.acc_d, accumulate=False)
        kx.side_close(L.Q, 0, denom64, acc_i=self.acc_i, acc_d=self.acc_d, cur=cur_side, model=model_side)
        self.chunks_done = 1
        self.slot = 0

    # ---- what the round did, for operators (host copies; the first call waits for the round's kernels) ----------
    def _fetch(self):
        if self._host is None:
            self._check_complete()
            if not self.chunks_done:
                raise RuntimeError("the round is not finalized yet")
            with self._on():
                self._host = (self._score.cpu().numpy(), self.coef.cpu().numpy(), int(self._n_sel.cpu()[0]))
        return self._host

    def scores(self) -> np.ndarray:
        """float64[K]: every upload's Krum score, in arrival order (+inf for an upload with an inf or NaN)."""
        return self._fetch()[0].copy()

    def selected(self) -> np.ndarray:
        """bool[K]: the uploads that entered the mean."""
        return self._fetch()[1] != 0

    @property
    def n_selected(self) -> int:
        """How many uploads entered the mean (the denominator; 0: the model was left as it was)."""
        return self._fetch()[2]

    @property
    def rejected(self) -> int:
        """Rows with a non-finite score."""
        return int((~np.isfinite(self._fetch()[0])).sum())

    def gram(self) -> np.ndarray:
        """float64[K, K]: the Gram matrix of the updates against the round's starting model."""
        self._fetch()
        with self._on():
            return self._gram.cpu().numpy().reshape(self.K, self.K)
