"""A FedAvg round aggregated by Bulyan: Krum run theta times, the winner removed each time, and then, for every
parameter, the mean of the beta selected values closest to their median.

Server-side robust aggregation after El Mhamdi, Guerraoui and Rouault (ICML 2018).  Multi-Krum (``krum_round``)
resists a colluding minority that stays inside the honest range in every coordinate, but hands its winners over whole:
one hidden coordinate with a huge value still moves the model.  The trimmed means (``trim_round``,
``deep_trim_round``) are safe per coordinate but blind to collusion.  Bulyan composes the two.  For a round that starts
from model ``L`` with K uploads in arrival order and f assumed bad (include/fedbulyan.h has the contract):

    theta = K - 2f - 2 rows selected;  beta = theta - 2f = K - 4f - 2 values kept per parameter;  4f + 3 <= K
    selection   theta times: score every remaining row by its n - f - 2 nearest remaining rows (fp64, from fk_gram's
                matrix), pick the smallest (score, arrival), remove it
    per column  med = the lower median of the selected values; keep the beta values closest to med (ties to the
                earlier arrival); new value = their sum in arrival order / float(beta)

theta is two less than the paper's K - 2f, so that the last Krum call still sees the 2f + 3 rows Krum needs.  What is
aggregated is the whole fp32 bucket; the int64 side table takes plain FedAvg's path with denominator K.  An upload
with an inf or NaN anywhere is never picked; up to f + 1 of them still leave a full selection, with more no upload
can be scored, the picks run out, and the model is then left as it was.

``BulyanRound`` is what ``TorchModelAdapter._apply_round`` and the aggregator mixins use of ``DeviceRound``, over the
ordinary fp32 ``ClientStaging``.  All K rows are resident: a round larger than the staging capacity is refused when
it begins (there is no chunk folding).  Opt-in (``TorchModelAdapter.begin_round(bulyan=...)``,
``DeviceAggregatorMixin.device_bulyan``); FedAvg and — as the mean followed by the existing server step — fed-yogi,
fed-adam, fed-adagrad or fed-avgm.  Norm clipping, the trimmed means, Krum, the geometric median, every upload
format, cohort signatures, sharded layouts, FedBuff and q-FedAvg are refused.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import kernels as kx
from . import kernels_bulyan as kb
from . import kernels_krum as kk
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout, ClientStaging
from .round import on_stream
from .state import DeviceStream


def refuse(what: str) -> NotImplementedError:
    """The error of a combination Bulyan aggregation does not take."""
    return NotImplementedError(f"bulyan (BulyanSpec / device_bulyan) combined with {what} is not supported: Bulyan "
                               f"aggregation takes FedAvg and server-optimizer rounds of float32 uploads to one whole "
                               f"model on one device")


class BulyanSpec:
    """``f``: a non-negative int — the uploads assumed bad."""

    __slots__ = ("f",)

    def __init__(self, f):
        if isinstance(f, BulyanSpec):
            f = f.f
        if isinstance(f, (bool, np.bool_)) or not isinstance(f, (int, np.integer)):
            raise ValueError(f"BulyanSpec: f={f!r} must be an int >= 0")
        if int(f) < 0:
            raise ValueError(f"BulyanSpec: f={f!r} must be an int >= 0")
        object.__setattr__(self, "f", int(f))

    def __setattr__(self, name, value):
        raise AttributeError("BulyanSpec is immutable")

    def __repr__(self):
        return f"BulyanSpec({self.f!r})"

    def __eq__(self, other):
        return isinstance(other, BulyanSpec) and other.f == self.f

    def __hash__(self):
        return hash(("bulyan", self.f))

    def counts(self, K: int) -> tuple:
        """(theta, beta) of a round of K uploads; ValueError when the round cannot take f."""
        K = int(K)
        if K < 1:
            raise ValueError("a round needs K >= 1 client results")
        try:
            return kb.counts(K, self.f)  # (the bounds live there)
        except ValueError as e:
            raise ValueError(f"{self!r}: {e}") from None


class BulyanRound:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, aggregating by Bulyan."""

    policy = "fedavg"
    cg = None        # never client-sharded
    head = 0         # no head launch, no small-round mirror path
    sig_plan = None  # no cohort signatures

    def __init__(self, layout: BucketLayout, device, K: int, bulyan: BulyanSpec, *, staging: ClientStaging,
                 last_f32: torch.Tensor, capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None,
                 policy: str = "fedavg"):
        if not isinstance(bulyan, BulyanSpec):
            raise TypeError(f"bulyan: expected a BulyanSpec, got {type(bulyan).__name__}")
        if policy != "fedavg":
            raise refuse(f"a {policy} round")
        if layout.world != 1:
            raise refuse("a parameter-sharded layout")
        self.theta, self.beta = bulyan.counts(K)  # (refuses K < 1)
        self.layout, self.device, self.K, self.bulyan = layout, torch.device(device), int(K), bulyan
        self.f = bulyan.f
        cap = min(staging.capacity, capacity or staging.capacity)
        if self.K > cap:
            raise ValueError(f"a Bulyan round needs all K={self.K} uploads resident, the staging capacity is {cap}: "
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
            self._gram = torch.zeros(self.K * self.K, dtype=torch.float64, device=self.device)
            self._picks = torch.full((self.theta,), -1, dtype=torch.int32, device=self.device)
            self._sel = torch.full((self.theta,), -1, dtype=torch.int32, device=self.device)
            self._n_sel = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._kept = torch.zeros(self.K, dtype=torch.int64, device=self.device)
            self._ws = kk.gram_workspace(self.K, L.P, self.device)
            self._sws = kb.select_workspace(self.K, self.device)
        self.acc_i, self.acc_d = staging.side_scratch
        self._host = None  # (picks, kept, n_sel) once fetched

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
        staging slots [slot, slot + n), written there on the device (tools/bulyan_measure.py)."""
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
        """Gram, the iterated selection, then ``out`` <- per column the mean around the median of the selected rows
        (fk_gram, fbl_select, fbl_reduce — no host synchronisation in between); the side table as
        ``DeviceRound.finalize_mean`` (server-optimizer rounds take ``out`` as the mean, then the existing step)."""
        if yogi is not None:
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)")
        self._check_complete()
        if self.chunks_done:
            raise RuntimeError("the round is already finalized")
        if float(denom32) != float(np.float32(self.K)):
            raise ValueError(f"a Bulyan round of K={self.K} uploads divides its kept values by beta itself; the "
                             f"caller's denominator must be float32(K), not {denom32}")
        self.staging.drain()
        L, st, K = self.layout, self.staging, self.K
        kk.gram(st.x, K, L.P, self.last_f32, self._gram, self._ws)
        kb.select(self._gram, K, self.f, self._picks, self._sel, self._n_sel, self._sws)
        if L.P > 0:
            kb.reduce_bulyan(st.x, K, L.P, self._sel, self._n_sel, self.theta, self.beta, self.last_f32, out,
                             mirror=mirror, kept=self._kept)
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
                self._host = (self._picks.cpu().numpy(), self._kept.cpu().numpy(), int(self._n_sel.cpu()[0]))
        return self._host

    def selected(self) -> np.ndarray:
        """int32[n_selected]: the uploads Krum picked, in selection order."""
        picks, _, n = self._fetch()
        return picks[:n].copy()

    def kept(self) -> np.ndarray:
        """int64[K]: in how many of the P columns each upload, in arrival order, was one of the beta kept values."""
        return self._fetch()[1].copy()

    @property
    def n_selected(self) -> int:
        """How many uploads were picked; below theta the model was left as it was."""
        return self._fetch()[2]

    def gram(self) -> np.ndarray:
        """float64[K, K]: the Gram matrix of the updates against the round's starting model."""
        self._fetch()
        with self._on():
            return self._gram.cpu().numpy().reshape(self.K, self.K)
