"""A FedAvg round whose new model is the geometric median of the uploads (RFA: robust federated aggregation).

Server-side robust aggregation after Pillutla, Kakade and Harchaoui ("Robust Aggregation for Federated Learning"),
by the smoothed Weiszfeld iteration.  The norm clip of ``clip_round`` needs a bound, the trimmed mean of ``trim_round``
a count and Krum of ``krum_round`` an f, and Krum throws f whole uploads away even when nobody lies; the geometric
median has nothing to tune, a breakdown point of 1/2, and on an honest round lands near the mean.  For a round that
starts from model ``L`` with K uploads ``x_k`` in arrival order (include/fedgeomed.h has the contract):

    d_k = x_k - L (fp32)          start: w = the mean of the updates clipped to the median update norm
    R times:  q_k = |d_k - sum_j w_j d_j|^2;   w_k = (1 / max(sqrt(q_k), nu)) / sum of those over the finite q
    new model = L + sum_k float(w_k) d_k

Every Weiszfeld iterate lies in the affine hull of the uploads, so ``method="gram"`` takes one fp64 Gram matrix of
the updates (fk_gram, on the matrix unit) and runs all R iterations in K-space, where every q_k is a quadratic form
in G; the model is touched once more, by fcl_reduce with the final weights.  ``method="stream"`` keeps the iterate as
an fp32 model and takes the distances from fcl_row_sqnorms against it: 2 + 2R passes over K x P, which is cheaper
once K is large (the Gram grows with K^2).  ``method="auto"`` takes the Gram when K <= 12 (1 + 2R) — a function of
(K, R) alone, so a given round gives the same bits everywhere.  The two methods agree to the last bits of the model,
not bit for bit.

What is aggregated is the whole fp32 bucket — parameters and fp32 buffers (BatchNorm statistics) alike; the int64
side table takes plain FedAvg's path with denominator K.  An upload with an inf or NaN anywhere has a non-finite
distance and weight 0 in every iteration; when no upload is finite the model is left as it was.

``GeoMedRound`` is what ``TorchModelAdapter._apply_round`` and the aggregator mixins use of ``DeviceRound``, over the
ordinary fp32 ``ClientStaging``.  All K rows must be resident: a round larger than the staging capacity is refused
when it begins (there is no chunk folding).  Opt-in (``TorchModelAdapter.begin_round(geomed=...)``,
``DeviceAggregatorMixin.device_geomed``); FedAvg and — as the median followed by the existing YoGi step — fed-yogi, and likewise fed-adam, fed-adagrad and fed-avgm.
Norm clipping, trimming, Krum, 16-bit, MXFP8 and top-k uploads, cohort signatures, sharded layouts, FedBuff and
q-FedAvg are refused.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _native_geomed as NG
from . import kernels as kx
from . import kernels_clip as kc
from . import kernels_geomed as kg
from . import kernels_krum as kk
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout, ClientStaging
from .round import on_stream
from .state import DeviceStream

METHODS = ("auto", "gram", "stream")
AUTO_GRAM_PASSES = 12  # auto: the Gram when K <= AUTO_GRAM_PASSES * (1 + 2R)


def refuse(what: str) -> NotImplementedError:
    """The error of a combination geometric-median aggregation does not take."""
    return NotImplementedError(f"geomed (GeoMedSpec / device_geomed) combined with {what} is not supported: "
                               f"geometric-median aggregation takes FedAvg and fed-yogi rounds of float32 uploads to "
                               f"one whole model on one device")


class GeoMedSpec:
    """``iters``: the Weiszfeld iterations R of a round, an int in [1, 64].  ``nu``: the smoothing, a finite float
    > 0 — a distance below it counts as nu.  ``method``: "gram", "stream" or "auto"."""

    __slots__ = ("iters", "nu", "method")

    def __init__(self, iters=4, nu=1e-6, method="auto"):
        if isinstance(iters, GeoMedSpec):
            iters, nu, method = iters.iters, iters.nu, iters.method
        if isinstance(iters, (bool, np.bool_)) or not isinstance(iters, (int, np.integer)):
            raise ValueError(f"GeoMedSpec: iters={iters!r} must be an int in [1, {NG.MAX_ITERS}]")
        iters = int(iters)
        if not 1 <= iters <= NG.MAX_ITERS:
            raise ValueError(f"GeoMedSpec: iters={iters!r} must be an int in [1, {NG.MAX_ITERS}] (FGM_MAX_ITERS)")
        if isinstance(nu, (bool, np.bool_)) or not isinstance(nu, (int, float, np.integer, np.floating)):
            raise ValueError(f"GeoMedSpec: nu={nu!r} must be a finite float > 0")
        nu = float(nu)
        if not (math.isfinite(nu) and nu > 0.0):
            raise ValueError(f"GeoMedSpec: nu={nu!r} must be a finite float > 0")
        if method not in METHODS:
            raise ValueError(f"GeoMedSpec: method={method!r} must be one of {METHODS}")
        object.__setattr__(self, "iters", iters)
        object.__setattr__(self, "nu", nu)
        object.__setattr__(self, "method", str(method))

    @classmethod
    def of(cls, what) -> "GeoMedSpec":
        """The spec of what ``begin_round(geomed=...)`` and ``device_geomed`` take: a spec, an int (iters) or True."""
        if isinstance(what, GeoMedSpec):
            return what
        if what is True:
            return cls()
        if isinstance(what, (bool, np.bool_)):
            raise ValueError(f"GeoMedSpec: geomed={what!r} must be True, an int (iters) or a GeoMedSpec")
        return cls(what)

    def __setattr__(self, name, value):
        raise AttributeError("GeoMedSpec is immutable")

    def __repr__(self):
        return f"GeoMedSpec(iters={self.iters!r}, nu={self.nu!r}, method={self.method!r})"

    def __eq__(self, other):
        return (isinstance(other, GeoMedSpec) and other.iters == self.iters and other.nu == self.nu
                and other.method == self.method)

    def __hash__(self):
        return hash((self.iters, self.nu, self.method))

    def resolve(self, K: int) -> str:
        """"gram" or "stream" for a round of K uploads — a function of (K, iters) alone; ValueError when the round
        cannot take K."""
        K = int(K)
        if K < 1:
            raise ValueError("a round needs K >= 1 client results")
        if K > NG.MAX_K:
            raise ValueError(f"{self!r}: K={K} exceeds the limit FGM_MAX_K = {NG.MAX_K}")
        if self.method != "auto":
            return self.method
        return "gram" if K <= AUTO_GRAM_PASSES * (1 + 2 * self.iters) else "stream"


class GeoMedRound:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, finishing at the geometric median."""

    policy = "fedavg"
    cg = None        # never client-sharded
    head = 0         # no head launch, no small-round mirror path
    sig_plan = None  # no cohort signatures

    def __init__(self, layout: BucketLayout, device, K: int, geomed: GeoMedSpec, *, staging: ClientStaging,
                 last_f32: torch.Tensor, capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None,
                 policy: str = "fedavg"):
        if not isinstance(geomed, GeoMedSpec):
            raise TypeError(f"geomed: expected a GeoMedSpec, got {type(geomed).__name__}")
        if policy != "fedavg":
            raise refuse(f"a {policy} round")
        if layout.world != 1:
            raise refuse("a parameter-sharded layout")
        self.method = geomed.resolve(K)  # (refuses K < 1 and K > FGM_MAX_K)
        self.layout, self.device, self.K, self.geomed = layout, torch.device(device), int(K), geomed
        self.iters, self.nu = geomed.iters, geomed.nu
        cap = min(staging.capacity, capacity or staging.capacity)
        if self.K > cap:
            raise ValueError(f"a geometric-median round needs all K={self.K} uploads resident, the staging capacity "
                             f"is {cap}: there is no chunk folding (raise capacity=, or lower K)")
        self.dstream, self.staging, self.cap, self.last_f32 = dstream, staging, cap, last_f32
        staging.generation += 1  # a new round takes the staging slots over
        self.generation = staging.generation
        self.n = self.slot = self.chunks_done = 0
        L, K, R, dev = layout, self.K, self.iters, self.device
        with self._on():
            if staging.side_scratch is None:
                staging.side_scratch = (torch.empty(L.ldq, dtype=torch.int64, device=dev),
                                        torch.empty(L.ldq, dtype=torch.float64, device=dev))
            self.chain = torch.zeros(L.ld, dtype=torch.float32, device=dev)
            self._w = torch.zeros(K, dtype=torch.float64, device=dev)
            self.coef = torch.zeros(K, dtype=torch.float32, device=dev)
            self._q = torch.zeros((R, K), dtype=torch.float64, device=dev)
            self._obj = torch.zeros(R, dtype=torch.float64, device=dev)
            self._n_valid = torch.zeros(1, dtype=torch.int32, device=dev)
            if self.method == "gram":
                self._gram = torch.zeros(K * K, dtype=torch.float64, device=dev)
                self._ws = kk.gram_workspace(K, L.P, dev)
                self._ws2 = kg.dist2_workspace(K, dev)
                self._q0 = self._z = None
            else:
                self._gram = None
                self._q0 = torch.zeros(K, dtype=torch.float64, device=dev)
                self._ws = kc.workspace(K, L.P, dev)
                self._z = torch.zeros(L.ld, dtype=torch.float32, device=dev)  # the iterate, as a model
        self.acc_i, self.acc_d = staging.side_scratch
        self._host = None  # (weights, objective, dist2, n_valid, start_dist2) once fetched

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
        staging slots [slot, slot + n), written there on the device (tools/geomed_measure.py)."""
        if n < 0 or self.slot + n > self.cap or self.n + n > self.K:
            raise ValueError(f"adopt_resident: {n} arrivals do not fit (slot {self.slot} of {self.cap}, "
                             f"{self.n} of K={self.K})")
        self.slot += n
        self.n += n

    def _check_complete(self):
        if self.n != self.K:
            raise RuntimeError(f"finalize with {self.n} of K={self.K} results")

    def _gram_round(self, out, mirror):
        L, x, K = self.layout, self.staging.x, self.K
        kk.gram(x, K, L.P, self.last_f32, self._gram, self._ws)
        kg.start(self._gram, K, self._w, self.coef, self._n_valid, stride=K + 1)
        for t in range(self.iters):
            kg.gram_dist2(self._gram, K, self._w, self._q[t], self._ws2)
            kg.weights(self._q[t], K, self.nu, self._w, self.coef, self._obj[t:t + 1], self._n_valid)
        if L.P > 0:
            kc.reduce_clip(x, K, L.P, self.last_f32, self.coef, self.chain)
            kg.finish(self.chain, self.last_f32, self._n_valid, L.P, out, mirror=mirror)

    def _stream_round(self, out, mirror):
        L, x, K, R = self.layout, self.staging.x, self.K, self.iters
        kc.row_sqnorms(x, K, L.P, self.last_f32, self._q0, self._ws)
        kg.start(self._q0, K, self._w, self.coef, self._n_valid)
        if L.P > 0:
            kc.reduce_clip(x, K, L.P, self.last_f32, self.coef, self.chain)
            kg.finish(self.chain, self.last_f32, self._n_valid, L.P, self._z)
        for t in range(R):
            kc.row_sqnorms(x, K, L.P, self._z, self._q[t], self._ws)
            kg.weights(self._q[t], K, self.nu, self._w, self.coef, self._obj[t:t + 1], self._n_valid)
            if L.P > 0:
                kc.reduce_clip(x, K, L.P, self.last_f32, self.coef, self.chain)
                last = t == R - 1
                kg.finish(self.chain, self.last_f32, self._n_valid, L.P, out if last else self._z,
                          mirror=mirror if last else None)

    @on_stream
    def finalize_mean(self, denom32: float, denom64: float, *, out: torch.Tensor, cur_side: torch.Tensor,
                      model_side: Optional[torch.Tensor] = None, yogi: Optional[dict] = None,
                      mirror: Optional[torch.Tensor] = None):
        """The Weiszfeld iterations by the round's method, then ``out`` <- the round's starting model plus the
        weighted updates (no host synchronisation in between); the side table as ``DeviceRound.finalize_mean``
        (fed-yogi rounds take ``out`` as the mean, then the existing fa_yogi_step)."""
        if yogi is not None:
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)")
        self._check_complete()
        if self.chunks_done:
            raise RuntimeError("the round is already finalized")
        if float(denom32) != float(np.float32(self.K)):
            raise ValueError(f"a geometric-median round of K={self.K} uploads normalises its weights itself; the "
                             f"caller's denominator must be float32(K), not {denom32}")
        self.staging.drain()
        L, st, K = self.layout, self.staging, self.K
        if self.method == "gram":
            self._gram_round(out, mirror)
        else:
            self._stream_round(out, mirror)
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
                if self.method == "gram":
                    q0 = self._gram.view(self.K, self.K).diagonal().cpu().numpy().copy()
                else:
                    q0 = self._q0.cpu().numpy()
                self._host = (self._w.cpu().numpy(), self._obj.cpu().numpy(), self._q.cpu().numpy(),
                              int(self._n_valid.cpu()[0]), q0)
        return self._host

    def weights(self) -> np.ndarray:
        """float64[K]: every upload's final weight, in arrival order (0 for an upload with an inf or NaN); the model
        took their fp32 roundings."""
        return self._fetch()[0].copy()

    def objective(self) -> np.ndarray:
        """float64[R]: ``objective()[t]`` is the sum of the finite uploads' distances to the iterate that iteration t
        started from."""
        return self._fetch()[1].copy()

    def dist2(self) -> np.ndarray:
        """float64[R, K]: ``dist2()[t]`` are the squared distances of the uploads to the iterate that iteration t
        started from (non-finite for an upload with an inf or NaN)."""
        return self._fetch()[2].copy()

    def start_dist2(self) -> np.ndarray:
        """float64[K]: the squared update norms the start weights were made from."""
        return self._fetch()[4].copy()

    @property
    def n_valid(self) -> int:
        """How many uploads had a finite distance in the last iteration (0: the model was left as it was)."""
        return self._fetch()[3]

    @property
    def rejected(self) -> int:
        """Uploads with a non-finite distance in the last iteration."""
        return self.K - self._fetch()[3]

    def gram(self) -> np.ndarray:
        """float64[K, K]: the Gram matrix of the updates against the round's starting model (``method`` "gram")."""
        if self.method != "gram":
            raise RuntimeError("gram(): a streamed geometric-median round has no Gram matrix")
        self._fetch()
        with self._on():
            return self._gram.cpu().numpy().reshape(self.K, self.K)
