"""A FedAvg round whose client updates are clipped to a norm bound on the device before they are averaged, with
optional Gaussian noise on the mean (server-side clipping against poisoned uploads; central DP-FedAvg).

The reference's examples clip on the client (``clip_grad_norm_(delta_weight, max_norm=3.)`` in
examples/poisoning_setting and examples/differential_privacy, clip_norm.py:57-60); a malicious client does not clip
itself, so here the aggregator does it, next to the staged rows.  For a round that starts from model ``L`` with K
uploads ``x_k`` in arrival order (include/fedclip.h; fp32, rounded to nearest, never fused, unless marked):

    d_k   = x_k - L                     sq_k = sum double(d_k)^2 (fp64)      r_k = M / (sqrt(sq_k) + 1e-6) (fp64)
    c_k   = 0 if sq_k is not finite else (float(r_k) if r_k < 1 else 1)
    chain = +0;  chain += c_k * d_k     for k in arrival order with c_k != 0
    m     = chain / float(K);  m += sigma * z when sigma > 0;  new model = L + m

What is clipped is the whole fp32 bucket — parameters and fp32 buffers (BatchNorm statistics) alike; the int64 side
table takes plain FedAvg's path.  A row whose norm is not finite (an inf or NaN anywhere in the upload) is rejected:
it contributes nothing, but still counts in the denominator K (DP-FedAvg's fixed denominator).  ``sigma`` is
``noise_multiplier * M / K``; what privacy that buys is the user's to account for.

``ClippedRound`` is what ``TorchModelAdapter._apply_round`` and the aggregator mixins use of ``DeviceRound``, over the
ordinary fp32 ``ClientStaging``.  Opt-in (``TorchModelAdapter.begin_round(clip=ClipSpec(...))``,
``DeviceAggregatorMixin.device_clip_norm``); FedAvg and — as the clipped mean followed by the existing YoGi step —
fed-yogi, fed-adam, fed-adagrad or fed-avgm (the mean, then the server step).  16-bit uploads, cohort signatures, sharded layouts, FedBuff and q-FedAvg are refused.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import kernels as kx
from . import kernels_clip as kc
from .bucket import _NULL_CTX as _NULL
from .bucket import BucketLayout, ClientStaging
from .round import on_stream
from .state import DeviceStream


def refuse(what: str) -> NotImplementedError:
    """The error of a combination norm-clipped aggregation does not take."""
    return NotImplementedError(f"clip (ClipSpec / device_clip_norm) combined with {what} is not supported: "
                               f"norm-clipped aggregation takes FedAvg and fed-yogi rounds of float32 uploads to one "
                               f"whole model on one device")


class ClipSpec:
    """``max_norm`` M: the bound on each client's update norm (finite, > 0).  ``noise_multiplier`` (>= 0): Gaussian
    noise of standard deviation ``noise_multiplier * M / K`` on the mean; 0 adds none.  ``seed``: of the noise
    stream (``fa_dp_normals``)."""

    __slots__ = ("max_norm", "noise_multiplier", "seed")

    def __init__(self, max_norm: float, noise_multiplier: float = 0.0, seed: int = 0):
        try:
            M, nm = float(max_norm), float(noise_multiplier)
        except (TypeError, ValueError):
            raise ValueError(f"ClipSpec: max_norm={max_norm!r} and noise_multiplier={noise_multiplier!r} must be "
                             f"numbers") from None
        if not (math.isfinite(M) and M > 0):
            raise ValueError(f"ClipSpec: max_norm={max_norm!r} must be finite and > 0")
        if not (math.isfinite(nm) and nm >= 0):
            raise ValueError(f"ClipSpec: noise_multiplier={noise_multiplier!r} must be finite and >= 0")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
            raise ValueError(f"ClipSpec: seed={seed!r} must be an integer")
        object.__setattr__(self, "max_norm", M)
        object.__setattr__(self, "noise_multiplier", nm)
        object.__setattr__(self, "seed", int(seed))

    def __setattr__(self, name, value):
        raise AttributeError("ClipSpec is immutable")

    def __repr__(self):
        return f"ClipSpec(max_norm={self.max_norm!r}, noise_multiplier={self.noise_multiplier!r}, seed={self.seed!r})"

    def sigma(self, K: int) -> float:
        """The noise's standard deviation on the mean of K clients, in Python double."""
        return float(self.noise_multiplier * self.max_norm / K)


def noise_stride(P: int) -> int:
    """Draws one applied round takes from the noise stream: round_up(P, 2) (the stream is made in pairs)."""
    return (int(P) + 1) // 2 * 2


class ClippedRound:
    """What ``_apply_round`` and the aggregator mixins use of ``DeviceRound``, with every update clipped."""

    policy = "fedavg"
    cg = None        # never client-sharded
    head = 0         # no head launch, no small-round mirror path
    sig_plan = None  # no cohort signatures

    def __init__(self, layout: BucketLayout, device, K: int, clip: ClipSpec, *, staging: ClientStaging,
                 last_f32: torch.Tensor, capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None,
                 noise_offset: int = 0, policy: str = "fedavg"):
        if not isinstance(clip, ClipSpec):
            raise TypeError(f"clip: expected a ClipSpec, got {type(clip).__name__}")
        if policy != "fedavg":
            raise refuse(f"a {policy} round")
        if K < 1:
            raise ValueError("a round needs K >= 1 client results")
        if layout.world != 1:
            raise refuse("a parameter-sharded layout")
        self.layout, self.device, self.K, self.clip = layout, torch.device(device), int(K), clip
        self.dstream, self.staging, self.last_f32 = dstream, staging, last_f32
        self.cap = min(staging.capacity, capacity or staging.capacity)
        staging.generation += 1  # a new round takes the staging slots over
        self.generation = staging.generation
        self.n = self.slot = self.chunks_done = 0
        self.noise_offset = int(noise_offset)
        self.sigma = clip.sigma(self.K)
        L = layout
        with self._on():
            if staging.side_scratch is None:
                staging.side_scratch = (torch.empty(L.ldq, dtype=torch.int64, device=self.device),
                                        torch.empty(L.ldq, dtype=torch.float64, device=self.device))
            self.chain = torch.zeros(L.ld, dtype=torch.float32, device=self.device)
            self.sqnorm = torch.zeros(self.K, dtype=torch.float64, device=self.device)
            self.coef = torch.zeros(self.K, dtype=torch.float32, device=self.device)
            self._rejected = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._ws = kc.workspace(self.cap, L.P, self.device)
        self.acc_i, self.acc_d = staging.side_scratch
        self._host = None  # (norms, coefficients, rejected) once fetched

    def _on(self):
        ds = self.dstream
        return _NULL if ds is None or DeviceStream.current() is ds else ds

    def add(self, update, *, weight: Optional[float] = None, loss=None, learning_rate=None, q=None):
        """Stage one arriving upload (in arrival order)."""
        if self.n >= self.K:
            raise RuntimeError(f"round already has its K={self.K} results")
        if self.slot == self.cap:
            self._fold_chunk()
        self.staging.put(self.slot, update)
        self.slot += 1
        self.n += 1

    def adopt_resident(self, n: int):
        """Measurement hook, as ``DeviceRound.adopt_resident``: take ``n`` arrivals whose updates are ALREADY in the
        staging slots [slot, slot + n), written there on the device (tools/clip_reduce_measure.py)."""
        if n < 0 or self.slot + n > self.cap or self.n + n > self.K:
            raise ValueError(f"adopt_resident: {n} arrivals do not fit (slot {self.slot} of {self.cap}, "
                             f"{self.n} of K={self.K})")
        self.slot += n
        self.n += n

    def _reduce_chunk(self):
        """Norms, coefficients and the clipped chain of the staged chunk, and its side-table sums."""
        self.staging.drain()
        L, st, n = self.layout, self.staging, self.slot
        first = self.chunks_done == 0
        if n > 0:
            k0 = self.n - n  # arrival index of the chunk's first row
            sq, c = self.sqnorm[k0:k0 + n], self.coef[k0:k0 + n]
            kc.row_sqnorms(st.x, n, L.P, self.last_f32, sq, self._ws)
            kc.clip_coefs(sq, n, self.clip.max_norm, c, self._rejected)
            kc.reduce_clip(st.x, n, L.P, self.last_f32, c, self.chain, acc_in=None if first else self.chain)
        kx.side_accumulate(st.xi, n, L.Q, 0, acc_i=self.acc_i, acc_d=self.acc_d, accumulate=not first)
        self.chunks_done += 1
        self.slot = 0

    @on_stream
    def _fold_chunk(self):
        """Fold the staged chunk into the running clipped chain (not the last chunk of the round)."""
        self._reduce_chunk()

    def _check_complete(self):
        if self.n != self.K:
            raise RuntimeError(f"finalize with {self.n} of K={self.K} results")

    @on_stream
    def finalize_mean(self, denom32: float, denom64: float, *, out: torch.Tensor, cur_side: torch.Tensor,
                      model_side: Optional[torch.Tensor] = None, yogi: Optional[dict] = None,
                      mirror: Optional[torch.Tensor] = None):
        """Reduce the last chunk, then ``out`` <- the round's starting model plus the (noised) clipped mean
        (fcl_finish); the side table as ``DeviceRound.finalize_mean`` (fed-yogi rounds take ``out`` as the mean, then
        the existing fa_yogi_step)."""
        if yogi is not None:
            raise refuse("the fused FedYoGi epilogue (take the mean, then yogi_step)")
        self._check_complete()
        den = float(np.float32(self.K))
        if float(denom32) != den:
            raise ValueError(f"a clipped round divides by its fixed denominator K={self.K}, not {denom32}")
        L = self.layout
        self._reduce_chunk()
        z, sigma = None, self.sigma
        if sigma > 0 and L.P > 0:
            z = torch.empty(kx._cols(L.P), dtype=torch.float32, device=self.device)
            kx.dp_normals(z, self.clip.seed, self.noise_offset)
        kc.finish(self.chain, self.last_f32, L.P, den, out, z=z, sigma=sigma if z is not None else 0.0, mirror=mirror)
        kx.side_close(L.Q, 0, denom64, acc_i=self.acc_i, acc_d=self.acc_d, cur=cur_side, model=model_side)

    @property
    def next_noise_offset(self) -> int:
        """The noise offset of the round after this one."""
        return self.noise_offset + noise_stride(self.layout.P)

    # ---- what the round did, for operators (host copies; the first call waits for the round's kernels) ----------
    def _fetch(self):
        if self._host is None:
            self._check_complete()
            if self.slot:
                raise RuntimeError("the round is not finalized yet")
            with self._on():
                self._host = (self.sqnorm.cpu().numpy(), self.coef.cpu().numpy(), int(self._rejected.cpu()[0]))
        return self._host

    def norms(self) -> np.ndarray:
        """float64[K]: every client's update norm sqrt(sq_k), in arrival order (inf / NaN for a rejected row)."""
        with np.errstate(invalid="ignore"):
            return np.sqrt(self._fetch()[0])

    def coefficients(self) -> np.ndarray:
        """float32[K]: the coefficient each update entered the mean with (1: unclipped; 0: rejected)."""
        return self._fetch()[1].copy()

    @property
    def rejected(self) -> int:
        """Rows rejected for a non-finite norm."""
        return self._fetch()[2]
