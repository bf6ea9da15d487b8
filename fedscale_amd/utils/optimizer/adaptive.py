"""Device-resident adaptive server optimizers: FedAdam and FedAdagrad (Reddi et al., "Adaptive Federated
Optimization", ICLR 2021, Algorithm 2 — the two rules beside FedYoGi) and FedAvgM (Hsu et al., 2019: server momentum).
The reference ships none of them; the surface is ``YoGi``'s (fedscale_amd/utils/optimizer/yogi.py).

State (``m``, and ``v`` for the two adaptive rules) persists across rounds in the object and lives in HBM as one flat
fp32 vector each, over the model's fp32 entries.  The int64 entries of a state_dict (``num_batches_tracked``) have no
gradient and get no state: they take the round's FedAvg mean, as a round without a server step writes them.

Per parameter, with g = mean - last, every operation one fp32 rounding (include/fedserveropt.h):

    FedAdam     m = beta*m + (1-beta)*g    v = beta2*v + (1-beta2)*g*g    new = last + eta * (m / (sqrt(v) + tau))
    FedAdagrad  m = beta*m + (1-beta)*g    v = v + g*g                    new = last + eta * (m / (sqrt(v) + tau))
    FedAvgM     m = beta*m + g             -                              new = last + eta * m

The first step takes m = 0 and v = v0 (default fp32(tau*tau), the paper's v_{-1} >= tau^2).  There is no bias
correction: Algorithm 2 has none.  FedAvgM with beta = 0 and eta = 1 gives last + (mean - last), which in fp32 is not
always the mean.

Two ways in, as with YoGi: ``update(gradients)`` — the reference's list of gradient tensors -> list of step tensors
(``fso_step`` with last = 0) — and the aggregation path (TorchModelAdapter._apply_round), which hands ``step_args()``
to ``kernels_serveropt.step`` after the mean has been reduced into its own buffer.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from ... import kernels_serveropt as kso
from ...bucket import BucketLayout


def _f32(x: float) -> float:
    return float(np.float32(x))


class _ServerRule:
    """What the three rules share: the state, its views, the pickling and the reference-typed ``update``."""

    rule: str = ""       #: the kernel's rule name (kernels_serveropt.RULES)
    has_v: bool = True   #: whether the rule keeps a second-moment vector
    DEFAULT_ETA = 1e-2   #: the server learning rate when ``args`` has no ``server_eta``
    #: a round leaves device state (m, v) a caller can read: the adapter orders the caller's stream after the round
    exposes_device_state = True

    def __init__(self, eta=1e-2, tau=1e-3, beta=0.9, beta2=0.99, v0=None):
        self.eta = eta
        self.tau = tau
        self.beta = beta
        self.beta2 = beta2
        self.v0 = v0
        self.layout: Optional[BucketLayout] = None
        self.m = self.v = None
        self.initialized = False  # becomes True after the first step

    _HPARAMS = ("eta", "tau", "beta", "beta2", "v0")

    def __getstate__(self):
        """Pickle the hyper-parameters and (host copies of) the m/v state."""
        st = {k: self.__dict__[k] for k in self._HPARAMS + ("initialized",)}
        st["_layout_args"] = None
        st["_state"] = None
        if self.layout is not None:
            L = self.layout
            st["_layout_args"] = (L.names, [e.shape for e in L.entries], [e.dtype for e in L.entries], L.rank, L.world)
            st["_state"] = tuple(None if t is None else t.cpu() for t in (self.m, self.v))
        return st

    def __setstate__(self, st):
        _ServerRule.__init__(self, *(st[k] for k in self._HPARAMS))
        if st.get("_layout_args") is not None:
            self.bind(BucketLayout(*st["_layout_args"]), torch.device("cuda", torch.cuda.current_device()))
            for dst, src in zip((self.m, self.v), st["_state"]):
                if dst is not None:
                    dst.copy_(src)
        self.initialized = st["initialized"]

    # ---- state ----------------------------------------------------------------------------------
    def bind(self, layout: BucketLayout, device):
        """Allocate m (and v) for ``layout`` (idempotent for the same layout).  The buffers are not cleared by the
        first step, which does not read them (FSO_INIT); they are zeroed here only so that a reader sees zeros."""
        if self.layout is not None:
            if (self.layout.names == layout.names and self.layout.P == layout.P and self.layout.Q == layout.Q
                    and self.layout.p0 == layout.p0):
                return
            raise ValueError(f"{type(self).__name__} state is bound to a different model layout")
        self.layout = layout
        dev = torch.device(device)
        self.m = torch.zeros(layout.ld, dtype=torch.float32, device=dev)
        self.v = torch.zeros(layout.ld, dtype=torch.float32, device=dev) if self.has_v else None

    def fp32_hparams(self) -> dict:
        """Scalars as the kernel takes them (Python double -> fp32; 1-beta and tau*tau in double first)."""
        v0 = self.tau * self.tau if self.v0 is None else self.v0
        return dict(eta=_f32(self.eta), tau=_f32(self.tau), beta=_f32(self.beta), omb=_f32(1.0 - self.beta),
                    beta2=_f32(self.beta2), omb2=_f32(1.0 - self.beta2), v0=_f32(v0))

    def step_args(self) -> dict:
        """The keyword arguments of ``kernels_serveropt.step`` / ``step_parts`` this optimizer supplies."""
        return dict(init=not self.initialized, **self.fp32_hparams())

    def step(self, mean_f32: torch.Tensor, last_f32: torch.Tensor, out_f32: torch.Tensor, P: int):
        """One step on the device: the new model into ``out_f32``, m and v in place."""
        kso.step(self.rule, mean_f32, last_f32, self.m, self.v, out_f32, P, **self.step_args())
        self.initialized = True

    @property
    def m_t(self) -> List[Optional[torch.Tensor]]:
        return self._views(self.m)

    @property
    def v_t(self) -> List[Optional[torch.Tensor]]:
        return self._views(self.v)

    def _views(self, f):
        """Per-tensor views in state_dict order; None at the int64 entries, which have no state."""
        if not self.initialized or self.layout is None or f is None:
            return []
        if self.layout.world != 1:
            raise RuntimeError(f"per-tensor views of a sharded {type(self).__name__} state are not available; "
                               f"use .m/.v")
        return [f[e.offset:e.offset + e.numel].view(e.shape) if e.kind == "f" else None for e in self.layout.entries]

    # ---- reference API --------------------------------------------------------------------------
    def update(self, gradients):
        """The list-in, list-out form of yogi.py:15-36: returns the step per tensor (the kernel with last = 0).  A
        float64 gradient (from an int64 buffer) has no state and comes back unchanged: last + g is the mean."""
        gradients = list(gradients)
        if len(gradients) == 0:
            return gradients
        dev = gradients[0].device if gradients[0].device.type == "cuda" else torch.device("cuda",
                                                                                             torch.cuda.current_device())
        names = [str(i) for i in range(len(gradients))]
        dtypes = [torch.int64 if g.dtype == torch.float64 else g.dtype for g in gradients]
        layout = BucketLayout(names, [tuple(g.shape) for g in gradients], dtypes)
        self.bind(layout, dev)
        cur = torch.zeros(layout.ld, dtype=torch.float32, device=dev)
        for e in layout.f_entries:
            cur[e.offset:e.offset + e.numel].copy_(gradients[e.index].detach().reshape(-1).to(dev))
        zero = torch.zeros_like(cur)
        step = torch.empty_like(cur)
        self.step(cur, zero, step, layout.P)
        return [step[e.offset:e.offset + e.numel].view(e.shape).to(gradients[e.index].device) if e.kind == "f"
                else gradients[e.index] for e in layout.entries]


class FedAdam(_ServerRule):
    rule = "adam"


class FedAdagrad(_ServerRule):
    rule = "adagrad"


class FedAvgM(_ServerRule):
    rule = "avgm"
    has_v = False
    DEFAULT_ETA = 1.0

    def __init__(self, eta=1.0,tau=1e-3, beta=0.9, beta2=0.99, v0=None):
        super().__init__(eta, tau, beta, beta2, v0)


#: ``gradient_policy`` / TorchServerOptimizer mode -> the optimizer class
MODES = {"fed-adam": FedAdam, "fed-adagrad": FedAdagrad, "fed-avgm": FedAvgM}
