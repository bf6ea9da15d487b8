"""A sign round whose uploads were rotated by the seeded block Hadamard transform before they were encoded.

The executor encodes y = H D e / 64 instead of e (fedscale_amd/cloud/execution/rotate_upload.py; include/fedrotate.h
states the transform), over P' = round_up(P, 4096) columns.  The rotation is linear, so everything ``SignRound``
does up to the chain is done here unchanged over rows of P' columns: ``RotatedSignStaging`` is a ``SignStaging`` whose
row geometry comes from P', ``fsg_reduce`` chains the rotated rows in arrival order.  The round then pays one inverse
transform of the chain (``frt_unrotate``, in place: one pass over P' floats beside K passes over bit rows) and closes
with the same ``fcl_finish`` over [0, P): new model = L + unrotate(chain) / K.

All uploads of a round carry one seed (``ROTATE_KEY``).  The round adopts its first arrival's and refuses, before
anything is staged, an upload without one and an upload with another.

Opt-in (``TorchModelAdapter(upload_sign="sign1", upload_rotate="rht4096")``); what ``SignRound`` refuses is refused.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import kernels as kx
from . import kernels_clip as kc
from . import kernels_rotate as kr
from . import kernels_sign as kg
from .bucket import BucketLayout
from .cloud.execution.rotate_upload import ROT_BLOCK, ROTATE_KEY
from .cloud.execution.rotate_upload import padded as padded_cols
from .round import on_stream
from .sign_round import SignRound, SignStaging
from .state import DeviceStream

ROTATIONS = ("rht4096",)


def check_rotation(rot) -> str:
    """``rot`` when it names a rotation; ValueError otherwise."""
    if rot not in ROTATIONS:
        raise ValueError(f"upload_rotate {rot!r}: expected 'rht4096'")
    return rot


def refuse(what: str, rot: str = "rht4096") -> NotImplementedError:
    """The error of a combination the rotated sign upload path does not take."""
    return NotImplementedError(f"upload_rotate={rot!r} combined with {what} is not supported: the rotation goes "
                               f"around 1-bit sign delta uploads (upload_sign='sign1') of one whole model on one "
                               f"device")


class _RotatedColumns:
    """A layout as a rotated row sees it: P is P' = round_up(P, 4096), everything else is the layout's."""

    def __init__(self, layout: BucketLayout):
        self._layout = layout
        self.P = padded_cols(layout.P)

    def __getattr__(self, name):
        if name == "_layout":  # not set yet (copying, unpickling): no delegation, no recursion
            raise AttributeError(name)
        return getattr(self._layout, name)


def seed_of(update) -> Optional[int]:
    """The seed an upload carries (a dict's ``ROTATE_KEY``, a list's last array), or None when it carries none."""
    if type(update) is dict:
        v = update.get(ROTATE_KEY)
    else:
        update = list(update)
        v = update[-1] if update else None
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    v = np.asarray(v)
    if v.dtype != np.uint64 or v.shape != (1,):
        return None
    return int(v[0])


def strip_seed(update):
    """The upload without its seed: what a ``SignStaging`` takes."""
    if type(update) is dict:
        return {k: v for k, v in update.items() if k != ROTATE_KEY}
    return list(update)[:-1]


class RotatedSignStaging(SignStaging):
    """A ``SignStaging`` for rotated uploads: rows of P' columns — ``bits`` [capacity, round_up(P' / 8, 16)], ``scales``
    [capacity, round_up(P' / 256, 4)] — and the same int64 side table.  ``layout`` is the model's layout with P
    replaced by P' (what ``SignStaging`` sizes and checks its rows by), ``model_layout`` the model's own, ``columns``
    P'."""

    def __init__(self, layout: BucketLayout, device, capacity: int, dstream: Optional[DeviceStream] = None,
                 ring: int = 2):
        super().__init__(_RotatedColumns(layout), device, capacity, dstream=dstream, ring=ring)
        self.model_layout = layout
        self.columns = self.layout.P


class RotatedSignRound(SignRound):
    """A ``SignRound`` whose chain has P' columns and is rotated back once before the finish."""

    def __init__(self, layout: BucketLayout, device, K: int, policy: str, *, staging: RotatedSignStaging,
                 last_f32: torch.Tensor, capacity: Optional[int] = None, dstream: Optional[DeviceStream] = None,
                 rotation: str = "rht4096"):
        if not isinstance(staging, RotatedSignStaging):
            raise TypeError(f"staging: expected a RotatedSignStaging, got {type(staging).__name__}")
        super().__init__(layout, device, K, policy, staging=staging, last_f32=last_f32, capacity=capacity,
                         dstream=dstream)
        self.upload_rotate = check_rotation(rotation)
        self.columns = staging.columns
        self.seed = None  # the round's seed: its first arrival's
        with self._on():
            self.chain = torch.zeros(max(ROT_BLOCK, self.columns), dtype=torch.float32, device=self.device)

    def add(self, update, *, weight: Optional[float] = None, loss=None, learning_rate=None, q=None):
        """Stage one arriving rotated sign upload (in arrival order); an upload without a seed, or with another than
        the round's, is refused here with nothing staged."""
        if self.n >= self.K:
            raise RuntimeError(f"round already has its K={self.K} results")
        seed = seed_of(update)
        if seed is None:
            raise ValueError(f"{ROTATE_KEY}: the upload carries no uint64 [1] seed (upload_rotate="
                             f"{self.upload_rotate!r}; a plain sign upload is not a rotated one: see "
                             f"rotate_upload.compress_sign_rotated); the round's seed is "
                             f"{'not set yet' if self.seed is None else hex(self.seed)}")
        if self.seed is not None and seed != self.seed:
            raise ValueError(f"{ROTATE_KEY}: the upload was rotated under seed {seed:#x}, this round's uploads under "
                             f"seed {self.seed:#x}: rows of two rotations cannot be chained")
        super().add(strip_seed(update), weight=weight, loss=loss, learning_rate=learning_rate, q=q)
        self.seed = seed

    def _reduce_chunk(self):
        """The staged chunk's rotated deltas onto the chain of P' columns, and its side-table sums."""
        L, st, n = self.layout, self.staging, self.slot
        first = self.chunks_done == 0
        if n > 0 and self.columns > 0:
            kg.reduce_sign(st.bits, st.scales, n, self.columns, self.chain, acc_in=None if first else self.chain)
        kx.side_accumulate(st.xi, n, L.Q, 0, acc_i=self.acc_i, acc_d=self.acc_d, accumulate=not first)
        self.chunks_done += 1
        self.slot = 0

    @on_stream
    def finalize_mean(self, denom32: float, denom64: float, *, out: torch.Tensor, cur_side: torch.Tensor,
                      model_side: Optional[torch.Tensor] = None, yogi: Optional[dict] = None,
                      mirror: Optional[torch.Tensor] = None):
        """Reduce the last chunk over P' columns, rotate the chain back in place (frt_unrotate), then ``out`` <- the
        round's starting model plus the mean delta over [0, P) (fcl_finish); the side table as
        ``SignRound.finalize_mean``."""
        from .sign_round import refuse as refuse_sign

        if yogi is not None:
            raise refuse_sign("the fused FedYoGi epilogue (take the mean, then yogi_step)", self.upload_sign)
        self._check_complete()
        den = float(np.float32(self.K))
        if float(denom32) != den:
            raise ValueError(f"a sign-delta round divides by its client count K={self.K}, not {denom32}")
        L = self.layout
        self._reduce_chunk()
        if L.P > 0:
            kr.unrotate(self.chain, L.P, self.seed, self.chain)
        kc.finish(self.chain, self.last_f32, L.P, den, out, mirror=mirror)
        kx.side_close(L.Q, 0, denom64, acc_i=self.acc_i, acc_d=self.acc_d, cur=cur_side, model=model_side)
