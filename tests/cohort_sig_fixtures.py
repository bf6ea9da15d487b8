"""Loader for the Auxo signature fixtures tests/golden/auxo_sig_*.npz (written by
tests/golden/gen_golden_auxo_sig.py from the reference's own ``register_gradient`` and the numpy / sklearn
lines of its ``cohort_clustering``).  One .npz per fixture, no .json beside it (golden_io.scenario_names lists
json + npz pairs as aggregation scenarios).

Arrays: ``names`` (state_dict keys), ``model/<i>`` (the cohort's model, tensor i; fp32 tensors are stored as
float16 where that is exact), the K uploads either as
``uploads/<i>`` ([K, *shape]) or — the config 1 layout, to keep the file small — as ``udelta/<i>`` (int8
[K, *shape]) with ``udelta_scale``: upload = model + float32(delta) * scale, one fp32 multiply and add; the
generator feeds the reference exactly what this loader returns.  Expected: ``sig`` [K, D], ``mean`` [D],
``centered`` [K, D] float16 and, where the centred matrix is finite, sklearn's ``normalized`` [K, D].
"""
from __future__ import annotations

import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("auxo_sig_mixed_k9", "auxo_sig_femnist_cnn_k10", "auxo_sig_tiny_k5", "auxo_sig_values_k6")


class SigFixture:
    def __init__(self, name: str, arrays=None):
        self.name = name
        if arrays is None:
            z = np.load(os.path.join(GOLDEN, name + ".npz"))  # allow_pickle stays False
            arrays = {k: z[k] for k in z.files}
        self.arrays = arrays
        self.names = [str(n) for n in arrays["names"]]
        self.T = len(self.names)
        self.model = [a.astype(np.float32) if a.dtype == np.float16 else a  # (stored as float16 when that is exact)
                      for a in (arrays[f"model/{i}"] for i in range(self.T))]
        if "udelta_scale" in arrays:
            sc = np.float32(arrays["udelta_scale"])
            ups = [self.model[i][None] + arrays[f"udelta/{i}"].astype(np.float32) * sc for i in range(self.T)]
        else:
            ups = [arrays[f"uploads/{i}"] for i in range(self.T)]
        self.K = int(ups[0].shape[0])
        assert all(u.dtype == m.dtype and u.shape[1:] == m.shape for u, m in zip(ups, self.model))
        self._ups = ups

    def upload(self, k: int) -> dict:
        """Client k's ``update_weight``: name -> ndarray (torch_client.py:76-78)."""
        return {n: np.array(u[k]) for n, u in zip(self.names, self._ups)}

    def module(self) -> torch.nn.Module:
        from tests.golden_io import StateDictModule

        return StateDictModule(self.names, [torch.from_numpy(np.array(m)) for m in self.model])

    def expected(self, key: str):
        return self.arrays.get(key)


def load(name: str) -> SigFixture:
    return SigFixture(name)
