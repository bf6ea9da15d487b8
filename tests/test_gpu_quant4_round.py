"""End to end on the MI355X: rounds of K = 5 in two chunks over the ``TorchModelAdapter(upload_fp4="mxfp4")`` a mixin
with ``device_upload_fp4`` builds, on a tiny model, equal ``L + chain / K`` of the numpy restatement bit for bit, int64
side table included; under fed-adam, that mean followed by the restated step of tests/serveropt_fixtures.py."""
import argparse

import numpy as np
import pytest
import torch

from tests import quant4_fixtures as q4f
from tests import serveropt_fixtures as sf
from tests.golden_io import DEFAULT_ARGS, StateDictModule

pytestmark = pytest.mark.gpu

F32 = np.float32
K, CAP = 5, 3
NAMES = ["conv.weight", "conv.bias", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var",
         "bn.num_batches_tracked", "fc.weight", "fc.bias"]
SHAPES = [(6, 2, 3, 3), (6,), (6,), (6,), (6,), (6,), (), (10, 24), (11,)]
ADAM = dict(server_eta=0.02, server_tau=1e-3, server_beta=0.9, server_beta2=0.99)


def _init():
    rng = np.random.default_rng(5)
    return [torch.tensor(11, dtype=torch.int64) if n == "bn.num_batches_tracked"
            else torch.from_numpy((rng.standard_normal(s) * 0.1).astype(F32)) for n, s in zip(NAMES, SHAPES)]


def _aggregator(policy):
    """The aggregator whose own init_model builds the adapter from device_upload_fp4 and the policy's optimizer."""
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    args = argparse.Namespace(**{**DEFAULT_ARGS, "gradient_policy": policy, **ADAM})

    class Base:
        def init_model(self):
            self.model_wrapper = StateDictModule(NAMES, _init())
            self.model_wrapper.get_model = lambda m=self.model_wrapper: m

    class Agg(DeviceAggregator, Base):
        device_upload_fp4, device_round_capacity, device = "mxfp4", CAP, "cuda:0"

    agg = Agg(None, args)
    agg.init_model()
    assert type(agg.model_wrapper) is TorchModelAdapter and agg.model_wrapper.upload_fp4 == "mxfp4"
    return agg, agg.model_wrapper


def _flat(values):
    return np.concatenate([np.asarray(v, dtype=F32).reshape(-1) for v in values if np.asarray(v).dtype == F32])


@pytest.mark.parametrize("policy", (None, "fed-adam"))
def test_rounds_match_the_restatement(gpu_device, policy):
    from fedscale_amd.cloud.execution.quant4_upload import compress_delta4
    from fedscale_amd.quant4_round import Quant4Round, Quant4Staging

    agg, adapter = _aggregator(policy)
    rng = np.random.default_rng(17)
    m = v = None
    for r in range(2):
        L = [t.numpy() for t in adapter.get_weights()]
        states = [{n: np.asarray(a + 5 + k, dtype=np.int64) if a.dtype == np.int64 else
                   np.asarray(a + rng.standard_normal(a.shape) * 10.0 ** rng.uniform(-4, 0), dtype=F32)
                   for n, a in zip(NAMES, L)} for k in range(K)]
        rows = [q4f.quantize(_flat(st.values()) - _flat(L))[:2] for st in states]
        agg.start_round(K)
        for k, st in enumerate(states):
            up, _ = compress_delta4(st, L)
            if k == 1:  # the same upload as device tensors, and as a list
                up = {n: torch.from_numpy(np.array(a)).to(gpu_device) for n, a in up.items()}
            elif k == 2:
                up = list(up.values())
            agg.on_result({"client_id": k, "update_weight": up, "moving_loss": 0.5})
            if k < K - 1:
                rnd = agg._device_round
                assert type(rnd) is Quant4Round and type(adapter.staging) is Quant4Staging
                assert rnd.chunks_done == (1 if k >= CAP else 0)
        want = _flat(L) + q4f.chain(rows, P=_flat(L).size) / F32(K)
        if policy == "fed-adam":
            hp = sf.hparams(eta=ADAM["server_eta"], tau=ADAM["server_tau"], beta=ADAM["server_beta"],
                            beta2=ADAM["server_beta2"])
            m, v, want = sf.step("adam", want, _flat(L), m, v, hp, r == 0)
        got = [t.numpy() for t in adapter.get_weights()]
        assert sf.bits_equal(_flat(got), want), (policy, r, sf.first_difference(_flat(got), want))
        assert got[6].dtype == np.int64 and int(got[6]) == int(L[6]) + 5 + 2  # the counter: the mean of +5 .. +9
    assert adapter.staging.q4.shape == (CAP, adapter.layout.ld // 2) and adapter.staging.scales.shape[0] == CAP
