"""End to end on the MI355X: rounds over ``TorchModelAdapter(upload_lowrank=4)`` and over a mixin with
``device_upload_lowrank = 4`` on a small model (a conv, a linear, a BatchNorm with its int64 counter, biases), K = 5,
two rounds, a staging capacity of 2 (chunk folds).  With integer factors the new weights are ``L + ref / K`` in numpy
float32 bit for bit; under fed-adam they are the mean-then-step restatement of tests/serveropt_fixtures.py; an upload
in float64 or with a wrong factor shape raises at ``add`` and names the entry."""
import argparse

import numpy as np
import pytest
import torch

from tests import lowrank_fixtures as lf
from tests import serveropt_fixtures as sf
from tests.golden_io import DEFAULT_ARGS, StateDictModule

pytestmark = pytest.mark.gpu

F32 = np.float32
K, RANK, CAP = 5, 4, 2
NAMES = ["conv.weight", "conv.bias", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var",
         "bn.num_batches_tracked", "fc.weight", "fc.bias"]
SHAPES = [(6, 2, 3, 3), (6,), (6,), (6,), (6,), (6,), (), (10, 24), (10,)]
F_SHAPES = [s for n, s in zip(NAMES, SHAPES) if n != "bn.num_batches_tracked"]
ADAM = dict(server_eta=0.02, server_tau=1e-3, server_beta=0.9, server_beta2=0.99)


def _init():
    rng = np.random.default_rng(5)
    return [torch.tensor(11, dtype=torch.int64) if n == "bn.num_batches_tracked"
            else torch.from_numpy((rng.standard_normal(s) * 0.1).astype(F32)) for n, s in zip(NAMES, SHAPES)]


def _uploads(rng, counter):
    """K integer uploads: factors of the conv and the linear weight, dense integer deltas, the counter + 5."""
    ups = []
    for _ in range(K):
        u = {}
        for n, s in zip(NAMES, SHAPES):
            if n == "bn.num_batches_tracked":
                u[n] = np.asarray(counter + 5, dtype=np.int64)
            elif lf.factored(s, RANK):
                u[n] = rng.integers(-4, 5, size=(RANK, sum(lf.matrix_dims(s)))).astype(F32)
            else:
                u[n] = rng.integers(-4, 5, size=s).astype(F32)
        ups.append(u)
    return ups


def _adapter(via, policy):
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator
    from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    args = argparse.Namespace(**{**DEFAULT_ARGS, "gradient_policy": policy, **ADAM})
    if via == "mixin":  # the aggregator's own init_model builds the adapter from device_upload_lowrank
        class Base:
            def init_model(self):
                self.model_wrapper = StateDictModule(NAMES, _init())
                self.model_wrapper.get_model = lambda m=self.model_wrapper: m

        class Agg(DeviceAggregator, Base):
            device_upload_lowrank = RANK
            device_round_capacity = CAP
            device = "cuda:0"

            def __init__(self):
                DeviceAggregator.__init__(self, None, args)
                self.init_model()

        agg = Agg()
        assert type(agg.model_wrapper) is TorchModelAdapter and agg.model_wrapper.upload_lowrank == RANK
        return agg, agg.model_wrapper
    adapter = TorchModelAdapter(StateDictModule(NAMES, _init()), device="cuda:0", staging_capacity=CAP,
                                optimizer=TorchServerOptimizer(policy, args, "cuda:0"), upload_lowrank=RANK)
    return DeviceAggregator(adapter, args), adapter


def _flat(values):
    return np.concatenate([np.asarray(v, dtype=F32).reshape(-1) for v in values if np.asarray(v).dtype == F32])


@pytest.mark.parametrize("via,policy", [("adapter", None), ("mixin", None), ("adapter", "fed-adam")])
def test_rounds_match_the_restatement(via, policy):
    from fedscale_amd.lowrank_round import LowRankRound

    agg, adapter = _adapter(via, policy)
    rng = np.random.default_rng(17)
    m = v = None
    for r in range(2):
        L = [t.numpy() for t in adapter.get_weights()]
        ups = _uploads(rng, L[NAMES.index("bn.num_batches_tracked")])
        agg.start_round(K)
        for k, u in enumerate(ups):
            agg.on_result({"client_id": k, "update_weight": dict(u), "moving_loss": 0.5})
            assert k == K - 1 or type(agg._device_round) is LowRankRound
        ref = lf.ref64([[u[n] for n in NAMES if n != "bn.num_batches_tracked"] for u in ups], F_SHAPES, RANK)
        want = _flat(L) + ref.astype(F32) / F32(K)  # integer sums: exact in fp32
        if policy == "fed-adam":
            hp = sf.hparams(eta=ADAM["server_eta"], tau=ADAM["server_tau"], beta=ADAM["server_beta"],
                            beta2=ADAM["server_beta2"])
            m, v, want = sf.step("adam", want, _flat(L), m, v, hp, r == 0)
        got = [t.numpy() for t in adapter.get_weights()]
        assert sf.bits_equal(_flat(got), want), (via, policy, r, sf.first_difference(_flat(got), want))
        i = NAMES.index("bn.num_batches_tracked")
        assert got[i].dtype == np.int64 and int(got[i]) == int(L[i]) + 5


@pytest.mark.parametrize("what", ("float64", "shape"))
def test_a_bad_upload_raises_at_add_and_names_the_entry(what):
    _, adapter = _adapter("adapter", None)
    L = [t.numpy() for t in adapter.get_weights()]
    up = _uploads(np.random.default_rng(1), L[6])[0]
    up["fc.weight"] = up["fc.weight"].astype(np.float64) if what == "float64" else up["fc.weight"][:, :-1]
    rnd = adapter.begin_round(K, "fedavg")
    with pytest.raises(TypeError, match="fc.weight"):
        rnd.add(up)
