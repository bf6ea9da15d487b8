"""End to end on the MI355X: FetchSGD rounds over ``TorchModelAdapter(upload_sketch=...)`` against the numpy round of
tests/sketch_fixtures.py, bit for bit — K = 3 uploads, a model of P = 3 C + 5 fp32 columns and one int64 entry,
C = 1024, R = 5, rho = 0.9, k = 7."""
import pickle

import numpy as np
import pytest
import torch

from fedscale_amd.cloud.execution.sketch_upload import SKETCH_KEY, SketchSpec, compress_sketch
from tests import sketch_fixtures as fx
from tests.golden_io import DEFAULT_ARGS, StateDictModule

pytestmark = pytest.mark.gpu
K, C, R, RHO, TOP, SEED = 3, 1024, 5, 0.9, 7, 12345
NAMES = ["w", "n", "b"]
SPEC = SketchSpec(rows=R, cols=C, k=TOP, momentum=RHO, seed=SEED)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _flat(values):
    return np.concatenate([np.asarray(v, dtype=np.float32).reshape(-1) for v in values if v.dtype == np.float32])


def _adapter(capacity=None):
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    g = torch.Generator().manual_seed(0)
    init = [torch.randn(3, C, generator=g), torch.tensor(7), torch.randn(5, generator=g)]
    return TorchModelAdapter(StateDictModule(NAMES, init), device="cuda:0", staging_capacity=capacity,
                             upload_sketch=SPEC)


def _states(rng, L):
    """K client states around L: small noise everywhere and a few columns every client moves far."""
    heavy = rng.choice(3 * C + 5, 5, replace=False)
    out = []
    for _ in range(K):
        e = (0.01 * rng.standard_normal(3 * C + 5)).astype(np.float32)
        e[heavy] += rng.choice([-1.0, 1.0], 5).astype(np.float32) * 3
        x = _flat(L) + e
        out.append({"w": x[:3 * C].reshape(3, C), "n": np.array(7, dtype=np.int64), "b": x[3 * C:]})
    return out


def _upload(k, st, L, dev):
    """Client 1 sketches on the device and uploads device tensors; the others on the host."""
    if k == 1:
        st = {n: torch.from_numpy(v).to(dev) for n, v in st.items()}
    up = compress_sketch(st, dict(zip(NAMES, L)), SPEC)
    return {n: torch.from_numpy(np.asarray(v)).to(dev) for n, v in up.items()} if k == 1 else up


def _run(capacity, rounds=3):
    from fedscale_amd.sketch_round import SketchRound, SketchStaging

    adapter = _adapter(capacity)
    rng = np.random.default_rng(1)
    Su = Se = np.zeros((R, C), dtype=np.float32)
    history = []
    for r in range(rounds):
        L = [t.numpy() for t in adapter.get_weights()]
        states = _states(rng, L)
        tables = [fx.sketch(_flat(st.values()) - _flat(L), R, C, SEED) for st in states]
        rnd = adapter.begin_round(K, "fedavg")
        assert type(rnd) is SketchRound and type(adapter.staging) is SketchStaging and rnd.cap == min(capacity, K)
        for k, st in enumerate(states):
            up = _upload(k, st, L, adapter.device)
            assert np.array_equal(_bits(torch.as_tensor(up[SKETCH_KEY]).cpu().numpy()), _bits(tables[k]))
            rnd.add(up)
        adapter.apply_round(rnd, float(np.float32(K)), float(K))
        new, Su, Se, idx = fx.fetch_round(_flat(L), tables, Su, Se, RHO, TOP, SEED)
        got = adapter.get_weights()
        gu, ge = adapter._sketch_state.host()
        assert rnd.nonfinite() == 0 and rnd.chunks_done == (2 if capacity < K else 1)
        assert np.array_equal(rnd.idx.cpu().numpy(), idx) and int(got[1]) == 7, r
        assert np.array_equal(_bits(_flat([t.numpy() for t in got])), _bits(new)), r
        assert np.array_equal(_bits(gu), _bits(Su)) and np.array_equal(_bits(ge), _bits(Se)), r
        history.append([t.clone() for t in got] + [torch.from_numpy(gu.copy()), torch.from_numpy(ge.copy())])
    return adapter, history


def test_rounds_are_the_restatement_and_two_chunks_change_no_bit(gpu_device):
    (_, whole), (_, folded) = _run(3), _run(2)
    for a, b in zip(whole, folded):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_nan_upload_is_refused_and_pickle_and_set_weights_carry_the_state(gpu_device):
    from fedscale_amd.sketch_round import SketchNonFiniteError

    adapter, _ = _run(3, rounds=1)
    L = [t.numpy() for t in adapter.get_weights()]
    before = [t.clone() for t in adapter.get_weights()] + [torch.from_numpy(a.copy()) for a in
                                                             adapter._sketch_state.host()]
    assert before[-1].abs().sum() > 0
    states = _states(np.random.default_rng(5), L)
    states[1]["w"][2, 17] = np.nan
    rnd = adapter.begin_round(K, "fedavg")
    for k, st in enumerate(states):
        rnd.add(_upload(k, st, L, adapter.device))
    with pytest.raises(SketchNonFiniteError, match="unchanged"):
        adapter.apply_round(rnd, float(np.float32(K)), float(K))
    assert rnd.nonfinite() >= R
    twin = pickle.loads(pickle.dumps(adapter))
    for a in (adapter, twin):
        after = [t.clone() for t in a.get_weights()] + [torch.from_numpy(x.copy()) for x in a._sketch_state.host()]
        assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert twin.upload_sketch == SPEC
    adapter.set_weights([t.numpy() for t in before[:3]])
    assert all(not a.any() for a in adapter._sketch_state.host())
    for kw, word in ((dict(policy="fedbuff"), "fedbuff"), (dict(trim=1), "trim"), (dict(krum=1), "krum"),
                     (dict(clip=object()), "clip"), (dict(geomed=True), "geomed"),
                     (dict(signatures=True), "signatures")):
        with pytest.raises(NotImplementedError, match="upload_sketch=.*" + word):
            adapter.begin_round(4, kw.pop("policy", "fedavg"), **kw)


def test_a_round_through_the_mixins_device_upload_sketch_under_gradient_policy_fed_avg(gpu_device):
    """The aggregator's own init_model builds the adapter, with the server optimizer of a job whose config names
    FedAvg: the same bits as the first round of the adapter driven directly."""
    import argparse

    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    direct, want = _run(3, rounds=1)
    args = argparse.Namespace(**dict(DEFAULT_ARGS, gradient_policy="fed-avg"))

    class Base:
        def init_model(self):
            self.model_wrapper = _adapter(3).get_model()
            self.model_wrapper.get_model = lambda m=self.model_wrapper: m

    class Agg(DeviceAggregator, Base):
        device_upload_sketch = SPEC
        device = "cuda:0"

        def __init__(self):
            DeviceAggregator.__init__(self, None, args)
            self.init_model()

    agg = Agg()
    adapter = agg.model_wrapper
    assert type(adapter) is TorchModelAdapter and adapter.upload_sketch == SPEC and adapter.optimizer.mode == "fed-avg"
    L = [t.numpy() for t in adapter.get_weights()]
    agg.start_round(K)
    for k, st in enumerate(_states(np.random.default_rng(1), L)):
        agg.on_result({"client_id": k, "update_weight": _upload(k, st, L, adapter.device), "moving_loss": 0.5})
    got = [t for t in adapter.get_weights()] + [torch.from_numpy(a.copy()) for a in adapter._sketch_state.host()]
    assert all(torch.equal(x, y) for x, y in zip(got, want[0]))
