"""End to end on the MI355X: rounds over an adapter with ``upload_topk`` against the numpy restatement of the
contract (tests/sparse_fixtures.py: select, chain in arrival order, L + chain / K) on a mixed layout — odd sizes, a
0-d and an empty fp32 entry, int64 counters whose side table follows the fp32 oracle.  K = 7 with a staging capacity
of 3 (chunk folds) and of 7 (none) agree bit for bit; FedAvg is bit-exact, fed-yogi is bit-exact in m and v and meets
the project's rtol 1e-6 on the model; uploads arrive as dicts, lists, device tensors and through
``deserialize_response`` of their pickle; a malformed device row is counted by ``rejected()`` and adds nothing."""
import argparse
import copy
import pickle

import numpy as np
import pytest
import torch

from tests import sparse_fixtures as sf
from tests.golden_io import DEFAULT_ARGS, StateDictModule, assert_state_close, assert_state_equal

pytestmark = pytest.mark.gpu

K = 7
DENSITY = 0.05
SHAPES = [("conv.weight", (5, 7)), ("bn.num_batches_tracked", None), ("scale", ()), ("empty", (0,)),
          ("fc.weight", (33, 17)), ("counts", (3,)), ("fc.bias", (5021,))]


def _model():
    rng = np.random.default_rng(7)
    names, tensors = [], []
    for name, shape in SHAPES:
        names.append(name)
        if name == "bn.num_batches_tracked":
            tensors.append(torch.tensor(11, dtype=torch.int64))
        elif name == "counts":
            tensors.append(torch.from_numpy(rng.integers(0, 50, size=shape).astype(np.int64)))
        else:
            tensors.append(torch.from_numpy(np.asarray(rng.standard_normal(shape) * 0.05, dtype=np.float32)))
    return names, tensors


def _args(policy):
    a = dict(DEFAULT_ARGS)
    a["gradient_policy"] = policy
    return argparse.Namespace(**a)


def _flat(values):
    f = [np.asarray(v, dtype=np.float32).reshape(-1) for v in values if np.asarray(v).dtype == np.float32]
    return np.concatenate(f) if f else np.zeros(0, dtype=np.float32)


def _client_states(rng, names, L, n=K):
    """n trained states around the round's model ``L`` (a list of arrays): deltas of mixed magnitude per entry."""
    out = []
    for k in range(n):
        st = {}
        for name, a in zip(names, L):
            if a.dtype == np.int64:
                st[name] = np.asarray(a + 5 + k, dtype=np.int64)
            else:
                mag = 10.0 ** rng.uniform(-4, 0)
                st[name] = np.asarray(a + rng.standard_normal(a.shape) * mag, dtype=np.float32)
        out.append(st)
    return out


def _want_round(L, states, density, skip=()):
    """(the restated new fp32 bucket, the rows) of a round: e_k = x_k - L in fp32, its top-k pairs, chained in arrival
    order without the rows in ``skip``, L + chain / K."""
    from fedscale_amd.cloud.execution.sparse_upload import count_of

    Lf = _flat(L)
    k = count_of(density, Lf.size)
    rows = [sf.select(sf.delta(_flat(st.values()), Lf), k)[:2] for st in states]
    kept = [r for j, r in enumerate(rows) if j not in skip]
    return sf.finish(Lf, sf.chain(kept, Lf.size), len(states)), rows


def _mean_with(L, states, new_f):
    """The round's mean in the reference's list form: fp32 entries from the restated bucket, int64 entries as the fp32
    oracle averages them."""
    from oracle.cpu_reference import fedavg_close, fedavg_step

    acc = []
    for i, st in enumerate(states):
        acc = fedavg_step(acc, dict(st), i == 0)
    mean = fedavg_close(acc, len(states))
    o = 0
    for i, a in enumerate(L):
        if a.dtype == np.float32:
            mean[i] = new_f[o:o + a.size].reshape(a.shape)
            o += a.size
    return mean


def _send(how, up, dev, agg):
    from fedscale_amd.cloud.execution.sparse_upload import IDX_KEY

    if how == "list":
        return list(up.values())
    if how == "device":
        return {n: torch.from_numpy(np.array(a).view(np.int32) if n == IDX_KEY else np.array(a)).to(dev)
                for n, a in up.items()}
    if how == "pickle":
        return agg.deserialize_response(pickle.dumps({"update_weight": up}))["update_weight"]
    return up


def _run(policy, capacity, via_mixin_attr, dev="cuda:0", rounds=2, density=DENSITY, all_device=False):
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator
    from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
    from fedscale_amd.cloud.execution.sparse_upload import IDX_KEY, VAL_KEY, compress_topk, count_of
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.sparse_round import SparseRound, SparseStaging
    from oracle.cpu_reference import OracleModel, OracleModelAdapter, OracleServerOptimizer

    names, init = _model()
    args = _args(policy)
    if via_mixin_attr:  # the aggregator's own init_model builds the adapter from device_upload_topk
        class Base:
            def init_model(self):
                self.model_wrapper = StateDictModule(names, init)
                self.model_wrapper.get_model = lambda m=self.model_wrapper: m

        class Agg(DeviceAggregator, Base):
            device_upload_topk = density
            device_round_capacity = capacity
            device = dev

            def __init__(self):
                DeviceAggregator.__init__(self, None, args)
                self.init_model()

        agg = Agg()
        adapter = agg.model_wrapper
        assert type(adapter) is TorchModelAdapter and adapter.upload_topk == density
    else:
        adapter = TorchModelAdapter(StateDictModule(names, init), device=dev,
                                    optimizer=TorchServerOptimizer(policy, args, dev), staging_capacity=capacity,
                                    upload_topk=density)
        agg = DeviceAggregator(adapter, args)
    ref = OracleModelAdapter(OracleModel(names, init), OracleServerOptimizer(policy, args))
    rng = np.random.default_rng(3)
    history = []
    kmax = count_of(density, adapter.layout.P)
    for rnd in range(rounds):
        L = [t.numpy() for t in adapter.get_weights()]  # what the executors are sent for this round
        states = _client_states(rng, names, L)
        new_f, rows = _want_round(L, states, density)
        agg.start_round(K)
        for k, st in enumerate(states):
            up, _ = compress_topk(st, L, density=density)
            assert list(up) == ["bn.num_batches_tracked", "counts", IDX_KEY, VAL_KEY]
            assert np.array_equal(up[IDX_KEY], rows[k][0]) and up[VAL_KEY].tobytes() == rows[k][1].tobytes()
            how = "device" if all_device else {1: "device", 2: "pickle", 3: "list"}.get(k, "dict")
            agg.on_result({"client_id": k, "update_weight": _send(how, up, torch.device(dev), agg),
                           "moving_loss": 0.5})
            if k == 0:
                r = agg._device_round
                assert type(r) is SparseRound and type(adapter.staging) is SparseStaging and r.cap == min(capacity, K)
            if k == 4:
                assert agg._device_round.chunks_done == (1 if capacity < K else 0)
        ref.set_weights(copy.deepcopy(_mean_with(L, states, new_f)), client_training_results=[])
        got, want = adapter.get_weights(), [t.numpy() for t in ref.get_weights()]
        ctx = f"{policy} capacity {capacity} round {rnd}"
        if policy is None:
            assert_state_equal(got, want, ctx)
        else:
            assert_state_close(got, want, 1e-6, ctx)
            y, oy = adapter.optimizer.gradient_controller, ref.optimizer.gradient_controller
            for i, a in enumerate(L):
                if a.dtype == np.float32:
                    assert torch.equal(y.m_t[i].cpu(), oy.m_t[i]) and torch.equal(y.v_t[i].cpu(), oy.v_t[i]), (ctx, i)
        history.append([t.clone() for t in got])
        ref.model.load_state_dict({n: t for n, t in zip(names, got)})  # same trajectory
    st = adapter.staging
    assert st.kmax == kmax and st.idx.shape == st.val.shape == (min(capacity, K), (kmax + 3) // 4 * 4)
    assert st.nnz.shape == (min(capacity, K),) and st.offsets.shape[1] == min(capacity, K)
    return history


def test_fedavg_rounds_are_the_restatement_and_folds_change_no_bit(gpu_device):
    folded, whole = _run(None, 3, False), _run(None, 7, False)
    for a, b in zip(folded, whole):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_host_and_device_tensor_uploads_give_the_same_bits(gpu_device):
    mixed, device = _run(None, 3, False), _run(None, 3, False, all_device=True)
    for a, b in zip(mixed, device):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_fed_yogi_rounds(gpu_device):
    _run("fed-yogi", 3, False)


def test_rounds_through_the_mixins_device_upload_topk(gpu_device):
    a, b = _run(None, 3, True), _run(None, 3, False)
    for x, y in zip(a, b):
        assert all(torch.equal(p, q) for p, q in zip(x, y))


def test_density_one_sends_every_column(gpu_device):
    """Every column sent: the round is the dense in-order chain of the deltas."""
    _run(None, 3, False, rounds=1, density=1.0)


def test_a_malformed_device_row_is_rejected_and_adds_nothing(gpu_device):
    """A device-tensor upload is checked on the device: a row with a descending pair contributes nothing, the mean
    still divides by K, and rejected() counts it — across a chunk fold."""
    from fedscale_amd.cloud.execution.sparse_upload import IDX_KEY, compress_topk
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    dev = torch.device("cuda:0")
    names, init = _model()
    adapter = TorchModelAdapter(StateDictModule(names, init), device=dev, staging_capacity=2, upload_topk=DENSITY)
    L = [t.numpy() for t in adapter.get_weights()]
    states = _client_states(np.random.default_rng(5), names, L, n=5)
    want, rows = _want_round(L, states, DENSITY, skip=(1, 4))
    rnd = adapter.begin_round(5, "fedavg")
    for k, st in enumerate(states):
        up, _ = compress_topk(st, L, density=DENSITY)
        if k in (1, 4):
            bad = up[IDX_KEY].copy()
            if k == 1:
                bad[[5, 6]] = bad[[6, 5]]        # a descending pair
            else:
                bad[-1] = adapter.layout.P       # an index = P
            up = dict(up)
            up[IDX_KEY] = bad
            with pytest.raises(ValueError, match=IDX_KEY):  # the host path refuses it outright ...
                rnd.staging.put(0, up)
            up = _send("device", up, dev, None)  # ... the device path flags it
        rnd.add(up)
    assert rnd.rejected() == 1  # rows 0 .. 3 are folded so far
    adapter.apply_round(rnd, float(np.float32(5)), 5.0)
    assert rnd.rejected() == 2
    got = _flat([t.numpy() for t in adapter.get_weights()])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    full, _ = _want_round(L, states, DENSITY)
    assert not np.array_equal(full.view(np.uint32), want.view(np.uint32))


def test_a_dense_upload_names_the_problem_and_refusals_reach_no_round(gpu_device):
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    names, init = _model()
    adapter = TorchModelAdapter(StateDictModule(names, init), device="cuda:0", upload_topk=DENSITY)
    rnd = adapter.begin_round(2, "fedavg")
    with pytest.raises(TypeError, match="__topk_idx__"):
        rnd.add({n: t.numpy() for n, t in zip(names, init)})
    assert rnd.n == 0
    for kw, word in ((dict(policy="fedbuff"), "fedbuff"), (dict(policy="qfedavg"), "qfedavg"),
                     (dict(signatures=True), "cohort signatures"), (dict(trim=1), "trim"),
                     (dict(clip=object()), "clip")):
        with pytest.raises(NotImplementedError, match=r"upload_topk=0\.05.*" + word):
            adapter.begin_round(2, kw.pop("policy", "fedavg"), **kw)


def test_upload_topk_unset_changes_nothing(gpu_device):
    from fedscale_amd.bucket import ClientStaging
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.round import DeviceRound

    names, init = _model()
    adapter = TorchModelAdapter(StateDictModule(names, init), device="cuda:0")
    assert adapter.upload_topk is None and adapter.upload_quant is None and adapter.upload_dtype is None
    rnd = adapter.begin_round(2, "fedavg")
    assert type(rnd) is DeviceRound and type(adapter.staging) is ClientStaging
