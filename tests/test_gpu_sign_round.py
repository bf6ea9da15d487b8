"""End to end on the MI355X: rounds over an adapter with ``upload_sign="sign1"`` against the numpy restatement of the
contract (tests/sign_fixtures.py: encode, dequantise, chain in arrival order, L + chain / K) on a mixed layout — odd
sizes, a 0-d and an empty fp32 entry, int64 counters whose side table follows the fp32 oracle.  K = 7 with a staging
capacity of 4 (a chunk fold) and of 7 (none) agree bit for bit; FedAvg is bit-exact, fed-yogi is bit-exact in m and
v and meets the project's rtol 1e-6 on the model; uploads arrive as dicts, lists, device tensors and through
``deserialize_response`` of their pickle, and the executors feed their residuals back from round to round."""
import argparse
import copy
import pickle

import numpy as np
import pytest
import torch

from tests import sign_fixtures as sg
from tests.golden_io import DEFAULT_ARGS, StateDictModule, assert_state_close, assert_state_equal

pytestmark = pytest.mark.gpu

K = 7
SHAPES = [("conv.weight", (5, 7)), ("bn.num_batches_tracked", None), ("scale", ()), ("empty", (0,)),
          ("fc.weight", (33, 17)), ("counts", (3,)), ("fc.bias", (1021,))]


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


def _want_round(L, states, residuals):
    """(the restated new fp32 bucket, the rows, the new residuals) of a round: e_k = (x_k - L) + r_k in fp32, encoded,
    dequantised, chained in arrival order, L + chain / K."""
    Lf = _flat(L)
    enc = [sg.encode(sg.delta(_flat(st.values()), Lf, r)) for st, r in zip(states, residuals)]
    rows = [(b, s) for b, s, _ in enc]
    return sg.finish(Lf, sg.chain(rows, P=Lf.size), len(states)), rows, [r for _, _, r in enc]


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
    from fedscale_amd.cloud.execution.sign_upload import BITS_KEY, SCALES_KEY

    if how == "list":
        return list(up.values())
    if how == "device":
        return {n: torch.from_numpy(np.array(a)).to(dev) for n, a in up.items()}
    if how == "pickle":
        return agg.deserialize_response(pickle.dumps({"update_weight": up}))["update_weight"]
    assert list(up)[-2:] == [BITS_KEY, SCALES_KEY]
    return up


def _run(policy, capacity, via_mixin_attr, dev="cuda:0", rounds=3):
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator
    from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
    from fedscale_amd.cloud.execution.sign_upload import BITS_KEY, SCALES_KEY, compress_sign
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.sign_round import SignRound, SignStaging
    from oracle.cpu_reference import OracleModel, OracleModelAdapter, OracleServerOptimizer

    names, init = _model()
    args = _args(policy)
    if via_mixin_attr:  # the aggregator's own init_model builds the adapter from device_upload_sign
        class Base:
            def init_model(self):
                self.model_wrapper = StateDictModule(names, init)
                self.model_wrapper.get_model = lambda m=self.model_wrapper: m

        class Agg(DeviceAggregator, Base):
            device_upload_sign = "sign1"
            device_round_capacity = capacity
            device = dev

            def __init__(self):
                DeviceAggregator.__init__(self, None, args)
                self.init_model()

        agg = Agg()
        adapter = agg.model_wrapper
        assert type(adapter) is TorchModelAdapter and adapter.upload_sign == "sign1"
    else:
        adapter = TorchModelAdapter(StateDictModule(names, init), device=dev,
                                    optimizer=TorchServerOptimizer(policy, args, dev), staging_capacity=capacity,
                                    upload_sign="sign1")
        agg = DeviceAggregator(adapter, args)
    ref = OracleModelAdapter(OracleModel(names, init), OracleServerOptimizer(policy, args))
    rng = np.random.default_rng(3)
    history = []
    residuals = [None] * K  # every executor's error-feedback state, kept between rounds
    for rnd in range(rounds):
        L = [t.numpy() for t in adapter.get_weights()]  # what the executors are sent for this round
        states = _client_states(rng, names, L)
        new_f, rows, want_res = _want_round(L, states, residuals)
        agg.start_round(K)
        for k, st in enumerate(states):
            up, residuals[k] = compress_sign(st, L, residual=residuals[k], residual_out=True)
            assert np.array_equal(up[BITS_KEY], rows[k][0])
            assert np.array_equal(up[SCALES_KEY].view(np.uint32), rows[k][1].view(np.uint32))
            assert np.array_equal(residuals[k].view(np.uint32), want_res[k].view(np.uint32))
            how = {1: "device", 2: "pickle", 3: "list"}.get(k, "dict")
            agg.on_result({"client_id": k, "update_weight": _send(how, up, torch.device(dev), agg),
                           "moving_loss": 0.5})
            if k == 0:
                r = agg._device_round
                assert type(r) is SignRound and type(adapter.staging) is SignStaging and r.cap == min(capacity, K)
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
    P = adapter.layout.P
    assert adapter.staging.bits.shape == (min(capacity, K), sg.bit_stride(P))
    assert adapter.staging.scales.shape == (min(capacity, K), sg.scale_stride(P))
    return history


def test_fedavg_rounds_are_the_restatement_and_a_fold_changes_no_bit(gpu_device):
    folded, whole = _run(None, 4, False), _run(None, 7, False)
    for a, b in zip(folded, whole):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_fed_yogi_rounds(gpu_device):
    _run("fed-yogi", 4, False, rounds=2)


def test_rounds_through_the_mixins_device_upload_sign(gpu_device):
    a, b = _run(None, 4, True, rounds=2), _run(None, 4, False, rounds=2)
    for x, y in zip(a, b):
        assert all(torch.equal(p, q) for p, q in zip(x, y))


def test_a_nan_block_makes_exactly_its_256_columns_nan(gpu_device):
    from fedscale_amd.cloud.execution.sign_upload import SCALES_KEY, compress_sign
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    names, init = _model()
    adapter = TorchModelAdapter(StateDictModule(names, init), device="cuda:0", upload_sign="sign1")
    L = [t.numpy() for t in adapter.get_weights()]
    states = _client_states(np.random.default_rng(5), names, L, 3)
    states[1]["fc.weight"].reshape(-1)[300] = np.nan  # column 35 + 1 + 300 = 336 of the bucket: block 1
    rnd = adapter.begin_round(3, "fedavg")
    for st in states:
        up, _ = compress_sign(st, L)
        rnd.add(up)
    assert not np.isnan(up[SCALES_KEY]).any()
    s1 = compress_sign(states[1], L)[0][SCALES_KEY]
    assert np.array_equal(np.isnan(s1), np.arange(s1.size) == 1) and s1.view(np.uint32)[1] == 0x7FC00000
    adapter.apply_round(rnd, float(np.float32(3)), 3.0)
    got = _flat([t.numpy() for t in adapter.get_weights()])
    want, _, _ = _want_round(L, states, [None] * 3)
    nan = np.zeros(got.size, dtype=bool)
    nan[256:512] = True
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def test_a_float32_upload_names_its_entry_and_refusals_reach_no_round(gpu_device):
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    names, init = _model()
    adapter = TorchModelAdapter(StateDictModule(names, init), device="cuda:0", upload_sign="sign1")
    rnd = adapter.begin_round(2, "fedavg")
    with pytest.raises(TypeError, match=r"conv\.weight.*float32"):
        rnd.add({n: t.numpy() for n, t in zip(names, init)})
    assert rnd.n == 0
    for kw, word in ((dict(policy="fedbuff"), "fedbuff"), (dict(policy="qfedavg"), "qfedavg"),
                     (dict(signatures=True), "cohort signatures"), (dict(trim=1), "trim")):
        with pytest.raises(NotImplementedError, match="upload_sign='sign1'.*" + word):
            adapter.begin_round(2, kw.pop("policy", "fedavg"), **kw)
    for kw in (dict(krum=1), dict(geomed=True)):
        with pytest.raises(NotImplementedError, match=r"upload_sign='sign1' \(1-bit sign delta uploads\)"):
            adapter.begin_round(4, "fedavg", **kw)


def test_upload_sign_unset_changes_nothing(gpu_device):
    """An adapter built with upload_sign=None is the adapter built without the keyword: the same round and staging
    classes, and a plain fp32 round's model bit for bit."""
    from fedscale_amd.bucket import ClientStaging
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.round import DeviceRound

    names, init = _model()
    outs = []
    for kw in ({}, {"upload_sign": None}):
        adapter = TorchModelAdapter(StateDictModule(names, init), device="cuda:0", **kw)
        assert adapter.upload_sign is None and adapter.upload_quant is None and adapter.upload_dtype is None
        assert "upload_sign" not in adapter.__dict__
        L = [t.numpy() for t in adapter.get_weights()]
        states = _client_states(np.random.default_rng(8), names, L, 3)
        rnd = adapter.begin_round(3, "fedavg")
        assert type(rnd) is DeviceRound and type(adapter.staging) is ClientStaging
        for st in states:
            rnd.add(st)
        adapter.apply_round(rnd, float(np.float32(3)), 3.0)
        outs.append([t.clone() for t in adapter.get_weights()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
