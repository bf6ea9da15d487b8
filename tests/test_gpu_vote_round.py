"""End to end on the MI355X: rounds over an adapter with ``upload_vote`` against the numpy restatement of the contract
(include/fedvote.h: sign bits of x - L, the integer tally, L + the vote's step) on test_gpu_sign_round's mixed layout —
odd sizes, a 0-d and an empty fp32 entry, int64 counters whose side table follows the fp32 oracle."""
import copy
import pickle

import numpy as np
import pytest
import torch

from tests.golden_io import StateDictModule, assert_state_close, assert_state_equal
from tests.test_gpu_sign_round import K, _args, _client_states, _flat, _mean_with, _model

pytestmark = pytest.mark.gpu
ETA = 0.01


def _want(L, states, eta, mode):
    """(the restated new fp32 bucket, the integer tally, every client's bits)."""
    Lf = _flat(L)
    bits = [np.packbits(np.signbit(_flat(st.values()) - Lf), bitorder="little") for st in states]
    c = sum(np.unpackbits(b, bitorder="little")[:Lf.size].astype(np.int64) for b in bits)
    v, k = len(states) - 2 * c, len(states)
    if mode == "majority":
        s = np.where(v > 0, np.float32(eta), np.where(v < 0, -np.float32(eta), np.float32(0))).astype(np.float32)
    else:
        s = np.float32(eta) * (v.astype(np.float32) / np.float32(k))
    return Lf + s, c, bits


def _send(how, up, dev, agg):
    if how == "list":
        return list(up.values())
    if how == "device":
        return {n: torch.from_numpy(np.array(a)).to(dev) for n, a in up.items()}
    if how == "pickle":
        return agg.deserialize_response(pickle.dumps({"update_weight": up}))["update_weight"]
    return up


def _run(policy, capacity, via_mixin_attr, mode="majority", dev="cuda:0", rounds=3, poison=False):
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator
    from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
    from fedscale_amd.cloud.execution.vote_upload import VOTE_BITS_KEY, VoteSpec, compress_vote
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.vote_round import VoteRound, VoteStaging
    from oracle.cpu_reference import OracleModel, OracleModelAdapter, OracleServerOptimizer

    names, init = _model()
    args = _args(policy)
    spec = VoteSpec(ETA, mode)
    if via_mixin_attr:  # the aggregator's own init_model builds the adapter from device_upload_vote
        class Base:
            def init_model(self):
                self.model_wrapper = StateDictModule(names, init)
                self.model_wrapper.get_model = lambda m=self.model_wrapper: m

        class Agg(DeviceAggregator, Base):
            device_upload_vote = ETA  # a bare float is VoteSpec(ETA)
            device_round_capacity = capacity
            device = dev

            def __init__(self):
                DeviceAggregator.__init__(self, None, args)
                self.init_model()

        agg = Agg()
        adapter = agg.model_wrapper
        assert type(adapter) is TorchModelAdapter and adapter.upload_vote == spec
    else:
        adapter = TorchModelAdapter(StateDictModule(names, init), device=dev,
                                    optimizer=TorchServerOptimizer(policy, args, dev), staging_capacity=capacity,
                                    upload_vote=spec)
        agg = DeviceAggregator(adapter, args)
    ref = OracleModelAdapter(OracleModel(names, init), OracleServerOptimizer(policy, args))
    rng = np.random.default_rng(3)
    history = []
    for rnd in range(rounds):
        L = [t.numpy() for t in adapter.get_weights()]  # what the executors are sent for this round
        states = _client_states(rng, names, L)
        if poison:  # two Byzantine clients: each still has one vote per coordinate
            for name, a in zip(names, L):
                if a.dtype == np.float32:
                    states[1][name] = np.full(a.shape, np.nan, dtype=np.float32)
                    states[2][name] = np.full(a.shape, 1e30, dtype=np.float32)
        new_f, tally, bits = _want(L, states, ETA, mode)
        agg.start_round(K)
        for k, st in enumerate(states):
            up = compress_vote(st, L)
            assert np.array_equal(up[VOTE_BITS_KEY], bits[k])
            how = {1: "device", 2: "pickle", 3: "list"}.get(k, "dict")
            agg.on_result({"client_id": k, "update_weight": _send(how, up, torch.device(dev), agg),
                           "moving_loss": 0.5})
            if k == 0:
                r = agg._device_round
                assert type(r) is VoteRound and type(adapter.staging) is VoteStaging and r.cap == min(capacity, K)
            if k == 4:
                assert r.chunks_done == (1 if capacity < K else 0)
        assert np.array_equal(r.counts.cpu().numpy(), tally)  # readable after the round
        ref.set_weights(copy.deepcopy(_mean_with(L, states, new_f)), client_training_results=[])
        got, want = adapter.get_weights(), [t.numpy() for t in ref.get_weights()]
        ctx = f"{policy} {mode} capacity {capacity} round {rnd}"
        if policy is None:
            assert_state_equal(got, want, ctx)
        else:
            assert_state_close(got, want, 1e-6, ctx)
            y, oy = adapter.optimizer.gradient_controller, ref.optimizer.gradient_controller
            for i, a in enumerate(L):
                if a.dtype == np.float32:
                    assert torch.equal(y.m_t[i].cpu(), oy.m_t[i]) and torch.equal(y.v_t[i].cpu(), oy.v_t[i]), (ctx, i)
        if poison:
            Lf, gf = _flat(L), _flat([t.numpy() for t in got])
            e = np.float32(ETA)
            ok = [gf.view(np.uint32) == w.view(np.uint32) for w in (Lf + e, Lf - e, Lf + np.float32(0))]
            assert np.isfinite(gf).all() and (ok[0] | ok[1] | ok[2]).all()
        history.append([t.clone() for t in got])
        ref.model.load_state_dict({n: t for n, t in zip(names, got)})  # same trajectory
    assert adapter.staging.bits.shape[0] == min(capacity, K)
    return history


def test_majority_rounds_are_the_restatement_and_a_fold_changes_no_bit(gpu_device):
    folded, whole = _run(None, 4, False), _run(None, 7, False)
    for a, b in zip(folded, whole):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("policy,mode", [(None, "mean"), ("fed-yogi", "majority")])
def test_a_mean_round_and_a_fed_yogi_round(gpu_device, policy, mode):
    _run(policy, 4, False, mode=mode, rounds=1 if policy is None else 2)


def test_a_round_through_the_mixins_device_upload_vote(gpu_device):
    a, b = _run(None, 4, True, rounds=1), _run(None, 4, False, rounds=1)
    assert all(torch.equal(p, q) for p, q in zip(a[0], b[0]))


def test_poisoned_clients_have_one_vote_each(gpu_device):
    _run(None, 7, False, rounds=1, poison=True)


def test_refusals_name_upload_vote_and_unset_changes_nothing(gpu_device):
    from fedscale_amd.bucket import ClientStaging
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.round import DeviceRound

    names, init = _model()
    adapter = TorchModelAdapter(StateDictModule(names, init), device="cuda:0", upload_vote=ETA)
    rnd = adapter.begin_round(2, "fedavg")
    with pytest.raises(TypeError, match=r"conv\.weight.*float32"):
        rnd.add({n: t.numpy() for n, t in zip(names, init)})
    assert rnd.n == 0
    for kw, word in ((dict(policy="fedbuff"), "fedbuff"), (dict(policy="qfedavg"), "qfedavg"), (dict(trim=1), "trim"),
                     (dict(krum=1), "krum")):
        with pytest.raises(NotImplementedError, match="upload_vote=.*" + word):
            adapter.begin_round(4, kw.pop("policy", "fedavg"), **kw)
    with pytest.raises(NotImplementedError, match="upload_vote=.*upload_sign"):
        TorchModelAdapter(StateDictModule(names, init), device="cuda:0", upload_vote=ETA, upload_sign="sign1")
    outs = []
    for kw in ({}, {"upload_vote": None}):
        adapter = TorchModelAdapter(StateDictModule(names, init), device="cuda:0", **kw)
        assert adapter.upload_vote is None and "upload_vote" not in adapter.__dict__
        L = [t.numpy() for t in adapter.get_weights()]
        rnd = adapter.begin_round(3, "fedavg")
        assert type(rnd) is DeviceRound and type(adapter.staging) is ClientStaging
        for st in _client_states(np.random.default_rng(8), names, L, 3):
            rnd.add(st)
        adapter.apply_round(rnd, float(np.float32(3)), 3.0)
        outs.append([t.clone() for t in adapter.get_weights()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
