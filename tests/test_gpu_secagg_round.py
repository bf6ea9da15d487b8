"""End to end on the MI355X: secure-aggregation rounds over an adapter with ``upload_secagg`` against the numpy
restatement of the contract (tests/secagg_fixtures.py).  Seven clients on a 4-regular ring graph, two of them dropped:
the new model equals the restatement bit for bit, equals the same round with no masks at all (the masks cancel
exactly), and its int64 entry equals plain FedAvg's; a staging capacity of 3 (chunk folds) changes no bit; a fed-yogi
round is the restated mean pushed through the existing YoGi step; a key left out of the unmask is caught by the range
check before the adapter commits; the result stays within the fixed-point rounding of plain arithmetic; and the
aggregator mixin drives all of it through its hook."""
import argparse

import numpy as np
import pytest
import torch

from tests import secagg_fixtures as sf
from tests.golden_io import DEFAULT_ARGS, StateDictModule

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRAPH_K = 7
ARRIVED = [6, 0, 1, 3, 4]  # arrival order; clients 2 and 5 dropped
NONCE = (41, 0, 9)
F, B = 16, 20
SHAPES = [("conv.weight", (5, 7)), ("bn.num_batches_tracked", None), ("scale", ()), ("empty", (0,)),
          ("fc.weight", (33, 17)), ("fc.bias", (1021,)), ("head.weight", (50, 50))]  # P = 4118 in six fp32 entries


def _model(shapes=SHAPES):
    rng = np.random.default_rng(7)
    names, tensors = [], []
    for name, shape in shapes:
        names.append(name)
        if shape is None:
            tensors.append(torch.tensor(11, dtype=torch.int64))
        else:
            tensors.append(torch.from_numpy(np.asarray(rng.standard_normal(shape) * 0.05, dtype=np.float32)))
    return names, tensors


def _args(policy=None):
    a = dict(DEFAULT_ARGS)
    a["gradient_policy"] = policy
    return argparse.Namespace(**a)


def _flat(values):
    f = [np.asarray(v, dtype=np.float32).reshape(-1) for v in values if np.asarray(v).dtype == np.float32]
    return np.concatenate(f) if f else np.zeros(0, dtype=np.float32)


def _states(rng, names, L, n):
    """n trained states around ``L``: updates of mixed magnitude per entry, every |d| < 8 (no element is clamped at
    f = 16, b = 20: B / 2^f is just under 16)."""
    out = []
    for k in range(n):
        st = {}
        for nm, a in zip(names, L):
            if a.dtype == np.int64:
                st[nm] = np.asarray(a + 5 + k, dtype=np.int64)
            else:
                mag = 10.0 ** rng.uniform(-4, 0)
                st[nm] = np.asarray(a + np.clip(rng.standard_normal(a.shape) * mag, -7.5, 7.5), dtype=np.float32)
        out.append(st)
    return out


_CASE = {}


def _case():
    """The shared round, made once and left unchanged: the model, the graph, the arrived clients' states, their
    uploads (masked and plain) and the restated results."""
    if _CASE:
        return _CASE
    from fedscale_amd.cloud.execution.secagg_upload import compress_secagg, encode_update
    from fedscale_amd.secagg_round import SecAggSpec

    names, init = _model()
    L = [t.numpy() for t in init]
    rng = np.random.default_rng(3)
    graph = sf.RingGraph(rng, GRAPH_K, reach=2)
    states = _states(rng, names, L, len(ARRIVED))
    spec = SecAggSpec(F, B)
    masked, plain = [], []
    for st, u in zip(states, ARRIVED):
        self_key, add, sub = graph.client_keys(u)
        up, stats = compress_secagg(st, L, spec, self_key=self_key, add_keys=add, sub_keys=sub, nonce=NONCE,
                                    return_stats=True)
        assert stats == (0, 0)
        masked.append(up)
        plain.append(encode_update(st, L, spec)[0])
    xs = [_flat(st.values()) for st in states]
    want, bad, total, clamped = sf.round_model(xs, _flat(L), F, B, graph, ARRIVED, NONCE)
    assert bad == 0 and clamped == 0
    # the executor's bytes are the restatement's
    q0 = sf.masked_upload(sf.encode(xs[0], _flat(L), F, B)[0], graph, ARRIVED[0], NONCE)
    assert np.array_equal(np.concatenate([masked[0][n].reshape(-1) for n, a in zip(names, L) if a.dtype == np.float32]),
                          q0)
    _CASE.update(names=names, init=init, L=L, graph=graph, states=states, spec=spec, masked=masked, plain=plain,
                 xs=xs, want=want, total=total)
    return _CASE


def _adapter(policy=None, capacity=None, spec=None, shapes=None):
    from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    names, init = _model(shapes) if shapes else (_case()["names"], _case()["init"])
    kw = {} if spec is False else {"upload_secagg": spec or _case()["spec"]}
    return TorchModelAdapter(StateDictModule(names, init), device=DEV,
                             optimizer=TorchServerOptimizer(policy, _args(policy), DEV), staging_capacity=capacity, **kw)


def _run_round(adapter, uploads, sub, add, nonce=NONCE, how=()):
    n = len(uploads)
    rnd = adapter.begin_round(n, "fedavg")
    for k, up in enumerate(uploads):
        if k in how:  # device tensors of the same bits, and a list upload
            up = {nm: torch.from_numpy(np.asarray(a).view(np.int32) if a.dtype == np.uint32 else np.asarray(a)).to(DEV)
                  for nm, a in up.items()} if how[k] == "device" else list(up.values())
        rnd.add(up)
    rnd.unmask(sub, add, nonce)
    adapter.apply_round(rnd, float(np.float32(n)), float(n))
    return rnd


def _plain_fedavg(states, policy=None):
    """The same states through an adapter without the option: whole fp32 weights, in the clear."""
    a = _adapter(policy, spec=False)
    rnd = a.begin_round(len(states), "fedavg")
    for st in states:
        rnd.add(st)
    a.apply_round(rnd, float(np.float32(len(states))), float(len(states)))
    return a


def test_ring_graph_round_with_dropouts_equals_the_restatement_and_the_unmasked_round(gpu_device):
    from fedscale_amd.secagg_round import MaskedStaging, SecAggRound

    c = _case()
    sub, add = c["graph"].unmask_keys(ARRIVED)
    histories = []
    for capacity in (None, 3):  # 3: the round folds a chunk after its third upload
        a = _adapter(capacity=capacity)
        rnd = _run_round(a, c["masked"], sub, add, how={1: "device", 2: "list"})
        assert type(rnd) is SecAggRound and type(a.staging) is MaskedStaging
        assert rnd.chunks_done == (2 if capacity else 1) and rnd.n_keys == len(sub) + len(add) == 13
        assert rnd.out_of_range() == 0
        got = a.get_weights()
        assert np.array_equal(_flat([t.numpy() for t in got]).view(np.uint32), c["want"].view(np.uint32)), capacity
        assert np.array_equal(rnd.total.cpu().numpy().view(np.uint32)[:c["want"].size], c["total"])
        histories.append(got)
    assert all(torch.equal(x, y) for x, y in zip(*histories))
    # the same round with no masks at all: the masks cancel exactly
    a = _adapter()
    rnd = _run_round(a, c["plain"], [], [])
    assert rnd.n_keys == 0
    assert all(torch.equal(x, y) for x, y in zip(a.get_weights(), histories[0]))
    # the int64 entry is plain FedAvg's
    p = _plain_fedavg(c["states"])
    i = c["names"].index("bn.num_batches_tracked")
    assert histories[0][i].dtype == torch.int64 and torch.equal(histories[0][i], p.get_weights()[i])
    assert int(histories[0][i]) == 11 + 5 + 2  # mean of 11 + 5 + k, k = 0 .. 4


def test_result_is_within_the_fixed_point_rounding_of_plain_arithmetic(gpu_device):
    """|new - (L + mean_k (x_k - L))| <= 2^-(f+1) + 2^-22 (|L| + max_k |x_k|) for every column, the reference mean in
    float64: the first term is the rounding of rint, the second covers the fp32 roundings of x - L, of the cast of the
    mean and of the final add."""
    c = _case()
    sub, add = c["graph"].unmask_keys(ARRIVED)
    a = _adapter()
    _run_round(a, c["masked"], sub, add)
    new = _flat([t.numpy() for t in a.get_weights()]).astype(np.float64)
    L = _flat(c["L"]).astype(np.float64)
    X = np.stack(c["xs"]).astype(np.float64)
    for x in c["xs"]:  # the restatement: no element was clamped
        assert sf.encode(x, _flat(c["L"]), F, B)[1:] == (0, 0)
    ref = L + (X - L).mean(axis=0)
    bound = 2.0 ** -(F + 1) + 2.0 ** -22 * (np.abs(L) + np.abs(X).max(axis=0))
    err = np.abs(new - ref)
    print(f"max err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


def test_fed_yogi_round_is_the_restated_mean_through_yogi_step(gpu_device):
    from fedscale_amd import kernels as kx

    c = _case()
    sub, add = c["graph"].unmask_keys(ARRIVED)
    a = _adapter("fed-yogi")
    last = a._snapshot().f32.clone()
    _run_round(a, c["masked"], sub, add)
    y = a.optimizer.gradient_controller
    P, ld = a.layout.P, a.layout.ld
    mean = torch.zeros(ld, dtype=torch.float32, device=DEV)
    mean[:P] = torch.from_numpy(c["want"]).to(DEV)  # the restatement's mean: L + sum / (2^f n)
    m, v, out = (torch.zeros(ld, dtype=torch.float32, device=DEV) for _ in range(3))
    kx.yogi_step(mean, last, m, v, out, P, init=True, **y.fp32_hparams())
    assert torch.equal(y.m[:P], m[:P]) and torch.equal(y.v[:P], v[:P])
    got = torch.from_numpy(_flat([t.numpy() for t in a.get_weights()])).to(DEV)
    assert torch.equal(got.view(torch.int32), out[:P].view(torch.int32))
    assert not torch.equal(got, mean[:P])  # (the step did something)
    # the int64 entry follows the same path as a plain fed-yogi round's
    p = _plain_fedavg(c["states"], "fed-yogi")
    i = c["names"].index("bn.num_batches_tracked")
    assert torch.equal(a.get_weights()[i], p.get_weights()[i])


def test_a_key_left_out_of_unmask_is_caught_before_the_adapter_commits(gpu_device):
    """P = 4096, K = 5, one pairwise key missing: a column stays in range with probability (2 K B + 1) / 2^32 =
    0.0024, so the expected out-of-range share is 0.9976."""
    from fedscale_amd.cloud.execution.secagg_upload import compress_secagg
    from fedscale_amd.secagg_round import SecAggSpec, SecAggUnmaskError

    shapes = [("w", (4096,))]  # (no int64 entry: the finish also writes the adapter's pinned egress mirror)
    names, init = _model(shapes)
    L = [t.numpy() for t in init]
    rng = np.random.default_rng(8)
    graph = sf.RingGraph(rng, GRAPH_K, reach=2)
    states = _states(rng, names, L, len(ARRIVED))
    xs = [_flat(st.values()) for st in states]
    _, want_bad, _, _ = sf.round_model(xs, _flat(L), F, B, graph, ARRIVED, NONCE, skip_pair=(1, 2))
    assert want_bad >= 4096 // 2
    sub, add = graph.unmask_keys(ARRIVED, skip_pair=(1, 2))  # client 2 dropped; client 1 added that mask
    for verify in (True, False):
        spec = SecAggSpec(F, B, verify=verify)
        ups = []
        for st, u in zip(states, ARRIVED):
            self_key, ka, ks_ = graph.client_keys(u)
            ups.append(compress_secagg(st, L, spec, self_key=self_key, add_keys=ka, sub_keys=ks_, nonce=NONCE))
        a = _adapter(spec=spec, shapes=shapes)
        before = [t.clone() for t in a.get_weights()]
        if verify:
            with pytest.raises(SecAggUnmaskError, match="not applied") as e:
                _run_round(a, ups, sub, add)
            assert e.value.count == want_bad and e.value.P == 4096
            assert all(torch.equal(x, y) for x, y in zip(a.get_weights(), before))  # the old model
            # the round after it, with every key, is an ordinary one
            rnd = _run_round(a, ups, *graph.unmask_keys(ARRIVED))
            assert rnd.out_of_range() == 0 and not torch.equal(a.get_weights()[0], before[0])
        else:
            rnd = _run_round(a, ups, sub, add)
            assert rnd.out_of_range() == want_bad >= 4096 // 2


def test_a_round_is_finished_only_after_exactly_one_unmask(gpu_device):
    c = _case()
    a = _adapter()
    rnd = a.begin_round(len(ARRIVED), "fedavg")
    for up in c["plain"]:
        rnd.add(up)
    with pytest.raises(RuntimeError, match="unmask"):
        a.apply_round(rnd, float(np.float32(5)), 5.0)
    with pytest.raises(RuntimeError, match="before the round was finished"):
        rnd.out_of_range()
    rnd.unmask([], [])
    with pytest.raises(RuntimeError, match="already called"):
        rnd.unmask([], [])
    with pytest.raises(TypeError, match=r"conv\.weight.*float32"):  # a float32 upload names the entry
        a.begin_round(2, "fedavg").add(c["states"][0])
    with pytest.raises(ValueError, match="K=2049"):
        a.begin_round(2049, "fedavg")


def test_the_mixin_drives_the_round_through_its_hook(gpu_device):
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.secagg_round import SecAggRound

    c = _case()
    names, init, graph = c["names"], c["init"], c["graph"]

    class Base:
        def init_model(self):
            self.model_wrapper = StateDictModule(names, init)
            self.model_wrapper.get_model = lambda m=self.model_wrapper: m

    class NoHook(DeviceAggregator, Base):
        device_upload_secagg = c["spec"]
        device_round_capacity = 3
        device = DEV

        def __init__(self):
            DeviceAggregator.__init__(self, None, _args())
            self.init_model()

    class Agg(NoHook):
        def device_secagg_unmask(self, client_ids):
            self.asked = list(client_ids)
            sub, add = graph.unmask_keys(client_ids)
            return sub, add, NONCE

    agg = Agg()
    adapter = agg.model_wrapper
    assert type(adapter) is TorchModelAdapter and adapter.upload_secagg == c["spec"]
    agg.start_round(len(ARRIVED))
    for up, u in zip(c["masked"], ARRIVED):
        agg.on_result({"client_id": u, "update_weight": up, "moving_loss": 0.5})
        assert agg._device_round is None or type(agg._device_round) is SecAggRound
    assert agg.asked == ARRIVED and agg._device_round is None
    got = adapter.get_weights()
    assert np.array_equal(_flat([t.numpy() for t in got]).view(np.uint32), c["want"].view(np.uint32))
    assert len(agg.model_weights) == len(got)  # the round's mean, as the reference keeps it
    # without the hook the round cannot close, and the model stays what it was
    bare = NoHook()
    before = [t.clone() for t in bare.model_wrapper.get_weights()]
    bare.start_round(len(ARRIVED))
    for up, u in zip(c["masked"][:-1], ARRIVED):
        bare.on_result({"client_id": u, "update_weight": up, "moving_loss": 0.5})
    with pytest.raises(NotImplementedError, match="device_secagg_unmask"):
        bare.on_result({"client_id": ARRIVED[-1], "update_weight": c["masked"][-1], "moving_loss": 0.5})
    assert all(torch.equal(x, y) for x, y in zip(bare.model_wrapper.get_weights(), before))
