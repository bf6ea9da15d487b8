"""CPU checks of the secure-aggregation path: the ChaCha20 word stream against its known answers, the encoder and the
finish on crafted values, exact cancellation over a mask graph with dropouts, SecAggSpec and the K * B bound, every
refused combination, the wire format's errors, the executor's host path against the restatement
(tests/secagg_fixtures.py), and pickling."""
import pickle
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from fedscale_amd.bucket import BucketLayout
from fedscale_amd.cloud.execution import secagg_upload as su
from fedscale_amd.cloud.execution.secagg_upload import compress_secagg, encode_update
from fedscale_amd.kernels_secagg import check_nonce, keys_array
from fedscale_amd.secagg_round import SecAggRound, SecAggSpec, SecAggUnmaskError, refuse, upload_plan_secagg
from fedscale_amd.state import ShardGroup
from tests import secagg_fixtures as sf


# ---- the mask stream ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kat", sf.KATS, ids=["rfc8439-2.3.2", "zero-key", "counter-crosses-2^31"])
def test_known_answers(kat):
    """Vectors 1 and 2 are published (RFC 8439); vector 3 comes only from the numpy restatement that reproduces them —
    no crypto library was at hand to cross-check it."""
    want = sf.kat_words(kat)
    for impl in (sf.stream, su.keystream):
        got = impl(kat["key"], kat["nonce"], kat["col0"], kat["P"])[kat["lo"]:]
        assert got.dtype == np.uint32 and np.array_equal(got, want), impl.__module__


def test_stream_slices_at_any_col0_equal_slices_of_one_long_stream():
    rng = np.random.default_rng(1)
    key, nonce = sf.make_keys(rng, 1)[0], (7, 8, 9)
    whole = sf.stream(key, nonce, 0, 4096 + 77)
    for col0, P in ((0, 1), (16, 15), (16, 16), (32, 17), (1024, 1025), (4080, 93), (4096, 77), (48, 0)):
        for impl in (sf.stream, su.keystream):
            assert np.array_equal(impl(key, nonce, col0, P), whole[col0:col0 + P]), (col0, P)
    for bad in (8, 17, -16):
        with pytest.raises(ValueError, match="multiple of 16"):
            su.keystream(key, nonce, bad, 4)
    with pytest.raises(ValueError, match="2\\^36"):
        su.keystream(key, nonce, (1 << 36) - 16, 17)
    assert su.keystream(key, nonce, (1 << 36) - 16, 16).shape == (16,)  # the last block of a stream


def test_keys_and_nonces_are_validated():
    k = keys_array([bytes(range(32)), sf.RFC_KEY])
    assert k.dtype == np.uint32 and k.shape == (2, 8) and np.array_equal(k[0], k[1])  # little-endian words
    assert keys_array([]).shape == (0, 8)
    with pytest.raises(ValueError, match="key 1"):
        keys_array([sf.RFC_KEY, (1, 2, 3)])
    with pytest.raises(ValueError, match="key 0"):
        keys_array([bytes(31)])
    with pytest.raises(ValueError, match="key 0"):
        keys_array([(1 << 32,) + (0,) * 7])
    assert check_nonce([1, 2, 0xFFFFFFFF]) == (1, 2, 0xFFFFFFFF)
    for bad in ((1, 2), (1, 2, 1 << 32), (-1, 0, 0), 5):
        with pytest.raises(ValueError, match="nonce"):
            check_nonce(bad)


# ---- encode and finish on crafted values ----------------------------------------------------------------------------
def test_encode_on_crafted_values():
    x, base, q, n_clamped, n_nan = sf.crafted_encode_case()
    got, cl, nn = sf.encode(x, base, 16, 20)
    assert np.array_equal(got.view(np.int32), q) and (cl, nn) == (n_clamped, n_nan)
    with np.errstate(invalid="ignore"):
        words, stats = su.encode_host(x - base, SecAggSpec())
    assert np.array_equal(words.view(np.int32), q) and stats == (n_clamped, n_nan)
    # other specs: f = 0 rounds to integers, b = 1 keeps {-1, 0, 1}
    got, cl, nn = sf.encode(np.float32([0.5, 1.5, 2.5, -7.0, 0.4]), np.zeros(5, np.float32), 0, 1)
    assert got.view(np.int32).tolist() == [0, 1, 1, -1, 0] and (cl, nn) == (3, 0)  # 2, 2 and -7 are clamped
    w, st = su.encode_host(np.float32([0.5, 1.5, 2.5, -7.0, 0.4]), SecAggSpec(0, 1))
    assert w.view(np.int32).tolist() == [0, 1, 1, -1, 0] and st == (3, 0)


@pytest.mark.parametrize("n", [3, 7])
def test_finish_on_crafted_sums(n):
    total, bad = sf.crafted_finish_case(n)
    last = np.linspace(-1, 1, total.size).astype(np.float32)
    out, count = sf.finish(total, last, 16, 20, n)
    assert count == bad == 4  # INT32_MIN, nB + 1, -nB - 1, INT32_MAX
    s = total.view(np.int32).astype(np.int64)
    assert s[0] == -(1 << 31)
    # the division rounds once, in float64, and the cast to fp32 once more
    for i in (1, 8, 9, 10, 11, 12, 13, 14):
        from fractions import Fraction

        exact = Fraction(int(s[i]), n << 16)
        m64 = np.float64(int(s[i]) * 2.0 ** -16) / np.float64(n)
        assert abs(Fraction(float(m64)) - exact) <= abs(exact) * Fraction(1, 1 << 52)
        assert out[i] == np.float32(last[i] + np.float32(m64))
    assert out[2] == last[2]  # s = 0


# ---- cancellation ---------------------------------------------------------------------------------------------------
def test_masks_cancel_exactly_over_a_ring_graph_with_dropouts():
    rng = np.random.default_rng(2)
    K, P, nonce = 7, 37, (11, 0, 3)
    graph = sf.RingGraph(rng, K, reach=2)
    assert len(graph.pairs) == 14 and all(sum(1 for p in graph.pairs if u in p) == 4 for u in range(K))  # 4-regular
    arrived = [6, 0, 1, 3, 4]  # clients 2 and 5 dropped
    last = rng.normal(0, 1, P).astype(np.float32)
    xs = [last + rng.normal(0, 0.05, P).astype(np.float32) for _ in arrived]
    qs = [sf.encode(x, last, 16, 20)[0] for x in xs]
    rows = [sf.masked_upload(q, graph, u, nonce) for q, u in zip(qs, arrived)]
    total = sf.reduce(rows)
    # before unmasking, every column is out of range
    assert sf.finish(total, last, 16, 20, len(arrived))[1] == P
    sub, add = graph.unmask_keys(arrived)
    assert len(sub) + len(add) == 5 + 8  # five self masks; each of the two dropped clients had four neighbours
    unmasked = sf.mask_sum(total, add, sub, nonce)
    plain = sf.reduce(qs)
    assert np.array_equal(unmasked, plain)
    assert np.array_equal(unmasked.view(np.int32).astype(np.int64),
                          sum(q.view(np.int32).astype(np.int64) for q in qs))  # no wrap: the integer sum itself
    out, bad, tot, clamped = sf.round_model(xs, last, 16, 20, graph, arrived, nonce)
    out0, bad0, tot0, _ = sf.round_model(xs, last, 16, 20)
    assert bad == bad0 == 0 and clamped == 0 and np.array_equal(tot, tot0) and np.array_equal(out, out0)
    # one pairwise key left out: nearly every column leaves the range
    _, bad1, _, _ = sf.round_model(xs, last, 16, 20, graph, arrived, nonce, skip_pair=(1, 2))
    assert bad1 >= P // 2


# ---- the executor's host path ---------------------------------------------------------------------------------------
def _state():
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                              torch.nn.Linear(4 * 26 * 26, 3))
    base = OrderedDict((k, v.clone()) for k, v in net.state_dict().items())
    sd = OrderedDict((k, v + 0.01 * torch.randn_like(v) if v.dtype == torch.float32 else v + 5)
                     for k, v in base.items())
    return sd, base


def _flat(d, lay):
    return np.concatenate([np.asarray(d[e.name]).reshape(-1) for e in lay.f_entries])


def test_compress_secagg_host_path_equals_the_restatement():
    sd, base = _state()
    lay = BucketLayout.from_state_dict(sd)
    rng = np.random.default_rng(4)
    keys = sf.make_keys(rng, 4)
    spec, nonce = SecAggSpec(14, 18), (3, 1, 4)
    x = _flat({k: v.numpy() for k, v in sd.items()}, lay)
    L = _flat({k: v.numpy() for k, v in base.items()}, lay)
    q, cl, nn = sf.encode(x, L, 14, 18)
    enc, stats = encode_update(sd, base, spec)
    assert stats == (cl, nn) == (0, 0) and np.array_equal(_flat(enc, lay), q)
    up, stats = compress_secagg(sd, list(base.values()), spec, self_key=keys[0], add_keys=[keys[1], bytes(32)],
                                sub_keys=[keys[2]], nonce=nonce, return_stats=True)
    want = sf.mask_sum(q, [keys[0], keys[1], (0,) * 8], [keys[2]], nonce)
    assert stats == (0, 0) and list(up) == list(sd)
    assert np.array_equal(_flat(up, lay), want)
    for e in lay.entries:
        v = up[e.name]
        assert v.shape == e.shape and v.dtype == (np.uint32 if e.kind == "f" else np.int64)
    assert int(up["1.num_batches_tracked"]) == int(sd["1.num_batches_tracked"])  # int64 entries travel unmasked
    # no self key, no pairs: the plain encoding
    none = compress_secagg(sd, base, spec, self_key=None, add_keys=[], sub_keys=[])
    assert np.array_equal(_flat(none, lay), q)
    # a NaN and an overflow are reported
    sd2 = OrderedDict(sd)
    w = sd["3.bias"].clone()
    w[0], w[1] = float("nan"), 1e30
    sd2["3.bias"] = w
    _, stats = encode_update(sd2, base, spec)
    assert stats == (1, 1)
    # the upload pickles, and what comes back is what the staging takes
    back = pickle.loads(pickle.dumps(up))
    plan = upload_plan_secagg(lay, back)
    assert len(plan) == lay.T and all(type(v) is np.ndarray for _, v in plan)
    with pytest.raises(ValueError, match="base shape"):
        compress_secagg(sd, {**base, "3.bias": base["3.bias"][:2]}, spec, self_key=None, add_keys=[], sub_keys=[])
    with pytest.raises(TypeError, match="SecAggSpec"):
        compress_secagg(sd, base, (16, 20), self_key=None, add_keys=[], sub_keys=[])


def test_wire_format_errors_name_the_entry():
    sd, base = _state()
    lay = BucketLayout.from_state_dict(sd)
    good, _ = encode_update(sd, base, SecAggSpec())
    plan = upload_plan_secagg(lay, list(good.values()))  # a list in layout order
    assert len(plan) == lay.T
    tens = {k: torch.from_numpy(np.asarray(v).view(np.int32) if v.dtype == np.uint32 else np.asarray(v))
            for k, v in good.items()}
    plan = upload_plan_secagg(lay, tens)  # CPU int32 tensors of the same bits become uint32 arrays
    assert all(type(v) is np.ndarray for _, v in plan) and plan[0][1].dtype == np.uint32
    assert np.array_equal(plan[0][1], good["0.weight"])
    with pytest.raises(TypeError, match=r"0\.weight.*float32"):
        upload_plan_secagg(lay, {k: v.numpy() for k, v in sd.items()})
    with pytest.raises(TypeError, match=r"0\.weight.*torch\.float32"):
        upload_plan_secagg(lay, dict(sd))
    bad = dict(good)
    bad["0.weight"] = good["0.weight"].view(np.int32)
    with pytest.raises(TypeError, match=r"0\.weight.*int32"):
        upload_plan_secagg(lay, bad)
    bad = dict(good)
    bad["3.bias"] = good["3.bias"][:2]
    with pytest.raises(TypeError, match=r"3\.bias.*shape"):
        upload_plan_secagg(lay, bad)
    bad = dict(good)
    bad["1.num_batches_tracked"] = np.asarray(7, dtype=np.int32)
    with pytest.raises(TypeError, match=r"1\.num_batches_tracked.*int32"):
        upload_plan_secagg(lay, bad)
    with pytest.raises(ValueError, match="tensors"):
        upload_plan_secagg(lay, list(good.values())[:-1])


# ---- the spec, the bound and the refusals ---------------------------------------------------------------------------
def _adapter_stub(**attrs):
    """What ``TorchModelAdapter.begin_round`` reads of an adapter before it touches a device: no device at all."""
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    stub = types.SimpleNamespace(**attrs)
    stub._begin_secagg_round = types.MethodType(TorchModelAdapter._begin_secagg_round, stub)
    return stub


def test_spec_validation():
    s = SecAggSpec()
    assert (s.frac_bits, s.mag_bits, s.verify, s.bound) == (16, 20, True, (1 << 20) - 1)
    assert s == SecAggSpec(16, 20) and hash(s) == hash(SecAggSpec(16, 20)) and s != SecAggSpec(16, 20, verify=False)
    assert SecAggSpec(s) == s and SecAggSpec.of(True) == s and SecAggSpec.of(s) is s
    assert pickle.loads(pickle.dumps(SecAggSpec(3, 9, False))) == SecAggSpec(3, 9, False)
    assert "frac_bits=16" in repr(s)
    with pytest.raises(AttributeError, match="immutable"):
        s.frac_bits = 3
    for kw in ({"frac_bits": -1}, {"frac_bits": 31}, {"frac_bits": 1.5}, {"frac_bits": True}, {"mag_bits": 0},
               {"mag_bits": 31}, {"mag_bits": "20"}, {"verify": 1}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            SecAggSpec(**kw)
    assert SecAggSpec(0, 1).bound == 1 and SecAggSpec(30, 30).bound == (1 << 30) - 1
    for bad in (False, 16, "yes", None):
        with pytest.raises(TypeError, match="SecAggSpec"):
            SecAggSpec.of(bad)


def test_the_round_size_bound():
    s = SecAggSpec()
    assert s.max_clients() == 2048 and s.check_clients(2048) == 2048
    with pytest.raises(ValueError, match="K=2049.*K <= 2048"):
        s.check_clients(2049)
    assert SecAggSpec(16, 30).max_clients() == 2 and SecAggSpec(16, 1).max_clients() == (1 << 31) - 1
    with pytest.raises(ValueError, match="K >= 1"):
        s.check_clients(0)
    # begin_round refuses it before a device is touched (the stub has none)
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    one = types.SimpleNamespace(world=1)
    stub = _adapter_stub(upload_secagg=s, shards=one, layout=one)
    with pytest.raises(ValueError, match="K=2049"):
        TorchModelAdapter._begin_secagg_round(stub, 2049, "fedavg", None, False, None, None, None, None)
    with pytest.raises(ValueError, match="K=2049"):
        TorchModelAdapter.begin_round(stub, 2049, "fedavg")
    with pytest.raises(ValueError, match="K=3"):
        SecAggRound(None, "cpu", 3, "fedavg", SecAggSpec(16, 30), staging=None, last_f32=None)


def test_refused_combinations_at_the_adapter_say_why():
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    net, spec = torch.nn.Linear(4, 2), SecAggSpec()
    why = "individual uploads"
    with pytest.raises(NotImplementedError, match="upload_secagg.*ShardedModelAdapter.*" + why):
        ShardedModelAdapter(net, devices=[0, 1], upload_secagg=spec)
    for mode in ("params", "clients"):
        with pytest.raises(NotImplementedError, match="upload_secagg.*shard.*" + why):
            TorchModelAdapter(net, shards=ShardGroup(0, 2, None, mode), upload_secagg=spec)
    with pytest.raises(NotImplementedError, match="upload_secagg.*q-fedavg.*" + why):
        TorchModelAdapter(net, optimizer=types.SimpleNamespace(mode="q-fedavg"), upload_secagg=spec)
    with pytest.raises(NotImplementedError, match="upload_secagg.*upload_dtype='bfloat16'"):
        TorchModelAdapter(net, upload_dtype="bfloat16", upload_secagg=spec)
    with pytest.raises(NotImplementedError, match="upload_secagg.*upload_quant='mxfp8'"):
        TorchModelAdapter(net, upload_quant="mxfp8", upload_secagg=spec)
    with pytest.raises(NotImplementedError, match="upload_secagg.*upload_topk=0.1"):
        TorchModelAdapter(net, upload_topk=0.1, upload_secagg=spec)
    with pytest.raises(TypeError, match="SecAggSpec"):
        TorchModelAdapter(net, upload_secagg=16)
    # begin_round of an adapter with upload_secagg (no device is reached before the refusal)
    stub = _adapter_stub(upload_secagg=spec)
    begin = TorchModelAdapter.begin_round
    for kw, what in (({"signatures": True}, "cohort signatures"), ({"clip": object()}, "clip"), ({"trim": 1}, "trim"),
                     ({"krum": 1}, "krum"), ({"geomed": True}, "geomed")):
        with pytest.raises(NotImplementedError, match="upload_secagg.*" + what + ".*" + why):
            begin(stub, 4, "fedavg", **kw)
    for policy in ("fedbuff", "qfedavg"):
        with pytest.raises(NotImplementedError, match="upload_secagg.*" + policy + ".*" + why):
            begin(stub, 4, policy)
    two = types.SimpleNamespace(world=2)
    for shards, layout in ((two, types.SimpleNamespace(world=1)), (types.SimpleNamespace(world=1), two)):
        with pytest.raises(NotImplementedError, match="upload_secagg.*shard"):
            begin(_adapter_stub(upload_secagg=spec, shards=shards, layout=layout), 4, "fedavg")
    with pytest.raises(NotImplementedError, match="upload_secagg.*fedbuff"):
        SecAggRound(None, "cpu", 4, "fedbuff", spec, staging=None, last_f32=None)
    assert isinstance(refuse("x"), NotImplementedError)
    assert issubclass(SecAggUnmaskError, RuntimeError)
    e = SecAggUnmaskError(4000, 4096, 5, spec)
    assert e.count == 4000 and "4000 of 4096" in str(e) and "not applied" in str(e)


def test_refused_combinations_at_the_mixin_say_why():
    from fedscale_amd.cloud.aggregation import aggregator as agg

    assert agg.DeviceAggregatorMixin.device_upload_secagg is None
    assert agg.DeviceAsyncAggregatorMixin.device_upload_secagg is None  # inherited
    spec = SecAggSpec()
    for attr, value, what in (("device_clip_norm", 1.0, "device_clip_norm"), ("device_trim", 1, "device_trim"),
                              ("device_krum", 1, "device_krum"), ("device_geomed", True, "device_geomed"),
                              ("device_upload_dtype", "float16", "device_upload_dtype='float16'"),
                              ("device_upload_quant", "mxfp8", "device_upload_quant='mxfp8'"),
                              ("device_upload_topk", 0.1, "device_upload_topk=0.1"),
                              ("device_shards", [0, 1], "device_shards")):
        A = type("A", (agg.DeviceAggregatorMixin,), {"device_upload_secagg": spec, attr: value})
        with pytest.raises(NotImplementedError, match="upload_secagg.*" + what + ".*individual uploads"):
            A()._secagg_spec()
    ok = type("A", (agg.DeviceAggregatorMixin,), {"device_upload_secagg": True})
    assert ok()._secagg_spec() == spec and agg.DeviceAggregatorMixin()._secagg_spec() is None
    with pytest.raises(TypeError, match="SecAggSpec"):
        type("A", (agg.DeviceAggregatorMixin,), {"device_upload_secagg": 16})()._secagg_spec()

    class Base:
        def init_model(self):
            self.model_wrapper = types.SimpleNamespace(get_model=lambda: torch.nn.Linear(4, 2))

    class S(agg.DeviceAggregatorMixin, Base):
        device_upload_secagg = spec
        device_shards = [0, 1]
        args = types.SimpleNamespace(gradient_policy=None)

    with pytest.raises(NotImplementedError, match="upload_secagg.*device_shards"):
        S().init_model()

    class B(agg.DeviceAsyncAggregatorMixin):
        device_upload_secagg = spec

    with pytest.raises(NotImplementedError, match="upload_secagg.*DeviceAsyncAggregatorMixin"):
        B().update_weight_aggregation({"client_id": 0, "update_weight": {}})

    class C(agg.DeviceCohortAggregatorMixin):
        device_upload_secagg = spec

    with pytest.raises(NotImplementedError, match="upload_secagg.*DeviceCohortAggregatorMixin"):
        C().update_weight_aggregation({"client_id": 0, "update_weight": {}})
    # the hook's default names itself
    with pytest.raises(NotImplementedError, match="device_secagg_unmask"):
        agg.DeviceAggregatorMixin().device_secagg_unmask([0, 1])


def test_pickling_an_adapter_carries_the_option():
    from fedscale_amd.cloud.internal import torch_model_adapter as tma

    net, spec = torch.nn.Linear(4, 2), SecAggSpec(12, 18, verify=False)
    stub = types.SimpleNamespace(upload_secagg=spec, upload_topk=None, upload_quant=None, upload_dtype=None,
                                 optimizer=None, get_model=lambda: net)
    fn, args = tma.TorchModelAdapter.__reduce__(stub)
    assert fn is tma._rebuild_with_upload_secagg and args[1] is net and args[3] == spec
    fn2, args2 = pickle.loads(pickle.dumps((fn, (args[0], None, None, args[3]))))  # the rebuild and the spec pickle
    assert fn2 is fn and args2[3] == spec
    import inspect

    params = inspect.signature(tma.TorchModelAdapter.__init__).parameters
    assert "upload_secagg" not in params  # keyword-only through the wrapper; the positional layout is what it was
    assert list(params)[-1] == "upload_quant"
