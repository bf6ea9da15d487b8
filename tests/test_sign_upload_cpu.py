"""The executor side of the 1-bit sign path without a GPU: compress_sign's host path against the restatement of the
contract (tests/sign_fixtures.py) byte for byte, planted values, the wire format through pickle and ingress, the
validation of uploads, the refused combinations, the mixins' pass-through and the adapter's pickling."""
import pickle
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from fedscale_amd import ingress
from fedscale_amd.bucket import BucketLayout
from fedscale_amd.cloud.execution.sign_upload import BITS_KEY, SCALES_KEY, compress_sign
from fedscale_amd.sign_round import FORMATS, SignRound, check_format, upload_plan_sign
from fedscale_amd.state import ShardGroup
from tests import sign_fixtures as sg

F32 = np.float32


def _u32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _one_entry(e):
    """A one-entry state whose update against a +0 base is ``e`` exactly."""
    e = np.ascontiguousarray(e, dtype=F32)
    return {"w": e}, {"w": np.zeros_like(e)}


def _check(e, residual=None):
    """compress_sign's host path on the update ``e`` (+ residual) against the restatement, byte for byte."""
    up, r = compress_sign(*_one_entry(e), residual=residual, residual_out=True)
    bits, scales, res = sg.encode(sg.delta(e, np.zeros_like(e), residual))
    assert list(up) == [BITS_KEY, SCALES_KEY]
    assert up[BITS_KEY].dtype == np.uint8 and up[BITS_KEY].shape == (sg.bit_bytes(e.size),)
    assert up[SCALES_KEY].dtype == F32 and up[SCALES_KEY].shape == (sg.blocks(e.size),)
    assert np.array_equal(up[BITS_KEY], bits)
    assert np.array_equal(_u32(up[SCALES_KEY]), _u32(scales))
    assert r.dtype == F32 and np.array_equal(_u32(r), _u32(res))
    return up, r


def test_host_path_equals_the_restatement_on_the_contracts_cases():
    for name, e in sg.contract_cases().items():
        _check(e)
        fb, fs, fr = sg.encode_fast(e)  # the array form of the restatement the GPU tests use at large sizes
        b, s, r = sg.encode(e)
        assert np.array_equal(fb, b) and np.array_equal(_u32(fs), _u32(s)) and np.array_equal(_u32(fr), _u32(r)), name


def test_the_fixed_add_order_decides_the_scale():
    """A block whose fp64 sum depends on the order: 2^53 in lane 0 of quarter 0 and ones elsewhere.  In the
    contract's order each lane first adds its four quarters (1 + 1 + 1 + 1, exact), and the butterfly then meets
    2^53 last; the restatement and the host path agree on the bits, and a plain left-to-right sum does not give
    the same fp64 value."""
    e = np.ones(256, dtype=F32)
    e[0] = F32(2.0 ** 53)
    up, _ = _check(e)
    t = [((abs(float(e[l])) + 1.0) + 1.0) + 1.0 for l in range(64)]
    for m in (32, 16, 8, 4, 2, 1):
        t = [t[l] + t[l ^ m] for l in range(64)]
    assert up[SCALES_KEY][0] == F32(t[0] / 256.0)
    seq = 0.0
    for v in e:
        seq += float(v)
    assert seq == 2.0 ** 53 and t[0] == 2.0 ** 53 + 252  # 2^53 + 1 + 1 + ... loses every one; the order keeps 252


def test_planted_values_land_where_the_contract_says():
    rng = np.random.default_rng(5)
    # -0.0 counts as negative: its bit is set, and with a scale s its residual is -0 - (-s) = +s
    e = rng.standard_normal(300).astype(F32)
    e[13] = -0.0
    up, r = _check(e)
    assert (up[BITS_KEY][13 // 8] >> (13 % 8)) & 1 == 1
    assert r[13] == up[SCALES_KEY][0] and up[SCALES_KEY][0] > 0
    # a block of zeros: scale +0.0 (bits 0), residual e - (+-0) = e
    e = rng.standard_normal(3 * 256).astype(F32)
    e[256:512] = 0.0
    up, r = _check(e)
    assert _u32(up[SCALES_KEY])[1] == 0 and not up[BITS_KEY][32:64].any() and not r[256:512].any()
    # a NaN block and an inf block: scale bits 0x7FC00000, zero bits, +0.0 residual; the neighbours are untouched
    for bad in (np.nan, np.inf, -np.inf):
        e = -np.abs(rng.standard_normal(3 * 256)).astype(F32)  # every bit set, so zero bits are the rule's doing
        e[256 + 77] = bad
        up, r = _check(e)
        assert _u32(up[SCALES_KEY])[1] == 0x7FC00000
        assert not up[BITS_KEY][32:64].any() and (up[BITS_KEY][:32] == 0xFF).all() and (up[BITS_KEY][64:] == 0xFF).all()
        assert (_u32(r[256:512]) == 0).all() and np.isfinite(up[SCALES_KEY][[0, 2]]).all()
    # a partial last block with n_b = 1 and n_b = 255: the mean divides by n_b, the padding bits are 0
    for n_b in (1, 255):
        e = np.full(256 + n_b, -3.0, dtype=F32)
        up, r = _check(e)
        assert up[SCALES_KEY][1] == F32(3.0) and up[SCALES_KEY][0] == F32(3.0)
        last = up[BITS_KEY][-1]
        assert last == (1 << ((256 + n_b) % 8 or 8)) - 1 and not r.any()
    for P in (1, 7, 8, 9, 255, 256, 257):
        e = (rng.standard_normal(P) * 7).astype(F32)
        up, _ = _check(e)
        if P % 8:
            assert up[BITS_KEY][-1] >> (P % 8) == 0  # padding bits of the last byte


def test_two_rounds_with_the_residual_fed_back_equal_the_restatement():
    rng = np.random.default_rng(9)
    P = 700
    L = rng.standard_normal(P).astype(F32)
    x1 = (L + rng.standard_normal(P).astype(F32) * F32(0.01)).astype(F32)
    x2 = (L + rng.standard_normal(P).astype(F32) * F32(0.02)).astype(F32)
    up1, r1 = compress_sign({"w": x1}, {"w": L}, residual_out=True)
    up2, r2 = compress_sign({"w": x2}, [L], residual=r1)  # residual_out defaults to true with a residual
    b1, s1, w1 = sg.encode(sg.delta(x1, L))
    b2, s2, w2 = sg.encode(sg.delta(x2, L, w1))
    assert np.array_equal(up1[BITS_KEY], b1) and np.array_equal(_u32(up1[SCALES_KEY]), _u32(s1))
    assert np.array_equal(_u32(r1), _u32(w1))
    assert np.array_equal(up2[BITS_KEY], b2) and np.array_equal(_u32(up2[SCALES_KEY]), _u32(s2))
    assert np.array_equal(_u32(r2), _u32(w2))
    # what the encoding leaves behind is what it did not send: deq + residual_out = e to fp32 rounding, exactly here
    # where e - deq is exact (Sterbenz does not apply in general, so only the definition is asserted)
    e2 = sg.delta(x2, L, w1)
    assert np.array_equal(_u32(w2), _u32((e2 - sg.dequantize(b2, s2, P)).astype(F32)))
    assert compress_sign({"w": x1}, {"w": L})[1] is None
    with pytest.raises(ValueError, match="residual: expected a flat float32 vector of 700"):
        compress_sign({"w": x1}, {"w": L}, residual=r1[:-1])
    with pytest.raises(ValueError, match="residual: expected a flat float32 vector of 700"):
        compress_sign({"w": x1}, {"w": L}, residual=r1.astype(np.float64))


def _state():
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                              torch.nn.Linear(4 * 26 * 26, 40))
    base = OrderedDict((k, v.clone()) for k, v in net.state_dict().items())
    sd = OrderedDict((k, v + 0.01 * torch.randn_like(v) if v.dtype == torch.float32 else v + 5)
                     for k, v in base.items())
    return sd, base


def test_blocks_run_across_entry_boundaries_and_int64_entries_pass_through():
    sd, base = _state()
    lay = BucketLayout.from_state_dict(sd)
    sizes = [v.numel() for v in sd.values() if v.dtype == torch.float32]
    assert any(s % 256 for s in np.cumsum(sizes)[:-1])  # an entry boundary inside a block
    e = np.concatenate([(sd[n] - base[n]).numpy().reshape(-1) for n in sd if sd[n].dtype == torch.float32])
    bits, scales, _ = sg.encode_fast(e)
    for b in (list(base.values()), base):
        up, r = compress_sign(sd, b)
        assert r is None and type(up) is dict
        assert list(up) == ["1.num_batches_tracked", BITS_KEY, SCALES_KEY]  # no float32 entry appears
        assert up["1.num_batches_tracked"].dtype == np.int64 and int(up["1.num_batches_tracked"]) == 5
        assert up[BITS_KEY].shape == (sg.bit_bytes(lay.P),) and up[SCALES_KEY].shape == (sg.blocks(lay.P),)
        assert np.array_equal(up[BITS_KEY], bits) and np.array_equal(_u32(up[SCALES_KEY]), _u32(scales))
    side, b, s = upload_plan_sign(lay, up)
    assert [e.name for e, _ in side] == ["1.num_batches_tracked"] and b is up[BITS_KEY] and s is up[SCALES_KEY]
    side, b, s = upload_plan_sign(lay, list(up.values()))  # a list: side entries, then bits, then scales
    assert len(side) == 1 and b is up[BITS_KEY] and s is up[SCALES_KEY]
    tens = {n: torch.from_numpy(np.array(v)) for n, v in up.items()}
    side, b, s = upload_plan_sign(lay, tens)  # CPU tensors become arrays
    assert type(b) is np.ndarray and np.array_equal(b, up[BITS_KEY]) and np.array_equal(_u32(s), _u32(up[SCALES_KEY]))
    with pytest.raises(ValueError, match="base has 2 entries"):
        compress_sign(sd, list(base.values())[:2])
    for key in (BITS_KEY, SCALES_KEY):
        with pytest.raises(ValueError, match=f"entry named '{key}'"):
            compress_sign({**sd, key: torch.zeros(3)}, {**base, key: torch.zeros(3)})


def test_a_pickled_upload_through_ingress_stages_the_same_arrays():
    sd, base = _state()
    lay = BucketLayout.from_state_dict(sd)
    up, _ = compress_sign(sd, base)
    payload = pickle.dumps({"client_id": 3, "update_weight": up, "moving_loss": 0.5})
    assert len(payload) < lay.P * 9 // 64 + 1024  # 9/64 byte per parameter on the wire
    got = ingress.loads(payload)
    assert got["client_id"] == 3 and got["moving_loss"] == 0.5
    back = got["update_weight"]
    assert list(back) == list(up)
    for n in up:
        assert back[n].dtype == up[n].dtype and back[n].shape == up[n].shape and np.array_equal(back[n], up[n]), n
    side, b, s = upload_plan_sign(lay, back)
    assert np.array_equal(b, up[BITS_KEY]) and b.dtype == np.uint8 and b.flags.c_contiguous
    assert np.array_equal(_u32(s), _u32(up[SCALES_KEY])) and int(side[0][1]) == 5
    plain = pickle.loads(payload)["update_weight"]
    for n in up:
        assert np.array_equal(plain[n], up[n]), n


def test_validation_names_the_entry_that_does_not_fit():
    sd, base = _state()
    lay = BucketLayout.from_state_dict(sd)
    good, _ = compress_sign(sd, base)
    upload_plan_sign(lay, good)

    def bad(**kw):
        u = dict(good)
        u.update(kw)
        return u

    def without(key):
        return {k: v for k, v in good.items() if k != key}

    with pytest.raises(TypeError, match=r"0\.weight.*float32.*sign bits"):  # whole weights: a float32 array
        upload_plan_sign(lay, {n: v.numpy() for n, v in sd.items()})
    with pytest.raises(TypeError, match=r"0\.weight.*float32"):  # float32 entries beside the bits
        upload_plan_sign(lay, {**{n: v.numpy() for n, v in sd.items()}, **good})
    with pytest.raises(TypeError, match=BITS_KEY + ".*carries no such array"):
        upload_plan_sign(lay, without(BITS_KEY))
    with pytest.raises(TypeError, match=SCALES_KEY + ".*carries no such array"):
        upload_plan_sign(lay, without(SCALES_KEY))
    with pytest.raises(TypeError, match=BITS_KEY + ".*float32.*uint8"):
        upload_plan_sign(lay, bad(**{BITS_KEY: good[BITS_KEY].astype(np.float32)}))
    with pytest.raises(TypeError, match=SCALES_KEY + ".*float64.*float32"):
        upload_plan_sign(lay, bad(**{SCALES_KEY: good[SCALES_KEY].astype(np.float64)}))
    with pytest.raises(TypeError, match=BITS_KEY + ".*shape"):
        upload_plan_sign(lay, bad(**{BITS_KEY: good[BITS_KEY][:-1]}))
    with pytest.raises(TypeError, match=SCALES_KEY + ".*shape"):
        upload_plan_sign(lay, bad(**{SCALES_KEY: np.concatenate([good[SCALES_KEY], good[SCALES_KEY][:1]])}))
    with pytest.raises(TypeError, match=r"1\.num_batches_tracked.*int32"):
        upload_plan_sign(lay, bad(**{"1.num_batches_tracked": np.asarray(7, dtype=np.int32)}))
    with pytest.raises(ValueError, match="non-float32 entries"):
        upload_plan_sign(lay, without("1.num_batches_tracked"))
    with pytest.raises(ValueError, match="arrays"):
        upload_plan_sign(lay, list(good.values())[1:])
    with pytest.raises(TypeError, match=SCALES_KEY + ".*torch.float64"):
        upload_plan_sign(lay, bad(**{SCALES_KEY: torch.from_numpy(good[SCALES_KEY].astype(np.float64))}))


def test_refused_combinations_name_the_combination():
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    assert FORMATS == ("sign1",) and check_format("sign1") == "sign1"
    net = torch.nn.Linear(4, 2)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*ShardedModelAdapter"):
        ShardedModelAdapter(net, devices=[0, 1], upload_sign="sign1")
    for mode in ("params", "clients"):
        with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*shard"):
            TorchModelAdapter(net, shards=ShardGroup(0, 2, None, mode), upload_sign="sign1")
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*q-fedavg"):
        TorchModelAdapter(net, optimizer=types.SimpleNamespace(mode="q-fedavg"), upload_sign="sign1")
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*upload_dtype='bfloat16'"):
        TorchModelAdapter(net, upload_dtype="bfloat16", upload_sign="sign1")
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*upload_quant='mxfp8'"):
        TorchModelAdapter(net, upload_quant="mxfp8", upload_sign="sign1")
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*upload_topk=0\.01"):
        TorchModelAdapter(net, upload_topk=0.01, upload_sign="sign1")
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*upload_secagg"):
        TorchModelAdapter(net, upload_secagg=True, upload_sign="sign1")
    for bad in ("sign", "mxfp8", 1, True):
        with pytest.raises(ValueError, match="upload_sign"):
            TorchModelAdapter(net, upload_sign=bad)
    # begin_round of an adapter with upload_sign (no device is reached before the refusal)
    stub = types.SimpleNamespace(upload_sign="sign1")
    begin = TorchModelAdapter._begin_sign_round  # (K, policy, capacity, signatures, clip, trim)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*cohort signatures"):
        begin(stub, 4, "fedavg", None, True, None, None)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*fedbuff"):
        begin(stub, 4, "fedbuff", None, False, None, None)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*qfedavg"):
        begin(stub, 4, "qfedavg", None, False, None, None)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*clip"):
        begin(stub, 4, "fedavg", None, False, object(), None)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*trim"):
        begin(stub, 4, "fedavg", None, False, None, 1)
    for world in ((2, 1), (1, 2)):
        sharded = types.SimpleNamespace(upload_sign="sign1", shards=types.SimpleNamespace(world=world[0]),
                                        layout=types.SimpleNamespace(world=world[1]))
        with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*sharded"):
            begin(sharded, 4, "fedavg", None, False, None, None)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*fedbuff"):
        SignRound(None, "cpu", 4, "fedbuff", staging=types.SimpleNamespace(fmt="sign1"), last_f32=None)
    # the robust rounds and secure aggregation refuse the format by its name
    robust = types.SimpleNamespace(upload_sign="sign1", upload_topk=None, upload_quant=None, upload_dtype=None)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1' \(1-bit sign delta uploads\)"):
        TorchModelAdapter._check_krum(robust, "fedavg", False, None, None, 1)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1' \(1-bit sign delta uploads\)"):
        TorchModelAdapter._check_geomed(robust, "fedavg", False, None, None, None, True)
    masked = types.SimpleNamespace(upload_sign="sign1", upload_secagg=object())
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1' \(1-bit sign delta uploads\)"):
        TorchModelAdapter._begin_secagg_round(masked, 4, "fedavg", None, False, None, None, None, None)


def test_mixins_pass_device_upload_sign_through_and_refuse_what_the_format_does_not_take():
    from fedscale_amd.cloud.aggregation import aggregator as agg

    assert agg.DeviceAggregatorMixin.device_upload_sign is None
    assert agg.DeviceAsyncAggregatorMixin.device_upload_sign is None  # inherited
    assert agg.DeviceCohortAggregatorMixin.device_upload_sign is None

    class Base:
        def init_model(self):
            self.model_wrapper = types.SimpleNamespace(get_model=lambda: torch.nn.Linear(4, 2))

    class A(agg.DeviceAggregatorMixin, Base):
        device_upload_sign = "sign1"
        device_shards = [0, 1]
        args = types.SimpleNamespace(gradient_policy=None)

    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*ShardedModelAdapter"):
        A().init_model()

    class One(agg.DeviceAggregatorMixin, Base):  # one device: the keyword reaches TorchModelAdapter, which checks it
        device_upload_sign = "no-such-format"
        args = types.SimpleNamespace(gradient_policy=None)

    with pytest.raises(ValueError, match="upload_sign 'no-such-format'"):
        One().init_model()

    class B(agg.DeviceAsyncAggregatorMixin):
        device_upload_sign = "sign1"

    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*DeviceAsyncAggregatorMixin"):
        B().update_weight_aggregation({"client_id": 0, "update_weight": {}})

    for attr, val in (("device_krum", 1), ("device_geomed", True), ("device_upload_secagg", True)):
        C = type("C", (agg.DeviceAggregatorMixin,), {"device_upload_sign": "sign1", attr: val})
        spec = {"device_krum": "_krum_spec", "device_geomed": "_geomed_spec", "device_upload_secagg": "_secagg_spec"}
        with pytest.raises(NotImplementedError, match=r"device_upload_sign='sign1' \(1-bit sign delta uploads\)"):
            getattr(C(), spec[attr])()


def test_pickling_an_adapter_carries_the_keyword():
    from fedscale_amd.cloud.internal import torch_model_adapter as tma

    net = torch.nn.Linear(4, 2)
    stub = types.SimpleNamespace(upload_sign="sign1", upload_topk=None, upload_quant=None, upload_dtype=None,
                                 optimizer=None, get_model=lambda: net)
    fn, args = tma.TorchModelAdapter.__reduce__(stub)
    assert fn is tma._rebuild_with_upload_sign and args == (types.SimpleNamespace, net, None, "sign1")
    seen = {}

    class Fake:
        def __init__(self, model, optimizer, upload_sign=None):
            seen.update(model=model, optimizer=optimizer, upload_sign=upload_sign)

    assert type(fn(Fake, *args[1:])) is Fake and seen == dict(model=net, optimizer=None, upload_sign="sign1")
    assert tma.TorchModelAdapter.upload_sign is None  # unset: the class default, and __reduce__ is what it was
    plain = types.SimpleNamespace(upload_quant=None, upload_dtype=None, optimizer=None, get_model=lambda: net)
    assert tma.TorchModelAdapter.__reduce__(plain) == (types.SimpleNamespace, (net, None))
