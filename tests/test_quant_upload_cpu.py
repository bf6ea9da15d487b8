"""The MXFP8 delta-upload path without a device: ``compress_delta``'s host path against the numpy restatement of the
contract (tests/quant_fixtures.py) byte for byte on the contract's edge cases, the derived error bound, the round
trip of an upload through ``pickle`` and ``ingress.loads``, the validation a ``QuantStaging`` applies to an upload,
and the combinations that are refused."""
import pickle
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from fedscale_amd import ingress
from fedscale_amd.bucket import BucketLayout
from fedscale_amd.cloud.execution.quant_upload import SCALES_KEY, compress_delta
from fedscale_amd.quant_round import QuantRound, upload_plan8
from fedscale_amd.state import ShardGroup
from tests import quant_fixtures as qf

CASES = qf.contract_cases()


def _one_entry(d):
    """(state, base) of one float32 entry whose delta is exactly ``d``: x = d against a base of +0 (a nonzero base
    would round the subtraction, and the delta would no longer be ``d``)."""
    return OrderedDict(w=d.copy()), OrderedDict(w=np.zeros_like(d))


def _codes_of(up, names):
    return np.concatenate([np.asarray(up[n]).reshape(-1) for n in names])


@pytest.mark.parametrize("name", list(CASES))
def test_host_path_equals_the_restatement_byte_for_byte(name):
    d = CASES[name]
    state, base = _one_entry(d)
    up = compress_delta(state, base)
    assert list(up) == ["w", SCALES_KEY]
    want_codes, want_s = qf.quantize(d)
    assert up["w"].dtype == np.uint8 and up["w"].shape == d.shape
    assert up[SCALES_KEY].dtype == np.uint8 and up[SCALES_KEY].shape == (qf.blocks(d.size),)
    assert np.array_equal(up[SCALES_KEY], want_s), name
    finite = np.repeat(want_s != 255, qf.BLOCK)[:d.size]  # codes of a NaN / inf block are unspecified
    assert np.array_equal(up["w"][finite], want_codes[:d.size][finite]), name
    assert not np.any((want_codes & 0x7F) == 0x7F)  # the quantiser emits no NaN code
    assert qf.error_bound_holds(d, want_codes, want_s), name


def test_the_planted_values_land_where_the_contract_says():
    s = qf.quantize(CASES["amax_at_448_threshold"])
    assert s[1][0] == 107 and s[0][5] == 0x7E  # 448 * 2^-20: scale 107, code 448
    s = qf.quantize(CASES["amax_just_above_448_threshold"])
    assert s[1][0] == 108 and s[0][7] == (0x80 | 0x76)  # the next fp32 above: scale 108, code -224
    codes, sc = qf.quantize(CASES["amax_flt_max"])
    assert sc[0] == 246 and codes[0] == 0x7E and codes[1] == 0xFE  # saturated
    codes, sc = qf.quantize(CASES["amax_below_2^-127"])
    assert sc[0] == 10 and not np.any(codes & 0x7F)
    codes, sc = qf.quantize(CASES["negative_zero_block"])
    assert sc[0] == 10 and np.all(codes == 0x80)  # -0 stays -0
    assert qf.quantize(CASES["nan_block_between_finite_blocks"])[1].tolist()[1] == 255
    assert qf.quantize(CASES["inf_block"])[1].tolist()[2] == 255
    assert qf.TABLE[0x76] == 224.0 and qf.TABLE[0x7E] == 448.0 and np.isnan(qf.TABLE[0x7F]) and np.isnan(qf.TABLE[0xFF])
    for P in (1, 31, 33, 95):  # padding codes of a partial block are 0
        codes, sc = qf.quantize(CASES[f"P={P}"])
        assert codes.size == qf.blocks(P) * 32 and not np.any(codes[P:])
    # a tie rounds to the even code: halfway between 0x08 (2^-6) and 0x09 goes to 0x08, between 0x09 and 0x0A to 0x0A
    mid = np.asarray([448.0, (qf.POS[8] + qf.POS[9]) / 2, (qf.POS[9] + qf.POS[10]) / 2], dtype=np.float32)
    assert qf.quantize(mid)[0][:3].tolist() == [0x7E, 0x08, 0x0A]


def test_blocks_run_across_entries_and_other_dtypes_pass_through():
    rng = np.random.default_rng(5)
    state = OrderedDict([("a", torch.from_numpy(rng.standard_normal((4, 5)).astype(np.float32))),
                         ("n", torch.tensor(7, dtype=torch.int64)),
                         ("b", torch.from_numpy((rng.standard_normal(30) * 1e-3).astype(np.float32))),
                         ("e", torch.zeros(0, dtype=torch.float32)),
                         ("s", torch.tensor(0.5))])
    base = [torch.from_numpy(rng.standard_normal(tuple(v.shape)).astype(np.float32)) if v.dtype == torch.float32
            else v.clone() for v in state.values()]
    names = ["a", "b", "e", "s"]
    d = np.concatenate([(state[n].numpy() - b.numpy()).reshape(-1)
                        for n, b in zip(state, base) if state[n].dtype == torch.float32])
    assert d.size == 51  # block 0: all of "a" and the first 12 of "b"
    want_codes, want_s = qf.quantize(d)
    for b in (base, OrderedDict(zip(state, base))):  # a list in the state's order, and a dict
        up = compress_delta(state, b)
        assert list(up) == list(state) + [SCALES_KEY]
        assert up["n"].dtype == np.int64 and int(up["n"]) == 7
        assert [up[n].shape for n in names] == [(4, 5), (30,), (0,), ()]
        assert np.array_equal(_codes_of(up, names), want_codes[:51])
        assert np.array_equal(up[SCALES_KEY], want_s) and want_s.size == 2
    with pytest.raises(ValueError, match="base has 2 entries"):
        compress_delta(state, base[:2])
    with pytest.raises(ValueError, match="b: base shape"):
        compress_delta(state, [base[0], base[1], base[2][:5], base[3], base[4]])


def _state():
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                              torch.nn.Linear(4 * 26 * 26, 400))
    base = OrderedDict((k, v.clone()) for k, v in net.state_dict().items())
    sd = OrderedDict((k, v + 0.01 * torch.randn_like(v) if v.dtype == torch.float32 else v + 5)
                     for k, v in base.items())
    return sd, base


def test_the_wire_format_round_trips_through_pickle_and_ingress():
    sd, base = _state()
    up = compress_delta(sd, list(base.values()))
    payload = pickle.dumps({"client_id": 3, "update_weight": up, "moving_loss": 0.5})
    got = ingress.loads(payload)
    assert got["client_id"] == 3 and got["moving_loss"] == 0.5
    back = got["update_weight"]
    assert list(back) == list(up) and list(back)[-1] == SCALES_KEY
    for k in up:
        assert back[k].dtype == up[k].dtype and back[k].shape == up[k].shape and np.array_equal(back[k], up[k]), k
    big = back["3.weight"]  # 400 x 2704 codes = 1.08 MB
    assert big.nbytes > 1 << 19 and not big.flags.owndata and not big.flags.writeable
    plain = pickle.loads(payload)["update_weight"]
    assert all(plain[k].tobytes() == back[k].tobytes() and plain[k].dtype == back[k].dtype for k in up)
    lay = BucketLayout.from_state_dict(sd)
    plan, scales = upload_plan8(lay, back)  # the read-only views are what the staging takes
    assert len(plan) == lay.T and scales.shape == (qf.blocks(lay.P),)


def test_validation_names_the_entry_that_does_not_fit():
    sd, base = _state()
    lay = BucketLayout.from_state_dict(sd)
    good = compress_delta(sd, base)
    plan, scales = upload_plan8(lay, good)
    assert len(plan) == lay.T and all(type(v) is np.ndarray for _, v in plan) and scales is good[SCALES_KEY]
    plan, scales = upload_plan8(lay, list(good.values()))  # a list in layout order, the scale array last
    assert len(plan) == lay.T and scales is good[SCALES_KEY]
    tens = {k: torch.from_numpy(np.array(v)) for k, v in good.items()}
    plan, scales = upload_plan8(lay, tens)
    assert all(type(v) is np.ndarray for _, v in plan) and type(scales) is np.ndarray  # CPU tensors become arrays
    assert np.array_equal(plan[0][1], good["0.weight"])

    f32 = {k: v.numpy() for k, v in sd.items()}
    f32[SCALES_KEY] = good[SCALES_KEY]
    with pytest.raises(TypeError, match=r"0\.weight.*float32"):
        upload_plan8(lay, f32)
    with pytest.raises(TypeError, match=r"0\.weight.*torch\.float32"):
        upload_plan8(lay, {**{k: v for k, v in sd.items()}, SCALES_KEY: good[SCALES_KEY]})
    with pytest.raises(TypeError, match=SCALES_KEY):  # a float32 upload of whole weights: no scale array at all
        upload_plan8(lay, {k: v.numpy() for k, v in sd.items()})
    bad = dict(good)
    bad["3.bias"] = good["3.bias"][:5]
    with pytest.raises(TypeError, match=r"3\.bias.*shape"):
        upload_plan8(lay, bad)
    bad = dict(good)
    bad["1.num_batches_tracked"] = np.asarray(7, dtype=np.int32)
    with pytest.raises(TypeError, match=r"1\.num_batches_tracked.*int32"):
        upload_plan8(lay, bad)
    bad = dict(good)
    bad[SCALES_KEY] = good[SCALES_KEY][:-1]
    with pytest.raises(TypeError, match=SCALES_KEY + ".*shape"):
        upload_plan8(lay, bad)
    bad[SCALES_KEY] = good[SCALES_KEY].astype(np.int8)
    with pytest.raises(TypeError, match=SCALES_KEY + ".*int8"):
        upload_plan8(lay, bad)
    with pytest.raises(ValueError, match="tensors"):
        upload_plan8(lay, list(good.values())[:-1])


def test_refused_combinations_name_the_combination():
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    net = torch.nn.Linear(4, 2)
    with pytest.raises(NotImplementedError, match="upload_quant='mxfp8'.*ShardedModelAdapter"):
        ShardedModelAdapter(net, devices=[0, 1], upload_quant="mxfp8")
    for mode in ("params", "clients"):
        with pytest.raises(NotImplementedError, match="upload_quant='mxfp8'.*shard"):
            TorchModelAdapter(net, shards=ShardGroup(0, 2, None, mode), upload_quant="mxfp8")
    with pytest.raises(NotImplementedError, match="upload_quant='mxfp8'.*q-fedavg"):
        TorchModelAdapter(net, optimizer=types.SimpleNamespace(mode="q-fedavg"), upload_quant="mxfp8")
    with pytest.raises(NotImplementedError, match="upload_quant='mxfp8'.*upload_dtype='bfloat16'"):
        TorchModelAdapter(net, upload_dtype="bfloat16", upload_quant="mxfp8")
    with pytest.raises(ValueError, match="mxfp8"):
        TorchModelAdapter(net, upload_quant="mxfp4")
    with pytest.raises(ValueError, match="float16"):  # as before
        TorchModelAdapter(net, upload_dtype="float32")
    # begin_round of an adapter with upload_quant (no device is reached before the refusal)
    stub = types.SimpleNamespace(upload_quant="mxfp8", upload_dtype=None)
    begin = TorchModelAdapter._begin_quant_round  # (K, policy, capacity, signatures, clip, trim)
    with pytest.raises(NotImplementedError, match="upload_quant='mxfp8'.*cohort signatures"):
        begin(stub, 4, "fedavg", None, True, None, None)
    with pytest.raises(NotImplementedError, match="upload_quant='mxfp8'.*fedbuff"):
        begin(stub, 4, "fedbuff", None, False, None, None)
    with pytest.raises(NotImplementedError, match="upload_quant='mxfp8'.*qfedavg"):
        begin(stub, 4, "qfedavg", None, False, None, None)
    with pytest.raises(NotImplementedError, match="upload_quant='mxfp8'.*clip"):
        begin(stub, 4, "fedavg", None, False, object(), None)
    with pytest.raises(NotImplementedError, match="upload_quant='mxfp8'.*trim"):
        begin(stub, 4, "fedavg", None, False, None, 1)
    with pytest.raises(NotImplementedError, match="upload_quant='mxfp8'.*fedbuff"):
        QuantRound(None, "cpu", 4, "fedbuff", staging=types.SimpleNamespace(fmt="mxfp8"), last_f32=None)


def test_mixins_pass_device_upload_quant_through_and_fedbuff_is_refused():
    from fedscale_amd.cloud.aggregation import aggregator as agg

    assert agg.DeviceAggregatorMixin.device_upload_quant is None
    assert agg.DeviceAsyncAggregatorMixin.device_upload_quant is None  # inherited

    class Base:
        def init_model(self):
            self.model_wrapper = types.SimpleNamespace(get_model=lambda: torch.nn.Linear(4, 2))

    class A(agg.DeviceAggregatorMixin, Base):
        device_upload_quant = "mxfp8"
        device_shards = [0, 1]
        args = types.SimpleNamespace(gradient_policy=None)

    with pytest.raises(NotImplementedError, match="upload_quant='mxfp8'.*ShardedModelAdapter"):
        A().init_model()

    class B(agg.DeviceAsyncAggregatorMixin):
        device_upload_quant = "mxfp8"

    with pytest.raises(NotImplementedError, match="upload_quant='mxfp8'.*DeviceAsyncAggregatorMixin"):
        B().update_weight_aggregation({"client_id": 0, "update_weight": {}})


def test_pickling_an_adapter_carries_the_keyword():
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    net = torch.nn.Linear(4, 2)
    stub = types.SimpleNamespace(upload_quant="mxfp8", upload_dtype=None, optimizer=None, get_model=lambda: net)
    _, args = TorchModelAdapter.__reduce__(stub)
    import inspect

    params = list(inspect.signature(TorchModelAdapter.__init__).parameters)[1:]
    assert params[-1] == "upload_quant" and len(args) == len(params)
    kw = dict(zip(params, args))
    assert kw["upload_quant"] == "mxfp8" and kw["upload_dtype"] is None and kw["model"] is net
