"""The 16-bit upload path without a device: ``compress_update`` on CPU state against numpy / torch, the round trip
of a compressed update through ``ingress.loads``, the validation a ``HalfStaging`` applies to an upload, and the
combinations that are refused."""
import pickle
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from fedscale_amd import ingress
from fedscale_amd.bucket import BucketLayout
from fedscale_amd.cloud.execution.half_upload import compress_update
from fedscale_amd.half_round import HalfRound, upload_plan16
from fedscale_amd.state import ShardGroup


def _state(big: bool = False):
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                              torch.nn.Linear(4 * 26 * 26, 400 if big else 10))
    sd = OrderedDict((k, v.clone()) for k, v in net.state_dict().items())
    sd["1.num_batches_tracked"] += 5
    w = sd["0.weight"].reshape(-1)  # values the two formats round differently, and what they cannot hold
    w[:12] = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.9, 65520.0, 1e-7, -6e-8, 3.4e38, -3.4e38,
                           float("inf"), float("-inf"), 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])
    return sd


def test_float16_equals_numpy_astype():
    sd = _state()
    up = compress_update(sd, "float16")
    assert list(up) == list(sd)
    for k, v in sd.items():
        if v.dtype == torch.float32:
            assert up[k].dtype == np.float16 and up[k].shape == tuple(v.shape)
            with np.errstate(over="ignore"):
                want = v.numpy().astype(np.float16)
            assert np.array_equal(up[k].view(np.uint16), want.view(np.uint16)), k
        else:
            assert up[k].dtype == np.int64 and np.array_equal(up[k], v.numpy()), k
    assert np.isinf(up["0.weight"].reshape(-1)[3]) and up["0.weight"].reshape(-1)[2] == np.float16(65504.0)


def test_bfloat16_bits_equal_torch_cpu():
    sd = _state()
    for state in (sd, OrderedDict((k, v.numpy()) for k, v in sd.items())):  # tensors, and numpy arrays
        up = compress_update(state, "bfloat16")
        for k, v in sd.items():
            if v.dtype == torch.float32:
                want = v.to(torch.bfloat16).view(torch.int16).numpy()
                assert up[k].dtype == np.uint16 and np.array_equal(up[k].view(np.int16), want), k
            else:
                assert up[k].dtype == np.int64 and np.array_equal(up[k], v.numpy()), k


def test_torch_dtypes_are_accepted_and_others_refused():
    sd = _state()
    a = compress_update(sd, torch.bfloat16)
    b = compress_update(sd, "bfloat16")
    assert all(np.array_equal(a[k], b[k]) for k in sd)
    for bad in ("float32", "fp16", torch.float32, None):
        with pytest.raises(ValueError, match="float16"):
            compress_update(sd, bad)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_ingress_round_trips_a_compressed_update(dtype):
    """The pickled dict comes back with equal arrays of the same dtypes; the large 16-bit arrays are views of the
    payload (read-only), as the float32 arrays of a float32 upload are."""
    up = compress_update(_state(big=True), dtype)
    payload = pickle.dumps({"client_id": 3, "update_weight": up, "moving_loss": 0.5})
    got = ingress.loads(payload)
    assert got["client_id"] == 3 and got["moving_loss"] == 0.5
    back = got["update_weight"]
    assert list(back) == list(up)
    for k in up:
        assert back[k].dtype == up[k].dtype and back[k].shape == up[k].shape, k
        assert np.array_equal(back[k].view(np.uint16) if up[k].dtype != np.int64 else back[k],
                              up[k].view(np.uint16) if up[k].dtype != np.int64 else up[k]), k
    big = back["3.weight"]  # 400 x 2704 x 2 bytes = 2.2 MB
    assert big.nbytes > 1 << 19 and not big.flags.owndata and not big.flags.writeable
    plain = pickle.loads(payload)["update_weight"]
    assert all(plain[k].tobytes() == back[k].tobytes() and plain[k].dtype == back[k].dtype for k in up)


def _layout():
    sd = _state()
    return sd, BucketLayout.from_state_dict(sd)


def test_validation_names_the_entry_that_does_not_fit():
    sd, lay = _layout()
    good16 = compress_update(sd, "float16")
    goodbf = compress_update(sd, "bfloat16")
    assert len(upload_plan16(lay, good16, "float16")) == lay.T
    assert len(upload_plan16(lay, goodbf, "bfloat16")) == lay.T
    assert len(upload_plan16(lay, list(goodbf.values()), "bfloat16")) == lay.T  # a list in layout order
    as_i16 = {k: (v.view(np.int16) if v.dtype == np.uint16 else v) for k, v in goodbf.items()}
    assert len(upload_plan16(lay, as_i16, "bfloat16")) == lay.T
    tens = {k: (v.to(torch.bfloat16) if v.dtype == torch.float32 else v) for k, v in sd.items()}
    plan = upload_plan16(lay, tens, "bfloat16")
    assert all(type(v) is np.ndarray for _, v in plan)  # CPU tensors become host arrays
    assert np.array_equal(plan[0][1].view(np.uint16), goodbf["0.weight"])

    f32 = {k: v.numpy() for k, v in sd.items()}
    with pytest.raises(TypeError, match=r"0\.weight.*float32"):
        upload_plan16(lay, f32, "float16")
    with pytest.raises(TypeError, match=r"0\.weight.*float32"):
        upload_plan16(lay, f32, "bfloat16")
    with pytest.raises(TypeError, match=r"0\.weight.*float16"):  # float16 arrays offered to a bfloat16 staging
        upload_plan16(lay, good16, "bfloat16")
    with pytest.raises(TypeError, match=r"0\.weight.*uint16"):   # and bfloat16 bits to a float16 staging
        upload_plan16(lay, goodbf, "float16")
    bad = dict(good16)
    bad["3.bias"] = good16["3.bias"][:5]
    with pytest.raises(TypeError, match=r"3\.bias.*shape"):
        upload_plan16(lay, bad, "float16")
    bad = dict(good16)
    bad["1.num_batches_tracked"] = np.asarray(7, dtype=np.int32)
    with pytest.raises(TypeError, match=r"1\.num_batches_tracked.*int32"):
        upload_plan16(lay, bad, "float16")
    bad = {k: (v.to(torch.float16) if v.dtype == torch.float32 else v) for k, v in sd.items()}
    with pytest.raises(TypeError, match=r"0\.weight.*torch\.float16"):
        upload_plan16(lay, bad, "bfloat16")
    with pytest.raises(ValueError, match="tensors"):
        upload_plan16(lay, list(good16.values())[:-1], "float16")


def test_refused_combinations_name_the_combination():
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    net = torch.nn.Linear(4, 2)
    with pytest.raises(NotImplementedError, match="upload_dtype='bfloat16'.*ShardedModelAdapter"):
        ShardedModelAdapter(net, devices=[0, 1], upload_dtype="bfloat16")
    for mode in ("params", "clients"):
        with pytest.raises(NotImplementedError, match="upload_dtype='float16'.*shard"):
            TorchModelAdapter(net, shards=ShardGroup(0, 2, None, mode), upload_dtype="float16")
    with pytest.raises(NotImplementedError, match="upload_dtype='float16'.*q-fedavg"):
        TorchModelAdapter(net, optimizer=types.SimpleNamespace(mode="q-fedavg"), upload_dtype="float16")
    with pytest.raises(ValueError, match="float16"):
        TorchModelAdapter(net, upload_dtype="float32")
    # begin_round of an adapter with upload_dtype (no device is reached before the refusal)
    stub = types.SimpleNamespace(upload_dtype="bfloat16")
    with pytest.raises(NotImplementedError, match="upload_dtype='bfloat16'.*cohort signatures"):
        TorchModelAdapter._begin_half_round(stub, 4, "fedavg", None, True)
    with pytest.raises(NotImplementedError, match="upload_dtype='bfloat16'.*qfedavg"):
        TorchModelAdapter._begin_half_round(stub, 4, "qfedavg", None, False)
    with pytest.raises(NotImplementedError, match="upload_dtype='float16'.*qfedavg"):
        HalfRound(None, "cpu", 4, "qfedavg", staging=types.SimpleNamespace(dtype="float16"))


def test_mixin_passes_device_upload_dtype_through():
    from fedscale_amd.cloud.aggregation import aggregator as agg

    assert agg.DeviceAggregatorMixin.device_upload_dtype is None
    assert agg.DeviceAsyncAggregatorMixin.device_upload_dtype is None  # inherited

    class Base:
        def init_model(self):
            self.model_wrapper = types.SimpleNamespace(get_model=lambda: torch.nn.Linear(4, 2))

    class A(agg.DeviceAggregatorMixin, Base):
        device_upload_dtype = "bfloat16"
        device_shards = [0, 1]
        args = types.SimpleNamespace(gradient_policy=None)

    with pytest.raises(NotImplementedError, match="upload_dtype='bfloat16'.*ShardedModelAdapter"):
        A().init_model()
