"""End to end on the MI355X: aggregators over an adapter with ``upload_dtype`` against the CPU oracle fed the
widened uploads — two rounds of K = 6 on the smoke model (Conv + BatchNorm + Linear: the int64 side table is live),
a staging capacity of 4 forcing a fold, uploads made by ``compress_update``, one per round arriving as device
tensors and one through ``ingress.loads`` of its pickle.  FedAvg and FedBuff are bit-exact; fed-yogi meets smoke()'s
rule (rtol 1e-6 on the model: the reference's CPU torch.sqrt is not IEEE)."""
import argparse
import pickle

import numpy as np
import pytest
import torch

from tests import half_fixtures as hf

pytestmark = pytest.mark.gpu

DTYPES = ("float16", "bfloat16")
K = 6


def _net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                               torch.nn.Linear(4 * 26 * 26, 10))


def _args(policy):
    return argparse.Namespace(gradient_policy=policy, yogi_eta=3e-3, yogi_tau=1e-8, yogi_beta=0.9, yogi_beta2=0.99,
                              learning_rate=0.05, qfed_q=1.0)


def _as_device_tensors(up, dtype, dev):
    out = {}
    for n, a in up.items():
        if a.dtype == np.int64:
            out[n] = torch.from_numpy(np.asarray(a)).to(dev)
        elif dtype == "float16":
            out[n] = torch.from_numpy(a).to(dev)
        else:
            out[n] = torch.from_numpy(a.view(np.int16)).to(dev).view(torch.bfloat16)
    return out


def _run(dtype, policy, asynchronous, dev):
    from fedscale_amd import ingress
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator, DeviceAsyncAggregator
    from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
    from fedscale_amd.cloud.execution.half_upload import compress_update
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.half_round import HalfRound
    from oracle.cpu_reference import OracleAggregator, OracleModel, OracleModelAdapter, OracleServerOptimizer

    net = _net()
    names = list(net.state_dict().keys())
    init = [t.clone() for t in net.state_dict().values()]
    args = _args(policy)
    adapter = TorchModelAdapter(net, device=dev, optimizer=TorchServerOptimizer(policy, args, dev),
                                staging_capacity=4, upload_dtype=dtype)
    ref = OracleModelAdapter(OracleModel(names, init), OracleServerOptimizer(policy, args))
    if asynchronous:
        agg, oagg = DeviceAsyncAggregator(adapter, args), OracleAggregator(ref, args, asynchronous=True)
        for a in (agg, oagg):
            a.round = 7
            for k in range(K):
                a.client_task_model_version[k] = 7 - (k * 2) % 5
    else:
        agg, oagg = DeviceAggregator(adapter, args), OracleAggregator(ref, args)
    rng = np.random.default_rng(0)
    for rnd in range(2):
        agg.start_round(K)
        oagg.start_round(K)
        for k in range(K):
            state = {n: (torch.from_numpy(t.numpy() + rng.normal(0, 0.01, size=t.shape).astype(np.float32))
                         if t.dtype == torch.float32 else t + 5 + k) for n, t in zip(names, init)}
            up = compress_update(state, dtype)
            wide = {n: (a if a.dtype == np.int64 else hf.widen(a, dtype)) for n, a in up.items()}
            if k == 1:
                sent = _as_device_tensors(up, dtype, torch.device(dev))
            elif k == 2:
                sent = ingress.loads(pickle.dumps({"update_weight": up}))["update_weight"]
            elif k == 3:
                sent = list(up.values())
            else:
                sent = up
            oagg.on_result({"client_id": k, "update_weight": wide, "moving_loss": 0.5})
            agg.on_result({"client_id": k, "update_weight": sent, "moving_loss": 0.5})
            if k == 0:
                assert type(agg._device_round) is HalfRound and agg._device_round.cap == 4
            if k == 4:
                assert agg._device_round.chunks_done == 1  # the capacity of 4 forced a fold
        for a, b in zip(adapter.get_weights(), ref.get_weights()):
            assert a.dtype == b.dtype and a.shape == b.shape
            if policy is None:
                assert torch.equal(a, b), (dtype, policy, asynchronous, rnd)
            else:  # fed-yogi: smoke()'s rule
                ad, bd = a.double(), b.double()
                scale = torch.maximum(bd.abs(), bd.pow(2).mean().sqrt()) if bd.numel() else bd
                assert bool(((ad - bd).abs() <= 1e-6 * scale).all()), (dtype, policy, rnd)
        mean = list(agg.model_weights)  # the reference's Aggregator.model_weights: the fp32 / float64 mean
        for a, b in zip(mean, oagg.model_weights):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (dtype, policy, asynchronous, rnd)
        ref.model.load_state_dict({n: t for n, t in zip(names, adapter.get_weights())})  # same trajectory
    assert adapter.staging.x16.dtype == (torch.float16 if dtype == "float16" else torch.bfloat16)
    assert adapter.staging.x16.shape == (4, adapter.layout.ld)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("policy", [None, "fed-yogi"])
def test_device_aggregator_with_16_bit_uploads(gpu_device, dtype, policy):
    _run(dtype, policy, False, "cuda:0")


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_async_aggregator_with_16_bit_uploads(gpu_device, dtype):
    _run(dtype, None, True, "cuda:0")


def test_float32_upload_to_a_16_bit_staging_names_the_entry(gpu_device):
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    net = _net()
    adapter = TorchModelAdapter(net, device="cuda:0", upload_dtype="float16")
    rnd = adapter.begin_round(2, "fedavg")
    with pytest.raises(TypeError, match=r"0\.weight.*float32"):
        rnd.add({n: t.numpy() for n, t in net.state_dict().items()})
    assert rnd.n == 0
    with pytest.raises(NotImplementedError, match="upload_dtype='float16'.*qfedavg"):
        adapter.begin_round(2, "qfedavg")
    with pytest.raises(NotImplementedError, match="upload_dtype='float16'.*cohort signatures"):
        adapter.begin_round(2, "fedavg", signatures=True)


def test_upload_dtype_unset_changes_nothing(gpu_device):
    from fedscale_amd.bucket import ClientStaging
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.round import DeviceRound

    adapter = TorchModelAdapter(_net(), device="cuda:0")
    assert adapter.upload_dtype is None
    rnd = adapter.begin_round(2, "fedavg")
    assert type(rnd) is DeviceRound and type(adapter.staging) is ClientStaging
