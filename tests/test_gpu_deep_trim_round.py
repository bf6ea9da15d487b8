"""Deep trimmed-mean rounds end to end on the MI355X: ``TorchModelAdapter.begin_round(deep_trim=...)`` and the
aggregator mixin with ``device_deep_trim`` against the numpy restatement of tests/trim_fixtures.py, bit for bit, on
the small model of tests/test_gpu_trim_round.py (fp32 parameters, BatchNorm buffers, an int64 entry; one upload scaled
by 1e15, one carrying NaNs)."""
import numpy as np
import pytest
import torch

from tests import trim_fixtures as tf
from tests.test_gpu_trim_round import _assert_model, _bits, _Case, _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K, spec, t", [(40, "median", 19), (100, 0.2, 20), (35, 17, 17)])
def test_round_through_begin_round(gpu_device, K, spec, t):
    from fedscale_amd.deep_trim_round import DeepTrimmedRound, DeepTrimSpec

    case = _Case(K)
    want, want_dropped = tf.trimmed_mean(case.x, t)
    assert np.isfinite(want).all() and not np.isfinite(tf.fedavg_of(case.x)).all()
    adapter = case.adapter()
    rnd = _run(case, adapter, deep_trim=spec)
    assert type(rnd) is DeepTrimmedRound and rnd.t == t and rnd.deep_trim == DeepTrimSpec(spec)
    _assert_model(case, adapter.get_weights(), want, (K, spec))
    d = rnd.dropped()
    assert d.dtype == np.int64 and np.array_equal(d, want_dropped) and d.sum() == 2 * t * case.P


def test_zero_is_the_untrimmed_round(gpu_device):
    case = _Case(7, seed=1, poisoned=False)
    a, b = case.adapter(), case.adapter()
    rnd = _run(case, a, deep_trim=0)
    _run(case, b)
    assert np.array_equal(_bits(case.flat_of_weights(a.get_weights())), _bits(case.flat_of_weights(b.get_weights())))
    _assert_model(case, a.get_weights(), tf.fedavg_of(case.x), "deep_trim=0")
    assert rnd.t == 0 and rnd.dropped().sum() == 0


def test_fed_yogi_on_the_deep_trimmed_mean(gpu_device):
    """The mean feeds the existing YoGi step: the new model is fa_yogi_step's on the restated mean."""
    from fedscale_amd import kernels as kx
    from tests.golden_io import Scenario

    case = _Case(40)
    args = Scenario("fedyogi_mixed_3rounds").args()
    want_mean, _ = tf.trimmed_mean(case.x, 19)
    adapter = case.adapter(policy="fed-yogi", args=args)
    _run(case, adapter, deep_trim="median")
    got = case.flat_of_weights(adapter.get_weights())
    other = case.adapter(policy="fed-yogi", args=args)  # the same step, by hand, on a second adapter's buffers
    L, dev = other.layout, other.device
    y = other.optimizer.gradient_controller
    y.bind(L, dev)
    mean = torch.zeros(L.ld, dtype=torch.float32, device=dev)
    mean[:L.P] = torch.from_numpy(want_mean).to(dev)
    out = torch.zeros(L.ld, dtype=torch.float32, device=dev)
    kx.yogi_step(mean, other._snapshot().f32, y.m, y.v, out, L.P, init=True, **y.fp32_hparams())
    want = out[:L.P].cpu().numpy()
    assert np.isfinite(want).all() and np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), _bits(want_mean))


def test_round_through_the_mixin(gpu_device):
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator
    from fedscale_amd.deep_trim_round import DeepTrimmedRound

    case = _Case(40)
    want, want_dropped = tf.trimmed_mean(case.x, 19)

    class MedianAggregator(DeviceAggregator):
        device_deep_trim = "median"

    adapter = case.adapter()
    agg = MedianAggregator(adapter)
    agg.start_round(case.K)
    rnd = None
    for k in range(case.K):
        agg.on_result({"client_id": k + 1, "update_weight": case.upload(k, "dict" if k % 2 else "list"),
                       "moving_loss": 1.0})
        rnd = rnd or agg._device_round
    assert type(rnd) is DeepTrimmedRound and rnd.t == 19 and agg._device_round is None
    _assert_model(case, adapter.get_weights(), want, "mixin")
    assert np.array_equal(rnd.dropped(), want_dropped)


def test_a_round_above_the_capacity_is_refused(gpu_device):
    case = _Case(40)
    adapter = case.adapter()
    with pytest.raises(ValueError, match="all K=40 uploads resident.*capacity is 4"):
        adapter.begin_round(40, "fedavg", capacity=4, deep_trim="median")
    assert adapter.staging is None  # refused before anything was allocated or launched
    _run(case, adapter, deep_trim="median")  # the same adapter still runs a round that fits
    _assert_model(case, adapter.get_weights(), tf.trimmed_mean(case.x, 19)[0], "after the refusal")
