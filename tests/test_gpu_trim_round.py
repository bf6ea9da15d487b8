"""Trimmed-mean rounds end to end on the MI355X: ``TorchModelAdapter.begin_round(trim=...)`` and the aggregator mixin
with ``device_trim`` against the numpy restatement of tests/trim_fixtures.py, bit for bit, on a small model with fp32
parameters, BatchNorm buffers and an int64 ``num_batches_tracked`` — one upload scaled by 1e15, one carrying NaNs."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import trim_fixtures as tf

pytestmark = pytest.mark.gpu

SCALED, NANS = 3, 6  # the client whose update is scaled by 1e15, and the one that uploads NaNs


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(1, 3, 3)
        self.bn = torch.nn.BatchNorm2d(3)
        self.fc = torch.nn.Linear(27, 5)


class _Case:
    """The model, its layout, and K uploads as per-entry arrays and as flat fp32 rows in the bucket's order."""

    def __init__(self, K, seed=0, poisoned=True, scaled=SCALED, nans=NANS, net=_Net):
        from fedscale_amd.bucket import BucketLayout

        torch.manual_seed(5)
        self.net = net
        self.model = net()
        sd = self.model.state_dict()
        self.names, self.init = list(sd.keys()), [v.clone() for v in sd.values()]
        self.layout = BucketLayout.from_state_dict(OrderedDict(zip(self.names, self.init)))
        self.P, self.K = self.layout.P, K
        assert net is not _Net or (self.P == 182 and len(self.layout.i_entries) == 1)
        rng = np.random.default_rng(40 + seed)
        self.uploads = []
        for k in range(K):
            vals = []
            for v in self.init:
                a = v.numpy()
                if a.dtype == np.int64:
                    vals.append(np.asarray(10 + 2 * k, dtype=np.int64).reshape(a.shape))  # the mean is an integer
                    continue
                d = rng.standard_normal(a.shape).astype(np.float32) * np.float32(0.05)
                if poisoned and k == scaled:
                    d = d * np.float32(1e15)
                u = (a + d).astype(np.float32)
                if poisoned and k == nans:
                    u.reshape(-1)[::3] = np.nan
                vals.append(u)
            self.uploads.append(vals)
        self.x = np.stack([self.flat(u) for u in self.uploads])
        self.side = sum(10 + 2 * k for k in range(K)) // K
        assert sum(10 + 2 * k for k in range(K)) % K == 0

    def flat(self, values):
        buf = np.zeros(self.P, dtype=np.float32)
        for e in self.layout.f_entries:
            buf[e.offset:e.offset + e.numel] = np.asarray(values[e.index], dtype=np.float32).reshape(-1)
        return buf

    def flat_of_weights(self, got):
        return self.flat([t.numpy() for t in got])

    def upload(self, k, form="dict"):
        return dict(zip(self.names, self.uploads[k])) if form == "dict" else list(self.uploads[k])

    def adapter(self, capacity=None, policy=None, args=None):
        from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
        from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

        torch.manual_seed(5)
        opt = TorchServerOptimizer(policy, args, "cuda:0") if policy else None
        return TorchModelAdapter(self.net(), optimizer=opt, device="cuda:0", staging_capacity=capacity)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(case, adapter, **kw):
    K = case.K
    rnd = adapter.begin_round(K, "fedavg", **kw)
    for k in range(K):
        rnd.add(case.upload(k, "dict" if k % 2 else "list"))
    adapter.apply_round(rnd, float(np.float32(K)), float(K))
    return rnd


def _assert_model(case, got, want_flat, what):
    flat = case.flat_of_weights(got)
    bad = np.flatnonzero(_bits(flat) != _bits(want_flat))
    assert bad.size == 0, (what, bad[:5], flat[bad[:5]], want_flat[bad[:5]])
    for e in case.layout.f_entries:
        assert got[e.index].dtype == torch.float32 and tuple(got[e.index].shape) == tuple(e.shape)
    for e in case.layout.i_entries:  # the int64 entry is plain FedAvg's, denominator K
        assert got[e.index].dtype == torch.int64 and int(got[e.index]) == case.side, (what, e.name)


def test_poisoned_round_through_begin_round(gpu_device):
    from fedscale_amd.round import DeviceRound
    from fedscale_amd.trim_round import TrimmedRound, TrimSpec

    case = _Case(10)
    want, want_dropped = tf.trimmed_mean(case.x, 2)
    assert np.isfinite(want).all() and not np.isfinite(tf.fedavg_of(case.x)).all()
    adapter = case.adapter()
    rnd = _run(case, adapter, trim=2)
    assert type(rnd) is TrimmedRound and rnd.policy == "fedavg" and rnd.t == 2 and rnd.trim == TrimSpec(2)
    got = adapter.get_weights()
    _assert_model(case, got, want, "trim=2")
    assert all(bool(torch.isfinite(g).all()) for g in got)
    d = rnd.dropped()
    assert d.dtype == np.int64 and np.array_equal(d, want_dropped) and d.sum() == 4 * case.P
    # the scaled upload is an extreme of nearly every column; the NaN upload is dropped high wherever it holds NaN
    assert d[SCALED].sum() > 0.9 * case.P and d[NANS, 1] >= (case.P + 2) // 3
    mean = case.flat([np.asarray(a) for a in adapter.round_mean_weights()])  # no server step: the mean IS the model
    assert np.array_equal(_bits(mean), _bits(want))
    # the plain round on the same uploads is not finite
    plain = case.adapter()
    prnd = _run(case, plain)
    assert type(prnd) is DeviceRound
    assert not np.isfinite(case.flat_of_weights(plain.get_weights())).all()


def test_poisoned_round_through_the_mixin(gpu_device):
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator
    from fedscale_amd.trim_round import TrimmedRound

    case = _Case(10)
    want, want_dropped = tf.trimmed_mean(case.x, 2)

    class TrimmedAggregator(DeviceAggregator):
        device_trim = 0.2  # floor(0.2 * 10) = 2 per side

    adapter = case.adapter()
    agg = TrimmedAggregator(adapter)
    agg.start_round(case.K)
    rnd = None
    for k in range(case.K):
        agg.on_result({"client_id": k + 1, "update_weight": case.upload(k, "dict" if k % 2 else "list"),
                       "moving_loss": 1.0})
        if k == 0:
            rnd = agg._device_round
            assert type(rnd) is TrimmedRound and rnd.t == 2
    assert agg._device_round is None
    _assert_model(case, adapter.get_weights(), want, "mixin")
    assert np.array_equal(rnd.dropped(), want_dropped)
    mean = [torch.from_numpy(np.asarray(a)) for a in agg.model_weights]
    assert np.array_equal(_bits(case.flat_of_weights(mean)), _bits(want))


def test_small_model_without_int64_entries_takes_the_mirror_path(gpu_device):
    """A model that qualifies for the egress mirror: ft_reduce writes the new model's pinned snapshot itself, and
    get_weights() — served from that snapshot — has the restatement's bits."""
    case = _Case(5, seed=4, scaled=1, nans=3, net=lambda: torch.nn.Linear(7, 5))
    assert case.P == 40 and not case.layout.i_entries
    adapter = case.adapter()
    L = adapter.layout
    assert L.Q == 0 and L.P_full * 4 <= adapter.EGRESS_MIRROR_MAX_BYTES  # (_mirror_target: the round gets a mirror)
    rnd = _run(case, adapter, trim=1)
    want, want_dropped = tf.trimmed_mean(case.x, 1)
    flat = case.flat_of_weights(adapter.get_weights())
    assert np.isfinite(want).all() and np.array_equal(_bits(flat), _bits(want))
    assert np.array_equal(rnd.dropped(), want_dropped)


def test_trim_zero_is_the_untrimmed_round(gpu_device):
    case = _Case(7, seed=1, poisoned=False)
    a, b = case.adapter(), case.adapter()
    rnd = _run(case, a, trim=0)
    _run(case, b)
    ga, gb = a.get_weights(), b.get_weights()
    assert np.array_equal(_bits(case.flat_of_weights(ga)), _bits(case.flat_of_weights(gb)))
    _assert_model(case, ga, tf.fedavg_of(case.x), "trim=0")
    assert rnd.t == 0 and rnd.dropped().sum() == 0


@pytest.mark.parametrize("K", [9, 10])
def test_median_is_numpys(gpu_device, K):
    case = _Case(K, seed=2, poisoned=False)
    adapter = case.adapter()
    rnd = _run(case, adapter, trim="median")
    assert rnd.t == (K - 1) // 2
    _assert_model(case, adapter.get_weights(), np.median(case.x, axis=0), ("median", K))


def test_fed_yogi_on_the_trimmed_mean(gpu_device):
    """The trimmed mean feeds the existing YoGi step: the new model is fa_yogi_step's on the restated mean."""
    from fedscale_amd import kernels as kx
    from tests.golden_io import Scenario

    case = _Case(10)
    args = Scenario("fedyogi_mixed_3rounds").args()
    want_mean, _ = tf.trimmed_mean(case.x, 2)
    adapter = case.adapter(policy="fed-yogi", args=args)
    _run(case, adapter, trim=2)
    got = case.flat_of_weights(adapter.get_weights())
    # the same step, by hand, on a second adapter's buffers
    other = case.adapter(policy="fed-yogi", args=args)
    L, dev = other.layout, other.device
    y = other.optimizer.gradient_controller
    y.bind(L, dev)
    mean = torch.zeros(L.ld, dtype=torch.float32, device=dev)
    mean[:L.P] = torch.from_numpy(want_mean).to(dev)
    out = torch.zeros(L.ld, dtype=torch.float32, device=dev)
    kx.yogi_step(mean, other._snapshot().f32, y.m, y.v, out, L.P, init=True, **y.fp32_hparams())
    want = out[:L.P].cpu().numpy()
    assert np.isfinite(want).all() and np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), _bits(want_mean))  # the step really moved the model off the mean


def test_two_rounds_back_to_back(gpu_device):
    """The second round on the same adapter (and staging) sees nothing of the first's thresholds or counts."""
    first, second = _Case(10), _Case(10, seed=9, scaled=0, nans=8)
    adapter = first.adapter()
    r1 = _run(first, adapter, trim=2)
    want1, dropped1 = tf.trimmed_mean(first.x, 2)
    _assert_model(first, adapter.get_weights(), want1, "round 1")
    r2 = _run(second, adapter, trim=3)
    want2, dropped2 = tf.trimmed_mean(second.x, 3)
    _assert_model(second, adapter.get_weights(), want2, "round 2")
    assert np.array_equal(r2.dropped(), dropped2) and np.array_equal(r1.dropped(), dropped1)
    assert r1.staging is r2.staging and r2.generation == r1.generation + 1
    assert not np.array_equal(dropped1, dropped2) and dropped2.sum() == 6 * second.P


def test_a_round_above_the_capacity_is_refused(gpu_device):
    case = _Case(10)
    adapter = case.adapter()
    with pytest.raises(ValueError, match="all K=10 uploads resident.*capacity is 4"):
        adapter.begin_round(10, "fedavg", capacity=4, trim=2)
    assert adapter.staging is None  # refused before anything was allocated or launched
    small = case.adapter(capacity=9)
    with pytest.raises(ValueError, match="all K=10 uploads resident.*capacity is 9"):
        small.begin_round(10, "fedavg", trim="median")
    with pytest.raises(ValueError, match=r"ft_max_trim\(\) = 16"):
        adapter.begin_round(40, "fedavg", trim="median")
    rnd = _run(case, adapter, capacity=10, trim=2)  # the same adapter still runs a round that fits
    _assert_model(case, adapter.get_weights(), tf.trimmed_mean(case.x, 2)[0], "after the refusals")
    assert rnd.cap == 10
