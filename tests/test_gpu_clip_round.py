"""Norm-clipped rounds end to end on the MI355X: ``TorchModelAdapter.begin_round(clip=...)`` and the aggregator mixin
with ``device_clip_norm`` against the numpy restatement of tests/clip_fixtures.py, bit for bit — on the golden uploads
of ``fedavg_mixed_k7`` (int64 entries live, P odd) and ``fedavg_femnist_cnn_k10`` (the small-model egress mirror), with
one client's update scaled x 1000.  The restatement computes every squared norm exactly (math.fsum); each test first
asserts, on the host alone, that the last-bits freedom of the device's fp64 sum cannot move a coefficient."""
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import clip_fixtures as cf
from tests.golden_io import Scenario, StateDictModule, assert_state_close, assert_state_equal

pytestmark = pytest.mark.gpu

NAMES = ("fedavg_mixed_k7", "fedavg_femnist_cnn_k10")
SCALED = 2  # the client whose update is scaled x 1000
_SC = {}


class _Case:
    """A golden scenario's model and uploads as flat fp32 rows (the bucket's order), client SCALED scaled x 1000."""

    def __init__(self, name):
        from fedscale_amd.bucket import BucketLayout

        sc = self.sc = Scenario(name)
        self.names, self.K = sc.names, sc.meta["rounds"][0]
        self.init = sc.init_state()
        self.layout = BucketLayout.from_state_dict(OrderedDict(zip(self.names, self.init)))
        self.P = self.layout.P
        self.uploads = []
        for k in range(self.K):
            vals = sc.client(k)
            vals = list(vals.values()) if isinstance(vals, dict) else list(vals)
            vals = [np.array(v) for v in vals]
            if k == SCALED:
                for e in self.layout.f_entries:
                    i0 = self.init[e.index].numpy()
                    v = i0 + (vals[e.index] - i0) * np.float32(1000)
                    vals[e.index] = np.asarray(v, dtype=np.float32).reshape(e.shape)
            self.uploads.append(vals)
        self.last = self.flat([t.numpy() for t in self.init])
        self.x = np.stack([self.flat(u) for u in self.uploads])
        self.sq = [cf.sq_exact(r, self.last) for r in self.x]
        norms = np.sqrt(np.asarray(self.sq))
        honest = np.delete(norms, SCALED)
        assert norms[SCALED] > 100 * honest.max()
        self.bounds = {"above": 2.0 * float(norms.max()),
                       "between": math.sqrt(float(honest.max()) * float(norms[SCALED]))}

    def flat(self, values):
        buf = np.zeros(self.P, dtype=np.float32)
        for e in self.layout.f_entries:
            buf[e.offset:e.offset + e.numel] = np.asarray(values[e.index], dtype=np.float32).reshape(-1)
        return buf

    def unflat(self, flat):
        return {e.index: flat[e.offset:e.offset + e.numel].reshape(e.shape) for e in self.layout.f_entries}

    def upload(self, k, form):
        return dict(zip(self.names, self.uploads[k])) if form == "dict" else list(self.uploads[k])

    def adapter(self, capacity=None, policy=None, args=None):
        from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
        from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

        opt = TorchServerOptimizer(policy, args, "cuda:0") if policy else None
        return TorchModelAdapter(StateDictModule(self.names, self.init), optimizer=opt, device="cuda:0",
                                 staging_capacity=capacity)


def _case(name) -> _Case:
    if name not in _SC:
        _SC[name] = _Case(name)
    return _SC[name]


def _restate(x, last, M, K, sigma=0.0, z=None, sq=None):
    """(new model, coefficients) of one round by the restatement, after asserting its precondition."""
    sq = [cf.sq_exact(r, last) for r in x] if sq is None else sq
    assert all(cf.coef_is_stable(s, M) for s in sq), "a coefficient sits within 2^-40 of an fp32 rounding boundary"
    c = cf.coefs_of(sq, M)
    out, _ = cf.finish_of(cf.chain_of(x, last, c), last, K, sigma, z)
    return out, c


def _assert_fp32_entries(case, got, want_flat, what):
    want = case.unflat(want_flat)
    for i, w in want.items():
        g = got[i].numpy()
        assert g.dtype == np.float32 and g.shape == w.shape, (what, i)
        assert np.array_equal(g.reshape(-1).view(np.uint32), w.reshape(-1).view(np.uint32)), (what, case.names[i])


def _run_round(case, adapter, M, form="dict", noise=0.0, seed=0, x=None):
    from fedscale_amd.clip_round import ClippedRound, ClipSpec

    K = case.K
    rnd = adapter.begin_round(K, "fedavg", clip=ClipSpec(M, noise, seed))
    assert type(rnd) is ClippedRound and rnd.policy == "fedavg"
    for k in range(K):
        rnd.add(case.upload(k, form) if x is None else x[k])
    adapter.apply_round(rnd, float(np.float32(K)), float(K))
    return rnd


@pytest.mark.parametrize("form", ["dict", "list"])
@pytest.mark.parametrize("capacity", [None, 3])
@pytest.mark.parametrize("bound", ["above", "between"])
@pytest.mark.parametrize("name", NAMES)
def test_clipped_round_equals_the_restatement(gpu_device, name, bound, capacity, form):
    case = _case(name)
    M = case.bounds[bound]
    want, c = _restate(case.x, case.last, M, case.K, sq=case.sq)
    assert (c[SCALED] < 0.2) == (bound == "between") and (np.delete(c, SCALED) == 1).all()
    adapter = case.adapter(capacity)
    rnd = _run_round(case, adapter, M, form)
    got = adapter.get_weights()
    _assert_fp32_entries(case, got, want, (name, bound, capacity, form))
    gold = case.sc.expected(0)
    for e in case.layout.i_entries:  # the int64 entries are plain FedAvg's
        assert got[e.index].dtype == torch.int64 and np.array_equal(got[e.index].numpy(), gold[e.index]), e.name
    assert rnd.chunks_done == (1 if capacity is None else -(-case.K // 3)) and rnd.rejected == 0
    assert np.array_equal(rnd.coefficients().view(np.uint32), c.view(np.uint32))
    assert np.allclose(rnd.norms(), np.sqrt(np.asarray(case.sq)), rtol=1e-12, atol=0)
    assert adapter.clip_noise_offset == (case.P + 1) // 2 * 2  # every applied clipped round moves it on
    if bound == "above":  # nothing clipped: the new model is close to plain FedAvg of these uploads
        plain = case.last + np.mean((case.x - case.last).astype(np.float64), axis=0)
        assert np.allclose(want, plain, rtol=1e-4, atol=1e-4)


def test_fed_yogi_on_the_clipped_mean(gpu_device):
    """The clipped mean feeds the existing YoGi step: m and v bit-exact (round 0: no sqrt feeds back yet), the model
    within the project's rtol 1e-6."""
    from oracle.cpu_reference import (OracleModel, OracleModelAdapter, OracleServerOptimizer, fedavg_close,
                                      fedavg_step)

    case = _case("fedavg_mixed_k7")
    args = Scenario("fedyogi_mixed_3rounds").args()
    M = case.bounds["between"]
    mean_flat, _ = _restate(case.x, case.last, M, case.K, sq=case.sq)
    acc = None
    for k in range(case.K):
        acc = fedavg_step(acc, case.uploads[k], k == 0)
    weights = fedavg_close(acc, case.K)  # the int64 entries' float64 means are plain FedAvg's ...
    for i, w in case.unflat(mean_flat).items():
        weights[i] = w  # ... and the fp32 entries are the clipped mean re-based on the starting model
    ref = OracleModelAdapter(OracleModel(case.names, case.init), OracleServerOptimizer("fed-yogi", args))
    ref.set_weights(weights)
    adapter = case.adapter(3, "fed-yogi", args)
    _run_round(case, adapter, M)
    y = adapter.optimizer.gradient_controller
    assert_state_equal(y.m_t, ref.optimizer.gradient_controller.m_t, "yogi m")
    assert_state_equal(y.v_t, ref.optimizer.gradient_controller.v_t, "yogi v")
    assert_state_close(adapter.get_weights(), ref.get_weights(), 1e-6, "yogi model")


@pytest.mark.parametrize("capacity", [None, 3])
def test_a_poisoned_upload_is_rejected(gpu_device, capacity):
    """One client uploads NaN: the new model is finite, the round reports one rejected row, and the model is the
    restatement's over the other rows with the denominator still K."""
    case = _case("fedavg_femnist_cnn_k10")
    bad = 4
    x = case.x.copy()
    x[bad, 1000:1010] = np.nan
    ups = [case.upload(k, "dict") for k in range(case.K)]
    ups[bad] = {n: case.unflat(x[bad])[i].copy() for i, n in enumerate(case.names)}
    M = case.bounds["between"]
    want, c = _restate(x, case.last, M, case.K)
    assert c[bad] == 0 and np.isfinite(want).all()
    adapter = case.adapter(capacity)
    rnd = _run_round(case, adapter, M, x=ups)
    got = adapter.get_weights()
    assert all(bool(torch.isfinite(t).all()) for t in got)
    _assert_fp32_entries(case, got, want, "poisoned")
    assert rnd.rejected == 1 and rnd.coefficients()[bad] == 0 and np.isnan(rnd.norms()[bad])
    # the restatement over the other rows alone, the denominator still K
    keep = [k for k in range(case.K) if k != bad]
    alone, _ = cf.finish_of(cf.chain_of(x[keep], case.last, c[keep]), case.last, case.K)
    assert np.array_equal(alone.view(np.uint32), want.view(np.uint32))


def test_two_rounds_with_noise_draw_different_normals(gpu_device):
    from fedscale_amd import kernels as kx

    case = _case("fedavg_mixed_k7")  # P = 155, odd: the offset moves on by round_up(P, 2)
    assert case.P % 2 == 1
    M, nm, seed = case.bounds["between"], 0.5, 77
    sigma = float(nm * M / case.K)
    adapter = case.adapter()
    cols = (case.P + 3) // 4 * 4
    last, zs = case.last, []
    for r in range(2):
        offset = r * (case.P + 1)
        assert adapter.clip_noise_offset == offset
        z = torch.empty(cols, dtype=torch.float32, device=gpu_device)
        kx.dp_normals(z, seed, offset)  # the device's own draws at the round's seed and offset
        zs.append(z.cpu().numpy()[:case.P])
        want, _ = _restate(case.x, last, M, case.K, sigma, zs[-1])
        rnd = _run_round(case, adapter, M, noise=nm, seed=seed)
        assert rnd.noise_offset == offset and rnd.sigma == sigma
        got = adapter.get_weights()
        _assert_fp32_entries(case, got, want, ("noise round", r))
        plain, _ = _restate(case.x, last, M, case.K)
        assert (plain != want).sum() > case.P // 2  # the noise is really in the model
        last = want  # the next round starts from this model
    assert adapter.clip_noise_offset == 2 * (case.P + 1)
    assert (zs[0] != zs[1]).sum() > case.P - 4 and abs(float(np.std(zs[0])) - 1) < 0.3


def test_mixin_end_to_end(gpu_device):
    from fedscale_amd.clip_round import ClippedRound
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator

    case = _case("fedavg_femnist_cnn_k10")
    M = case.bounds["between"]

    class ClippedAggregator(DeviceAggregator):
        device_clip_norm = M
        device_round_capacity = 4

    want, _ = _restate(case.x, case.last, M, case.K, sq=case.sq)
    adapter = case.adapter()
    agg = ClippedAggregator(adapter, case.sc.args())
    agg.start_round(case.K)
    for k in range(case.K):
        agg.on_result({"client_id": k + 1, "update_weight": case.upload(k, "dict" if k % 2 else "list"),
                       "moving_loss": 1.0})
        if k == 0:
            assert type(agg._device_round) is ClippedRound and agg._device_round.cap == 4
    assert agg._device_round is None
    _assert_fp32_entries(case, adapter.get_weights(), want, "mixin")
    mean = list(agg.model_weights)  # without a server step the clipped mean IS the new model
    _assert_fp32_entries(case, [torch.from_numpy(np.asarray(a)) for a in mean], want, "model_weights")


@pytest.mark.parametrize("name", NAMES)
def test_an_adapter_without_clip_is_what_it_was(gpu_device, name):
    from fedscale_amd.round import DeviceRound

    sc = Scenario(name)
    adapter = _case(name).adapter()
    K = sc.meta["rounds"][0]
    rnd = adapter.begin_round(K, "fedavg")
    assert type(rnd) is DeviceRound and adapter.clip_noise_offset == 0
    for k in range(K):
        rnd.add(sc.client(k))
    adapter.apply_round(rnd, float(np.float32(K)), float(K))
    assert_state_equal(adapter.get_weights(), sc.expected(0), name)
    assert adapter.clip_noise_offset == 0
