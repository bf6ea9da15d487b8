"""Geometric-median (RFA) rounds end to end on the MI355X: ``TorchModelAdapter.begin_round(geomed=...)`` and the
aggregator mixin with ``device_geomed`` against the numpy restatement of tests/geomed_fixtures.py, on a small model with
fp32 parameters, BatchNorm buffers and an int64 ``num_batches_tracked``.  The Gram method on the integer-valued round
(one upload scaled by 2^50, one all NaN, one sign-flipped and scaled by 8) is exact everywhere; otherwise the rounds
are compared bit for bit with the restatement continued from the device's own Gram (``method="gram"``) or streamed
squared distances (``method="stream"``), which are themselves held to their derived any-order bounds."""
import argparse

import numpy as np
import pytest
import torch

from tests import geomed_fixtures as gf
from tests import krum_fixtures as kf

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NU = 1e-6


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same64(got, want, what):
    """Equal bits wherever the restatement is finite, non-finite wherever it is not."""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    bad = np.argwhere(got[fin].view(np.uint64) != want[fin].view(np.uint64))
    assert bad.size == 0, (what, bad[:5], got[fin][bad[:5, 0]], want[fin][bad[:5, 0]])
    assert not np.isfinite(got[~fin]).any(), what


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


def _assert_readouts(rnd, want, what):
    _same64(rnd.weights(), want["w"], (what, "weights"))
    _same64(rnd.objective(), want["obj"], (what, "objective"))
    _same64(rnd.dist2(), want["q"], (what, "dist2"))
    _same64(rnd.start_dist2(), want["q0"], (what, "start_dist2"))
    assert rnd.n_valid == want["n_valid"] and rnd.rejected == rnd.K - want["n_valid"], what
    assert rnd.weights().dtype == F64 and rnd.objective().shape == (rnd.iters,)
    assert rnd.dist2().shape == (rnd.iters, rnd.K)


def _continued(case, rnd):
    """The restatement continued from what the device itself summed: its Gram, or its streamed squared distances."""
    if rnd.method == "gram":
        return gf.geomed_round(case.x, case.L, case.P, rnd.iters, rnd.nu, "gram", G=rnd.gram())
    hist = np.concatenate([rnd.start_dist2()[None, :], rnd.dist2()], axis=0)
    return gf.geomed_round(case.x, case.L, case.P, rnd.iters, rnd.nu, "stream", q_hist=hist)


def _assert_streamed_distances(case, rnd, cont):
    """Every streamed squared distance is within the any-order bound of the fsum reference against the very iterate
    the restatement (continued from the device's distances, so bit-equal iterates) holds at that step."""
    P = case.P
    ref0 = gf.sqnorms_ref(case.x, case.L, P)
    fin = np.isfinite(ref0)
    assert (np.abs(rnd.start_dist2()[fin] - ref0[fin]) <= gf.sqnorm_bound(ref0[fin], P)).all()
    worst = 0.0
    for t in range(rnd.iters):
        ref = gf.sqnorms_ref(case.x, cont["z"][t], P)
        err, bound = np.abs(rnd.dist2()[t][fin] - ref[fin]), gf.sqnorm_bound(ref[fin], P)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (t, float((err / bound).max()))
        assert not np.isfinite(rnd.dist2()[t][~fin]).any()
    print("streamed dist2 error / bound, max:", worst)
    return ref0


# ---- the integer round -----------------------------------------------------------------------------------------------
def test_integer_gram_round_through_begin_round(gpu_device):
    from fedscale_amd.geomed_round import GeoMedRound, GeoMedSpec
    from fedscale_amd.round import DeviceRound

    case = kf.Case(11)
    spec = GeoMedSpec(3, NU, "gram")
    want = gf.geomed_round(case.x, case.L, case.P, 3, NU, "gram")
    assert np.isfinite(want["out"]).all() and want["n_valid"] == 10
    adapter = case.adapter()
    rnd = _run(case, adapter, geomed=spec)
    assert type(rnd) is GeoMedRound and rnd.policy == "fedavg" and rnd.method == "gram" and rnd.geomed == spec
    assert (rnd.iters, rnd.nu) == (3, NU)
    G = rnd.gram()
    fin = np.isfinite(want["G"])
    assert G.shape == (11, 11) and fin.sum() == 100
    assert np.array_equal(G[fin].view(np.uint64), want["G"][fin].view(np.uint64))  # the Gram is exact
    _assert_model(case, adapter.get_weights(), want["out"], "gram")
    _assert_readouts(rnd, want, "gram")
    assert rnd.n_valid == 10 and rnd.rejected == 1
    w = rnd.weights()
    assert w[5] == 0 and w[2] * 2.0 ** 50 < 1 and abs(w.sum() - 1) < 1e-12
    mean = case.flat([np.asarray(a) for a in adapter.round_mean_weights()])  # no server step: the mean IS the model
    assert np.array_equal(_bits(mean), _bits(want["out"]))
    # the plain round on the same uploads is not finite
    plain = case.adapter()
    assert type(_run(case, plain)) is DeviceRound
    assert not np.isfinite(case.flat_of_weights(plain.get_weights())).all()


def test_integer_gram_round_through_the_mixin(gpu_device):
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator
    from fedscale_amd.geomed_round import GeoMedRound, GeoMedSpec

    case = kf.Case(11)
    want = gf.geomed_round(case.x, case.L, case.P, 3, NU, "gram")

    class GeoMedAggregator(DeviceAggregator):
        device_geomed = GeoMedSpec(3, NU, "gram")

    adapter = case.adapter()
    agg = GeoMedAggregator(adapter)
    agg.start_round(case.K)
    rnd = None
    for k in range(case.K):
        agg.on_result({"client_id": k + 1, "update_weight": case.upload(k, "dict" if k % 2 else "list"),
                       "moving_loss": 1.0})
        if k == 0:
            rnd = agg._device_round
            assert type(rnd) is GeoMedRound and rnd.method == "gram" and rnd.iters == 3
    assert agg._device_round is None
    _assert_model(case, adapter.get_weights(), want["out"], "mixin")
    _assert_readouts(rnd, want, "mixin")
    mean = [torch.from_numpy(np.asarray(a)) for a in agg.model_weights]
    assert np.array_equal(_bits(case.flat_of_weights(mean)), _bits(want["out"]))


def test_integer_stream_round(gpu_device):
    from fedscale_amd.geomed_round import GeoMedSpec

    case = kf.Case(11)
    adapter = case.adapter()
    rnd = _run(case, adapter, geomed=GeoMedSpec(3, NU, "stream"))
    assert rnd.method == "stream"
    with pytest.raises(RuntimeError, match="no Gram"):
        rnd.gram()
    cont = _continued(case, rnd)
    ref0 = _assert_streamed_distances(case, rnd, cont)
    fin = np.isfinite(ref0)
    assert np.array_equal(rnd.start_dist2()[fin].view(np.uint64), ref0[fin].view(np.uint64))  # integers: exact
    _assert_model(case, adapter.get_weights(), cont["out"], "stream")
    _assert_readouts(rnd, cont, "stream")
    assert rnd.n_valid == 10 and rnd.rejected == 1 and np.isfinite(cont["out"]).all()
    # and the Gram method's model is within the bound the issue sets for the two methods
    gram = gf.geomed_round(case.x, case.L, case.P, 3, NU, "gram")
    ulps = gf.ulps32(cont["out"], gram["out"], np.abs(case.L).max())
    print("stream (device) vs gram (restated):", ulps, "ulp")
    assert ulps <= gf.METHODS_TOL_ULPS


# ---- non-integer rounds ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("method", ["gram", "stream"])
def test_non_integer_round(gpu_device, method, lazy):
    from fedscale_amd.geomed_round import GeoMedSpec

    case = gf.lazy_case() if lazy else kf.nonint_case()
    adapter = case.adapter()
    rnd = _run(case, adapter, geomed=GeoMedSpec(4, NU, method))
    assert rnd.method == method and rnd.n_valid == case.K and rnd.rejected == 0
    cont = _continued(case, rnd)
    _assert_model(case, adapter.get_weights(), cont["out"], (method, lazy))
    _assert_readouts(rnd, cont, (method, lazy))
    if method == "gram":
        d = kf.diffs(case.x, case.L, case.P)
        assert (np.abs(rnd.gram() - kf.gram_fsum(d)) <= kf.gram_bound(d)).all()
    else:
        _assert_streamed_distances(case, rnd, cont)
    obj = rnd.objective()
    scale = np.abs(case.L).max()
    print(method, "lazy" if lazy else "plain", "objective", obj)
    assert np.isfinite(obj).all() and (np.diff(obj) <= 0).all() and obj[-1] < obj[0]
    ref, _ = gf.weiszfeld_fp64(case.x, case.L, case.P, 4, NU)
    ulps = gf.ulps32(case.flat_of_weights(adapter.get_weights()), ref, scale)
    print("vs the fp64 Weiszfeld:", ulps, "ulp")
    assert ulps <= gf.WEISZFELD_TOL_ULPS


# ---- auto ------------------------------------------------------------------------------------------------------------
def test_auto_resolves_by_k_and_iters(gpu_device):
    """K = 11 takes the Gram; K = 40 at one iteration (12 * 3 = 36 < 40) streams — rows written on the device and
    adopted, as tools/geomed_measure.py does — and both are the restatement continued from the device's sums."""
    from fedscale_amd.bucket import BucketLayout, ClientStaging
    from fedscale_amd.geomed_round import GeoMedRound, GeoMedSpec

    case = kf.Case(11)
    adapter = case.adapter()
    rnd = _run(case, adapter, geomed=True)
    assert rnd.geomed == GeoMedSpec() and rnd.method == "gram" == GeoMedSpec().resolve(11) and rnd.iters == 4
    _assert_model(case, adapter.get_weights(), _continued(case, rnd)["out"], "auto, K = 11")
    K, P = 40, 1000
    spec = GeoMedSpec(1)
    assert spec.resolve(K) == "stream" and spec.resolve(36) == "gram"
    L = BucketLayout(["w"], [(P,)], [torch.float32])
    st = ClientStaging(L, gpu_device, K, bulk=False)
    last = torch.zeros(L.ld, device=gpu_device)
    last[:P].normal_(0.0, 1.0)
    st.x[:K, :P].normal_(0.0, 0.05)
    st.x[:K, :P] += last[:P]
    st.x[7, :P] *= 1000.0
    r = GeoMedRound(L, gpu_device, K, spec, staging=st, last_f32=last, capacity=K)
    assert r.method == "stream"
    r.adopt_resident(K)
    out = torch.zeros(L.ld, device=gpu_device)
    side = torch.zeros(L.ldq, dtype=torch.float64, device=gpu_device)
    r.finalize_mean(float(np.float32(K)), float(K), out=out, cur_side=side)
    x, Lh = st.x[:K].cpu().numpy(), last.cpu().numpy()
    hist = np.concatenate([r.start_dist2()[None, :], r.dist2()], axis=0)
    cont = gf.geomed_round(x, Lh, P, 1, spec.nu, "stream", q_hist=hist)
    assert np.array_equal(_bits(out[:P].cpu().numpy()), _bits(cont["out"]))
    _same64(r.weights(), cont["w"], "adopted")
    ref = gf.sqnorms_ref(x, cont["z"][0], P)
    assert (np.abs(r.dist2()[0] - ref) <= gf.sqnorm_bound(ref, P)).all()
    assert r.weights()[7] < 0.1 * r.weights().mean()  # the far upload counts for little


# ---- edge cases ------------------------------------------------------------------------------------------------------
def _edge_case(K, rows):
    case = kf.Case(K, integer=False)
    case.x = rows(case).astype(F32)
    assert case.x.shape == (K, case.P)
    for k in range(K):
        for e in case.layout.f_entries:
            case.uploads[k][e.index] = case.x[k, e.offset:e.offset + e.numel].reshape(e.shape).copy()
    return case


@pytest.mark.parametrize("method", ["gram", "stream"])
def test_edge_cases(gpu_device, method):
    from fedscale_amd.geomed_round import GeoMedSpec

    spec = GeoMedSpec(3, NU, method)
    # K = 1: the upload itself
    case = kf.Case(1, integer=False)
    adapter = case.adapter()
    rnd = _run(case, adapter, geomed=spec)
    got = case.flat_of_weights(adapter.get_weights())
    assert rnd.weights().tolist() == [1.0] and rnd.n_valid == 1
    assert np.array_equal(_bits(got), _bits((case.L + (case.x[0] - case.L)).astype(F32)))
    # K = 2: the midpoint (updates on a grid of 1/4, so both halves are exact)
    grid = np.random.default_rng(4).integers(-4, 5, size=(2, case.P)).astype(F32) * F32(0.25)
    case = _edge_case(2, lambda c: c.L + grid)
    adapter = case.adapter()
    rnd = _run(case, adapter, geomed=spec)
    d = kf.diffs(case.x, case.L, case.P)
    assert rnd.weights().astype(F32).tolist() == [0.5, 0.5]  # (equal up to the rounding noise of the two distances)
    mid = (case.L + (F32(0.5) * d[0] + F32(0.5) * d[1])).astype(F32)
    assert np.array_equal(_bits(case.flat_of_weights(adapter.get_weights())), _bits(mid))
    # all uploads NaN: the model is unchanged
    case = _edge_case(3, lambda c: np.full((3, c.P), np.nan))
    adapter = case.adapter()
    rnd = _run(case, adapter, geomed=spec)
    assert rnd.n_valid == 0 and rnd.rejected == 3 and (rnd.weights() == 0).all()
    assert np.array_equal(_bits(case.flat_of_weights(adapter.get_weights())), _bits(case.L))
    # all uploads equal: the upload (every distance is below nu, so the weights stay equal)
    one = kf.Case(1, integer=False).x[0]
    case = _edge_case(4, lambda c: np.repeat(one[None, :], 4, axis=0))
    adapter = case.adapter()
    rnd = _run(case, adapter, geomed=spec)
    assert rnd.weights().tolist() == [0.25] * 4
    want = _continued(case, rnd)["out"]
    got = case.flat_of_weights(adapter.get_weights())
    assert np.array_equal(_bits(got), _bits(want)) and np.abs(got - one).max() <= np.spacing(np.abs(one).max())


# ---- FedYoGi, back-to-back rounds, refusals --------------------------------------------------------------------------
def test_fed_yogi_on_the_median(gpu_device):
    """The median feeds the existing YoGi step: the new model is fa_yogi_step's on the restated median."""
    from fedscale_amd import kernels as kx
    from fedscale_amd.geomed_round import GeoMedSpec
    from tests.golden_io import Scenario

    case = kf.Case(11)
    args = Scenario("fedyogi_mixed_3rounds").args()
    want_mean = gf.geomed_round(case.x, case.L, case.P, 3, NU, "gram")["out"]
    adapter = case.adapter(policy="fed-yogi", args=args)
    _run(case, adapter, geomed=GeoMedSpec(3, NU, "gram"))
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
    assert not np.array_equal(_bits(got), _bits(want_mean))  # the step really moved the model off the median


def test_two_rounds_back_to_back(gpu_device):
    """The second round on the same adapter (and staging) starts from the first's model, by the other method, and
    sees nothing of the first's weights."""
    from fedscale_amd.geomed_round import GeoMedSpec

    first = kf.Case(11)
    adapter = first.adapter()
    r1 = _run(first, adapter, geomed=GeoMedSpec(3, NU, "gram"))
    w1 = gf.geomed_round(first.x, first.L, first.P, 3, NU, "gram")
    _assert_model(first, adapter.get_weights(), w1["out"], "round 1")
    L2 = w1["out"]
    second = kf.Case(11)
    second.x = (first.x + (L2 - first.L).astype(F32)).astype(F32)
    second.L = L2
    for k in range(11):
        for e in second.layout.f_entries:
            second.uploads[k][e.index] = second.x[k, e.offset:e.offset + e.numel].reshape(e.shape).copy()
    r2 = _run(second, adapter, geomed=GeoMedSpec(2, 1e-3, "stream"))
    assert r1.staging is r2.staging and r2.generation == r1.generation + 1
    cont = _continued(second, r2)
    _assert_model(second, adapter.get_weights(), cont["out"], "round 2")
    _assert_readouts(r2, cont, "round 2")
    _assert_readouts(r1, w1, "round 1, read after round 2")
    assert r2.n_valid == 10 and (r2.iters, r2.nu, r2.method) == (2, 1e-3, "stream")


def test_a_round_above_the_capacity_is_refused(gpu_device):
    case = kf.Case(11)
    adapter = case.adapter()
    with pytest.raises(ValueError, match="all K=11 uploads resident.*capacity is 4"):
        adapter.begin_round(11, "fedavg", capacity=4, geomed=True)
    assert adapter.staging is None  # refused before anything was allocated or launched
    small = case.adapter(capacity=10)
    with pytest.raises(ValueError, match="all K=11 uploads resident.*capacity is 10"):
        small.begin_round(11, "fedavg", geomed=3)
    assert small.staging is None
    with pytest.raises(ValueError, match="FGM_MAX_K"):
        adapter.begin_round(4097, "fedavg", geomed=True)
    assert adapter.staging is None
    rnd = _run(case, adapter, capacity=11, geomed=3)  # the same adapter still runs a round that fits
    _assert_model(case, adapter.get_weights(), _continued(case, rnd)["out"], "after refusals")
    assert rnd.cap == 11


def test_refused_combinations_on_a_real_adapter(gpu_device):
    from fedscale_amd.clip_round import ClipSpec
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    case = kf.Case(11)
    adapter = case.adapter()
    for kw, what in ((dict(clip=ClipSpec(3.0)), "clip"), (dict(trim=1), "trim"), (dict(krum=3), "krum"),
                     (dict(signatures=True), "cohort")):
        with pytest.raises(NotImplementedError, match=f"geomed.*{what}"):
            adapter.begin_round(11, "fedavg", geomed=True, **kw)
    for policy in ("fedbuff", "qfedavg"):
        with pytest.raises(NotImplementedError, match=f"geomed.*{policy} round"):
            adapter.begin_round(11, policy, geomed=True)
    assert adapter.staging is None
    half = TorchModelAdapter(case.net(), device="cuda:0", upload_dtype="bfloat16")
    with pytest.raises(NotImplementedError, match="geomed.*upload_dtype='bfloat16'"):
        half.begin_round(11, "fedavg", geomed=True)
    assert half.staging is None
    q = TorchModelAdapter(case.net(), device="cuda:0", upload_quant="mxfp8")
    with pytest.raises(NotImplementedError, match="geomed.*upload_quant"):
        q.begin_round(11, "fedavg", geomed=True)
    assert q.staging is None
    topk = TorchModelAdapter(case.net(), device="cuda:0", upload_topk=0.1)
    with pytest.raises(NotImplementedError, match="geomed.*upload_topk=0.1"):
        topk.begin_round(11, "fedavg", geomed=True)
    assert topk.staging is None
    qargs = argparse.Namespace(gradient_policy="q-fedavg", yogi_eta=3e-3, yogi_tau=1e-8, yogi_beta=0.9,
                               yogi_beta2=0.99, learning_rate=0.05, qfed_q=1.0)
    qopt = case.adapter(policy="q-fedavg", args=qargs)
    with pytest.raises(NotImplementedError, match="geomed.*q-fedavg server optimizer"):
        qopt.begin_round(11, "fedavg", geomed=True)
    assert qopt.staging is None
    # a wrong denominator, a readout before the finish, and a second finalize
    rnd = adapter.begin_round(11, "fedavg", geomed=3)
    for k in range(11):
        rnd.add(case.upload(k))
    with pytest.raises(RuntimeError, match="not finalized"):
        rnd.weights()
    with pytest.raises(ValueError, match=r"float32\(K\)"):
        adapter.apply_round(rnd, 5.0, 5.0)
    adapter.apply_round(rnd, float(np.float32(11)), 11.0)
    with pytest.raises(RuntimeError, match="already finalized"):
        rnd.finalize_mean(float(np.float32(11)), 11.0, out=torch.zeros(rnd.layout.ld, device=gpu_device),
                          cur_side=torch.zeros(rnd.layout.ldq, dtype=torch.float64, device=gpu_device))
    _assert_model(case, adapter.get_weights(), _continued(case, rnd)["out"], "after the refusals")
