"""Krum / Multi-Krum rounds end to end on the MI355X: ``TorchModelAdapter.begin_round(krum=...)`` and the aggregator
mixin with ``device_krum`` against the numpy restatement of tests/krum_fixtures.py, on a small model with fp32
parameters, BatchNorm buffers and an int64 ``num_batches_tracked``.  The integer-valued round (one upload scaled by
2^50, one all NaN, one sign-flipped and scaled by 8) is exact everywhere: scores, kept set and model bit for bit.  The
non-integer round is compared bit for bit in the model once the reference scores have shown a gap at the cut that the
Gram's summation order cannot close."""
import numpy as np
import pytest
import torch

from tests import krum_fixtures as kf

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


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


def _honest(case):
    h = np.ones(case.K, dtype=bool)
    h[list(case.bad)] = False
    return h


def test_integer_round_through_begin_round(gpu_device):
    from fedscale_amd.krum_round import KrumRound, KrumSpec
    from fedscale_amd.round import DeviceRound

    case = kf.Case(11)
    want = kf.krum_round(case.x, case.L, case.P, 3, 8)
    assert np.array_equal(want["c"] != 0, _honest(case)) and np.isfinite(want["out"]).all()
    adapter = case.adapter()
    rnd = _run(case, adapter, krum=3)
    assert type(rnd) is KrumRound and rnd.policy == "fedavg" and (rnd.f, rnd.m) == (3, 8) and rnd.krum == KrumSpec(3)
    got = adapter.get_weights()
    _assert_model(case, got, want["out"], "krum=3")
    assert np.array_equal(rnd.selected(), _honest(case)) and rnd.selected().dtype == np.bool_
    assert np.array_equal(_bits64(rnd.scores()), _bits64(want["score"])) and rnd.scores().dtype == np.float64
    assert rnd.n_selected == want["n_sel"] == 8 and rnd.rejected == 1
    G = rnd.gram()
    fin = np.isfinite(want["G"])
    assert G.shape == (11, 11) and np.array_equal(_bits64(G[fin]), _bits64(want["G"][fin])) and fin.sum() == 100
    mean = case.flat([np.asarray(a) for a in adapter.round_mean_weights()])  # no server step: the mean IS the model
    assert np.array_equal(_bits(mean), _bits(want["out"]))
    # the plain round on the same uploads is not finite
    plain = case.adapter()
    assert type(_run(case, plain)) is DeviceRound
    assert not np.isfinite(case.flat_of_weights(plain.get_weights())).all()


def test_integer_round_through_the_mixin(gpu_device):
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator
    from fedscale_amd.krum_round import KrumRound

    case = kf.Case(11)
    want = kf.krum_round(case.x, case.L, case.P, 3, 8)

    class KrumAggregator(DeviceAggregator):
        device_krum = 0.3  # floor(0.3 * 11) = 3

    adapter = case.adapter()
    agg = KrumAggregator(adapter)
    agg.start_round(case.K)
    rnd = None
    for k in range(case.K):
        agg.on_result({"client_id": k + 1, "update_weight": case.upload(k, "dict" if k % 2 else "list"),
                       "moving_loss": 1.0})
        if k == 0:
            rnd = agg._device_round
            assert type(rnd) is KrumRound and (rnd.f, rnd.m) == (3, 8)
    assert agg._device_round is None
    _assert_model(case, adapter.get_weights(), want["out"], "mixin")
    assert np.array_equal(rnd.selected(), _honest(case)) and rnd.n_selected == 8
    mean = [torch.from_numpy(np.asarray(a)) for a in agg.model_weights]
    assert np.array_equal(_bits(case.flat_of_weights(mean)), _bits(want["out"]))


def test_krum_proper_keeps_one_upload(gpu_device):
    case = kf.Case(11)
    want = kf.krum_round(case.x, case.L, case.P, 3, 1)
    adapter = case.adapter()
    rnd = _run(case, adapter, krum=(3, 1))
    assert (rnd.f, rnd.m) == (3, 1) and rnd.n_selected == 1
    best = int(np.flatnonzero(rnd.selected())[0])
    assert rnd.selected().sum() == 1 and _honest(case)[best] and best == int(np.flatnonzero(want["c"])[0])
    _assert_model(case, adapter.get_weights(), want["out"], "m=1")
    assert np.array_equal(_bits(want["out"]), _bits(case.x[best]))  # L + (x - L) / 1 on integers: the upload itself


def test_non_integer_round(gpu_device):
    from fedscale_amd.krum_round import KrumSpec

    case = kf.nonint_case()
    K, f, m = kf.NONINT
    d = kf.diffs(case.x, case.L, case.P)
    ref = kf.krum_round(case.x, case.L, case.P, f, m, G=kf.gram_fsum(d))
    sc = np.sort(ref["score"])
    bound = kf.score_bound(d, f).max()
    print("score gap at the cut:", float(sc[m] - sc[m - 1]), "bound:", float(bound))
    assert sc[m] - sc[m - 1] > 1000 * bound > 0  # the kept set cannot depend on the Gram's summation order
    adapter = case.adapter()
    rnd = _run(case, adapter, krum=KrumSpec(f, m))
    assert np.array_equal(rnd.selected(), ref["c"] != 0) and rnd.n_selected == m
    assert not rnd.selected()[list(case.bad)].any()
    assert (np.abs(rnd.scores() - ref["score"]) <= kf.score_bound(d, f)).all()
    assert (np.abs(rnd.gram() - ref["G"]) <= kf.gram_bound(d)).all()
    _assert_model(case, adapter.get_weights(), ref["out"], "non-integer")  # chain and finish: bit-defined
    # and the rest of the round is the restatement continued from the device's own Gram, bit for bit
    cont = kf.krum_round(case.x, case.L, case.P, f, m, G=rnd.gram())
    assert np.array_equal(_bits64(rnd.scores()), _bits64(cont["score"]))


def test_fed_yogi_on_the_selected_mean(gpu_device):
    """The selected mean feeds the existing YoGi step: the new model is fa_yogi_step's on the restated mean."""
    from fedscale_amd import kernels as kx
    from tests.golden_io import Scenario

    case = kf.Case(11)
    args = Scenario("fedyogi_mixed_3rounds").args()
    want_mean = kf.krum_round(case.x, case.L, case.P, 3, 8)["out"]
    adapter = case.adapter(policy="fed-yogi", args=args)
    _run(case, adapter, krum=3)
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
    """The second round on the same adapter (and staging) starts from the first's model and sees nothing of its
    scores."""
    first = kf.Case(11)
    adapter = first.adapter()
    r1 = _run(first, adapter, krum=3)
    w1 = kf.krum_round(first.x, first.L, first.P, 3, 8)
    _assert_model(first, adapter.get_weights(), w1["out"], "round 1")
    # the second round's uploads are the first's moved by the model's own movement: the same integer updates
    L2 = w1["out"]
    second = kf.Case(11)
    shift = (L2 - first.L).astype(np.float32)
    second.x = (first.x + shift).astype(np.float32)
    second.L = L2
    for k in range(11):
        for e in second.layout.f_entries:
            second.uploads[k][e.index] = second.x[k, e.offset:e.offset + e.numel].reshape(e.shape).copy()
    r2 = _run(second, adapter, krum=(3, 5))
    w2 = kf.krum_round(second.x, L2, second.P, 3, 5)
    _assert_model(second, adapter.get_weights(), w2["out"], "round 2")
    assert r1.staging is r2.staging and r2.generation == r1.generation + 1
    assert r2.n_selected == w2["n_sel"] == 5 and r1.n_selected == 8
    assert np.array_equal(_bits64(r2.scores()), _bits64(kf.scores_of(r2.gram(), 3)))


def test_a_round_above_the_capacity_is_refused(gpu_device):
    case = kf.Case(11)
    adapter = case.adapter()
    with pytest.raises(ValueError, match="all K=11 uploads resident.*capacity is 4"):
        adapter.begin_round(11, "fedavg", capacity=4, krum=3)
    assert adapter.staging is None  # refused before anything was allocated or launched
    small = case.adapter(capacity=10)
    with pytest.raises(ValueError, match="all K=11 uploads resident.*capacity is 10"):
        small.begin_round(11, "fedavg", krum=(3, 1))
    assert small.staging is None
    with pytest.raises(ValueError, match=r"2f \+ 3 <= K"):
        adapter.begin_round(8, "fedavg", krum=3)
    with pytest.raises(ValueError, match="m <= K - f"):
        adapter.begin_round(11, "fedavg", krum=(3, 9))
    assert adapter.staging is None
    rnd = _run(case, adapter, capacity=11, krum=3)  # the same adapter still runs a round that fits
    _assert_model(case, adapter.get_weights(), kf.krum_round(case.x, case.L, case.P, 3, 8)["out"], "after refusals")
    assert rnd.cap == 11


def test_refused_combinations_on_a_real_adapter(gpu_device):
    from fedscale_amd.clip_round import ClipSpec
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    case = kf.Case(11)
    adapter = case.adapter()
    for kw, what in ((dict(clip=ClipSpec(3.0)), "clip"), (dict(trim=1), "trim"), (dict(signatures=True), "cohort")):
        with pytest.raises(NotImplementedError, match=f"krum.*{what}"):
            adapter.begin_round(11, "fedavg", krum=3, **kw)
    for policy in ("fedbuff", "qfedavg"):
        with pytest.raises(NotImplementedError, match=f"krum.*{policy} round"):
            adapter.begin_round(11, policy, krum=3)
    assert adapter.staging is None
    half = TorchModelAdapter(case.net(), device="cuda:0", upload_dtype="bfloat16")
    with pytest.raises(NotImplementedError, match="krum.*upload_dtype='bfloat16'"):
        half.begin_round(11, "fedavg", krum=3)
    assert half.staging is None
    q = TorchModelAdapter(case.net(), device="cuda:0", upload_quant="mxfp8")
    with pytest.raises(NotImplementedError, match="krum.*upload_quant"):
        q.begin_round(11, "fedavg", krum=3)
    assert q.staging is None
    # a finished round refuses a second finalize and a wrong denominator
    rnd = adapter.begin_round(11, "fedavg", krum=3)
    for k in range(11):
        rnd.add(case.upload(k))
    with pytest.raises(ValueError, match=r"float32\(K\)"):
        adapter.apply_round(rnd, 5.0, 5.0)
