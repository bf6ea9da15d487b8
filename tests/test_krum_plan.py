"""Krum / Multi-Krum aggregation without a device: the numpy restatement of include/fedkrum.h against independent
routes (direct squared distances, a brute-force score loop, a crafted round), ``fk_gram_plan`` and
``fk_gram_workspace_bytes`` (host-only entry points of the built library) against their Python restatement, the shapes
the GPU tests rely on, ``KrumSpec`` validation, and the combinations that are refused — each before a device is
touched."""
import math
import types

import numpy as np
import pytest

from tests import krum_fixtures as kf


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,P", [(3, 1), (5, 7), (17, 100), (40, 333)])
def test_dist2_on_integer_data_is_the_direct_squared_distance(K, P):
    rng = np.random.default_rng(K * 1000 + P)
    x, L = kf.int_rows(rng, K, P, P + 4)
    d = kf.diffs(x, L, P)
    assert np.abs(d).max() <= 3 and (x[:, :P] == L[:P] + d).all() and np.isnan(x[:, P:]).all()
    G = kf.gram_ref(d)
    assert np.array_equal(G, kf.gram_fsum(d)) and np.array_equal(G, G.T)  # fsum is exact where the sum is
    di = d.astype(np.int64)
    direct = ((di[:, None, :] - di[None, :, :]) ** 2).sum(axis=2).astype(np.float64)
    d2 = kf.dist2_of(G)
    off = ~np.eye(K, dtype=bool)
    assert np.array_equal(d2[off], direct[off]) and np.isposinf(np.diag(d2)).all()


def test_dist2_clamps_and_maps_nan():
    G = np.asarray([[1.0, 2.0, np.nan], [2.0, 1.0, 0.5], [np.nan, 0.5, np.inf]])
    d2 = kf.dist2_of(G)
    assert d2[0, 1] == 0.0 and not np.signbit(d2[0, 1])  # v = -2: clamped to +0
    assert np.isposinf(d2[0, 2]) and np.isposinf(d2[1, 2]) and np.isposinf(d2[2, 1])  # NaN and inf - ... -> +inf


@pytest.mark.parametrize("K", [3, 4, 9, 30])
def test_scores_match_a_brute_force(K):
    rng = np.random.default_rng(K)
    x, L = kf.normal_rows(rng, K, 50, 52)
    d = kf.diffs(x, L, 50)
    d[1] = d[0]  # a tie: two equal rows
    G = kf.gram_ref(d)
    G[K - 1, :] = G[:, K - 1] = np.nan
    for f in range(0, (K - 3) // 2 + 1):
        a, b = kf.scores_of(G, f), kf.scores_brute(G, f)
        assert np.array_equal(_bits64(a), _bits64(b)), (K, f)
        assert np.isposinf(a[K - 1])
        assert np.isfinite(a[:K - 1]).all()  # the NaN row is among the f + 1 entries every other row leaves out


def test_select_breaks_ties_by_arrival_and_never_keeps_inf():
    sc = np.asarray([2.0, 1.0, 2.0, np.inf, 1.0, 0.5, np.inf])
    c, n = kf.select_of(sc, 3)
    assert c.tolist() == [0, 1, 0, 0, 1, 1, 0] and n == 3
    c, n = kf.select_of(sc, 4)
    assert c.tolist() == [1, 1, 0, 0, 1, 1, 0] and n == 4  # of the two 2.0, the earlier arrival
    c, n = kf.select_of(sc, 7)
    assert c.tolist() == [1, 1, 1, 0, 1, 1, 0] and n == 5  # fewer finite scores than m
    c, n = kf.select_of(np.full(4, np.inf), 2)
    assert c.tolist() == [0, 0, 0, 0] and n == 0
    L = np.asarray([1.5, -2.0, 0.0], dtype=np.float32)
    assert np.array_equal(kf.finish_of(np.ones(3, dtype=np.float32), L, 0).view(np.uint32), L.view(np.uint32))


def test_crafted_round_keeps_exactly_the_honest_rows():
    rng = np.random.default_rng(3)
    P = 182
    L = rng.integers(-4, 5, size=P).astype(np.float32)
    x, bad = kf.poisoned_int_round(rng, 11, P, L)
    r = kf.krum_round(x, L, P, 3, 8)
    honest = np.ones(11, dtype=bool)
    honest[list(bad)] = False
    assert np.array_equal(r["c"] != 0, honest) and r["n_sel"] == 8
    assert np.isposinf(r["score"][5]) and np.isfinite(r["score"][[2, 8]]).all()
    assert r["score"][honest].max() < r["score"][[2, 8]].min()
    d = kf.diffs(x, L, P)
    want = (L + d[honest].astype(np.float64).sum(axis=0) / 8).astype(np.float32)  # integer sums: exact in any order
    assert np.array_equal(r["out"].view(np.uint32), want.view(np.uint32))
    # Krum proper (m = 1) keeps the single best-scored honest row
    r1 = kf.krum_round(x, L, P, 3, 1)
    assert r1["n_sel"] == 1 and honest[int(np.flatnonzero(r1["c"])[0])]
    assert int(np.flatnonzero(r1["c"])[0]) == int(np.lexsort((np.arange(11), r["score"]))[0])


def test_non_integer_round_data_has_a_safe_selection_gap():
    """The data of test_gpu_krum_round's non-integer round: the gap between the m-th and (m+1)-th reference score
    exceeds 1000 x the derived error bound of a score, so the kept set cannot depend on the Gram's summation order."""
    case = kf.nonint_case()
    x, L, P = case.x, case.L, case.P
    K, f, m = kf.NONINT
    assert x.shape == (K, P) and not (x == np.rint(x)).all()
    d = kf.diffs(x, L, P)
    sc = np.sort(kf.scores_of(kf.gram_fsum(d), f))
    bound = kf.score_bound(d, f).max()
    assert np.isfinite(sc[:m + 1]).all() and sc[m] - sc[m - 1] > 1000 * bound > 0, (sc[m] - sc[m - 1], bound)


# ---- the plan ------------------------------------------------------------------------------------------------------
def _sweep():
    ks = (1, 2, 3, 63, 64, 65, 100, 128, 129, 1000, 2896, 2897, 4095, 4096)
    ps = (0, 1, 31, 32, 33, 127, 128, 129, 300, 301, 3001, 20_000, 1 << 20, 25_000_000, 25_557_032, 100_000_000)
    return [(K, P) for K in ks for P in ps]


def test_plan_and_workspace_equal_the_restatement():
    from fedscale_amd import kernels_krum as kk

    for K, P in _sweep():
        p = kk.gram_plan(K, P)
        assert p == kf.plan(K, P), (K, P)
        assert kk.gram_workspace_bytes(K, P) == kf.workspace_bytes(K, P) == p["nsplit"] * K * K * 8
        assert kk.gram_workspace_bytes(K, P) <= kf.MAX_WS  # the documented cap
        steps = max(1, -(-P // 32))
        per = p["split_cols"] // 32
        assert p["split_cols"] % 32 == 0 and (p["nsplit"] - 1) * per < steps <= p["nsplit"] * per  # no empty split
        assert 1 <= p["last_steps"] <= per and p["row_tile"] == 64 and p["step_cols"] == 32
        T = -(-K // 64)
        assert p["tiles"] == T * (T + 1) // 2


def test_plan_is_a_function_of_k_and_p_alone():
    """fk_gram_plan takes (K, P) and nothing else — no CU count, no device: the same answer before and after other
    plans were asked for, and without a GPU in the process."""
    from fedscale_amd import _native_krum as nk
    from fedscale_amd import kernels_krum as kk

    assert nk.SIGNATURES["fk_gram_plan"][1] == [nk._i32, nk._i64, nk._c_void_p]
    first = [kk.gram_plan(K, P) for K, P in _sweep()]
    assert first == [kk.gram_plan(K, P) for K, P in reversed(_sweep())][::-1]


def test_shapes_of_the_gpu_tests_meet_their_conditions():
    assert max(kf.GRAM_K) <= 200 and max(kf.GRAM_P) <= 20_000 and kf.NONINT_SHAPE[0] <= 200
    assert {3, 16, 17, 64, 65} <= set(kf.GRAM_K)
    assert any(kf.plan(K, 1)["tiles"] >= 6 for K in kf.GRAM_K)  # three row tiles: the tile (2, 1) is off the diagonal
    assert {1, 3, 4, 5, kf.STEP - 1, kf.STEP, kf.STEP + 1} <= set(kf.GRAM_P)
    for K in kf.GRAM_K:
        p = kf.plan(K, kf.P_SPLIT)
        per = p["split_cols"] // p["step_cols"]
        assert p["nsplit"] >= 2 and 2 <= p["last_steps"] < per, (K, p)
        assert kf.P_SPLIT % p["step_cols"] != 0 and kf.P_SPLIT % 4 != 0  # a ragged last step and a ragged float4
    p = kf.plan(*kf.NONINT_SHAPE)
    assert p["nsplit"] >= 2 and p["split_cols"] // p["step_cols"] >= 2
    assert {3, 63 + 1, 65, 66, 256, 257, 258, 512, 513, 514, 4095, 4096} <= set(kf.SCORE_K) and max(kf.SCORE_K) == kf.MAX_K


def test_bad_plan_arguments_are_refused():
    from fedscale_amd import _native_krum as nk
    from fedscale_amd._native import FedAggError

    buf = np.zeros(nk.PLAN_FIELDS, dtype=np.int64)
    for args in ((0, 10, buf.ctypes.data), (-1, 10, buf.ctypes.data), (4097, 10, buf.ctypes.data),
                 (3, -1, buf.ctypes.data), (3, 10, None)):
        with pytest.raises(FedAggError, match="fk_gram_plan.*nothing was launched"):
            nk.call("fk_gram_plan", *args)
    for args in ((0, 10), (4097, 10), (3, -1)):
        with pytest.raises(FedAggError, match="fk_gram_workspace_bytes.*nothing was launched"):
            nk.call("fk_gram_workspace_bytes", *args)
    with pytest.raises(FedAggError, match="FK_MAX_K"):
        nk.call("fk_gram_workspace_bytes", 4097, 10)


def test_binding_lists_every_symbol_of_the_header():
    import os
    import re

    from fedscale_amd import _native_krum as nk
    from fedscale_amd import buildinfo

    with open(os.path.join(buildinfo.ROOT, "include", "fedkrum.h")) as f:
        text = f.read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t)\s+(fk_\w+)\(", text, flags=re.M))
    assert declared == set(nk.SIGNATURES) and len(declared) == 7
    for name, value in (("FK_ABI_VERSION", nk.ABI_VERSION), ("FK_MAX_K", nk.MAX_K), ("FK_PLAN_FIELDS", nk.PLAN_FIELDS)):
        assert re.search(rf"^#define {name} +{value}\b", text, flags=re.M), name
    assert "fedscale_amd/csrc/krum_gram.hip" in buildinfo.SRCS and "include/fedkrum.h" in buildinfo.HDRS
    assert nk.load().fk_abi_version() == nk.ABI_VERSION and nk.MAX_K == kf.MAX_K


# ---- KrumSpec and the refusals -------------------------------------------------------------------------------------
def test_krum_spec_validates_on_construction():
    from fedscale_amd.krum_round import KrumSpec

    s = KrumSpec(2)
    assert (s.f, s.m) == (2, None) and KrumSpec(np.int64(3), np.int64(1)).m == 1 and type(KrumSpec(np.int64(3)).f) is int
    assert KrumSpec(0.25).f == 0.25 and type(KrumSpec(np.float32(0.25)).f) is float
    assert KrumSpec(KrumSpec(2, 1)) == KrumSpec(2, 1) and KrumSpec(0) != KrumSpec(0.0) and KrumSpec(2) != KrumSpec(2, 1)
    assert hash(KrumSpec(2, 1)) == hash(KrumSpec(2, 1))
    for bad in (True, False, np.True_, -1, 0.5, -0.1, 1.0, float("nan"), float("inf"), "krum", None, [1], (1, 2)):
        with pytest.raises(ValueError, match="KrumSpec"):
            KrumSpec(bad)
    for bad in (0, -1, True, 1.0, "1"):
        with pytest.raises(ValueError, match="KrumSpec.*m="):
            KrumSpec(1, bad)
    with pytest.raises(AttributeError):
        s.f = 3
    assert repr(KrumSpec(2, 1)) == "KrumSpec(2, m=1)"


def test_krum_spec_counts():
    from fedscale_amd.krum_round import KrumSpec

    assert KrumSpec(0).counts(3) == (0, 3) and KrumSpec(3).counts(11) == (3, 8) and KrumSpec(3, 1).counts(11) == (3, 1)
    assert KrumSpec(0.3).counts(11) == (int(math.floor(0.3 * 11)), 8) and KrumSpec(0.0).counts(3) == (0, 3)
    assert KrumSpec(4).counts(11) == (4, 7) and KrumSpec(2046).counts(4096) == (2046, 2050)
    for spec, K in ((KrumSpec(0), 2), (KrumSpec(1), 4), (KrumSpec(5), 12), (KrumSpec(0.49), 20)):
        with pytest.raises(ValueError, match=r"2f \+ 3 <= K"):
            spec.counts(K)
    with pytest.raises(ValueError, match="m <= K - f"):
        KrumSpec(3, 9).counts(11)
    with pytest.raises(ValueError, match="FK_MAX_K = 4096"):
        KrumSpec(1).counts(4097)
    with pytest.raises(ValueError, match="K >= 1"):
        KrumSpec(0).counts(0)


def _stub(**kw):
    base = dict(upload_dtype=None, shards=types.SimpleNamespace(world=1), layout=types.SimpleNamespace(world=1),
                optimizer=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_refused_combinations_name_the_combination():
    """Every refusal is a NotImplementedError naming the combination, raised before a device is touched (the stubs
    have none)."""
    from fedscale_amd.clip_round import ClipSpec
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.krum_round import KrumRound, KrumSpec

    check = TorchModelAdapter._check_krum
    for form, want in ((2, KrumSpec(2)), (0.2, KrumSpec(0.2)), ((2, 1), KrumSpec(2, 1)), ([2, 1], KrumSpec(2, 1)),
                       (KrumSpec(2, 3), KrumSpec(2, 3))):
        assert check(_stub(), "fedavg", False, None, None, form) == want  # the accepted forms
    assert check(_stub(optimizer=types.SimpleNamespace(mode="fed-yogi")), "fedavg", False, None, None, 2) == KrumSpec(2)
    with pytest.raises(NotImplementedError, match="krum.*clip"):
        check(_stub(), "fedavg", False, ClipSpec(3.0), None, 2)
    with pytest.raises(NotImplementedError, match="krum.*trim"):
        check(_stub(), "fedavg", False, None, 1, 2)
    with pytest.raises(NotImplementedError, match="krum.*upload_dtype='bfloat16'"):
        check(_stub(upload_dtype="bfloat16"), "fedavg", False, None, None, 2)
    with pytest.raises(NotImplementedError, match="krum.*upload_quant='mxfp8'"):
        check(_stub(upload_quant="mxfp8"), "fedavg", False, None, None, 2)
    with pytest.raises(NotImplementedError, match="krum.*upload_topk=0.1"):
        check(_stub(upload_topk=0.1), "fedavg", False, None, None, 2)
    with pytest.raises(NotImplementedError, match="krum.*cohort signatures"):
        check(_stub(), "fedavg", True, None, None, 2)
    with pytest.raises(NotImplementedError, match="krum.*shard"):
        check(_stub(shards=types.SimpleNamespace(world=2)), "fedavg", False, None, None, 2)
    with pytest.raises(NotImplementedError, match="krum.*parameter-sharded layout"):
        check(_stub(layout=types.SimpleNamespace(world=2)), "fedavg", False, None, None, 2)
    for policy in ("fedbuff", "qfedavg"):
        with pytest.raises(NotImplementedError, match=f"krum.*{policy} round"):
            check(_stub(), policy, False, None, None, 2)
    with pytest.raises(NotImplementedError, match="krum.*q-fedavg server optimizer"):
        check(_stub(optimizer=types.SimpleNamespace(mode="q-fedavg")), "fedavg", False, None, None, 2)
    with pytest.raises(ValueError, match="KrumSpec"):
        check(_stub(), "fedavg", False, None, None, True)
    # begin_round itself refuses before it looks at a staging area or a device
    me = _stub(_check_krum=lambda *a: check(_stub(), *a))
    with pytest.raises(NotImplementedError, match="krum.*fedbuff round"):
        TorchModelAdapter.begin_round(me, 11, "fedbuff", krum=1)
    with pytest.raises(NotImplementedError, match="krum.*clip"):
        TorchModelAdapter.begin_round(me, 11, "fedavg", clip=ClipSpec(3.0), krum=1)
    with pytest.raises(NotImplementedError, match="krum.*trim"):
        TorchModelAdapter.begin_round(me, 11, "fedavg", trim=1, krum=1)
    for attr in (dict(upload_topk=0.1), dict(upload_quant="mxfp8")):  # refused before the packed-row branches
        it = _stub(**attr)
        it._check_krum = lambda *a, it=it: check(it, *a)
        with pytest.raises(NotImplementedError, match="krum.*upload_"):
            TorchModelAdapter.begin_round(it, 11, "fedavg", krum=1)
    with pytest.raises(ValueError, match=r"2f \+ 3 <= K"):
        TorchModelAdapter.begin_round(me, 4, "fedavg", krum=1)
    with pytest.raises(NotImplementedError, match="krum.*ShardedModelAdapter"):
        ShardedModelAdapter.begin_round(types.SimpleNamespace(parts=[0, 1]), 11, "fedavg", krum=1)
    # a round above the capacity: refused before the staging is made (the stub has none to make)
    me = _stub(_check_krum=lambda *a: check(_stub(), *a), staging=None, staging_capacity=None,
               shards=types.SimpleNamespace(world=1, shards_clients=False))
    with pytest.raises(ValueError, match="all K=10 uploads resident.*capacity is 4"):
        TorchModelAdapter.begin_round(me, 10, "fedavg", capacity=4, krum=2)
    # the round's own checks
    lay, stg = types.SimpleNamespace(world=1), types.SimpleNamespace(capacity=4)
    with pytest.raises(NotImplementedError, match="krum.*fedbuff round"):
        KrumRound(lay, "cpu", 4, KrumSpec(0), staging=stg, last_f32=None, policy="fedbuff")
    with pytest.raises(NotImplementedError, match="krum.*parameter-sharded layout"):
        KrumRound(types.SimpleNamespace(world=2), "cpu", 4, KrumSpec(0), staging=stg, last_f32=None)
    with pytest.raises(TypeError, match="KrumSpec"):
        KrumRound(lay, "cpu", 4, 1, staging=stg, last_f32=None)
    with pytest.raises(ValueError, match="K >= 1"):
        KrumRound(lay, "cpu", 0, KrumSpec(0), staging=stg, last_f32=None)
    with pytest.raises(ValueError, match="all K=5 uploads resident.*capacity is 4"):
        KrumRound(lay, "cpu", 5, KrumSpec(1), staging=stg, last_f32=None)
    with pytest.raises(ValueError, match="all K=4 uploads resident.*capacity is 3"):
        KrumRound(lay, "cpu", 4, KrumSpec(0), staging=stg, last_f32=None, capacity=3)


def test_mixin_passes_device_krum_through():
    from fedscale_amd.cloud.aggregation import aggregator as agg
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.krum_round import KrumSpec

    assert agg.DeviceAggregatorMixin.device_krum is None and agg.DeviceAsyncAggregatorMixin.device_krum is None
    calls = []

    class Wrapper(TorchModelAdapter):
        optimizer = None

        def __init__(self):
            pass

        def begin_round(self, K, policy, **kw):
            calls.append((K, policy, kw))
            return types.SimpleNamespace(policy="fedavg", add=lambda u: None, n=0)

    def first_result(cls, *a):
        obj = cls(*(a or (Wrapper(),)))
        if not a:
            obj.start_round(5)
        if hasattr(obj, "client_task_model_version"):
            obj.client_task_model_version[1] = 0
        obj.on_result({"client_id": 1, "update_weight": {}}, *([0] if a else []))
        return obj

    class A(agg.DeviceAggregator):
        pass

    first_result(A)
    assert calls[-1] == (5, "fedavg", dict(capacity=None, keep_mean=True))  # unset: the call is what it was
    for form, want in ((1, KrumSpec(1)), (0.25, KrumSpec(0.25)), ((1, 1), KrumSpec(1, 1)), (KrumSpec(1, 2), KrumSpec(1, 2))):
        B = type("B", (agg.DeviceAggregator,), dict(device_krum=form))
        first_result(B)
        K, policy, kw = calls[-1]
        assert (K, policy) == (5, "fedavg") and kw.pop("krum") == want
        assert kw == dict(capacity=None, keep_mean=True)

    class Bad(agg.DeviceAggregator):
        device_krum = True

    with pytest.raises(ValueError, match="KrumSpec"):
        first_result(Bad)
    n = len(calls)
    for attrs, what in ((dict(device_clip_norm=3.0), "device_clip_norm"), (dict(device_trim=1), "device_trim"),
                        (dict(device_upload_dtype="float16"), "device_upload_dtype='float16'"),
                        (dict(device_upload_quant="mxfp8"), "device_upload_quant='mxfp8'"),
                        (dict(device_upload_topk=0.1), "device_upload_topk=0.1"),
                        (dict(device_shards=[0, 1]), "device_shards")):
        C = type("C", (agg.DeviceAggregator,), dict(device_krum=1, **attrs))
        with pytest.raises(NotImplementedError, match=f"krum.*{what}"):
            first_result(C)
    assert len(calls) == n  # refused before begin_round

    class Async(agg.DeviceAsyncAggregator):
        device_krum = 1

    c = Async(Wrapper())
    c.start_round(5)
    c.client_task_model_version[1] = 0
    with pytest.raises(NotImplementedError, match="krum.*DeviceAsyncAggregatorMixin"):
        c.on_result({"client_id": 1, "update_weight": {}})
    assert c.aggregation_denominator == 0  # refused before any state moved

    class Cohort(agg.DeviceCohortAggregator):
        device_krum = (1, 1)

    d = Cohort([Wrapper()], [5])
    with pytest.raises(NotImplementedError, match="krum.*DeviceCohortAggregatorMixin"):
        d.on_result({"client_id": 1, "update_weight": {}}, 0)
