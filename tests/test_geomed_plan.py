"""Geometric-median (RFA) aggregation without a device: the numpy restatement of include/fedgeomed.h against
independent routes (math.fsum, direct squared distances, crafted inputs, a plain fp64 Weiszfeld), the properties the
contract was chosen for (robustness on the poisoned round, a non-increasing objective, the two methods agreeing),
``GeoMedSpec`` validation, and the combinations that are refused — each before a device is touched."""
import math
import types

import numpy as np
import pytest

from tests import geomed_fixtures as gf
from tests import krum_fixtures as kf

F32, F64 = np.float32, np.float64
NU = 1e-6


def _bits64(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


# ---- the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", gf.WEIGHTS_K)
def test_fixed_order_sum_is_exact_on_integers(K):
    v = np.random.default_rng(K).integers(-1000, 1000, size=K).astype(F64)
    assert gf.S(v) == math.fsum(v.tolist())
    assert gf.S(np.zeros(K)) == 0.0 and not np.signbit(gf.S(np.zeros(K)))


def test_fixed_order_sum_has_the_documented_order():
    """Not just any order: 130 values whose sum depends on it, against the lanes and the butterfly written out."""
    v = np.random.default_rng(2).standard_normal(130)
    lanes = [0.0] * 64
    for i, x in enumerate(v.tolist()):
        lanes[i % 64] = lanes[i % 64] + x
    for m in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[i] + lanes[i ^ m] for i in range(64)]
    assert len({float(x) for x in lanes}) == 1 and gf.S(v) == lanes[0]
    seq = 0.0
    for x in v.tolist():
        seq = seq + x
    assert gf.S(v) != seq  # (the data do tell orders apart)


@pytest.mark.parametrize("K,P", [(1, 5), (3, 9), (17, 40), (300, 12)])
def test_gram_dist2_on_integer_data_is_the_direct_squared_distance(K, P):
    """Integer updates, an exact Gram and dyadic weights (multiples of 1/64, some exactly 0, not summing to 1): every
    product and sum of the restatement is exact, so it must equal |d_j - sum_k w_k d_k|^2 computed directly."""
    rng = np.random.default_rng(K * 100 + P)
    d = rng.integers(-3, 4, size=(K, P)).astype(F64)
    G = d @ d.T
    w = rng.integers(0, 5, size=K).astype(F64) / 64.0
    if K > 2:
        w[1] = 0.0
    s = (w[:, None] * d).sum(axis=0)  # multiples of 1/64 below 2^20: exact in any order
    direct = ((d - s) ** 2).sum(axis=1)
    assert np.array_equal(gf.gram_dist2_of(G, w), direct)


def test_gram_dist2_skips_zero_weight_rows():
    G = gf.symmetric(np.random.default_rng(3), 6, integer=True)
    w = np.asarray([0.25, 0.0, 0.5, 0.0, 0.125, 0.125])
    clean = gf.gram_dist2_of(G, w)
    bad = G.copy()
    bad[1, :] = bad[:, 1] = np.nan
    bad[3, :] = bad[:, 3] = np.inf
    got = gf.gram_dist2_of(bad, w)
    keep = np.asarray([0, 2, 4, 5])
    assert np.array_equal(_bits64(got[keep]), _bits64(clean[keep])) and not np.isfinite(got[[1, 3]]).any()


def test_start_picks_the_middle_valid_norm():
    q0 = np.asarray([9.0, np.nan, 4.0, 4.0, np.inf, 1.0, 16.0, -np.inf, 4.0])  # valid sorted: 1 4 4 4 9 16, n = 6
    w, c, n = gf.start_of(q0)
    assert n == 6  # med = sorted[3] = 4
    want = np.asarray([(2.0 / 3.0) / 6, 0, 1 / 6, 1 / 6, 0, 1 / 6, (2.0 / 4.0) / 6, 0, 1 / 6])
    assert np.array_equal(_bits64(w), _bits64(want)) and c.dtype == F32 and np.array_equal(c, want.astype(F32))
    w, c, n = gf.start_of(np.asarray([1.0, 4.0]))  # n = 2: the 1st (0-based) of two, the larger
    assert n == 2 and w.tolist() == [0.5, 0.5]
    w, c, n = gf.start_of(np.asarray([1.0, 4.0, 100.0]))
    assert n == 3 and w.tolist() == [1 / 3, 1 / 3, (2.0 / 10.0) / 3]
    w, c, n = gf.start_of(np.asarray([np.nan, np.inf]))
    assert n == 0 and w.tolist() == [0.0, 0.0] and not np.signbit(w).any()
    w, c, n = gf.start_of(np.asarray([0.0, 0.0, 0.0]))  # all uploads equal to L
    assert n == 3 and w.tolist() == [1 / 3] * 3


def test_weights_on_crafted_distances():
    q = np.asarray([np.nan, np.inf, -1e-30, 0.0, 0.25 * NU * NU, 4.0, -np.inf])
    w, c, obj, n = gf.weights_of(q, NU)
    assert n == 4 and obj == gf.S(np.asarray([0, 0, 0, 0, 0.5 * NU, 2.0, 0]))
    r = np.asarray([0, 0, 1 / NU, 1 / NU, 1 / NU, 0.5, 0])  # the clamped, the zero and the sub-nu distance count as nu
    assert np.array_equal(_bits64(w), _bits64(r / gf.S(r))) and (w[[0, 1, 6]] == 0).all()
    assert abs(w.sum() - 1) < 1e-15 and np.array_equal(c, w.astype(F32))
    w, c, obj, n = gf.weights_of(np.asarray([np.nan, np.inf, -np.inf]), NU)
    assert n == 0 and obj == 0.0 and w.tolist() == [0.0] * 3 and c.tolist() == [0.0] * 3
    w, c, obj, n = gf.weights_of(np.asarray([7.0]), NU)
    assert n == 1 and w.tolist() == [1.0] and obj == math.sqrt(7.0)


# ---- whole rounds --------------------------------------------------------------------------------------------------
def _honest(case):
    h = np.ones(case.K, dtype=bool)
    h[list(case.bad)] = False
    return h


@pytest.mark.parametrize("method", ["gram", "stream"])
def test_poisoned_round_stays_near_the_honest_mean(method):
    case = kf.Case(11)
    r = gf.geomed_round(case.x, case.L, case.P, 3, NU, method)
    assert np.isfinite(r["out"]).all() and r["n_valid"] == 10 and case.K - r["n_valid"] == 1
    assert r["c"][5] == 0 and r["w"][5] == 0  # the NaN upload
    assert r["w"][2] < 1e-12 and r["w"][2] * 2.0 ** 50 < 1  # the 2^50 upload: a weight that undoes its scale
    h = _honest(case)
    d = kf.diffs(case.x, case.L, case.P).astype(F64)
    mean = case.L.astype(F64) + d[h].mean(axis=0)
    alpha = 3 / 11
    bound = 2 * (1 - alpha) / (1 - 2 * alpha) * max(np.linalg.norm(case.x[k].astype(F64) - mean)
                                                    for k in np.flatnonzero(h))
    dist = np.linalg.norm(r["out"].astype(F64) - mean)
    print(f"{method}: distance to the honest mean {dist:.3f}, bound {bound:.2f}")
    assert dist < bound  # (observed: 0.88 against 33.7)
    plain = case.L + (np.nansum(d, axis=0) / 11).astype(F32)
    assert np.abs(plain).max() > 1e10  # what the plain mean of the finite uploads would have been


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("method", ["gram", "stream"])
def test_objective_is_non_increasing(method, lazy):
    case = gf.lazy_case() if lazy else kf.nonint_case()
    assert not lazy or np.array_equal(case.x[0], case.L)
    # The Gram method's iterate is never rounded: R = 8.  The streamed one is an fp32 model, and once a step moves the
    # objective by less than that rounding does (from the fourth step here) the condition is no longer the
    # iteration's to keep: the default R = 4, whose three steps are all above that floor.
    R = 8 if method == "gram" else 4
    obj = gf.geomed_round(case.x, case.L, case.P, R, NU, method)["obj"]
    print(method, "lazy" if lazy else "plain", obj)
    assert np.isfinite(obj).all() and (np.diff(obj) <= 0).all() and obj[-1] < obj[0]


@pytest.mark.parametrize("R", [1, 3, 4, 8])
def test_the_two_methods_agree_and_match_a_plain_weiszfeld(R):
    for name, case in (("integer", kf.Case(11)), ("nonint", kf.nonint_case()), ("lazy", gf.lazy_case())):
        g = gf.geomed_round(case.x, case.L, case.P, R, NU, "gram")
        s = gf.geomed_round(case.x, case.L, case.P, R, NU, "stream")
        scale = np.abs(case.L).max()
        between = gf.ulps32(g["out"], s["out"], scale)
        ref, _ = gf.weiszfeld_fp64(case.x, case.L, case.P, R, NU)
        vs_ref = max(gf.ulps32(g["out"], ref, scale), gf.ulps32(s["out"], ref, scale))
        print(f"{name} R={R}: gram vs stream {between} ulp, vs fp64 Weiszfeld {vs_ref:.3f} ulp")
        assert between <= gf.METHODS_TOL_ULPS
        assert vs_ref <= gf.WEISZFELD_TOL_ULPS


def test_edge_cases():
    rng = np.random.default_rng(8)
    P = 37
    L = rng.standard_normal(P).astype(F32)
    one = (L + rng.standard_normal((1, P)).astype(F32) * F32(0.1)).astype(F32)
    two = (L + rng.integers(-4, 5, size=(2, P)).astype(F32) * F32(0.25)).astype(F32)
    for method in ("gram", "stream"):
        r = gf.geomed_round(one, L, P, 3, NU, method)
        assert r["c"].tolist() == [1.0] and np.array_equal(r["out"], (L + (one[0] - L)).astype(F32))  # K = 1
        r = gf.geomed_round(two, L, P, 3, NU, method)
        assert r["c"].tolist() == [0.5, 0.5]  # K = 2: equal distances to the midpoint, the midpoint again
        nan = np.full((3, P), np.nan, dtype=F32)
        r = gf.geomed_round(nan, L, P, 3, NU, method)
        assert r["n_valid"] == 0 and np.array_equal(r["out"].view(np.uint32), L.view(np.uint32))  # all NaN: L
        same = np.repeat(one, 4, axis=0)
        r = gf.geomed_round(same, L, P, 3, NU, method)
        assert r["c"].tolist() == [0.25] * 4 and np.abs(r["out"] - one[0]).max() <= np.spacing(np.abs(one).max())


def test_shapes_of_the_gpu_tests_meet_their_conditions():
    assert {1, 2, 3, 63, 64, 65, 127, 128, 129, 4095, 4096} == set(gf.WEIGHTS_K)
    assert {1, 2, 3, 64, 65, 255, 256, 257, 513, 4096} == set(gf.DIST2_K) and max(gf.DIST2_K) == gf.MAX_K
    assert {1, 3, 4, 5, 1023, 4097} == set(gf.FINISH_P)
    q = gf.crafted_q(np.random.default_rng(0), 63, NU)
    assert np.isnan(q).sum() == 1 and np.isinf(q).sum() == 2 and (q == 0).sum() == 1 and (q < 0).sum() == 2
    assert ((q > 0) & (q < NU * NU)).sum() == 1


# ---- GeoMedSpec ----------------------------------------------------------------------------------------------------
def test_spec_validates_on_construction():
    from fedscale_amd.geomed_round import GeoMedSpec

    s = GeoMedSpec()
    assert (s.iters, s.nu, s.method) == (4, 1e-6, "auto")
    assert GeoMedSpec(np.int64(3), np.float32(0.5), "gram") == GeoMedSpec(3, 0.5, "gram")
    assert type(GeoMedSpec(np.int64(3)).iters) is int and type(GeoMedSpec(nu=1).nu) is float
    assert GeoMedSpec(GeoMedSpec(2, 1e-3, "stream")) == GeoMedSpec(2, 1e-3, "stream") != GeoMedSpec(2, 1e-3)
    assert hash(GeoMedSpec(2)) == hash(GeoMedSpec(2)) and GeoMedSpec(64).iters == 64
    assert GeoMedSpec.of(True) == GeoMedSpec() and GeoMedSpec.of(7) == GeoMedSpec(7) and GeoMedSpec.of(s) is s
    for bad in (True, False, 0, -1, 65, 1.0, "4", None, [4]):
        with pytest.raises(ValueError, match="GeoMedSpec.*iters"):
            GeoMedSpec(bad)
    for bad in (0, 0.0, -1e-6, float("nan"), float("inf"), "1e-6", None, True):
        with pytest.raises(ValueError, match="GeoMedSpec.*nu"):
            GeoMedSpec(4, bad)
    for bad in ("Gram", "weiszfeld", None, 1):
        with pytest.raises(ValueError, match="GeoMedSpec.*method"):
            GeoMedSpec(4, 1e-6, bad)
    for bad in (False, None, "yes", 2.0):
        with pytest.raises(ValueError, match="GeoMedSpec"):
            GeoMedSpec.of(bad)
    with pytest.raises(AttributeError):
        s.iters = 3
    assert repr(GeoMedSpec(2, 0.5, "gram")) == "GeoMedSpec(iters=2, nu=0.5, method='gram')"


def test_resolve_is_a_function_of_k_and_iters_alone():
    from fedscale_amd.geomed_round import GeoMedSpec

    for R in (1, 3, 4, 64):
        cut = 12 * (1 + 2 * R)
        for K in (1, 2, cut - 1, cut, cut + 1, 1000, 4096):
            if K > 4096:
                continue
            for nu in (1e-6, 3.0):  # nu does not enter
                assert GeoMedSpec(R, nu).resolve(K) == ("gram" if K <= cut else "stream") == gf.resolve(K, R)
            assert GeoMedSpec(R, method="gram").resolve(K) == "gram"
            assert GeoMedSpec(R, method="stream").resolve(K) == "stream"
    assert GeoMedSpec(4).resolve(100) == "gram" and GeoMedSpec(4).resolve(1000) == "stream"
    with pytest.raises(ValueError, match="K >= 1"):
        GeoMedSpec().resolve(0)
    with pytest.raises(ValueError, match="FGM_MAX_K = 4096"):
        GeoMedSpec(method="gram").resolve(4097)


# ---- the refusals --------------------------------------------------------------------------------------------------
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
    from fedscale_amd.geomed_round import GeoMedRound, GeoMedSpec

    check = TorchModelAdapter._check_geomed
    for form, want in ((True, GeoMedSpec()), (3, GeoMedSpec(3)), (GeoMedSpec(2, 1e-3, "stream"),) * 2):
        assert check(_stub(), "fedavg", False, None, None, None, form) == want  # the accepted forms
    yogi = _stub(optimizer=types.SimpleNamespace(mode="fed-yogi"))
    assert check(yogi, "fedavg", False, None, None, None, True) == GeoMedSpec()
    with pytest.raises(NotImplementedError, match="geomed.*clip"):
        check(_stub(), "fedavg", False, ClipSpec(3.0), None, None, True)
    with pytest.raises(NotImplementedError, match="geomed.*trim"):
        check(_stub(), "fedavg", False, None, 1, None, True)
    with pytest.raises(NotImplementedError, match="geomed.*krum"):
        check(_stub(), "fedavg", False, None, None, 1, True)
    with pytest.raises(NotImplementedError, match="geomed.*upload_dtype='bfloat16'"):
        check(_stub(upload_dtype="bfloat16"), "fedavg", False, None, None, None, True)
    with pytest.raises(NotImplementedError, match="geomed.*upload_quant='mxfp8'"):
        check(_stub(upload_quant="mxfp8"), "fedavg", False, None, None, None, True)
    with pytest.raises(NotImplementedError, match="geomed.*upload_topk=0.1"):
        check(_stub(upload_topk=0.1), "fedavg", False, None, None, None, True)
    with pytest.raises(NotImplementedError, match="geomed.*cohort signatures"):
        check(_stub(), "fedavg", True, None, None, None, True)
    with pytest.raises(NotImplementedError, match="geomed.*shard"):
        check(_stub(shards=types.SimpleNamespace(world=2)), "fedavg", False, None, None, None, True)
    with pytest.raises(NotImplementedError, match="geomed.*parameter-sharded layout"):
        check(_stub(layout=types.SimpleNamespace(world=2)), "fedavg", False, None, None, None, True)
    for policy in ("fedbuff", "qfedavg"):
        with pytest.raises(NotImplementedError, match=f"geomed.*{policy} round"):
            check(_stub(), policy, False, None, None, None, True)
    with pytest.raises(NotImplementedError, match="geomed.*q-fedavg server optimizer"):
        check(_stub(optimizer=types.SimpleNamespace(mode="q-fedavg")), "fedavg", False, None, None, None, True)
    with pytest.raises(ValueError, match="GeoMedSpec"):
        check(_stub(), "fedavg", False, None, None, None, False)
    # begin_round itself refuses before it looks at a staging area or a device
    me = _stub(_check_geomed=lambda *a: check(_stub(), *a))
    with pytest.raises(NotImplementedError, match="geomed.*fedbuff round"):
        TorchModelAdapter.begin_round(me, 11, "fedbuff", geomed=True)
    with pytest.raises(NotImplementedError, match="geomed.*clip"):
        TorchModelAdapter.begin_round(me, 11, "fedavg", clip=ClipSpec(3.0), geomed=True)
    with pytest.raises(NotImplementedError, match="geomed.*trim"):
        TorchModelAdapter.begin_round(me, 11, "fedavg", trim=1, geomed=True)
    with pytest.raises(NotImplementedError, match="geomed.*krum"):
        TorchModelAdapter.begin_round(me, 11, "fedavg", krum=1, geomed=True)
    for attr in (dict(upload_topk=0.1), dict(upload_quant="mxfp8")):  # refused before the packed-row branches
        it = _stub(**attr)
        it._check_geomed = lambda *a, it=it: check(it, *a)
        with pytest.raises(NotImplementedError, match="geomed.*upload_"):
            TorchModelAdapter.begin_round(it, 11, "fedavg", geomed=True)
    with pytest.raises(ValueError, match="FGM_MAX_K"):
        TorchModelAdapter.begin_round(me, 4097, "fedavg", geomed=True)
    with pytest.raises(NotImplementedError, match="geomed.*ShardedModelAdapter"):
        ShardedModelAdapter.begin_round(types.SimpleNamespace(parts=[0, 1]), 11, "fedavg", geomed=True)
    # a round above the capacity: refused before the staging is made (the stub has none to make)
    me = _stub(_check_geomed=lambda *a: check(_stub(), *a), staging=None, staging_capacity=None,
               shards=types.SimpleNamespace(world=1, shards_clients=False))
    with pytest.raises(ValueError, match="all K=10 uploads resident.*capacity is 4"):
        TorchModelAdapter.begin_round(me, 10, "fedavg", capacity=4, geomed=2)
    # the round's own checks
    lay, stg = types.SimpleNamespace(world=1), types.SimpleNamespace(capacity=4)
    with pytest.raises(NotImplementedError, match="geomed.*fedbuff round"):
        GeoMedRound(lay, "cpu", 4, GeoMedSpec(), staging=stg, last_f32=None, policy="fedbuff")
    with pytest.raises(NotImplementedError, match="geomed.*parameter-sharded layout"):
        GeoMedRound(types.SimpleNamespace(world=2), "cpu", 4, GeoMedSpec(), staging=stg, last_f32=None)
    with pytest.raises(TypeError, match="GeoMedSpec"):
        GeoMedRound(lay, "cpu", 4, 4, staging=stg, last_f32=None)
    with pytest.raises(ValueError, match="K >= 1"):
        GeoMedRound(lay, "cpu", 0, GeoMedSpec(), staging=stg, last_f32=None)
    with pytest.raises(ValueError, match="all K=5 uploads resident.*capacity is 4"):
        GeoMedRound(lay, "cpu", 5, GeoMedSpec(), staging=stg, last_f32=None)
    with pytest.raises(ValueError, match="all K=4 uploads resident.*capacity is 3"):
        GeoMedRound(lay, "cpu", 4, GeoMedSpec(), staging=stg, last_f32=None, capacity=3)


def test_binding_lists_every_symbol_of_the_header():
    import os
    import re

    from fedscale_amd import _native_geomed as ng
    from fedscale_amd import buildinfo

    with open(os.path.join(buildinfo.ROOT, "include", "fedgeomed.h")) as f:
        text = f.read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t)\s+(fgm_\w+)\(", text, flags=re.M))
    assert declared == set(ng.SIGNATURES) and len(declared) == 6
    for name, value in (("FGM_ABI_VERSION", ng.ABI_VERSION), ("FGM_MAX_K", ng.MAX_K), ("FGM_MAX_ITERS", ng.MAX_ITERS),
                        ("FGM_CHUNK", ng.CHUNK)):
        assert re.search(rf"^#define {name} +{value}\b", text, flags=re.M), name
    assert "fedscale_amd/csrc/geomed.hip" in buildinfo.SRCS and "include/fedgeomed.h" in buildinfo.HDRS
    assert ng.load().fgm_abi_version() == ng.ABI_VERSION
    assert (ng.MAX_K, ng.MAX_ITERS, ng.CHUNK) == (gf.MAX_K, gf.MAX_ITERS, gf.CHUNK)


def test_workspace_bytes_and_bad_arguments():
    """The host-only entry point (no GPU needed) and its refusals."""
    from fedscale_amd import _native_geomed as ng
    from fedscale_amd import kernels_geomed as kg
    from fedscale_amd._native import FedAggError

    for K in (1, 255, 256, 257, 512, 513, 4096):
        assert kg.dist2_workspace_bytes(K) == -(-K // 256) * K * 8
    for K in (0, -1, 4097):
        with pytest.raises(FedAggError, match="fgm_dist2_workspace_bytes.*nothing was launched"):
            ng.call("fgm_dist2_workspace_bytes", K)
    with pytest.raises(FedAggError, match="FGM_MAX_K"):
        ng.call("fgm_dist2_workspace_bytes", 4097)


def test_mixin_passes_device_geomed_through():
    from fedscale_amd.cloud.aggregation import aggregator as agg
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.geomed_round import GeoMedSpec

    assert agg.DeviceAggregatorMixin.device_geomed is None and agg.DeviceAsyncAggregatorMixin.device_geomed is None
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
    for form, want in ((True, GeoMedSpec()), (2, GeoMedSpec(2)), (GeoMedSpec(3, 1e-3, "gram"),) * 2):
        B = type("B", (agg.DeviceAggregator,), dict(device_geomed=form))
        first_result(B)
        K, policy, kw = calls[-1]
        assert (K, policy) == (5, "fedavg") and kw.pop("geomed") == want
        assert kw == dict(capacity=None, keep_mean=True)

    class Bad(agg.DeviceAggregator):
        device_geomed = False

    with pytest.raises(ValueError, match="GeoMedSpec"):
        first_result(Bad)
    n = len(calls)
    for attrs, what in ((dict(device_clip_norm=3.0), "device_clip_norm"), (dict(device_trim=1), "device_trim"),
                        (dict(device_upload_dtype="float16"), "device_upload_dtype='float16'"),
                        (dict(device_upload_quant="mxfp8"), "device_upload_quant='mxfp8'"),
                        (dict(device_upload_topk=0.1), "device_upload_topk=0.1"),
                        (dict(device_shards=[0, 1]), "device_shards")):
        C = type("C", (agg.DeviceAggregator,), dict(device_geomed=True, **attrs))
        with pytest.raises(NotImplementedError, match=f"geomed.*{what}"):
            first_result(C)
    D = type("D", (agg.DeviceAggregator,), dict(device_geomed=True, device_krum=1))
    with pytest.raises(NotImplementedError, match="geomed.*device_krum"):
        first_result(D)
    assert len(calls) == n  # refused before begin_round

    class Async(agg.DeviceAsyncAggregator):
        device_geomed = True

    c = Async(Wrapper())
    c.start_round(5)
    c.client_task_model_version[1] = 0
    with pytest.raises(NotImplementedError, match="geomed.*DeviceAsyncAggregatorMixin"):
        c.on_result({"client_id": 1, "update_weight": {}})
    assert c.aggregation_denominator == 0  # refused before any state moved

    class Cohort(agg.DeviceCohortAggregator):
        device_geomed = 2

    d = Cohort([Wrapper()], [5])
    with pytest.raises(NotImplementedError, match="geomed.*DeviceCohortAggregatorMixin"):
        d.on_result({"client_id": 1, "update_weight": {}}, 0)
