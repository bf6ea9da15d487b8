"""Trimmed-mean aggregation without a device: the numpy restatement of include/fedtrim.h against independent numpy
(np.sort, np.median, the FedAvg chain), ``ft_plan`` (a host-only entry point of the built library) against its Python
restatement, the shapes the GPU tests rely on, ``TrimSpec`` validation, and the combinations that are refused — each
before a device is touched."""
import math
import types

import numpy as np
import pytest

from tests import trim_fixtures as tf

CUS = (16, 64, 256, 304)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the restatement -----------------------------------------------------------------------------------------------
def test_order_key_is_the_documented_total_order():
    v = np.asarray([-np.inf, -1e15, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 1e15, np.inf], dtype=np.float32)
    k = tf.keys_of(v)
    assert (np.diff(k.astype(np.int64)) > 0).all() and k.min() > 0
    assert (tf.keys_of(tf.NANS) == 0xFFFFFFFF).all() and k.max() < 0xFFFFFFFF
    assert tf.keys_of(np.asarray([0.0], dtype=np.float32))[0] == 0x80000000


@pytest.mark.parametrize("K,t", [(3, 1), (4, 1), (5, 2), (9, 4), (10, 3), (33, 16), (40, 16), (40, 7)])
def test_kept_multiset_equals_the_sorted_middle(K, t):
    rng = np.random.default_rng(100 * K + t)
    P = 4000
    x = tf.tied_rows(rng, K, P, P, nan_share=0.08)
    x[:t + 1, ::10] = np.nan  # every tenth column holds more NaNs than the trim removes
    lo, hi, ties = tf.select_of(x, t)
    out, dropped, kept = tf.reduce_of(x, t, lo, hi, ties)
    key = tf.keys_of(x)
    assert (kept.sum(axis=0) == K - 2 * t).all()
    assert (lo != hi).any() and (K - 2 * t > 2 or (lo == hi).any())  # the heavy ties reach the lo == hi case
    got = np.sort(np.where(kept, key, 0), axis=0)[2 * t:]  # key 0 never occurs: the dropped sort first
    assert np.array_equal(got, np.sort(key, axis=0)[t:K - t])
    assert dropped.sum() == 2 * t * P and (dropped.sum(axis=0) == t * P).all()
    nans = np.isnan(x).sum(axis=0)
    assert (nans > t).any() and (nans <= t).any()
    assert np.isnan(out[nans > t]).all()  # more NaNs than the trim: honestly NaN
    clean = (nans <= t) & ~(np.isposinf(x).any(axis=0) & np.isneginf(x).any(axis=0))
    assert not np.isnan(out[clean]).any()  # NaNs are trimmed first from the top
    # the chain of the kept rows in arrival order, one column at a time
    for p in range(0, P, 97):
        rows = [x[k, p] for k in range(K) if kept[k, p]]
        c = rows[0]
        with np.errstate(all="ignore"):
            for r in rows[1:]:
                c = np.float32(c + r)
            want = np.float32(c) / np.float32(K - 2 * t)
        assert _bits(np.float32(want)) == _bits(out[p:p + 1]) or (np.isnan(want) and np.isnan(out[p]))


@pytest.mark.parametrize("K", [1, 2, 7, 40])
def test_t0_is_the_fedavg_chain(K):
    rng = np.random.default_rng(K)
    for x in (tf.tied_rows(rng, K, 500, 500, nan_share=0.0), tf.normal_rows(rng, K, 500, 500)):
        out, dropped = tf.trimmed_mean(x, 0)
        assert np.array_equal(_bits(out), _bits(tf.fedavg_of(x))) and dropped.sum() == 0
    neg = np.full((K, 4), -0.0, dtype=np.float32)
    assert (_bits(tf.trimmed_mean(neg, 0)[0]) == 0x80000000).all()  # the chain starts from x_0, not from +0


@pytest.mark.parametrize("K", [3, 4, 9, 10, 33, 34])
def test_median_equals_numpy(K):
    rng = np.random.default_rng(7 * K)
    t = (K - 1) // 2
    for x in (tf.normal_rows(rng, K, 3000, 3000), np.abs(tf.tied_rows(rng, K, 3000, 3000, nan_share=0.0))):
        x[np.isinf(x)] = 1e15  # (inf - inf cannot occur; -0 became +0: numpy's sort does not order the two zeros)
        out, _ = tf.trimmed_mean(x, t)
        assert np.array_equal(_bits(out), _bits(np.median(x, axis=0)))


def test_worked_example():
    x = np.asarray([[1, 5, np.nan, -0.0, 2], [2, 5, 1, 0.0, 2], [1e15, 5, 2, 0.0, 2], [3, 5, 3, -0.0, 2],
                    [-7, 5, np.nan, 7, 1]], dtype=np.float32)
    lo, hi, ties = tf.select_of(x, 1)
    assert list(lo[:2]) == list(tf.keys_of(np.asarray([-7, 5], dtype=np.float32)))
    assert list(hi[:3]) == [tf.keys_of(np.asarray([1e15], dtype=np.float32))[0], lo[1], 0xFFFFFFFF]
    assert list(ties) == [0x10001] * 5
    out, dropped, kept = tf.reduce_of(x, 1, lo, hi, ties)
    assert list(out[:2]) == [2.0, 5.0]
    # column 2 holds two NaNs against t = 1: NaN; column 3: -0 dropped low (row 0), 7 dropped high, +0 +0 -0 kept
    assert np.isnan(out[2]) and _bits(out[3:4])[0] == 0 and out[4] == 2.0
    assert kept[:, 1].tolist() == [False, False, True, True, True]  # ties: first come, first dropped, low then high
    assert dropped.tolist() == [[2, 2], [1, 1], [0, 1], [0, 0], [2, 1]]


# ---- the plan ------------------------------------------------------------------------------------------------------
def _sweep():
    ps = {0, 25_000_000, 25_557_032, 1 << 20, 100_000_000} | set(tf.SMALL_P)
    for cus in CUS:
        for geo in (tf.NARROW, tf.DEEP):
            for f in (tf.p_two_levels, tf.p_level0, tf.p_capped):
                p = f(cus, geo)
                ps.update({p - 1, p, p + 1})
    return sorted(ps)


def test_plan_equals_the_restatement():
    from fedscale_amd import kernels_trim as kt

    for cus in CUS:
        for P in _sweep():
            for K, t in ((1, 0), (3, 1), (5, 2), (9, 3), (1000, 4), (11, 5), (17, 8), (33, 16), (1000, 16)):
                assert kt.plan(cus, K, P, t) == tf.plan(cus, K, P, t), (cus, K, P, t)


def test_plans_cover_every_column_once():
    for cus in CUS:
        for P in _sweep():
            for kernel, T in (("select", 16), ("select", 4), ("reduce", 0)):
                launches = tf.plan(cus, 33, P, 16) if T == 16 else tf.plan(cus, 9, P, 4)
                col = 0
                for l in tf.of_kernel(launches, kernel):
                    assert l["col0"] == col and 1 <= l["grid"] <= l["tiles"]
                    col += l["tiles"] * tf.WAVES * l["V"] * tf.STRIP
                assert col >= P and (P == 0) == (col == 0), (cus, P, kernel)


def test_shapes_of_the_gpu_tests_take_the_paths_they_are_listed_for():
    for cus in CUS:
        seen = set()
        for name, K, t, P, tag in tf.shapes(cus):
            geo = tf.DEEP if tag == "deep" else tf.NARROW
            T = tf.depth_of(t)
            assert (T >= 8) == (tag == "deep") and 2 * t < K
            want_p, want = tf.expected_launches(cus, geo)[name.split("_T")[0]]
            assert want_p == P
            launches = tf.plan(cus, K, P, t)
            sel = [(l["V"], l["U"], l["col0"], l["tiles"], l["grid"]) for l in tf.of_kernel(launches, "select")]
            assert sel == want and {l["T"] for l in tf.of_kernel(launches, "select")} == {T}, (cus, name)
            red = [(l["V"], l["U"], l["col0"], l["tiles"], l["grid"]) for l in tf.of_kernel(launches, "reduce")]
            if tag == "narrow":
                assert red == want, (cus, name)
            seen.update((l["kernel"], l["T"], l["V"], l["U"]) for l in launches)
            if name.startswith("capped"):
                assert all(l["tiles"] == 2 * l["grid"] for l in tf.of_kernel(launches, "select"))
            if name.startswith("level0"):
                assert P % (tf.WAVES * geo["levels"][0][0] * tf.STRIP) != 0  # the last tile is ragged
        # every instantiation of both kernels is run by some shape: every T at every level of its geometry
        for T in tf.DEPTHS:
            for v, u in set((tf.DEEP if T >= 8 else tf.NARROW)["levels"]):
                assert ("select", T, v, u) in seen, (cus, T, v, u)
        for v, u in tf.NARROW["levels"]:
            assert ("reduce", 0, v, u) in seen
        for P in tf.SMALL_P:  # the small widths: level 2 alone
            assert {(l["V"], l["U"]) for l in tf.plan(cus, 3, P, 1)} == {(1, 8)}
            assert {(l["V"], l["U"]) for l in tf.plan(cus, 33, P, 16)} == {(1, 8), (1, 4)}
    cases = tf.row_cases()
    assert {(1, 0), (2, 0), (3, 1), (33, 16), (34, 16), (31, 15), (32, 15), (17, 1), (9, 0)} <= set(cases)
    assert {tf.depth_of(t) for _, t in cases if t} == set(tf.DEPTHS) and all(2 * t < K for K, t in cases)


def test_bad_plan_arguments_are_refused():
    from fedscale_amd import _native_trim as nt
    from fedscale_amd._native import FedAggError

    buf = np.zeros(8 * nt.PLAN_FIELDS, dtype=np.int64)
    d = buf.ctypes.data
    for args in ((0, 3, 10, 1, d, 8), (-4, 3, 10, 1, d, 8), (8, -1, 10, 0, d, 8), (8, 3, -10, 1, d, 8),
                 (8, 3, 10, -1, d, 8), (8, 3, 10, 1, d, -1), (8, 3, 10, 1, None, 8), (8, 2, 10, 1, d, 8),
                 (8, 0, 10, 0, d, 8), (8, 32, 10, 16, d, 8), (8, 100, 10, 17, d, 8)):
        with pytest.raises(FedAggError, match="ft_plan.*nothing was launched"):
            nt.call("ft_plan", *args)
    with pytest.raises(FedAggError, match=r"2t < K"):
        nt.call("ft_plan", 8, 2, 10, 1, d, 8)
    with pytest.raises(FedAggError, match=r"ft_max_trim\(\)=16"):
        nt.call("ft_plan", 8, 100, 10, 17, d, 8)
    assert nt.call("ft_plan", 8, 3, 10, 1, None, 0) == 2  # the count alone
    assert nt.call("ft_plan", 8, 3, 0, 1, None, 0) == 0 and nt.call("ft_plan", 8, 1, 10, 0, d, 8) == 1


def test_binding_lists_every_symbol_of_the_header():
    import os
    import re

    from fedscale_amd import _native_trim as nt
    from fedscale_amd import buildinfo, kernels_trim

    with open(os.path.join(buildinfo.ROOT, "include", "fedtrim.h")) as f:
        text = f.read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t)\s+(ft_\w+)\(", text, flags=re.M))
    assert declared == set(nt.SIGNATURES) and len(declared) == 5
    for name, value in (("FT_ABI_VERSION", nt.ABI_VERSION), ("FT_MAX_TRIM", nt.MAX_TRIM),
                        ("FT_PLAN_FIELDS", nt.PLAN_FIELDS), ("FT_KERNEL_SELECT", nt.KERNEL_SELECT),
                        ("FT_KERNEL_REDUCE", nt.KERNEL_REDUCE)):
        assert re.search(rf"^#define {name} +{value}\b", text, flags=re.M), name
    assert "fedscale_amd/csrc/trim_reduce.hip" in buildinfo.SRCS and "include/fedtrim.h" in buildinfo.HDRS
    assert nt.load().ft_abi_version() == nt.ABI_VERSION
    assert kernels_trim.max_trim() == nt.MAX_TRIM == tf.MAX_TRIM == max(tf.DEPTHS)


# ---- TrimSpec and the refusals -------------------------------------------------------------------------------------
def test_trim_spec_validates_on_construction():
    from fedscale_amd.trim_round import TrimSpec

    assert TrimSpec(0).trim == 0 and TrimSpec(np.int64(3)).trim == 3 and type(TrimSpec(np.int64(3)).trim) is int
    assert TrimSpec(0.25).trim == 0.25 and type(TrimSpec(np.float32(0.25)).trim) is float
    assert TrimSpec("median").trim == "median" and TrimSpec(TrimSpec(2)) == TrimSpec(2) and TrimSpec(0) != TrimSpec(0.0)
    for bad in (True, False, np.True_, -1, 0.5, -0.1, 1.0, float("nan"), float("inf"), "mean", "", None, [1], (1,)):
        with pytest.raises(ValueError, match="TrimSpec"):
            TrimSpec(bad)
    s = TrimSpec(2)
    with pytest.raises(AttributeError):
        s.trim = 3
    assert repr(s) == "TrimSpec(2)"


def test_trim_spec_count():
    from fedscale_amd.trim_round import TrimSpec

    assert [TrimSpec(2).count(K) for K in (5, 6, 1000)] == [2, 2, 2] and TrimSpec(0).count(1) == 0
    assert [TrimSpec("median").count(K) for K in (1, 2, 3, 4, 9, 10, 33, 34)] == [0, 0, 1, 1, 4, 4, 16, 16]
    assert [TrimSpec(0.2).count(K) for K in (1, 4, 5, 10, 14, 80)] == [0, 0, 1, 2, 2, 16]
    assert TrimSpec(0.1).count(30) == int(math.floor(0.1 * 30)) and TrimSpec(0.0).count(1) == 0
    assert TrimSpec(0.3).count(10) == 3 and TrimSpec(0.16).count(100) == 16
    for spec, K in ((TrimSpec(1), 2), (TrimSpec(2), 4), (TrimSpec(16), 32)):
        with pytest.raises(ValueError, match="2t < K"):
            spec.count(K)
    for spec, K in ((TrimSpec(17), 100), (TrimSpec("median"), 35), (TrimSpec(0.2), 85)):
        with pytest.raises(ValueError, match=r"ft_max_trim\(\) = 16"):
            spec.count(K)
    with pytest.raises(ValueError, match="K >= 1"):
        TrimSpec(0).count(0)


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
    from fedscale_amd.trim_round import TrimmedRound, TrimSpec

    check = TorchModelAdapter._check_trim
    for form in (2, 0.2, "median", TrimSpec(2)):
        assert isinstance(check(_stub(), "fedavg", False, None, form), TrimSpec)  # the accepted forms
    assert check(_stub(optimizer=types.SimpleNamespace(mode="fed-yogi")), "fedavg", False, None, 2) == TrimSpec(2)
    with pytest.raises(NotImplementedError, match="trim.*clip"):
        check(_stub(), "fedavg", False, ClipSpec(3.0), 2)
    with pytest.raises(NotImplementedError, match="trim.*upload_dtype='bfloat16'"):
        check(_stub(upload_dtype="bfloat16"), "fedavg", False, None, 2)
    with pytest.raises(NotImplementedError, match="trim.*cohort signatures"):
        check(_stub(), "fedavg", True, None, 2)
    with pytest.raises(NotImplementedError, match="trim.*shard"):
        check(_stub(shards=types.SimpleNamespace(world=2)), "fedavg", False, None, 2)
    with pytest.raises(NotImplementedError, match="trim.*parameter-sharded layout"):
        check(_stub(layout=types.SimpleNamespace(world=2)), "fedavg", False, None, 2)
    for policy in ("fedbuff", "qfedavg"):
        with pytest.raises(NotImplementedError, match=f"trim.*{policy} round"):
            check(_stub(), policy, False, None, 2)
    with pytest.raises(NotImplementedError, match="trim.*q-fedavg server optimizer"):
        check(_stub(optimizer=types.SimpleNamespace(mode="q-fedavg")), "fedavg", False, None, 2)
    with pytest.raises(ValueError, match="TrimSpec"):
        check(_stub(), "fedavg", False, None, True)
    # begin_round itself refuses before it looks at a staging area or a device
    me = _stub(_check_trim=lambda *a: check(_stub(), *a))
    with pytest.raises(NotImplementedError, match="trim.*fedbuff round"):
        TorchModelAdapter.begin_round(me, 4, "fedbuff", trim=1)
    with pytest.raises(NotImplementedError, match="trim.*clip"):
        TorchModelAdapter.begin_round(me, 4, "fedavg", clip=ClipSpec(3.0), trim=1)
    with pytest.raises(ValueError, match="2t < K"):
        TorchModelAdapter.begin_round(me, 4, "fedavg", trim=2)
    with pytest.raises(NotImplementedError, match="trim.*ShardedModelAdapter"):
        ShardedModelAdapter.begin_round(types.SimpleNamespace(parts=[0, 1]), 4, "fedavg", trim=1)
    # a round above the capacity: refused before the staging is made (the stub has none to make)
    me = _stub(_check_trim=lambda *a: check(_stub(), *a), staging=None, staging_capacity=None,
               shards=types.SimpleNamespace(world=1, shards_clients=False))
    with pytest.raises(ValueError, match="all K=10 uploads resident.*capacity is 4"):
        TorchModelAdapter.begin_round(me, 10, "fedavg", capacity=4, trim=2)
    # the round's own checks
    lay, stg = types.SimpleNamespace(world=1), types.SimpleNamespace(capacity=4)
    with pytest.raises(NotImplementedError, match="trim.*fedbuff round"):
        TrimmedRound(lay, "cpu", 4, TrimSpec(1), staging=stg, policy="fedbuff")
    with pytest.raises(NotImplementedError, match="trim.*parameter-sharded layout"):
        TrimmedRound(types.SimpleNamespace(world=2), "cpu", 4, TrimSpec(1), staging=stg)
    with pytest.raises(TypeError, match="TrimSpec"):
        TrimmedRound(lay, "cpu", 4, 1, staging=stg)
    with pytest.raises(ValueError, match="K >= 1"):
        TrimmedRound(lay, "cpu", 0, TrimSpec(0), staging=stg)
    with pytest.raises(ValueError, match="all K=5 uploads resident.*capacity is 4"):
        TrimmedRound(lay, "cpu", 5, TrimSpec(1), staging=stg)
    with pytest.raises(ValueError, match="all K=4 uploads resident.*capacity is 3"):
        TrimmedRound(lay, "cpu", 4, TrimSpec(1), staging=stg, capacity=3)


def test_mixin_passes_device_trim_through():
    from fedscale_amd.cloud.aggregation import aggregator as agg
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.trim_round import TrimSpec

    assert agg.DeviceAggregatorMixin.device_trim is None and agg.DeviceAsyncAggregatorMixin.device_trim is None
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
            obj.start_round(3)
        if hasattr(obj, "client_task_model_version"):
            obj.client_task_model_version[1] = 0
        obj.on_result({"client_id": 1, "update_weight": {}}, *([0] if a else []))
        return obj

    class A(agg.DeviceAggregator):
        pass

    first_result(A)
    assert calls[-1] == (3, "fedavg", dict(capacity=None, keep_mean=True))  # unset: the call is what it was
    for form in (1, 0.25, "median"):
        class B(agg.DeviceAggregator):
            device_trim = form

        first_result(B)
        K, policy, kw = calls[-1]
        assert (K, policy) == (3, "fedavg") and kw.pop("trim") == TrimSpec(form)
        assert kw == dict(capacity=None, keep_mean=True)

    class Bad(agg.DeviceAggregator):
        device_trim = True

    with pytest.raises(ValueError, match="TrimSpec"):
        first_result(Bad)
    n = len(calls)
    for attrs, what in ((dict(device_clip_norm=3.0), "device_clip_norm"),
                        (dict(device_upload_dtype="float16"), "device_upload_dtype='float16'"),
                        (dict(device_shards=[0, 1]), "device_shards")):
        C = type("C", (agg.DeviceAggregator,), dict(device_trim=1, **attrs))
        with pytest.raises(NotImplementedError, match=f"trim.*{what}"):
            first_result(C)
    assert len(calls) == n  # refused before begin_round

    class Async(agg.DeviceAsyncAggregator):
        device_trim = 1

    c = Async(Wrapper())
    c.start_round(3)
    c.client_task_model_version[1] = 0
    with pytest.raises(NotImplementedError, match="trim.*DeviceAsyncAggregatorMixin"):
        c.on_result({"client_id": 1, "update_weight": {}})
    assert c.aggregation_denominator == 0  # refused before any state moved

    class Cohort(agg.DeviceCohortAggregator):
        device_trim = "median"

    d = Cohort([Wrapper()], [3])
    with pytest.raises(NotImplementedError, match="trim.*DeviceCohortAggregatorMixin"):
        d.on_result({"client_id": 1, "update_weight": {}}, 0)
