"""Norm-clipped aggregation without a device: ``fcl_reduce_plan`` and ``fcl_norm_plan`` (host-only entry points of
the built library) against their Python restatements, the shapes the GPU tests rely on, ``ClipSpec`` validation, the
combinations that are refused — each before a device is touched — and the mixin's three attributes."""
import types

import numpy as np
import pytest
import torch

from tests import clip_fixtures as cf

CUS = (8, 64, 256, 304)


def _sweep():
    ps = {0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099, 16383, 16384, 16385, 65536, 1 << 20, 25_000_000,
          25_557_032, 100_000_000}
    for cus in CUS:
        for f in (cf.p_two_levels, cf.p_level0, cf.p_capped):
            p = f(cus)
            ps.update({p - 1, p, p + 1})
        cap = cus * cf.CAP_PCT // 100
        t = (cap * 85 + 99) // 100
        ps.update({(64 * t - 64) * cf.STRIP, (64 * t - 64) * cf.STRIP + 1})  # either side of the level-0 threshold
        ps.update({16 * cus * cf.STRIP - 1, 16 * cus * cf.STRIP, 16 * cus * cf.STRIP + 1})  # ... and of level 1's
    ps.update({cf.P_NORM_TWO_PARTIALS, cf.NORM_TILE + 3, cf.NORM_TILE + 4, cf.P_NORM_NARROW_MAX, cf.NORM_WIDE_MIN_P,
               cf.P_NORM_WIDE})
    return sorted(ps)


def test_reduce_plan_equals_the_restatement():
    from fedscale_amd import kernels_clip as kc

    for cus in CUS:
        for P in _sweep():
            for K in (1, 5, 1000):
                assert kc.reduce_clip_plan(cus, K, P) == cf.plan(cus, K, P), (cus, K, P)


def test_norm_plan_and_workspace_equal_the_restatement():
    from fedscale_amd import kernels_clip as kc

    for cus in CUS:
        for P in _sweep():
            want = cf.norm_plan(cus, P)
            assert kc.norm_plan(cus, P) == want, (cus, P)
            for n in (0, 1, 7):
                assert kc.workspace_bytes(n, P) == max(8, n * want["tiles"] * 8), (n, P)


def test_plans_cover_every_column_once():
    for cus in CUS:
        for P in _sweep():
            col = 0
            for l in cf.plan(cus, 3, P):
                assert l["col0"] == col and l["grid"] >= 1 and l["tiles"] >= l["grid"]
                assert l["tiles"] % l["grid"] == 0 or l["V"] == 16  # only level 0 walks tiles, maybe raggedly
                col += l["tiles"] * cf.WAVES * l["sw"] * cf.STRIP
            assert col >= P and (P == 0) == (col == 0), (cus, P)


def test_shapes_of_the_gpu_tests_take_the_paths_they_are_listed_for():
    for cus in CUS:
        for name, (P, want) in cf.expected_plans(cus).items():
            assert cf.plan(cus, 3, P) == want, (cus, name)
        cap = cus * cf.CAP_PCT // 100
        assert cf.expected_plans(cus)["capped"][1][0]["tiles"] == 2 * cap
        wide = cf.norm_plan(cus, cf.P_NORM_WIDE)
        assert wide["tile_cols"] == 4096 and wide["tiles"] == 1025 and wide["waves"] == 4
        assert wide["grid"] * wide["waves"] < wide["tiles"] <= 2 * wide["grid"] * wide["waves"] or cus < 171
        narrow = cf.norm_plan(cus, cf.P_NORM_NARROW_MAX)
        assert narrow["tile_cols"] == 2048 and narrow["tiles"] == 2048 and narrow["waves"] == 2
    assert cf.P_NORM_WIDE % 4096 and cf.P_NORM_WIDE % 4 == 1
    part = cf.norm_plan(256, cf.P_NORM_TWO_PARTIALS)
    assert part["tiles"] == 65 and cf.P_NORM_TWO_PARTIALS % 4 == 3
    assert cf.norm_plan(256, 3) == dict(launches=1, tiles=0, grid=0, waves=2, tile_cols=2048)
    assert {u for _, u in cf.LEVELS} == {1, 4, 8} and cf.ks_for(1) == [1, 2, 3] and 17 in cf.ks_for(8)


def test_bad_plan_arguments_are_refused():
    from fedscale_amd import _native_clip as nc
    from fedscale_amd._native import FedAggError

    buf = np.zeros(8 * nc.PLAN_FIELDS, dtype=np.int64)
    for args in ((0, 1, 10, buf.ctypes.data, 8), (-4, 1, 10, buf.ctypes.data, 8), (8, -1, 10, buf.ctypes.data, 8),
                 (8, 1, -10, buf.ctypes.data, 8), (8, 1, 10, buf.ctypes.data, -1), (8, 1, 10, None, 8)):
        with pytest.raises(FedAggError, match="fcl_reduce_plan.*nothing was launched"):
            nc.call("fcl_reduce_plan", *args)
    assert nc.call("fcl_reduce_plan", 8, 1, 10, None, 0) == 1  # the count alone
    for args in ((0, 10, buf.ctypes.data), (8, -1, buf.ctypes.data), (8, 10, None)):
        with pytest.raises(FedAggError, match="fcl_norm_plan"):
            nc.call("fcl_norm_plan", *args)
    with pytest.raises(FedAggError, match="fcl_workspace_bytes"):
        nc.call("fcl_workspace_bytes", -1, 10)
    with pytest.raises(FedAggError, match="fcl_workspace_bytes"):
        nc.call("fcl_workspace_bytes", 1, -10)


def test_binding_lists_every_symbol_of_the_header():
    import os
    import re

    from fedscale_amd import _native_clip as nc
    from fedscale_amd import buildinfo

    with open(os.path.join(buildinfo.ROOT, "include", "fedclip.h")) as f:
        text = f.read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t)\s+(fcl_\w+)\(", text, flags=re.M))
    assert declared == set(nc.SIGNATURES) and len(declared) == 8
    assert f"#define FCL_ABI_VERSION {nc.ABI_VERSION}" in text and f"#define FCL_PLAN_FIELDS {nc.PLAN_FIELDS}" in text
    assert "fedscale_amd/csrc/clip_reduce.hip" in buildinfo.SRCS and "include/fedclip.h" in buildinfo.HDRS
    assert nc.load().fcl_abi_version() == nc.ABI_VERSION


def test_clip_spec_validates_on_construction():
    from fedscale_amd.clip_round import ClipSpec, noise_stride

    s = ClipSpec(3.0)
    assert (s.max_norm, s.noise_multiplier, s.seed) == (3.0, 0.0, 0)
    s = ClipSpec(np.float32(0.5), noise_multiplier=1.1, seed=np.int64(7))
    assert type(s.max_norm) is float and s.max_norm == 0.5 and s.noise_multiplier == 1.1 and s.seed == 7
    assert s.sigma(10) == float(1.1 * 0.5 / 10)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), None, "x"):
        with pytest.raises(ValueError, match="max_norm"):
            ClipSpec(bad)
    for bad in (-0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="noise_multiplier"):
            ClipSpec(1.0, noise_multiplier=bad)
    for bad in (1.5, "3", True, None):
        with pytest.raises(ValueError, match="seed"):
            ClipSpec(1.0, seed=bad)
    with pytest.raises(AttributeError):
        s.max_norm = 2.0
    assert [noise_stride(p) for p in (0, 1, 2, 3, 24492)] == [0, 2, 2, 4, 24492]


def _stub(**kw):
    base = dict(upload_dtype=None, shards=types.SimpleNamespace(world=1), layout=types.SimpleNamespace(world=1),
                optimizer=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_refused_combinations_name_the_combination():
    """Every new refusal is a NotImplementedError naming the combination, raised before a device is touched (the
    stubs have none)."""
    from fedscale_amd.clip_round import ClippedRound, ClipSpec
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    spec = ClipSpec(3.0)
    check = TorchModelAdapter._check_clip
    check(_stub(), "fedavg", False, spec)  # the accepted form
    check(_stub(optimizer=types.SimpleNamespace(mode="fed-yogi")), "fedavg", False, spec)
    with pytest.raises(NotImplementedError, match="clip.*upload_dtype='bfloat16'"):
        check(_stub(upload_dtype="bfloat16"), "fedavg", False, spec)
    with pytest.raises(NotImplementedError, match="clip.*cohort signatures"):
        check(_stub(), "fedavg", True, spec)
    with pytest.raises(NotImplementedError, match="clip.*shard"):
        check(_stub(shards=types.SimpleNamespace(world=2)), "fedavg", False, spec)
    with pytest.raises(NotImplementedError, match="clip.*parameter-sharded layout"):
        check(_stub(layout=types.SimpleNamespace(world=2)), "fedavg", False, spec)
    for policy in ("fedbuff", "qfedavg"):
        with pytest.raises(NotImplementedError, match=f"clip.*{policy} round"):
            check(_stub(), policy, False, spec)
    with pytest.raises(NotImplementedError, match="clip.*q-fedavg server optimizer"):
        check(_stub(optimizer=types.SimpleNamespace(mode="q-fedavg")), "fedavg", False, spec)
    with pytest.raises(TypeError, match="ClipSpec"):
        check(_stub(), "fedavg", False, 3.0)
    # begin_round itself refuses before it looks at a staging area or a device
    with pytest.raises(NotImplementedError, match="clip.*fedbuff round"):
        TorchModelAdapter.begin_round(_stub(_check_clip=lambda *a: check(_stub(), *a)), 4, "fedbuff", clip=spec)
    with pytest.raises(NotImplementedError, match="clip.*ShardedModelAdapter"):
        ShardedModelAdapter.begin_round(types.SimpleNamespace(parts=[0, 1]), 4, "fedavg", clip=spec)
    # the round's own checks
    with pytest.raises(NotImplementedError, match="clip.*fedbuff round"):
        ClippedRound(types.SimpleNamespace(world=1), "cpu", 4, spec, staging=None, last_f32=None, policy="fedbuff")
    with pytest.raises(NotImplementedError, match="clip.*parameter-sharded layout"):
        ClippedRound(types.SimpleNamespace(world=2), "cpu", 4, spec, staging=None, last_f32=None)
    with pytest.raises(TypeError, match="ClipSpec"):
        ClippedRound(types.SimpleNamespace(world=1), "cpu", 4, 3.0, staging=None, last_f32=None)
    with pytest.raises(ValueError, match="K >= 1"):
        ClippedRound(types.SimpleNamespace(world=1), "cpu", 0, spec, staging=None, last_f32=None)


def test_mixin_passes_its_three_attributes_through():
    from fedscale_amd.clip_round import ClipSpec
    from fedscale_amd.cloud.aggregation import aggregator as agg
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    M = agg.DeviceAggregatorMixin
    assert (M.device_clip_norm, M.device_clip_noise_multiplier, M.device_clip_seed) == (None, 0.0, 0)
    assert agg.DeviceAsyncAggregatorMixin.device_clip_norm is None  # inherited

    calls = []

    class Wrapper(TorchModelAdapter):
        optimizer = None

        def __init__(self):
            pass

        def begin_round(self, K, policy, **kw):
            calls.append((K, policy, kw))
            return types.SimpleNamespace(policy="fedavg", add=lambda u: None, n=0)

    class A(agg.DeviceAggregator):
        pass

    a = A(Wrapper())
    a.start_round(3)
    a.on_result({"client_id": 1, "update_weight": {}})
    assert calls[-1] == (3, "fedavg", dict(capacity=None, keep_mean=True))  # unset: the call is what it was

    class B(agg.DeviceAggregator):
        device_clip_norm = 3.0
        device_clip_noise_multiplier = 0.25
        device_clip_seed = 11

    b = B(Wrapper())
    b.start_round(3)
    b.on_result({"client_id": 1, "update_weight": {}})
    K, policy, kw = calls[-1]
    spec = kw.pop("clip")
    assert (K, policy, kw) == (3, "fedavg", dict(capacity=None, keep_mean=True))
    assert isinstance(spec, ClipSpec) and (spec.max_norm, spec.noise_multiplier, spec.seed) == (3.0, 0.25, 11)

    class Bad(agg.DeviceAggregator):
        device_clip_norm = -1.0

    bad = Bad(Wrapper())
    bad.start_round(3)
    with pytest.raises(ValueError, match="max_norm"):
        bad.on_result({"client_id": 1, "update_weight": {}})

    class Async(agg.DeviceAsyncAggregator):
        device_clip_norm = 3.0

    c = Async(Wrapper())
    c.start_round(3)
    c.client_task_model_version[1] = 0
    with pytest.raises(NotImplementedError, match="clip.*DeviceAsyncAggregatorMixin"):
        c.on_result({"client_id": 1, "update_weight": {}})
    assert c.aggregation_denominator == 0  # refused before any state moved

    class Cohort(agg.DeviceCohortAggregator):
        device_clip_norm = 3.0

    d = Cohort([Wrapper()], [3])
    with pytest.raises(NotImplementedError, match="clip.*DeviceCohortAggregatorMixin"):
        d.on_result({"client_id": 1, "update_weight": {}}, 0)


def test_restatement_on_a_worked_example():
    """The numpy restatement itself, on numbers small enough to check by hand."""
    last = np.asarray([1.0, 2.0, 3.0, 4.0], dtype=np.float32)
    x = np.stack([last + np.asarray([3, 4, 0, 0], dtype=np.float32),      # norm 5
                  last + np.asarray([0.5, 0, 0, 0], dtype=np.float32),    # norm 0.5
                  last + np.asarray([np.nan, 1, 1, 1], dtype=np.float32),  # rejected
                  last + np.asarray([0, 0, 30, 40], dtype=np.float32)])   # norm 50
    sq = [cf.sq_exact(r, last) for r in x]
    assert sq[:2] == [25.0, 0.25] and np.isnan(sq[2]) and sq[3] == 2500.0
    c = cf.coefs_of(sq, 5.0)
    assert c.dtype == np.float32 and c[1] == 1.0 and c[2] == 0.0
    assert c[0] == np.float32(5.0 / (5.0 + 1e-6)) and c[0] < 1 and c[3] == np.float32(5.0 / (50.0 + 1e-6))
    chain = cf.chain_of(x, last, c)
    assert np.isfinite(chain).all()
    assert abs(chain[0] - (3 * c[0] + np.float32(0.5))) < 1e-5 and abs(chain[3] - 4.0) < 1e-5
    out, m = cf.finish_of(chain, last, 4)
    assert np.array_equal(m, chain / np.float32(4)) and np.array_equal(out, last + m)
    z = np.asarray([1, -1, 0.5, 0], dtype=np.float32)
    out2, m2 = cf.finish_of(chain, last, 4, sigma=0.125, z=z)
    assert np.array_equal(m2, m + np.float32(0.125) * z) and np.array_equal(out2, last + m2)
    assert all(cf.coef_is_stable(s, 5.0) for s in sq)
    # chunks continue one chain
    a = cf.chain_of(x[:2], last, c[:2])
    assert np.array_equal(cf.chain_of(x[2:], last, c[2:], acc=a), chain)
