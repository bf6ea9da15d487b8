"""Deep trimmed-mean aggregation without a device: ``DeepTrimSpec``, the binding of include/feddeeptrim.h, ``fdt_plan``
and its refusals, and every refused combination on stubs."""
import os
import re
import types

import numpy as np
import pytest


def test_spec_forms_and_counts():
    from fedscale_amd.deep_trim_round import DeepTrimSpec
    from fedscale_amd.trim_round import TrimSpec

    assert DeepTrimSpec(np.int64(3)).trim == 3 and type(DeepTrimSpec(np.float32(0.25)).trim) is float
    assert DeepTrimSpec(DeepTrimSpec(2)) == DeepTrimSpec(2) and DeepTrimSpec(0) != DeepTrimSpec(0.0)
    assert repr(DeepTrimSpec(2)) == "DeepTrimSpec(2)"
    for bad in (True, np.True_, -1, 0.5, -0.1, float("nan"), "mean", None, [1]):
        with pytest.raises(ValueError, match="DeepTrimSpec"):
            DeepTrimSpec(bad)
    assert [DeepTrimSpec("median").count(K) for K in (1, 2, 3, 34, 35, 36, 1000, 4096)] == [0, 0, 1, 16, 17, 17, 499, 2047]
    assert [DeepTrimSpec(0.2).count(K) for K in (4, 85, 100, 1000)] == [0, 17, 20, 200]
    assert DeepTrimSpec(17).count(100) == 17 and DeepTrimSpec(0).count(1) == 0
    with pytest.raises(ValueError, match=r"ft_max_trim\(\) = 16"):  # the old family keeps its limit
        TrimSpec("median").count(35)
    for spec, K in ((DeepTrimSpec(1), 2), (DeepTrimSpec(50), 100)):
        with pytest.raises(ValueError, match="2t < K"):
            spec.count(K)
    with pytest.raises(ValueError, match=r"fdt_max_rows\(\) = 4096"):
        DeepTrimSpec(1).count(4097)


def test_binding_lists_every_symbol_of_the_header():
    from fedscale_amd import _native_deeptrim as nd
    from fedscale_amd import buildinfo, kernels_deeptrim

    with open(os.path.join(buildinfo.ROOT, "include", "feddeeptrim.h")) as f:
        text = f.read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t)\s+(fdt_\w+)\(", text, flags=re.M))
    assert declared == set(nd.SIGNATURES) and len(declared) == 4
    for name, value in (("FDT_ABI_VERSION", nd.ABI_VERSION), ("FDT_MAX_ROWS", nd.MAX_ROWS),
                        ("FDT_PLAN_FIELDS", nd.PLAN_FIELDS)):
        assert re.search(rf"^#define {name} +{value}\b", text, flags=re.M), name
    assert "fedscale_amd/csrc/deep_trim.hip" in buildinfo.SRCS and "include/feddeeptrim.h" in buildinfo.HDRS
    assert nd.load().fdt_abi_version() == nd.ABI_VERSION and kernels_deeptrim.max_rows() == nd.MAX_ROWS == 4096


@pytest.mark.parametrize("K, C", [(3, 64), (174, 64), (175, 32), (466, 32), (467, 16), (1000, 16), (1002, 16),
                                  (1003, 8), (1913, 8), (1914, 4), (3280, 4), (3281, 4), (4096, 4)])
def test_plan(K, C):
    """C is the widest power of two whose workgroup — K C + 136 C + 256 + 2 K words — fits 80 KiB, and 4 beyond."""
    from fedscale_amd import kernels_deeptrim as kd

    words = lambda c: K * c + 136 * c + 256 + 2 * K  # noqa: E731
    p = kd.plan(256, K, 1000 * C + 1, 1)
    assert p["C"] == C and p["lanes"] == 256 // C and p["lds"] == 4 * words(C)
    assert (C == 64 or 4 * words(2 * C) > 80 * 1024) and p["wgs"] == (2 if p["lds"] <= 80 * 1024 else 1)
    assert p["lds"] <= 104 * 1024 and p["rows"] % 2 == 1 and p["rows"] * p["lanes"] >= K > (p["rows"] - 2) * p["lanes"]
    assert p["tiles"] == 1001 and p["grid"] == 256 * p["wgs"]
    assert kd.plan(8, K, C, 1)["grid"] == 1 and kd.plan(8, K, 0, (K - 1) // 2) == dict(p, tiles=0, grid=0)


def test_refusals_without_a_gpu():
    from fedscale_amd import _native
    from fedscale_amd import _native_deeptrim as nd

    buf = np.zeros(nd.PLAN_FIELDS, dtype=np.int64)
    for args, what in (((0, 9, 10, 1), "cus=0"), ((8, 9, 10, 0), "t >= 1"), ((8, 8, 10, 4), "2t < K=8"),
                       ((8, 4097, 10, 1), r"fdt_max_rows\(\)=4096"), ((8, 9, -1, 1), "negative")):
        with pytest.raises(_native.FedAggError, match=f"{what}.*nothing was launched"):
            nd.call("fdt_plan", *args, buf.ctypes.data)
    # fdt_reduce checks its sizes and pointers before it looks for a device
    for args, what in (((None, 12, 9, 10, 1, 16, None, None, 0), "x is NULL"), ((16, 8, 9, 10, 1, 16, None, None, 0), "ld=8 < P"),
                       ((16, 12, 9, 10, 5, 16, None, None, 0), "2t < K"), ((16, 12, 9, 10, 1, None, None, None, 0), "out is NULL"),
                       ((16, 12, 9, 10, 1, 16, 4, None, 0), "16-byte"), ((16, 12, 9, 10, 1, 16, None, 4, 0), "8-byte")):
        with pytest.raises(_native.FedAggError, match=f"{what}.*nothing was launched"):
            nd.call("fdt_reduce", *args, None)


def _stub(**kw):
    base = dict(upload_dtype=None, shards=types.SimpleNamespace(world=1), layout=types.SimpleNamespace(world=1),
                optimizer=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_refused_combinations_name_the_combination():
    from fedscale_amd.cloud.aggregation import aggregator as agg
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.deep_trim_round import DeepTrimmedRound, DeepTrimSpec

    check = TorchModelAdapter._check_deep_trim
    none = (None, None, None, None)
    for form in (200, 0.2, "median", DeepTrimSpec(2)):
        assert isinstance(check(_stub(), "fedavg", False, *none, form), DeepTrimSpec)
    for mode in ("fed-yogi", "fed-adam", "fed-adagrad", "fed-avgm"):
        assert check(_stub(optimizer=types.SimpleNamespace(mode=mode)), "fedavg", False, *none, 2) == DeepTrimSpec(2)
    for i, word in enumerate(("clip", "trim", "krum", "geomed")):
        given = [None] * 4
        given[i] = object()
        with pytest.raises(NotImplementedError, match=f"deep_trim.*{word}"):
            check(_stub(), "fedavg", False, *given, 2)
    for attr in ("upload_secagg", "upload_vote", "upload_fp4", "upload_sketch", "upload_lowrank", "upload_sign",
                 "upload_topk", "upload_quant", "upload_dtype"):
        with pytest.raises(NotImplementedError, match=f"deep_trim.*{attr}='fmt'"):
            check(_stub(**{attr: "fmt"}), "fedavg", False, *none, 2)
    for kw, pol, sig, what in ((dict(), "fedavg", True, "cohort signatures"), (dict(), "fedbuff", False, "fedbuff round"),
                               (dict(), "qfedavg", False, "qfedavg round"),
                               (dict(shards=types.SimpleNamespace(world=2)), "fedavg", False, "shard"),
                               (dict(layout=types.SimpleNamespace(world=2)), "fedavg", False, "parameter-sharded layout"),
                               (dict(optimizer=types.SimpleNamespace(mode="q-fedavg")), "fedavg", False, "q-fedavg server")):
        with pytest.raises(NotImplementedError, match=f"deep_trim.*{what}"):
            check(_stub(**kw), pol, sig, *none, 2)
    # begin_round refuses before it looks at an upload format, a staging area or a device
    me = _stub(_check_deep_trim=lambda *a: check(_stub(upload_quant="mxfp8"), *a), upload_quant="mxfp8")
    with pytest.raises(NotImplementedError, match="deep_trim.*upload_quant='mxfp8'"):
        TorchModelAdapter.begin_round(me, 40, "fedavg", deep_trim="median")
    me = _stub(_check_deep_trim=lambda *a: check(_stub(), *a), staging=None, staging_capacity=None,
               shards=types.SimpleNamespace(world=1, shards_clients=False))
    with pytest.raises(ValueError, match="2t < K"):
        TorchModelAdapter.begin_round(me, 4, "fedavg", deep_trim=2)
    with pytest.raises(ValueError, match="all K=40 uploads resident.*capacity is 4"):
        TorchModelAdapter.begin_round(me, 40, "fedavg", capacity=4, deep_trim="median")
    with pytest.raises(NotImplementedError, match="deep_trim.*ShardedModelAdapter"):
        ShardedModelAdapter.begin_round(types.SimpleNamespace(parts=[0, 1]), 40, "fedavg", deep_trim=17)
    # the round's own checks
    lay, stg = types.SimpleNamespace(world=1), types.SimpleNamespace(capacity=4)
    with pytest.raises(ValueError, match="all K=5 uploads resident.*capacity is 4"):
        DeepTrimmedRound(lay, "cpu", 5, DeepTrimSpec(1), staging=stg)
    # the mixins
    assert agg.DeviceAggregatorMixin.device_deep_trim is None
    for attr in ("device_trim", "device_clip_norm", "device_krum", "device_geomed", "device_upload_secagg",
                 "device_upload_dtype", "device_upload_quant", "device_upload_topk", "device_upload_sign",
                 "device_upload_lowrank", "device_upload_vote", "device_upload_fp4", "device_upload_sketch"):
        me = type("A", (agg.DeviceAggregatorMixin,), {"device_deep_trim": "median", attr: 1, "device_shards": None})()
        with pytest.raises(NotImplementedError, match=f"deep_trim.*{attr}=1"):
            me._deep_trim_spec()
    for cls in (agg.DeviceAsyncAggregatorMixin, agg.DeviceCohortAggregatorMixin):
        me = type("A", (cls,), {"device_deep_trim": 0.2})()
        with pytest.raises(NotImplementedError, match="deep_trim.*Mixin"):
            me.update_weight_aggregation({})
