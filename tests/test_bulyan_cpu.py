"""Bulyan aggregation without a device: ``BulyanSpec``, the binding of include/fedbulyan.h, ``fbl_plan``, every refused
combination on stubs, and the numpy restatement of tests/bulyan_fixtures.py against a brute-force sort."""
import os
import re
import types

import numpy as np
import pytest

from tests import bulyan_fixtures as bf
from tests import trim_fixtures as tf


def test_spec_forms_and_counts():
    from fedscale_amd.bulyan_round import BulyanSpec

    assert BulyanSpec(np.int64(3)).f == 3 and BulyanSpec(BulyanSpec(2)) == BulyanSpec(2) != BulyanSpec(1)
    assert repr(BulyanSpec(2)) == "BulyanSpec(2)"
    for bad in (True, -1, 0.2, "2", None, [1]):
        with pytest.raises(ValueError, match="BulyanSpec"):
            BulyanSpec(bad)
    assert [BulyanSpec(f).counts(K) for f, K in ((0, 3), (1, 7), (2, 11), (16, 67), (255, 1025), (100, 1000),
                                                 (0, 4096))] == [(1, 1), (3, 1), (5, 1), (33, 1), (513, 3), (798, 598),
                                                                 (4094, 4094)]
    for f, K in ((0, 2), (1, 6), (250, 1002)):
        with pytest.raises(ValueError, match=r"4f \+ 3 <= K"):
            BulyanSpec(f).counts(K)
    with pytest.raises(ValueError, match="FK_MAX_K = 4096"):
        BulyanSpec(1).counts(4097)


def test_binding_lists_every_symbol_of_the_header():
    from fedscale_amd import _native
    from fedscale_amd import _native_bulyan as nb
    from fedscale_amd import buildinfo

    with open(os.path.join(buildinfo.ROOT, "include", "fedbulyan.h")) as f:
        text = f.read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t)\s+(fbl_\w+)\(", text, flags=re.M))
    assert declared == set(nb.SIGNATURES) and len(declared) == 5
    for name, value in (("FBL_ABI_VERSION", nb.ABI_VERSION), ("FBL_PLAN_FIELDS", nb.PLAN_FIELDS)):
        assert re.search(rf"^#define {name} +{value}\b", text, flags=re.M), name
    assert "fedscale_amd/csrc/bulyan.hip" in buildinfo.SRCS and "include/fedbulyan.h" in buildinfo.HDRS
    assert nb.load().fbl_abi_version() == nb.ABI_VERSION
    assert nb.call("fbl_select_workspace_bytes", 1000) >= 1000 * 999 * 12 + 2 * 1000 * 8
    buf = np.zeros(nb.PLAN_FIELDS, dtype=np.int64)
    for args, what in (((0, 9, 10), "cus=0"), ((8, 0, 10), "theta=0"), ((8, 4097, 10), "theta=4097"),
                       ((8, 9, -1), "negative")):
        with pytest.raises(_native.FedAggError, match=f"{what}.*nothing was launched"):
            nb.call("fbl_plan", *args, buf.ctypes.data)


@pytest.mark.parametrize("theta, lanes, rows, W", [(1, 16, 5, 64), (80, 16, 5, 64), (81, 16, 17, 64), (272, 16, 17, 64),
                                                   (273, 32, 33, 64), (315, 32, 33, 64), (316, 32, 33, 32),
                                                   (620, 32, 33, 32), (621, 32, 33, 16), (1056, 32, 33, 16),
                                                   (1057, 64, 65, 16), (1204, 64, 65, 16), (1205, 64, 65, 8),
                                                   (2275, 64, 65, 8), (2276, 64, 65, 4), (4096, 64, 65, 4)])
def test_plan(theta, lanes, rows, W):
    from fedscale_amd import kernels_bulyan as kb

    p = kb.plan(256, theta, 1000 * W + 1)
    assert (p["lanes"], p["rows"], p["W"]) == (lanes, rows, W) and p["lanes"] * p["rows"] >= theta
    assert 4 * theta * (W + 1) <= p["lds"] == min(4 * 65 * lanes * rows, 80 * 1024) and p["passes"] == W * lanes // 256
    assert W == 64 or W == 256 // lanes or 4 * theta * (2 * W + 1) > 80 * 1024
    assert p["tiles"] == 1001 and p["grid"] == min(1001, 256 * {5: 4, 17: 2, 33: 2, 65: 1}[rows])
    assert kb.plan(8, theta, W)["grid"] == 1 and kb.plan(8, theta, 0) == dict(p, tiles=0, grid=0)


def _stub(**kw):
    base = dict(upload_dtype=None, shards=types.SimpleNamespace(world=1), layout=types.SimpleNamespace(world=1),
                optimizer=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_refused_combinations_name_the_combination():
    from fedscale_amd.bulyan_round import BulyanSpec
    from fedscale_amd.cloud.aggregation import aggregator as agg
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    check = TorchModelAdapter._check_bulyan
    none = (None,) * 5
    assert check(_stub(), "fedavg", False, *none, 2) == check(_stub(), "fedavg", False, *none, BulyanSpec(2))
    for i, word in enumerate(("clip", "trim", "krum", "geomed", "deep_trim")):
        given = [None] * 5
        given[i] = object()
        with pytest.raises(NotImplementedError, match=f"bulyan.*{word}"):
            check(_stub(), "fedavg", False, *given, 2)
    for attr in ("upload_secagg", "upload_vote", "upload_fp4", "upload_sketch", "upload_lowrank", "upload_sign",
                 "upload_topk", "upload_quant", "upload_dtype"):
        with pytest.raises(NotImplementedError, match=f"bulyan.*{attr}='fmt'"):
            check(_stub(**{attr: "fmt"}), "fedavg", False, *none, 2)
    for kw, pol, sig, what in ((dict(), "fedavg", True, "cohort signatures"), (dict(), "fedbuff", False, "fedbuff round"),
                               (dict(), "qfedavg", False, "qfedavg round"),
                               (dict(shards=types.SimpleNamespace(world=2)), "fedavg", False, "shard"),
                               (dict(layout=types.SimpleNamespace(world=2)), "fedavg", False, "parameter-sharded layout"),
                               (dict(optimizer=types.SimpleNamespace(mode="q-fedavg")), "fedavg", False, "q-fedavg server")):
        with pytest.raises(NotImplementedError, match=f"bulyan.*{what}"):
            check(_stub(**kw), pol, sig, *none, 2)
    with pytest.raises(NotImplementedError, match="bulyan.*ShardedModelAdapter"):
        ShardedModelAdapter.begin_round(types.SimpleNamespace(parts=[0, 1]), 40, "fedavg", bulyan=2)
    # the mixins
    assert agg.DeviceAggregatorMixin.device_bulyan is None
    for attr in ("device_trim", "device_deep_trim", "device_clip_norm", "device_krum", "device_geomed",
                 "device_upload_secagg", "device_upload_dtype", "device_upload_quant", "device_upload_topk",
                 "device_upload_sign", "device_upload_lowrank", "device_upload_vote", "device_upload_fp4",
                 "device_upload_sketch"):
        me = type("A", (agg.DeviceAggregatorMixin,), {"device_bulyan": 2, attr: 1, "device_shards": None})()
        with pytest.raises(NotImplementedError, match=f"bulyan.*{attr}=1"):
            me._bulyan_spec()
    for cls in (agg.DeviceAsyncAggregatorMixin, agg.DeviceCohortAggregatorMixin):
        me = type("A", (cls,), {"device_bulyan": 2})()
        with pytest.raises(NotImplementedError, match="bulyan.*Mixin"):
            me.update_weight_aggregation({})


@pytest.mark.parametrize("K, f, bad", [(3, 0, 0), (7, 1, 0), (9, 1, 2), (11, 2, 0), (11, 2, 4)])
def test_restated_selection_equals_a_brute_force_sort(K, f, bad):
    rng = np.random.default_rng(K + bad)
    d = rng.integers(-3, 4, size=(K, 6)).astype(np.float64)
    d[K // 2] = d[0]  # a duplicate row: a zero distance and a tie
    d[1:1 + bad, 2] = np.nan
    G = d @ d.T
    picks, sel, n_sel, score0 = bf.select_of(G, f)
    dist = bf.dist2_of(G)
    left, want = list(range(K)), []
    for s in range(K - 2 * f - 2):
        scores = []
        for i in left:
            sc = 0.0
            for v in sorted(dist[i][j] for j in left if j != i)[:len(left) - f - 2]:
                sc = sc + v
            scores.append((sc, i))
        if s == 0:
            assert np.array_equal(score0, [sc for sc, _ in scores])
        sc, i = min(scores)
        if not np.isfinite(sc):
            break
        want.append(i)
        left.remove(i)
    pad = [-1] * (K - 2 * f - 2 - len(want))
    assert n_sel == len(want) == (0 if bad > f + 1 else K - 2 * f - 2)
    assert picks.tolist() == want + pad and sel.tolist() == sorted(want) + pad


@pytest.mark.parametrize("theta, beta", [(1, 1), (2, 1), (2, 2), (3, 1), (3, 3), (9, 5), (10, 8)])
def test_restated_mean_around_the_median_equals_a_brute_force_sort(theta, beta):
    rng = np.random.default_rng(10 * theta + beta)
    K, P = theta + 3, 40
    sel = np.sort(rng.permutation(K)[:theta]).astype(np.int32)
    x = bf.rows_of(rng, K, P + 4, P, sel)
    out, kept = bf.reduce_of(x[:, :P], sel, beta)
    want_kept = np.zeros(K, dtype=np.int64)
    for p in range(P):
        v = x[sel, p]
        key = tf.keys_of(v)
        med = v[sorted(range(theta), key=lambda r: (key[r], r))[(theta - 1) // 2]]
        with np.errstate(all="ignore"):
            e = np.abs(v - med)
        ekey = [0xFFFFFFFF if np.isnan(a) else int(a.view(np.uint32)) for a in e]
        rows = sorted(sorted(range(theta), key=lambda r: (ekey[r], r))[:beta])
        chain = v[rows[0]]
        with np.errstate(all="ignore"):
            for r in rows[1:]:
                chain = chain + v[r]
            want = chain / np.float32(beta)
        want_kept[sel[rows]] += 1
        assert (np.isnan(want) and np.isnan(out[p])) or want.view(np.uint32) == out[p].view(np.uint32), (p, want, out[p])
    assert np.array_equal(kept, want_kept) and kept.sum() == beta * P
