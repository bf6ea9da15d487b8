"""No GPU: the Count-Sketch contract (include/fedsketch.h) — the hash constants of the header, compress_sketch on the
host against the independent restatement of tests/sketch_fixtures.py, exact integer sums, SketchSpec, the refusals,
and one recovery condition on the restatement."""
import re

import numpy as np
import pytest
import torch

from fedscale_amd.cloud.execution import sketch_upload as su
from fedscale_amd.cloud.execution.sketch_upload import SKETCH_KEY, SketchSpec, compress_sketch
from tests import sketch_fixtures as fx
from tests.conftest import ROOT


def test_the_header_prints_the_hash_of_seed_0_row_0():
    text = open(f"{ROOT}/include/fedsketch.h").read()
    sign = [f"{fx.mix(fx.G, w):016x}" for w in range(4)]
    mask = [f"{fx.mix(2 * fx.G & fx.M64, b):016x}" for b in range(4)]
    assert sign[0] == "2d0f28c7e7e786b2" and mask[0] == "3c5b66874b9e8a84"
    for word in sign + mask:
        assert word in re.sub(r"\s+\*\s+", " ", text)
    assert [int(x) for x in su.mix(fx.G, np.arange(4))] == [fx.mix(fx.G, w) for w in range(4)]


@pytest.mark.parametrize("R,C,P,seed", [(1, 1024, 1, 0), (3, 1024, 1023, 1), (5, 2048, 3 * 2048 + 5, 2 ** 63 + 11),
                                        (7, 1024, 9 * 1024 + 1, 7)])
def test_compress_sketch_on_the_host_is_the_restatement(R, C, P, seed):
    rng = np.random.default_rng(P)
    a = P // 3
    state = {"w": rng.standard_normal(a).astype(np.float32), "n": np.array(5, dtype=np.int64),
             "v": rng.standard_normal(P - a).astype(np.float32)}
    base = {"w": rng.standard_normal(a).astype(np.float32), "n": np.array(3, dtype=np.int64),
            "v": rng.standard_normal(P - a).astype(np.float32)}
    up = compress_sketch(state, base, SketchSpec(rows=R, cols=C, seed=seed))
    assert list(up) == ["n", SKETCH_KEY] and up["n"] == 5
    e = np.concatenate([state["w"] - base["w"], state["v"] - base["v"]])
    want = fx.sketch(e, R, C, seed)
    assert up[SKETCH_KEY].dtype == np.float32 and up[SKETCH_KEY].shape == (R, C)
    assert np.array_equal(up[SKETCH_KEY].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("R,C,P", [(5, 1024, 20 * 1024 + 3), (3, 4096, 4096 * 2 + 100)])
def test_integer_updates_sum_exactly(R, C, P):
    """|e| <= 2047 and NB <= 21 blocks: every partial sum is an integer below 2^24, so any order gives these bits."""
    rng = np.random.default_rng(1)
    e = rng.integers(-2047, 2048, P).astype(np.float32)
    T = su.sketch_host(e, R, C, 9)
    for j in range(R):
        s = 1.0 - 2.0 * (fx.signs(9, j, P) >> np.uint32(31)).astype(np.float64)
        want = np.bincount(fx.buckets(9, j, P, C), weights=s * e, minlength=C)
        assert np.array_equal(T[j].astype(np.float64), want)


def test_spec_defaults_and_validation():
    s = SketchSpec()
    assert (s.rows, s.cols, s.k, s.momentum, s.seed) == (5, None, 0.01, 0.9, 0)
    assert s.cols_for(25_000_000) == 1 << 17 and s.cols_for(26_214_400) == 1 << 18 and s.cols_for(10) == 1024
    assert s.count(1000) == 10 and SketchSpec(k=7).count(1000) == 7 and SketchSpec(k=7).count(3) == 3
    assert SketchSpec(k=1).count(50) == 1 and SketchSpec(k=1.0).count(50) == 50
    assert SketchSpec.of(True) == SketchSpec()
    for bad in (dict(rows=2), dict(rows=True), dict(cols=1000), dict(cols=512), dict(cols=1 << 25), dict(k=0),
                dict(k=1.5), dict(k=True), dict(k="x"), dict(momentum=1.0), dict(momentum=-0.1), dict(seed=-1),
                dict(seed=1 << 64), dict(compression=0.5)):
        with pytest.raises(ValueError, match="upload_sketch"):
            SketchSpec(**bad)
    with pytest.raises(TypeError, match="SketchSpec"):
        SketchSpec.of(0.01)


def _args(policy):
    import argparse

    return argparse.Namespace(gradient_policy=policy, yogi_eta=3e-3, yogi_tau=1e-8, yogi_beta=0.9, yogi_beta2=0.99,
                              learning_rate=0.05, qfed_q=1.0)


def _adapter_kw():
    from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
    from fedscale_amd.cloud.internal.torch_model_adapter import _STEP_MODES
    from fedscale_amd.state import ShardGroup

    yield "upload_dtype", dict(upload_dtype="float16")
    yield "upload_quant", dict(upload_quant="mxfp8")
    yield "upload_topk", dict(upload_topk=0.1)
    yield "upload_secagg", dict(upload_secagg=True)
    yield "upload_sign", dict(upload_sign="sign1")
    yield "upload_lowrank", dict(upload_lowrank=2)
    yield "upload_vote", dict(upload_vote=0.01)
    yield "upload_fp4", dict(upload_fp4="mxfp4")
    yield "ShardGroup", dict(shards=ShardGroup(0, 2, mode="params"))
    yield "ShardGroup", dict(shards=ShardGroup(1, 2, mode="clients"))
    for policy in _STEP_MODES:  # fed-yogi, q-fedavg, fed-adam, fed-adagrad, fed-avgm
        yield policy, dict(optimizer=TorchServerOptimizer(policy, _args(policy), "cpu"))


@pytest.mark.parametrize("word,kw", list(_adapter_kw()))
def test_the_adapter_refuses_by_name_before_it_touches_a_device(word, kw):
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    with pytest.raises(NotImplementedError, match="upload_sketch=.*" + word):
        TorchModelAdapter(torch.nn.Linear(2, 2), upload_sketch=SketchSpec(cols=1024), **kw)


@pytest.mark.parametrize("policy", [None, "fed-avg", "fed-prox"])
def test_a_policy_whose_server_step_is_fedavg_is_taken(policy):
    """The aggregator always builds a server optimizer from the job's gradient_policy: one that names FedAvg, or a
    client-side term, is not a server step.  (Without a GPU the constructor then fails at its device.)"""
    from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    try:
        adapter = TorchModelAdapter(torch.nn.Linear(2, 2), upload_sketch=SketchSpec(cols=1024),
                                    optimizer=TorchServerOptimizer(policy, _args(policy), "cpu"))
    except RuntimeError as e:
        assert not torch.cuda.is_available(), e
    else:
        assert adapter.upload_sketch == SketchSpec(cols=1024)


@pytest.mark.parametrize("word,kw", [("clip", dict(clip=object())), ("trim", dict(trim=1)), ("krum", dict(krum=1)),
                                     ("geomed", dict(geomed=True)), ("signatures", dict(signatures=True)),
                                     ("fedbuff", dict(policy="fedbuff")), ("qfedavg", dict(policy="qfedavg"))])
def test_begin_round_refuses_by_name_before_it_touches_a_device(word, kw):
    import types

    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    stub = types.SimpleNamespace(upload_sketch=SketchSpec(cols=1024))  # a refusal reads nothing else
    a = dict(policy="fedavg", signatures=False, clip=None, trim=None, krum=None, geomed=None)
    a.update(kw)
    with pytest.raises(NotImplementedError, match="upload_sketch=.*" + word):
        TorchModelAdapter._begin_sketch_round(stub, 4, a["policy"], None, a["signatures"], a["clip"], a["trim"],
                                              a["krum"], a["geomed"])


def test_the_sharded_adapter_the_async_mixin_and_a_wrong_upload_are_refused():
    from fedscale_amd.bucket import BucketLayout
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAsyncAggregatorMixin
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter
    from fedscale_amd.sketch_round import upload_plan_sketch

    with pytest.raises(NotImplementedError, match="upload_sketch=.*ShardedModelAdapter"):
        ShardedModelAdapter(torch.nn.Linear(2, 2), devices=[0, 1], upload_sketch=SketchSpec())

    class Agg(DeviceAsyncAggregatorMixin):
        device_upload_sketch = SketchSpec()

    with pytest.raises(NotImplementedError, match="upload_sketch=.*fedbuff"):
        Agg().update_weight_aggregation({})
    lay = BucketLayout.from_state_dict({"w": torch.zeros(6), "n": torch.zeros((), dtype=torch.int64)})
    n, t = np.array(1, dtype=np.int64), np.zeros((3, 1024), dtype=np.float32)
    side, tab = upload_plan_sketch(lay, {"n": n, SKETCH_KEY: t}, 3, 1024)
    assert tab.shape == (3072,) and side[0][0].name == "n"
    for bad, err in (({"w": np.zeros(6, dtype=np.float32), "n": n}, TypeError),
                     ({"n": n, SKETCH_KEY: t.astype(np.float64)}, TypeError),
                     ({"n": n, SKETCH_KEY: t[:1]}, TypeError), ({SKETCH_KEY: t}, ValueError), ([t], ValueError)):
        with pytest.raises(err):
            upload_plan_sketch(lay, bad, 3, 1024)


def test_planted_heavy_columns_are_recovered():
    """P = 16 C, C = 1024, R = 5, unit Gaussian noise, 16 planted columns of magnitude 100, k = 16, seed 0: the
    recovered index set is the planted set.  Recovery is a property of most seeds, not of all: a light column that
    shares a bucket with heavy ones in three of the five rows takes their estimate whatever the magnitude (about one
    column in 30 000 at this shape; seed 2020 has one, seeds 0 to 7 have none)."""
    C, R, seed = 1024, 5, 0
    P = 16 * C
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(P).astype(np.float32)
    planted = np.sort(rng.choice(P, 16, replace=False))
    e[planted] = 100.0 * np.where(rng.random(16) < 0.5, -1.0, 1.0).astype(np.float32)
    est = fx.estimate(fx.sketch(e, R, C, seed), P, seed)
    assert np.array_equal(fx.topk(est, 16), planted)
