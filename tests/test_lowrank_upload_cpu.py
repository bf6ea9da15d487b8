"""The executor side of the low-rank upload path and the options that carry it, no GPU: ``factored`` at its
boundaries, one PowerSGD step against a float64 restatement, the residual's bits, seeded determinism, the adapter's
pickle and every refused combination."""
import pickle

import numpy as np
import pytest
import torch

from fedscale_amd.bucket import BucketLayout
from fedscale_amd.cloud.execution.lowrank_upload import LowRankCompressor, expand, factored, matrix_dims, pack_factors

R = 4
SHAPES = {"w": (48, 80), "c": (12, 3, 3, 3), "b": (48,), "n": ()}
# 10 x the error of the float64 restatement below on the same float32 data, measured here on the CPU: 4.29e-6 on "c",
# 3.60e-7 on "w" (the rank-4 deltas are rounded to float32 twice, which is all that keeps them from rank 4)
TOL = 4.3e-5


@pytest.mark.parametrize("shape,rank,want", [
    ((100,), 1, False), ((), 1, False),            # not a matrix
    ((5, 40), 4, True), ((4, 40), 4, False),       # min(O, I) > r
    ((40, 5), 4, True), ((40, 4), 4, False),
    ((9, 8), 4, True), ((8, 8), 4, False),         # r (O + I) < O I: 68 < 72, 64 = 64
    ((4, 5), 1, True), ((4, 5), 3, False),         # 9 < 20, 27 > 20
    ((6, 2, 3, 3), 4, True),                       # (6, 18): 96 < 108
])
def test_factored_at_its_boundaries(shape, rank, want):
    assert factored(shape, rank) is want


def _data(seed=0):
    rng = np.random.default_rng(seed)
    L = {n: np.asarray(rng.standard_normal(s), dtype=np.float32) for n, s in SHAPES.items()}
    x = {}
    for n, s in SHAPES.items():
        O, I = matrix_dims(s)
        d = rng.standard_normal((O, R)) @ rng.standard_normal((R, I)) * 0.1 if len(s) >= 2 else rng.standard_normal(s)
        x[n] = np.asarray(L[n] + d.reshape(s).astype(np.float32), dtype=np.float32)
    return x, L


def _layout():
    return BucketLayout(list(SHAPES), list(SHAPES.values()), [torch.float32] * len(SHAPES))


def test_a_delta_of_rank_r_survives_one_step():
    x, L = _data()
    c = LowRankCompressor(R, seed=3)
    got = expand(c.compress({n: torch.from_numpy(v) for n, v in x.items()}, L), _layout())
    for (n, s), g in zip(SHAPES.items(), got):
        d = x[n] - L[n]
        if not factored(s, R):
            assert np.array_equal(g, d)
            continue
        M = d.astype(np.float64).reshape(matrix_dims(s))
        P, _ = np.linalg.qr(M @ c._first_q(n, M.shape[1], torch.zeros(1)).double().numpy())
        e64 = np.linalg.norm(P @ (M.T @ P).T - M) / np.linalg.norm(M)
        e32 = np.linalg.norm((g - d).ravel().astype(np.float64)) / np.linalg.norm(M)
        print(f"{n}: float32 {e32:.3g}, float64 restatement {e64:.3g}")
        assert 10 * e64 <= TOL * 1.01 and e32 <= TOL


def test_the_residual_is_what_the_upload_leaves_bit_for_bit_and_feeds_the_next_round():
    x, L = _data(1)
    x["w"] += np.random.default_rng(2).standard_normal(SHAPES["w"]).astype(np.float32)  # full rank: a residual
    c = LowRankCompressor(R, seed=5)
    up = c.compress({n: torch.from_numpy(v) for n, v in x.items()}, L)
    M = torch.from_numpy(x["w"] - L["w"])
    Ut, V = torch.from_numpy(up["w"][:, :48]), torch.from_numpy(up["w"][:, 48:])
    assert torch.equal(c.residual["w"], M - Ut.t() @ V) and float(c.residual["w"].abs().max()) > 0
    assert np.array_equal(pack_factors(Ut, V), up["w"])
    off = LowRankCompressor(R, seed=5, error_feedback=False)
    off.compress({n: torch.from_numpy(v) for n, v in x.items()}, L)
    assert off.residual == {}
    second = c.compress({n: torch.from_numpy(v) for n, v in x.items()}, L)  # warm Q, M = delta + residual
    assert not np.array_equal(second["w"], up["w"])


def test_one_seed_gives_identical_bytes():
    x, L = _data(4)
    ups = [LowRankCompressor(R, seed=9).compress({n: torch.from_numpy(v) for n, v in x.items()}, L) for _ in range(2)]
    assert all(ups[0][n].tobytes() == ups[1][n].tobytes() and ups[0][n].dtype == np.float32 for n in SHAPES)
    other = LowRankCompressor(R, seed=10).compress({n: torch.from_numpy(v) for n, v in x.items()}, L)
    assert other["w"].tobytes() != ups[0]["w"].tobytes() and other["w"].shape == (R, 48 + 80)


# ---- the options ------------------------------------------------------------------------------------------------------
def _adapter_cls():
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    return TorchModelAdapter


class _Opt:
    mode = "q-fedavg"


@pytest.mark.parametrize("kw,name", [
    (dict(upload_dtype="float16"), "upload_dtype"), (dict(upload_quant="mxfp8"), "upload_quant"),
    (dict(upload_topk=0.1), "upload_topk"), (dict(upload_sign="sign1"), "upload_sign"),
    (dict(upload_secagg=True), "upload_secagg"), (dict(optimizer=_Opt()), "q-fedavg"),
])
def test_the_adapter_refuses_what_low_rank_uploads_do_not_combine_with(kw, name):
    with pytest.raises(NotImplementedError, match=f"(?s)upload_lowrank=4.*{name}|{name}.*upload_lowrank=4"):
        _adapter_cls()(torch.nn.Linear(8, 8), upload_lowrank=4, **kw)


@pytest.mark.parametrize("rank", (0, 65, 2.5, True, "4"))
def test_a_rank_outside_1_to_64_is_a_value_error(rank):
    with pytest.raises(ValueError, match="upload_lowrank"):
        _adapter_cls()(torch.nn.Linear(8, 8), upload_lowrank=rank)


@pytest.mark.parametrize("kw,name", [
    (dict(policy="fedbuff"), "fedbuff"), (dict(policy="qfedavg"), "qfedavg"), (dict(signatures=True), "signatures"),
    (dict(clip=object()), "clip"), (dict(trim=1), "trim"), (dict(krum=1), "krum"), (dict(geomed=True), "geomed"),
])
def test_begin_round_refuses_before_a_device_is_touched(kw, name):
    a = object.__new__(_adapter_cls())  # no device: the refusals come before anything is allocated
    a.upload_lowrank, a.optimizer = 4, None
    kw = dict(kw)
    with pytest.raises(NotImplementedError, match=f"(?s)upload_lowrank=4.*{name}|{name}.*upload_lowrank=4"):
        a.begin_round(5, kw.pop("policy", "fedavg"), **kw)


def test_the_other_ways_in_refuse_too_and_the_option_pickles():
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAsyncAggregatorMixin
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter
    from fedscale_amd.cloud.internal.torch_model_adapter import _rebuild_with_upload_lowrank

    with pytest.raises(NotImplementedError, match="(?s)upload_lowrank=4.*ShardedModelAdapter"):
        ShardedModelAdapter(torch.nn.Linear(8, 8), devices=[0, 1], upload_lowrank=4)

    class Agg(DeviceAsyncAggregatorMixin):
        device_upload_lowrank = 4

    with pytest.raises(NotImplementedError, match="(?s)upload_lowrank=4.*fedbuff"):
        Agg.update_weight_aggregation(object.__new__(Agg), {})
    a = object.__new__(_adapter_cls())
    a.upload_lowrank, a.optimizer, a.model = 4, None, torch.nn.Linear(2, 2)
    a._module_version = a._version = 0
    fn, args = a.__reduce__()
    assert fn is _rebuild_with_upload_lowrank and args[0] is _adapter_cls() and args[3] == 4
    assert pickle.loads(pickle.dumps((fn, args[3]))) == (fn, 4)
