"""The MXFP4 delta-upload path without a GPU: restatement, host path, plan, wire format, refusals."""
import pickle
import types

import numpy as np
import pytest
import torch

from fedscale_amd.bucket import BucketLayout
from fedscale_amd.cloud.execution.quant4_upload import CODES_KEY, SCALES_KEY, compress_delta4
from fedscale_amd.quant4_round import Quant4Round, upload_plan4
from fedscale_amd.state import ShardGroup
from tests import quant4_fixtures as q4f

CASES = q4f.contract_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_brute_force_and_the_host_path_equals_the_restatement(name):
    d = CASES[name]
    codes, s, res = q4f.quantize(d)
    NB = q4f.blocks(d.size)
    pad = np.zeros(NB * 32)
    pad[:d.size] = d.astype(np.float64)
    for b in range(NB):  # float64 nearest-grid search, a tie to the code whose low bit is 0
        blk = pad[32 * b:32 * b + 32]
        if not np.isfinite(blk).all():
            assert s[b] == 255 and not codes[32 * b:32 * b + 32].any()
            continue
        am = np.abs(blk).max()
        e = 2 if am == 0 else min(max(int(np.floor(np.log2(am))) + 125 + (am > 1.5 * 2.0 ** np.floor(np.log2(am))),
                                      2), 252)
        assert s[b] == e, (name, b)
        v = np.clip(blk * 2.0 ** (127 - e), -6.0, 6.0)
        dist = np.abs(np.abs(v)[:, None] - q4f.POS[None, :])
        best = np.array([min(np.flatnonzero(r == r.min()), key=lambda c: c & 1) for r in dist])
        assert np.array_equal(codes[32 * b:32 * b + 32] & 7, best), (name, b)
        assert np.array_equal(codes[32 * b:32 * b + 32] >> 3, np.signbit(blk).astype(np.uint8)), (name, b)
    up, r_out = compress_delta4(dict(w=torch.from_numpy(d.copy())), [torch.zeros(d.size)], residual_out=True)
    assert list(up) == [CODES_KEY, SCALES_KEY]
    assert np.array_equal(up[CODES_KEY], q4f.pack(codes)) and np.array_equal(up[SCALES_KEY], s)
    assert np.array_equal(r_out.view(np.uint32), res.view(np.uint32))


def test_round_trip_is_within_half_a_grid_step_where_nothing_saturates():
    d = CASES["random_binades"]
    codes, s, _ = q4f.quantize(d)
    sb = np.repeat(s.astype(np.int64), 32)
    v = d.astype(np.float64) * np.ldexp(1.0, 127 - sb)  # in units of the block's scale
    assert np.abs(v[sb < 252]).max() <= 6.0  # nothing clips below the upper clamp
    step = np.where(np.abs(v) < 2, 0.5, np.where(np.abs(v) < 4, 1.0, 2.0))
    err = np.abs(q4f.dequantize(codes, s).astype(np.float64) * np.ldexp(1.0, 127 - sb) - v)
    keep = (sb < 252) & (sb > 2)
    assert (err[keep] <= step[keep] / 2).all() and keep.sum() > 2000


# ---- fq4_reduce's launch plan, restated (strip_plan of fa_common.h with FQ4_GEO of quant4_reduce.hip) ----------------
WAVES, LEVELS, CAP_PCT, STRIP = 4, ((4, 4), (2, 4), (1, 8)), 75, 2048


def plan(cus: int, P: int) -> list:
    S, cap = ((P + 31) // 32 + 63) // 64, max(1, cus * CAP_PCT // 100)
    span = [WAVES * v for v, _ in LEVELS]

    def launch(lv, s0, t, g):
        return dict(V=LEVELS[lv][0], U=LEVELS[lv][1], col0=s0 * STRIP, tiles=t, sw=LEVELS[lv][0], grid=g)

    t0 = -(-S // span[0])
    if t0 * 100 >= cap * 85:  # one level-0 launch, its grid capped and evened out
        return [launch(0, 0, t0, -(-t0 // -(-t0 // cap)))]
    n1 = S // span[1] if 2 * (S // span[1]) >= cus else 0  # whole level-1 tiles when they cover half the CUs
    t2 = -(-(S - n1 * span[1]) // span[2])
    return ([launch(1, 0, n1, n1)] if n1 else []) + ([launch(2, n1 * span[1], t2, t2)] if t2 else [])


@pytest.mark.parametrize("cus", (1, 8, 104, 256, 304))
def test_plan_export_equals_the_restated_plan(cus):
    from fedscale_amd import kernels_quant4 as kq4

    for P in (1, 2048, 2049, 8 * 2048 + 1, 100_000, 1_000_000, 4_000_000, 25_000_000, 25_557_032):
        got = kq4.reduce4_plan(cus, 7, P)
        assert got == plan(cus, P), (cus, P)
        assert sum(l["tiles"] * WAVES * l["sw"] for l in got) * STRIP >= P
    assert kq4.reduce4_plan(cus, 7, 0) == []


def test_wire_format_validation_and_the_residual_identity():
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 2, 3), torch.nn.BatchNorm2d(2), torch.nn.Flatten(),
                              torch.nn.Linear(2 * 6 * 6, 3))
    base = {k: v.clone() for k, v in net.state_dict().items()}
    sd = {k: v + 0.01 * torch.randn_like(v) if v.dtype == torch.float32 else v + 5 for k, v in base.items()}
    lay = BucketLayout.from_state_dict(sd)
    up, r = compress_delta4(sd, base)
    assert r is None and list(up) == ["1.num_batches_tracked", CODES_KEY, SCALES_KEY]
    assert up[CODES_KEY].shape == (16 * q4f.blocks(lay.P),) and up[SCALES_KEY].shape == (q4f.blocks(lay.P),)
    back = pickle.loads(pickle.dumps(up))
    side, codes, scales = upload_plan4(lay, back)
    assert [e.name for e, _ in side] == ["1.num_batches_tracked"] and np.array_equal(codes, up[CODES_KEY])
    side2, codes2, _ = upload_plan4(lay, list(back.values()))  # a list: the side entries, the codes, the scales
    assert np.array_equal(codes2, codes) and len(side2) == 1
    # blocks run across the entries: the upload equals the restatement of the concatenated delta
    d = np.concatenate([(sd[k] - base[k]).numpy().reshape(-1) for k in sd if sd[k].dtype == torch.float32])
    want_c, want_s, _ = q4f.quantize(d)
    assert np.array_equal(codes, q4f.pack(want_c)) and np.array_equal(scales, want_s)
    with pytest.raises(TypeError, match="0.weight.*e2m1 codes"):
        upload_plan4(lay, {k: v.numpy() for k, v in sd.items()})
    with pytest.raises(TypeError, match=f"{SCALES_KEY}.*shape"):
        upload_plan4(lay, {**back, SCALES_KEY: back[SCALES_KEY][:-1]})
    with pytest.raises(ValueError, match="residual"):
        compress_delta4(sd, base, residual=np.zeros(3, dtype=np.float32))
    # d + r_in == deq + r_out exactly: multiples of 2^-6 under an amax of 6 per block, so that every fp32 add and
    # subtraction involved is exact
    rng = np.random.default_rng(8)
    d = (rng.integers(-380, 381, 4 * 32) / 64.0).astype(np.float32)
    d[::32] = 6.0
    r_in = (rng.integers(-3, 4, d.size) / 64.0).astype(np.float32)
    r_in[::32] = 0.0
    up, r_out = compress_delta4(dict(w=torch.from_numpy(d)), [torch.zeros(d.size)], residual=r_in)
    assert (up[SCALES_KEY] == 127).all()
    q = up[CODES_KEY]
    deq = q4f.dequantize(np.stack([q & 15, q >> 4], axis=-1).reshape(-1), up[SCALES_KEY])
    assert np.array_equal(d.astype(np.float64) + r_in, deq.astype(np.float64) + r_out) and r_out.any()


def test_refused_combinations_name_the_combination():
    from fedscale_amd.cloud.aggregation import aggregator as agg
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    net = torch.nn.Linear(4, 2)
    tag = "upload_fp4='mxfp4'.*"
    with pytest.raises(ValueError, match="mxfp4"):
        TorchModelAdapter(net, upload_fp4="mxfp8")
    with pytest.raises(NotImplementedError, match=tag + "ShardedModelAdapter"):
        ShardedModelAdapter(net, devices=[0, 1], upload_fp4="mxfp4")
    with pytest.raises(NotImplementedError, match=tag + "shard"):
        TorchModelAdapter(net, shards=ShardGroup(0, 2, None, "clients"), upload_fp4="mxfp4")
    with pytest.raises(NotImplementedError, match=tag + "q-fedavg"):
        TorchModelAdapter(net, optimizer=types.SimpleNamespace(mode="q-fedavg"), upload_fp4="mxfp4")
    for kw, word in ((dict(upload_dtype="bfloat16"), "upload_dtype"), (dict(upload_quant="mxfp8"), "upload_quant"),
                     (dict(upload_topk=0.1), "upload_topk"), (dict(upload_sign="sign1"), "upload_sign"),
                     (dict(upload_lowrank=2), "upload_lowrank"), (dict(upload_vote=0.1), "upload_vote"),
                     (dict(upload_secagg=True), "upload_secagg")):
        with pytest.raises(NotImplementedError, match=tag + word):
            TorchModelAdapter(net, upload_fp4="mxfp4", **kw)
    stub = types.SimpleNamespace(upload_fp4="mxfp4")
    begin = TorchModelAdapter._begin_fp4_round  # (K, policy, capacity, signatures, clip, trim, krum, geomed)
    for i, word in ((3, "cohort signatures"), (4, "clip"), (5, "trim"), (6, "krum"), (7, "geomed")):
        args = [4, "fedavg", None, False, None, None, None, None]
        args[i] = 1
        with pytest.raises(NotImplementedError, match=tag + word):
            begin(stub, *args)
    for policy in ("fedbuff", "qfedavg"):
        with pytest.raises(NotImplementedError, match=tag + policy):
            begin(stub, 4, policy, None, False, None, None, None, None)
    with pytest.raises(NotImplementedError, match=tag + "fedbuff"):
        Quant4Round(None, "cpu", 4, "fedbuff", staging=types.SimpleNamespace(fmt="mxfp4"), last_f32=None)

    class B(agg.DeviceAsyncAggregatorMixin):
        device_upload_fp4 = "mxfp4"

    with pytest.raises(NotImplementedError, match=tag + "DeviceAsyncAggregatorMixin"):
        B().update_weight_aggregation({"client_id": 0, "update_weight": {}})
