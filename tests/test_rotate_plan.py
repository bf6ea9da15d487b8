"""CPU checks of the rotated sign upload path that need no GPU: the binding table against include/fedrotate.h, the
build's source lists, the diagonal's known answers, the host transform against the restatement
(tests/rotate_fixtures.py) and the dense matrix, the fidelity the rotation buys, the refusals and the pickling of the
adapter keyword, the staging geometry, and the fields of the measured profile."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

from fedscale_amd import _native_rotate as nr
from fedscale_amd import buildinfo
from fedscale_amd.cloud.execution import rotate_upload as ru
from fedscale_amd.cloud.execution.sign_upload import BITS_KEY, SCALES_KEY, compress_sign, encode_host
from tests import rotate_fixtures as rf
from tests import sign_fixtures as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SIZES = (1, 4095, 4096, 4097, 3 * 4096 + 257)


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


# ---- binding and build ------------------------------------------------------------------------------------------------
def test_binding_table_lists_exactly_the_headers_symbols_and_version():
    with open(os.path.join(ROOT, "include", "fedrotate.h")) as f:
        hdr = f.read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(frt_\w+)\s*\(", body))
    assert declared == set(nr.SIGNATURES) == {"frt_abi_version", "frt_padded", "frt_rotate", "frt_unrotate"}
    assert int(re.search(r"#define FRT_ABI_VERSION (\d+)", hdr).group(1)) == nr.ABI_VERSION == 1
    assert int(re.search(r"#define FRT_BLOCK (\d+)", hdr).group(1)) == nr.BLOCK == rf.BLOCK == ru.ROT_BLOCK == 4096
    lib = nr.load()
    assert lib.frt_abi_version() == nr.ABI_VERSION
    for name in nr.SIGNATURES:
        assert hasattr(lib, name)
    for P in (0, 1, 4095, 4096, 4097, 25_000_000):
        assert lib.frt_padded(P) == rf.padded(P) == ru.padded(P)
    assert lib.frt_padded(-1) == -1
    msg = lib.fa_last_error_string().decode()
    assert "frt_padded" in msg and "nothing was launched" in msg


def test_the_unit_and_header_are_in_the_build():
    assert "fedscale_amd/csrc/rotate.hip" in buildinfo.SRCS and "include/fedrotate.h" in buildinfo.HDRS


# ---- the diagonal -----------------------------------------------------------------------------------------------------
def test_splitmix_known_answers_and_the_bit_to_column_mapping():
    assert tuple(rf.diag_word(0, w) for w in range(4)) == rf.SPLITMIX_SEED0
    d = ru.diag_bits(0, 256)
    assert d.dtype == np.uint8 and d.shape == (256,)
    for w, z in enumerate(rf.SPLITMIX_SEED0):
        for k in range(64):
            assert d[64 * w + k] == (z >> k) & 1, (w, k)
    for seed in (0, 1, 0xDEADBEEF, (1 << 64) - 1):
        for n in (1, 63, 64, 65, 4097):
            assert np.array_equal(ru.diag_bits(seed, n), rf.diag(seed, n).astype(np.uint8)), (seed, n)
    assert not np.array_equal(ru.diag_bits(1, 4096), ru.diag_bits(2, 4096))
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            ru.diag_bits(bad, 8)
    with pytest.raises(TypeError, match="seed"):
        ru.diag_bits(1.5, 8)


# ---- exactness --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", SIZES)
def test_host_transform_equals_the_restatement_bit_for_bit(P):
    rng = np.random.default_rng(P)
    x = (rng.standard_normal(P) * np.ldexp(1.0, rng.integers(-15, 15, P))).astype(F32)
    base = rng.standard_normal(P).astype(F32)
    for seed in (0, (1 << 64) - 1, 0x1234ABCD):
        for b in (None, base):
            y = ru.rotate_host(x, b, seed)
            assert y.shape == (rf.padded(P),) and y.dtype == F32
            assert _bits_equal(y, rf.rotate(x, b, seed)), (P, seed)
            assert _bits_equal(ru.unrotate_host(y, P, seed), rf.unrotate(y, P, seed)), (P, seed)
    with np.errstate(over="ignore"):
        err = np.abs(ru.unrotate_host(ru.rotate_host(base, None, 5), P, 5) - base).max()
    assert err < 4e-6  # twenty-four roundings of values of order one: a round trip exact to rounding


def test_integer_inputs_equal_the_dense_product_and_round_trip_exactly():
    rng = np.random.default_rng(3)
    x = rng.integers(-2047, 2048, 4096).astype(F32)
    x[:4] = (2047, -2047, 0, 0)
    for seed in (0, 99):
        y = ru.rotate_host(x, None, seed)
        assert np.array_equal(y.astype(np.float64), rf.dense(x, seed))
        assert _bits_equal(y, rf.rotate(x, None, seed))
        back = ru.unrotate_host(y, 4096, seed)
        nz = x != 0  # a zero column comes back as +0.0 xor d[p]: equal by value
        assert np.array_equal(back, x) and _bits_equal(back[nz], x[nz])
        assert _bits_equal(back, rf.unrotate(y, 4096, seed))
    ones = np.ones(4096, dtype=F32)  # all columns positive: the one non-zero output is column 0, the rest are +0.0 or
    y = rf.butterflies(ones)         # -0.0 by "lower minus upper": 1 - 1 = +0.0, never -(1 - 1)
    assert y[0] == 64.0 and not y[1:].any() and not np.signbit(y).any()
    assert _bits_equal(ru.rotate_host(ones, None, 7), rf.rotate(ones, None, 7))


# ---- fidelity ---------------------------------------------------------------------------------------------------------
def test_the_rotation_keeps_the_energy_of_a_sparse_update():
    """A 1 %-non-zero Gaussian vector: the plain scaled sign keeps less than 0.05 of its energy, the rotated one more
    than 0.5 (five seeds gave 0.009-0.011 and 0.645-0.651), both by the reference arithmetic alone."""
    P = 16 * 4096 + 1234
    rng = np.random.default_rng(11)
    e = np.where(rng.random(P) < 0.01, rng.standard_normal(P), 0.0).astype(F32)
    bits, scales, _ = encode_host(e)
    plain = rf.kept_energy(e, bits, scales)
    y = rf.rotate(e, None, 2026)
    bits, scales, _ = encode_host(y)
    rotated = rf.kept_energy(y, bits, scales)
    print(f"kept energy: plain {plain:.4f}, rotated {rotated:.4f}")
    assert plain < 0.05 and rotated > 0.5
    # orthonormal: what is kept in rotated space is kept in parameter space
    back = rf.unrotate(sg.dequantize(bits, scales, y.size), P, 2026).astype(np.float64)
    kept = 1.0 - ((e - back) ** 2).sum() / (e.astype(np.float64) ** 2).sum()
    assert abs(kept - rotated) < 1e-3


# ---- the upload -------------------------------------------------------------------------------------------------------
def _state(rng):
    return {"w": rng.standard_normal((3, 4096)).astype(F32), "n": np.array(4, dtype=np.int64),
            "b": rng.standard_normal(777).astype(F32)}


def test_host_upload_is_the_restatements_over_two_rounds_and_rerotate_converts_the_residual():
    rng = np.random.default_rng(8)
    base = _state(rng)
    seed, r, r_f = 0xABCDEF0123456789, None, None
    for rnd in range(2):
        state = {k: (v + (rng.standard_normal(v.shape) * 0.01).astype(F32) if v.dtype == F32 else v + 1)
                 for k, v in base.items()}
        up, r = ru.compress_sign_rotated(state, base, seed, residual=r, residual_out=True)
        flat = lambda s: np.concatenate([s["w"].reshape(-1), s["b"]])  # noqa: E731
        bits, scales, r_f = rf.encode(flat(state), flat(base), seed, r_f)
        P = 3 * 4096 + 777
        assert list(up) == ["n", BITS_KEY, SCALES_KEY, ru.ROTATE_KEY] and ru.ROTATE_KEY == rf.ROTATE_KEY
        assert up[BITS_KEY].shape == (rf.padded(P) // 8,) and up[SCALES_KEY].shape == (rf.padded(P) // 256,)
        assert np.array_equal(up[BITS_KEY], bits) and _bits_equal(up[SCALES_KEY], scales)
        assert up[ru.ROTATE_KEY].dtype == np.uint64 and up[ru.ROTATE_KEY].shape == (1,)
        assert int(up[ru.ROTATE_KEY][0]) == seed and int(up["n"]) == 5
        assert r.shape == (rf.padded(P),) and _bits_equal(r, r_f)
    assert _bits_equal(ru.rerotate(r, seed, 5), rf.rotate(rf.unrotate(r_f, r_f.size, seed), None, 5))
    with pytest.raises(ValueError, match="residual.*P'=16384"):
        ru.compress_sign_rotated(state, base, seed, residual=np.zeros(3 * 4096 + 777, dtype=F32))
    with pytest.raises(ValueError, match="residual"):
        ru.rerotate(np.zeros(100, dtype=F32), 1, 2)
    with pytest.raises(ValueError, match=ru.ROTATE_KEY):
        ru.compress_sign_rotated({ru.ROTATE_KEY: np.zeros(1, dtype=F32)}, {ru.ROTATE_KEY: np.zeros(1, dtype=F32)}, 1)
    up, none = ru.compress_sign_rotated(state, base, 1)
    assert none is None


def test_sign1_without_the_option_gives_the_bytes_it_gives_today():
    rng = np.random.default_rng(9)
    base = _state(rng)
    state = {k: v + 1 if v.dtype != F32 else v + F32(0.5) for k, v in base.items()}
    up, _ = compress_sign(state, base)
    P = 3 * 4096 + 777
    assert list(up) == ["n", BITS_KEY, SCALES_KEY] and up[BITS_KEY].shape == (sg.bit_bytes(P),)


# ---- refusals and pickling --------------------------------------------------------------------------------------------
def test_refused_combinations_name_the_combination():
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.rotate_round import ROTATIONS, check_rotation
    from fedscale_amd.state import ShardGroup

    assert ROTATIONS == ("rht4096",) and check_rotation("rht4096") == "rht4096"
    net = torch.nn.Linear(4, 2)
    with pytest.raises(NotImplementedError, match=r"upload_rotate='rht4096'.*upload_sign"):
        TorchModelAdapter(net, upload_rotate="rht4096")
    for bad in ("rht", "sign1", 4096, True):
        with pytest.raises(ValueError, match="upload_rotate"):
            TorchModelAdapter(net, upload_sign="sign1", upload_rotate=bad)
        with pytest.raises(ValueError, match="upload_rotate"):
            TorchModelAdapter(net, upload_rotate=bad)
    rot = dict(upload_sign="sign1", upload_rotate="rht4096")
    # everything upload_sign refuses stays refused, by upload_sign's name
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*ShardedModelAdapter"):
        ShardedModelAdapter(net, devices=[0, 1], **rot)
    with pytest.raises(NotImplementedError, match=r"upload_rotate='rht4096'.*ShardedModelAdapter"):
        ShardedModelAdapter(net, devices=[0, 1], upload_rotate="rht4096")
    for mode in ("params", "clients"):
        with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*shard"):
            TorchModelAdapter(net, shards=ShardGroup(0, 2, None, mode), **rot)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*q-fedavg"):
        TorchModelAdapter(net, optimizer=types.SimpleNamespace(mode="q-fedavg"), **rot)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*upload_dtype='bfloat16'"):
        TorchModelAdapter(net, upload_dtype="bfloat16", **rot)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*upload_quant='mxfp8'"):
        TorchModelAdapter(net, upload_quant="mxfp8", **rot)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*upload_topk=0\.01"):
        TorchModelAdapter(net, upload_topk=0.01, **rot)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*upload_secagg"):
        TorchModelAdapter(net, upload_secagg=True, **rot)
    stub = types.SimpleNamespace(**rot)
    begin = TorchModelAdapter._begin_sign_round  # (K, policy, capacity, signatures, clip, trim)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*cohort signatures"):
        begin(stub, 4, "fedavg", None, True, None, None)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*fedbuff"):
        begin(stub, 4, "fedbuff", None, False, None, None)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*clip"):
        begin(stub, 4, "fedavg", None, False, object(), None)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1'.*trim"):
        begin(stub, 4, "fedavg", None, False, None, 1)
    robust = types.SimpleNamespace(upload_topk=None, upload_quant=None, upload_dtype=None, **rot)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1' \(1-bit sign delta uploads\)"):
        TorchModelAdapter._check_krum(robust, "fedavg", False, None, None, 1)
    with pytest.raises(NotImplementedError, match=r"upload_sign='sign1' \(1-bit sign delta uploads\)"):
        TorchModelAdapter._check_geomed(robust, "fedavg", False, None, None, None, True)


def test_pickling_carries_both_keywords_and_an_unset_option_changes_nothing():
    from fedscale_amd.cloud.internal import torch_model_adapter as tma

    net = torch.nn.Linear(4, 2)
    stub = types.SimpleNamespace(upload_sign="sign1", upload_rotate="rht4096", upload_topk=None, upload_quant=None,
                                 upload_dtype=None, optimizer=None, get_model=lambda: net)
    fn, args = tma.TorchModelAdapter.__reduce__(stub)
    assert fn is tma._rebuild_with_upload_rotate and args == (types.SimpleNamespace, net, None, "sign1", "rht4096")
    seen = {}

    class Fake:
        def __init__(self, model, optimizer, upload_sign=None, upload_rotate=None):
            seen.update(model=model, optimizer=optimizer, upload_sign=upload_sign, upload_rotate=upload_rotate)

    assert type(fn(Fake, *args[1:])) is Fake
    assert seen == dict(model=net, optimizer=None, upload_sign="sign1", upload_rotate="rht4096")
    # unset: the class default, nothing on the instance, and __reduce__ is what it was
    assert tma.TorchModelAdapter.upload_rotate is None
    calls = []
    init = tma._takes_upload_rotate(lambda self, *a, **kw: calls.append((a, kw)))
    for kw in ({}, {"upload_rotate": None}):
        obj = types.SimpleNamespace()
        init(obj, 1, upload_sign="sign1", **kw)
        assert "upload_rotate" not in obj.__dict__ and calls[-1] == ((1,), {"upload_sign": "sign1"})
    obj = types.SimpleNamespace()
    init(obj, upload_rotate="rht4096")
    assert obj.__dict__ == {"upload_rotate": "rht4096"}
    sign_only = types.SimpleNamespace(upload_sign="sign1", upload_topk=None, upload_quant=None, upload_dtype=None,
                                      optimizer=None, get_model=lambda: net)
    fn, args = tma.TorchModelAdapter.__reduce__(sign_only)
    assert fn is tma._rebuild_with_upload_sign and args == (types.SimpleNamespace, net, None, "sign1")
    plain = types.SimpleNamespace(upload_quant=None, upload_dtype=None, optimizer=None, get_model=lambda: net)
    assert tma.TorchModelAdapter.__reduce__(plain) == (types.SimpleNamespace, (net, None))


def test_mixins_pass_device_upload_rotate_through_and_refuse_it_where_the_format_is_refused():
    from fedscale_amd.cloud.aggregation import aggregator as agg

    assert agg.DeviceAggregatorMixin.device_upload_rotate is None
    assert agg.DeviceAsyncAggregatorMixin.device_upload_rotate is None  # inherited
    assert agg.DeviceCohortAggregatorMixin.device_upload_rotate is None

    class Base:
        def init_model(self):
            self.model_wrapper = types.SimpleNamespace(get_model=lambda: torch.nn.Linear(4, 2))

    class Sharded(agg.DeviceAggregatorMixin, Base):
        device_upload_rotate = "rht4096"
        device_shards = [0, 1]
        args = types.SimpleNamespace(gradient_policy=None)

    with pytest.raises(NotImplementedError, match=r"upload_rotate='rht4096'.*ShardedModelAdapter"):
        Sharded().init_model()

    class Unknown(agg.DeviceAggregatorMixin, Base):  # one device: the keywords reach TorchModelAdapter, which checks
        device_upload_sign = "sign1"
        device_upload_rotate = "no-such-rotation"
        args = types.SimpleNamespace(gradient_policy=None)

    with pytest.raises(ValueError, match="upload_rotate 'no-such-rotation'"):
        Unknown().init_model()

    class Alone(agg.DeviceAggregatorMixin, Base):
        device_upload_rotate = "rht4096"
        args = types.SimpleNamespace(gradient_policy=None)

    with pytest.raises(NotImplementedError, match=r"upload_rotate='rht4096'.*upload_sign"):
        Alone().init_model()

    class Async(agg.DeviceAsyncAggregatorMixin):
        device_upload_rotate = "rht4096"

    with pytest.raises(NotImplementedError, match=r"upload_rotate='rht4096'.*DeviceAsyncAggregatorMixin"):
        Async().update_weight_aggregation({"client_id": 0, "update_weight": {}})

    spec = {"device_krum": "_krum_spec", "device_geomed": "_geomed_spec", "device_upload_secagg": "_secagg_spec"}
    for attr, val in (("device_krum", 1), ("device_geomed", True), ("device_upload_secagg", True)):
        C = type("C", (agg.DeviceAggregatorMixin,), {"device_upload_rotate": "rht4096", attr: val})
        with pytest.raises(NotImplementedError, match=r"device_upload_rotate='rht4096'"):
            getattr(C(), spec[attr])()


# ---- staging geometry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (4096 - 1, 4096, 4096 + 1, 2 * 4096 + 777))
def test_staging_geometry_comes_from_the_padded_columns(P):
    from fedscale_amd import kernels_sign as kg
    from fedscale_amd.rotate_round import _RotatedColumns, seed_of, strip_seed

    lay = types.SimpleNamespace(P=P, ld=(P + 63) // 64 * 64, Q=1, ldq=4, world=1, f_entries=[], i_entries=[])
    cols = _RotatedColumns(lay)
    Pp = rf.padded(P)
    assert cols.P == Pp and cols.ld == lay.ld and cols.ldq == 4 and cols.world == 1 and lay.P == P
    assert kg.bit_bytes(cols.P) == Pp // 8 and kg.blocks(cols.P) == Pp // 256
    assert kg.bit_stride(cols.P) == Pp // 8 and kg.scale_stride(cols.P) == Pp // 256  # whole blocks: no slack
    up = {"n": np.array(1), BITS_KEY: np.zeros(Pp // 8, np.uint8), SCALES_KEY: np.zeros(Pp // 256, F32),
          ru.ROTATE_KEY: np.array([7], dtype=np.uint64)}
    assert seed_of(up) == 7 and list(strip_seed(up)) == ["n", BITS_KEY, SCALES_KEY]
    assert seed_of(list(up.values())) == 7 and len(strip_seed(list(up.values()))) == 3
    assert seed_of(strip_seed(up)) is None and seed_of(list(strip_seed(up).values())) is None


# ---- the measured profile ---------------------------------------------------------------------------------------------
def test_the_measured_file_carries_the_fields_the_documents_quote():
    """profiles/rotate_measure.json (tools/rotate_measure.py, a run on the card): the two kernel shapes with each
    call's time, algorithmic bytes and share of the read ceiling, the three round shapes with the rotated round beside
    the plain one and the one-extra-pass prediction, and the kept-energy table.  No time is asserted."""
    with open(os.path.join(ROOT, "profiles", "rotate_measure.json")) as f:
        m = json.load(f)
    assert m["read_ceiling_Bps"] == 7.23e12 and m["build_defs"] == "" and m["calls_per_median"] >= 20
    kernels = {k["P"]: k for k in m["kernels"]}
    assert set(kernels) == {1_000_000, 25_000_000}
    for P, k in kernels.items():
        Pp = rf.padded(P)
        assert k["P_padded"] == Pp
        assert k["frt_rotate"]["bytes"] == 8 * P + 4 * Pp        # x and base read, y written: 12 B / column
        assert k["frt_unrotate"]["bytes"] == 4 * Pp + 4 * P      # y read, out written: 8 B / column
        assert k["fsg_sign_row"]["bytes"] == 4 * Pp + Pp // 8 + 4 * (Pp // 256)
        for name in ("frt_rotate", "frt_unrotate", "fsg_sign_row"):
            e = k[name]
            assert e["ms_median"] > 0 and e["TBps"] > 0 and 0 < e["share_of_read_ceiling"] <= 1.0, name
    rounds = {(r["K"], r["P"]): r for r in m["rounds"]}
    assert set(rounds) == {(100, 1_000_000), (100, 25_000_000), (1000, 25_000_000)}
    for r in rounds.values():
        assert r["plain_round_ms"] > 0 and r["rotated_round_ms"] > 0
        assert r["extra_ms"] == pytest.approx(r["rotated_round_ms"] - r["plain_round_ms"], abs=1e-3)
        assert r["predicted_extra_ms"] > 0 and isinstance(r["meets_prediction"], bool)
    fid = {f["update"]: f for f in m["kept_energy"]}
    assert set(fid) == {"gaussian", "laplace", "student_t_3", "sparse_1pct_gaussian", "gaussian_lognormal_scales",
                        "student_t_1.5"}
    for f in fid.values():
        assert 0 < f["sign1"] < 1 and 0 < f["sign1_rht4096"] < 1 and f["P"] > 0
