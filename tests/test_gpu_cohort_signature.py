"""Auxo cohort signatures on the device (fedscale_amd/cohort_signature.py, include/fedcohort.h) against the
reference's recorded results (tests/golden/auxo_sig_*.npz: the real ``register_gradient`` plus the numpy /
sklearn lines of ``cohort_clustering``).

Criteria: signatures, mean and centred matrix bit-exact (uint16 view; NaN only where the reference has NaN), on
every staging path; norms within the fp64 any-order summation bound D * 2^-52; normalized bit-exact against
half(float(c) / float(norm)) from the device's own norms, and against the fp64-exact normalisation no worse
than sklearn's own float16 result and within 1 float16 ulp; the Gram within the any-order bound for exact
f16 x f16 products accumulated in fp32, D * 2^-24 * sqrt(G_ii * G_jj) (plus 2^-14 * (|c_i|_1 + |c_j|_1) where
the matrix may hold float16 subnormals, which a matrix unit may flush), exactly symmetric and repeatable."""
import ctypes

import numpy as np
import pytest
import torch

from tests.cohort_sig_fixtures import FIXTURES, load

pytestmark = pytest.mark.gpu

FINITE = [n for n in FIXTURES if n != "auxo_sig_values_k6"]  # (its centred matrix holds inf / NaN by design)
MODES = ("mirror", "chunks3", "device")
_ROUNDS = {}


def _bits_equal(got, want, ctx):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float16 and want.dtype == np.float16 and got.shape == want.shape, ctx
    nan = np.isnan(want.astype(np.float32))
    assert np.array_equal(np.isnan(got.astype(np.float32)), nan), f"{ctx}: NaN where the reference has none"
    g, w = got.view(np.uint16)[~nan], want.view(np.uint16)[~nan]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{ctx}: {bad.size} of {w.size} differ, first {bad[:4]}: {g[bad[:4]]} != {w[bad[:4]]}"


def _round(name, mode, signatures=True):
    """One cohort round of the fixture through DeviceCohortAggregatorMixin (shared by the tests; never modified).
    mirror: host uploads, one chunk (a small round is read straight out of the staging's pinned mirror);
    chunks3: device_round_capacity = 3 (K = 9: three chunks, signatures taken in _fold_chunk and at the finish);
    device: uploads are torch tensors already on the GPU (the regular device staging slots)."""
    key = (name, mode, signatures)
    if key in _ROUNDS:
        return _ROUNDS[key]
    from fedscale_amd.cloud.aggregation.aggregator import DeviceCohortAggregator
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    fx = load(name)

    class Agg(DeviceCohortAggregator):
        device_cohort_signatures = signatures
        device_round_capacity = 3 if mode == "chunks3" else None

    w = TorchModelAdapter(fx.module(), device="cuda:0")
    agg = Agg([w], [fx.K])
    ids = [100 + 7 * k for k in range(fx.K)]
    for k in range(fx.K):
        up = fx.upload(k)
        if mode == "device":
            up = {n: torch.from_numpy(v).to("cuda:0") for n, v in up.items()}
        agg.on_result({"client_id": ids[k], "update_weight": up}, 0)
    out = _ROUNDS[key] = (fx, agg, w, ids)
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FIXTURES)
def test_signatures_mean_and_centred_are_bit_exact(gpu_device, name, mode):
    fx, agg, w, ids = _round(name, mode)
    sigs = agg.cohort_signatures[0]
    assert sigs.client_ids == ids and sigs.K == fx.K and sigs.D == fx.expected("sig").shape[1]
    raw = sigs.raw()
    assert raw.dtype == torch.float16 and raw.device.type == "cuda" and tuple(raw.shape) == (fx.K, sigs.D)
    _bits_equal(raw.cpu().numpy(), fx.expected("sig"), f"{name}/{mode} raw")
    _bits_equal(sigs.mean().cpu().numpy(), fx.expected("mean"), f"{name}/{mode} mean")
    _bits_equal(sigs.centered().cpu().numpy(), fx.expected("centered"), f"{name}/{mode} centered")
    assert sigs.centered() is not None and sigs._centered() is sigs._centered()  # computed once


@pytest.mark.parametrize("name", FIXTURES)
def test_staging_paths_give_identical_bits(gpu_device, name):
    got = [_round(name, m)[1].cohort_signatures[0].raw().cpu().numpy().view(np.uint16) for m in MODES]
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


@pytest.mark.parametrize("name", FINITE)
def test_norms_within_the_fp64_summation_bound(gpu_device, name):
    sigs = _round(name, "mirror")[1].cohort_signatures[0]
    c = sigs.centered().cpu().numpy().astype(np.float64)
    want = np.sqrt((c * c).sum(axis=1))
    got = sigs.norms().cpu().numpy()
    assert got.dtype == np.float64
    rel = np.abs(got - want) / np.where(want > 0, want, 1.0)
    print(f"{name}: norms max rel err {rel.max():.3g} (bound {sigs.D * 2.0 ** -52:.3g})")
    assert (rel <= sigs.D * 2.0 ** -52).all()


@pytest.mark.parametrize("name", FINITE)
def test_normalized_from_the_devices_own_norms_and_against_sklearn(gpu_device, name):
    fx, agg, _, _ = _round(name, "mirror")
    sigs = agg.cohort_signatures[0]
    c = sigs.centered().cpu().numpy()
    n = sigs.norms().cpu().numpy().copy()
    got = sigs.normalized().cpu().numpy()
    n[n == 0.0] = 1.0
    want = (c.astype(np.float32) / n.astype(np.float32)[:, None]).astype(np.float16)
    _bits_equal(got, want, f"{name} normalized")
    # against the fp64-exact normalisation of the same centred matrix: no worse than sklearn's float16 result
    c64 = c.astype(np.float64)
    n64 = np.sqrt((c64 * c64).sum(axis=1))
    n64[n64 == 0.0] = 1.0
    exact = c64 / n64[:, None]
    err_dev = np.abs(got.astype(np.float64) - exact)
    err_skl = np.abs(fx.expected("normalized").astype(np.float64) - exact)
    ulp = np.maximum(2.0 ** (np.floor(np.log2(np.maximum(np.abs(exact), 2.0 ** -14))) - 10), 2.0 ** -24)
    print(f"{name}: normalized max abs err device {err_dev.max():.3g}, sklearn {err_skl.max():.3g}, "
          f"device max ulps {(err_dev / ulp).max():.3f}")
    assert err_dev.max() <= err_skl.max()
    assert (err_dev <= ulp).all()


def test_normalize_leaves_a_zero_row_as_zeros(gpu_device):
    from fedscale_amd.cohort_signature import CohortSignatures

    rng = np.random.default_rng(0)
    row = rng.normal(0, 1e-2, size=(1, 200)).astype(np.float16)
    sig = torch.from_numpy(np.repeat(row, 3, axis=0)).to(gpu_device)  # identical rows: the centred matrix is zero
    s = CohortSignatures(sig, 3, 200)
    assert int(torch.count_nonzero(s.centered())) == 0 and int(torch.count_nonzero(s.norms())) == 0
    out = s.normalized().cpu().numpy()
    assert np.array_equal(out.view(np.uint16), np.zeros((3, 200), dtype=np.uint16))
    assert int(torch.count_nonzero(s.gram())) == 0
    # one zero row among others (fc_normalize directly, norms supplied)
    from fedscale_amd import cohort_signature as cs

    c = rng.normal(0, 1e-2, size=(4, 77)).astype(np.float16)
    c[2] = 0
    n = np.sqrt((c.astype(np.float64) ** 2).sum(axis=1))
    got = cs.normalize(torch.from_numpy(c).to(gpu_device), 4, 77, torch.from_numpy(n).to(gpu_device)).cpu().numpy()
    n[2] = 1.0
    _bits_equal(got, (c.astype(np.float32) / n.astype(np.float32)[:, None]).astype(np.float16), "normalize")
    assert not got[2].any()


def _gram_check(c16: np.ndarray, got: np.ndarray, subnormal_allowance: bool, ctx: str):
    K, D = c16.shape
    c64 = c16.astype(np.float64)
    g64 = c64 @ c64.T
    diag = np.sqrt(np.outer(np.diag(g64), np.diag(g64)))
    bound = D * 2.0 ** -24 * diag
    if subnormal_allowance:
        l1 = np.abs(c64).sum(axis=1)
        bound = bound + 2.0 ** -14 * (l1[:, None] + l1[None, :])
    err = np.abs(got.astype(np.float64) - g64)
    frac = (err / np.where(bound > 0, bound, 1.0)).max()
    print(f"{ctx}: max |G - G64| / bound = {frac:.3g}")
    assert got.dtype == np.float32 and got.shape == (K, K)
    assert (err <= bound).all(), f"{ctx}: {(err > bound).sum()} elements beyond the bound (max ratio {frac:.3g})"
    assert np.array_equal(got, got.T), f"{ctx}: not exactly symmetric"


def _gram_matrix(K, D, seed):
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-3, 0, size=(K, 1))  # rows of different magnitude
    c = (rng.normal(0, 1, size=(K, D)) * scale).astype(np.float16)
    c[np.abs(c.astype(np.float32)) < 2.0 ** -14] = 0  # no float16 subnormals
    return c


@pytest.mark.parametrize("D", [1, 7, 4097, 20001])
@pytest.mark.parametrize("K", [1, 5, 33, 64, 129])
def test_gram_of_supplied_matrices(gpu_device, K, D):
    from fedscale_amd import cohort_signature as cs

    c = _gram_matrix(K, D, 1000 * K + D)
    t = torch.from_numpy(c).to(gpu_device)
    got = cs.gram(t).cpu().numpy()
    _gram_check(c, got, False, f"gram K={K} D={D}")
    assert np.array_equal(cs.gram(t).cpu().numpy().view(np.uint32), got.view(np.uint32)), "second call differs"


def test_gram_of_a_padded_aligned_matrix(gpu_device):
    """The 16-byte load path (16-byte aligned base, row stride a multiple of 8) with K and D off the tile shape;
    the padding columns hold garbage that must not enter the result."""
    from fedscale_amd import cohort_signature as cs

    K, D, ldd = 70, 4100, 4160
    c = _gram_matrix(K, D, 5)
    buf = torch.full((K, ldd), 3.0, dtype=torch.float16, device=gpu_device)
    buf[:, :D] = torch.from_numpy(c).to(gpu_device)
    got = cs.gram(buf, K, D).cpu().numpy()
    _gram_check(c, got, False, "gram padded")
    assert np.array_equal(cs.gram(torch.from_numpy(c).to(gpu_device)).cpu().numpy(), got)  # = the element-wise path


@pytest.mark.parametrize("name", FINITE)
def test_gram_and_host_helpers_of_a_fixture(gpu_device, name):
    sigs = _round(name, "mirror")[1].cohort_signatures[0]
    c = sigs.centered().cpu().numpy()
    g = sigs.gram()
    assert g is sigs.gram()  # computed once
    _gram_check(c, g.cpu().numpy(), True, f"gram {name}")
    c64 = c.astype(np.float64)
    n = np.sqrt((c64 * c64).sum(axis=1))
    n1 = np.where(n > 0, n, 1.0)
    tol = sigs.D * 2.0 ** -24 + 2.0 ** -14 * 2 * np.abs(c64).sum(axis=1).max() / max((n1 * n1).min(), 1e-300)
    assert np.abs(sigs.cosine() - (c64 @ c64.T) / np.outer(n1, n1)).max() <= tol + 1e-12
    d2 = ((c64[:, None, :] - c64[None, :, :]) ** 2).sum(axis=2)
    scale = (n * n).max()
    assert np.abs(sigs.pairwise_sqdist() - d2).max() <= 4 * (sigs.D * 2.0 ** -24 * scale) + \
        2.0 ** -13 * 2 * np.abs(c64).sum(axis=1).max() + 1e-12
    cen, nrm = sigs.features()
    assert cen.dtype == np.float16 and nrm.dtype == np.float16 and cen.shape == nrm.shape == (sigs.K, sigs.D)
    assert np.array_equal(cen.view(np.uint16), c.view(np.uint16))


def test_signatures_off_changes_nothing_and_on_leaves_the_model_bit_identical(gpu_device):
    from oracle.cpu_reference import OracleCohortAggregator, OracleModel, OracleModelAdapter

    for name in ("auxo_sig_mixed_k9", "auxo_sig_femnist_cnn_k10"):
        fx, agg_off, w_off, _ = _round(name, "mirror", signatures=False)
        assert not hasattr(agg_off, "cohort_signatures") and not hasattr(agg_off, "_cohort_round_clients")
        ref = OracleModelAdapter(OracleModel(fx.names, [torch.from_numpy(np.array(m)) for m in fx.model]))
        oagg = OracleCohortAggregator([ref], [fx.K])
        for k in range(fx.K):
            oagg.on_result({"client_id": k, "update_weight": fx.upload(k)}, 0)
        want = ref.get_weights()
        for mode in MODES:
            w_on = _round(name, mode)[2]
            for a, b, c in zip(w_off.get_weights(), w_on.get_weights(), want):
                assert a.dtype == b.dtype == c.dtype and torch.equal(a, c) and torch.equal(b, c), (name, mode)


def test_fedbuff_rounds_keep_signatures_too(gpu_device):
    """DeviceRound with a signature plan under the FedBuff policy, two chunks: the same signature bits."""
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    fx = load("auxo_sig_mixed_k9")
    w = TorchModelAdapter(fx.module(), device="cuda:0")
    rnd = w.begin_round(fx.K, "fedbuff", capacity=5, signatures=True)
    for k in range(fx.K):
        rnd.add(fx.upload(k), weight=1.0 / (1 + k % 3) ** 0.5)
    den = sum(1.0 / (1 + k % 3) ** 0.5 for k in range(fx.K))
    w.apply_round(rnd, float(np.float32(den)), float(den))
    _bits_equal(rnd.cohort_signatures(range(fx.K)).raw().cpu().numpy(), fx.expected("sig"), "fedbuff raw")
    with pytest.raises(NotImplementedError):
        w.begin_round(3, "qfedavg", signatures=True)


def test_fedyogi_round_keeps_signatures_too(gpu_device):
    """A cohort whose adapter carries the fed-yogi server optimizer finishes through finalize_mean's other branch
    (the mean into its own buffer, then the YoGi step): the signatures are taken there too, against the model the
    round started from, in both of two consecutive rounds."""
    import argparse

    from fedscale_amd.cloud.aggregation.aggregator import DeviceCohortAggregator
    from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    fx = load("auxo_sig_mixed_k9")
    args = argparse.Namespace(gradient_policy="fed-yogi", yogi_eta=3e-3, yogi_tau=1e-8, yogi_beta=0.9,
                              yogi_beta2=0.99, learning_rate=0.05, qfed_q=1.0)
    w = TorchModelAdapter(fx.module(), device="cuda:0", optimizer=TorchServerOptimizer("fed-yogi", args, "cuda:0"))

    class Agg(DeviceCohortAggregator):
        device_cohort_signatures = True

    agg = Agg([w], [fx.K])
    for k in range(fx.K):
        agg.on_result({"client_id": k, "update_weight": fx.upload(k)}, 0)
    _bits_equal(agg.cohort_signatures[0].raw().cpu().numpy(), fx.expected("sig"), "fed-yogi raw")
    # the second round starts from the stepped model: last - x with that model, restated on the host
    model2 = [t.numpy() for t in w.get_weights()]
    agg.model_in_update[0] = 0
    for k in range(fx.K):
        agg.on_result({"client_id": k, "update_weight": fx.upload(k)}, 0)
    D = fx.expected("sig").shape[1]
    want = np.stack([np.concatenate([(m - fx.upload(k)[n]).reshape(-1).astype(np.float64)
                                     for n, m in zip(fx.names, model2)])[-D:].astype(np.float16)
                     for k in range(fx.K)])
    _bits_equal(agg.cohort_signatures[0].raw().cpu().numpy(), want, "fed-yogi raw, round 2")


def test_center_element_wise_path_matches_the_16_byte_path(gpu_device):
    """fc_center on a matrix whose row stride is odd (203 float16: no 16-byte loads or stores anywhere) and on a
    misaligned base: the same bits as numpy's order of operations and as the aligned, padded copy."""
    from fedscale_amd.cohort_signature import CohortSignatures

    rng = np.random.default_rng(12)
    K, D = 7, 203
    sig = (rng.normal(0, 1, size=(K, D)) * 10.0 ** rng.uniform(-4, 1, size=(1, D))).astype(np.float16)
    acc = sig[0].astype(np.float32)
    for k in range(1, K):
        acc = acc + sig[k].astype(np.float32)
    avg = (acc / np.float32(K)).astype(np.float16)
    cen = (sig.astype(np.float32) - avg.astype(np.float32)).astype(np.float16)
    odd = CohortSignatures(torch.from_numpy(sig).to(gpu_device), K, D)  # ldd = 203
    pad = torch.zeros(K, 256, dtype=torch.float16, device=gpu_device)
    pad[:, :D] = torch.from_numpy(sig).to(gpu_device)
    vec = CohortSignatures(pad, K, D)  # ldd = 256, 16-byte aligned
    shifted = torch.zeros(K * 208 + 1, dtype=torch.float16, device=gpu_device)[1:].view(K, 208)  # base 2 bytes off
    shifted[:, :D] = torch.from_numpy(sig).to(gpu_device)
    off = CohortSignatures(shifted, K, D)
    for name, s in (("odd stride", odd), ("aligned", vec), ("misaligned base", off)):
        _bits_equal(s.mean().cpu().numpy(), avg, f"{name} mean")
        _bits_equal(s.centered().cpu().numpy(), cen, f"{name} centered")
        c64 = cen.astype(np.float64)
        want = (c64 * c64).sum(axis=1)
        assert (np.abs(s.sumsq().cpu().numpy() - want) <= D * 2.0 ** -52 * want).all(), name
        _bits_equal(s.normalized().cpu().numpy(),
                    (cen.astype(np.float32) / s.norms().cpu().numpy().astype(np.float32)[:, None])
                    .astype(np.float16), f"{name} normalized")


def test_sharded_adapters_in_a_cohort_aggregator(gpu_device):
    """ShardedModelAdapter wrappers (two parts on the one GPU): with the switch off the cohort round works as it
    did and gives the oracle's bits; with it on, the first result raises NotImplementedError with a clear message."""
    from fedscale_amd.cloud.aggregation.aggregator import DeviceCohortAggregator
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter
    from oracle.cpu_reference import OracleCohortAggregator, OracleModel, OracleModelAdapter

    fx = load("auxo_sig_mixed_k9")
    w = ShardedModelAdapter(fx.module(), devices=[0, 0], transport="copy")
    try:
        agg = DeviceCohortAggregator([w], [fx.K])
        ref = OracleModelAdapter(OracleModel(fx.names, [torch.from_numpy(np.array(m)) for m in fx.model]))
        oagg = OracleCohortAggregator([ref], [fx.K])
        for k in range(fx.K):
            agg.on_result({"client_id": k, "update_weight": fx.upload(k)}, 0)
            oagg.on_result({"client_id": k, "update_weight": fx.upload(k)}, 0)
        for a, b in zip(w.get_weights(), ref.get_weights()):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert not hasattr(agg, "cohort_signatures")

        class On(DeviceCohortAggregator):
            device_cohort_signatures = True

        with pytest.raises(NotImplementedError, match="sharded over 2 parts"):
            On([w], [fx.K]).on_result({"client_id": 0, "update_weight": fx.upload(0)}, 0)
    finally:
        w.close()


# ---- operand checks of the new launching entry points (as tests/test_gpu_abi_operands.py for the old table) ----
K_, LD, LDD, Q_ = 40, 64, 64, 3


def _abi_cases(dev, st):
    def f(n, v, dt):
        return torch.full((n,), v, dtype=dt, device=dev)

    from fedscale_amd import _native_cohort as nc

    lib = nc.load()
    segs = np.asarray([[3, 0, 20], [40, 21, 24]], dtype=np.int64)
    isegs = np.asarray([[1, 20]], dtype=np.int64)
    ws_c = lib.fc_center_workspace_bytes(K_, LDD - 4)
    ws_g = lib.fc_gram_workspace_bytes(K_, LDD - 4)
    h = torch.float16
    cases = [
        ("fc_signature", dict(x=f(K_ * LD, 0.5, torch.float32), last=f(LD, 1.0, torch.float32),
                              xi=f(K_ * Q_, 3, torch.int64), last_i64=f(Q_, 5, torch.int64), sig_out=f(K_ * LDD, 9.0, h)),
         ["sig_out"], lambda p: (p["x"], LD, K_, p["last"], p["xi"], Q_, p["last_i64"], segs.ctypes.data, 2,
                                 isegs.ctypes.data, 1, p["sig_out"], LDD, st), {"x", "xi"}),
        ("fc_center", dict(sig=f(K_ * LDD, 0.25, h), avg16_out=f(LDD, 9.0, h), centered_out=f(K_ * LDD, 9.0, h),
                           sumsq_out=f(K_, 9.0, torch.float64), workspace=f(ws_c // 8, 9.0, torch.float64)),
         ["avg16_out", "centered_out", "sumsq_out"],
         lambda p: (p["sig"], LDD, K_, LDD - 4, p["avg16_out"], p["centered_out"], p["sumsq_out"], p["workspace"], st),
         set()),
        ("fc_normalize", dict(centered=f(K_ * LDD, 0.25, h), norm_in=f(K_, 2.0, torch.float64),
                              normalized_out=f(K_ * LDD, 9.0, h)), ["normalized_out"],
         lambda p: (p["centered"], LDD, K_, LDD - 4, p["norm_in"], p["normalized_out"], st), set()),
        ("fc_gram", dict(c=f(K_ * LDD, 0.25, h), gram_out=f(K_ * K_, 9.0, torch.float32),
                         workspace=f(max(4, ws_g // 4), 9.0, torch.float32)), ["gram_out"],
         lambda p: (p["c"], LDD, K_, LDD - 4, p["gram_out"], p["workspace"], st), set()),
    ]
    return lib, cases, (segs, isegs)


_STREAMS = []


def _abi_stream():
    """A non-null blocking stream (ordered after what torch filled on the null stream)."""
    if not _STREAMS:
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipStreamCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        s = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(s)) == 0
        _STREAMS.append(s.value)
    return _STREAMS[0]


def test_new_entry_points_reject_pageable_and_misplaced_pinned_operands(gpu_device):
    st = _abi_stream()
    lib, cases, keep = _abi_cases(gpu_device, st)
    pageable = np.zeros(1 << 17, dtype=np.float64)
    pinned = torch.zeros(1 << 17, dtype=torch.float64).pin_memory()
    launching = set()
    for name, ops, outs, args, host_ok in cases:
        fn = getattr(lib, name)
        launching.add(name)
        for bad_name in ops:
            for kind, bad in (("pageable", pageable.ctypes.data), ("pinned", pinned.data_ptr())):
                snap = {n: ops[n].clone() for n in outs if n != bad_name}
                rc = fn(*args({n: (bad if n == bad_name else t.data_ptr()) for n, t in ops.items()}))
                msg = lib.fa_last_error_string().decode()
                if kind == "pinned" and bad_name in host_ok:  # the staging's pinned mirror is read over PCIe
                    assert rc == 0, (name, bad_name, msg)
                    torch.cuda.synchronize()
                    continue
                want = "pageable" if kind == "pageable" else "pinned host memory"
                assert rc == -1 and want in msg and "nothing was launched" in msg and bad_name in msg, \
                    (name, bad_name, kind, rc, msg)
                torch.cuda.synchronize()
                for n, t in snap.items():
                    assert torch.equal(ops[n], t), f"{name}: {n} was written"
        rc = fn(*args({n: t.data_ptr() for n, t in ops.items()}))  # every operand valid: the call goes through
        assert rc == 0, (name, lib.fa_last_error_string().decode())
    torch.cuda.synchronize()
    from fedscale_amd import _native_cohort as nc

    assert set(nc.SIGNATURES) - {"fc_abi_version", "fc_center_workspace_bytes", "fc_gram_workspace_bytes"} == launching
    del keep


def test_new_entry_points_reject_a_too_short_buffer(gpu_device):
    """An operand whose extent the call needs lies partly outside its allocation (its own hipMalloc: torch's
    caching allocator would hand out a slice of a larger segment): refused, nothing launched."""
    st = _abi_stream()
    lib, cases, keep = _abi_cases(gpu_device, st)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    short = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(short), 256) == 0  # shorter than any operand's 40 rows (5 KB and more)
    try:
        for (name, ops, outs, args, _), bad_name in zip(cases, ("x", "sig", "normalized_out", "c")):
            snap = {n: ops[n].clone() for n in outs if n != bad_name}
            rc = getattr(lib, name)(*args({n: (short.value if n == bad_name else t.data_ptr())
                                           for n, t in ops.items()}))
            msg = lib.fa_last_error_string().decode()
            assert rc == -1 and bad_name in msg and "past the end of its allocation" in msg, (name, rc, msg)
            torch.cuda.synchronize()
            for n, t in snap.items():
                assert torch.equal(ops[n], t), f"{name}: {n} was written"
    finally:
        torch.cuda.synchronize()
        hip.hipFree(short)
    del keep
