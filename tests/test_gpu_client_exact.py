"""The client kernels (fedscale_amd/csrc/client_update.hip) past one launch group, against exact host references:
DP norms, clip and noise over more than MT_MAX = 64 tensors and tensors of more than 64 workgroups, the fused SGD
step over more than SGD_MAX = 48 tensors, every element (unaligned) path, and the counter-based N(0,1) stream
against its host twin.

Criteria.  Everything but the noise values is bit equality: with ``oracle.cpu_reference.dp_clip_exact`` under a
precondition asserted on the reference alone (``client_kernel_models.dp_precondition``), with numpy's separately
rounded fp32 ops for recover / clip / upload, with ``sgd_prox_step_ref`` for the fused step (fma or not).  Outputs
are compared over their whole allocations: what lies between the views keeps the value the test put there.  The
noise values are compared with the float64 twin under a derived bound (test_noise_stream_matches_the_twin).

The inputs and expected results come from tests/client_kernel_models.py; tests/test_client_oracle.py shows on a
host restatement of each kernel that one planted indexing mistake at a time changes these results."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle.cpu_reference import dp_clip_exact, dp_normals_ref, dp_privatize
from tests import client_kernel_models as ckm
from tests.client_kernel_models import F32, F64, same_bits

pytestmark = pytest.mark.gpu


def _to_dev(a: np.ndarray, dev):
    t = torch.from_numpy(a.copy()).to(dev)
    assert t.data_ptr() % 16 == 0  # a view's offset modulo 4 elements is its distance from the 16-byte grid
    return t


def _normals(dev, n, seed, off):
    from fedscale_amd import kernels as kx

    return kx.dp_normals(torch.empty(n, dtype=torch.float32, device=dev), seed, off).cpu().numpy()


def _draws(dev, sizes, offs, seed):
    """The device's own N(0,1) draws for every tensor of a list, in one download."""
    from fedscale_amd import kernels as kx

    buf = torch.empty(sum(sizes) + 1, dtype=torch.float32, device=dev)
    o = 0
    for n, off in zip(sizes, offs):
        kx.dp_normals(buf[o:o + n], seed, off)
        o += n
    host = buf.cpu().numpy()
    return [host[a:a + n] for a, n in zip(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int), sizes)]


# ------------------------------------------------------------------------------------------------------------------
# a / b. the noise stream
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ckm.NOISE_SEEDS)
def test_noise_stream_matches_the_twin(gpu_device, seed):
    """fa_dp_normals against dp_normals_ref at offsets 0, 1, 4095, 2^33 - 3 (the pair counter passes 2^32 inside the
    read) and 2^40 + 1:  |z - z_ref| <= 4.5 * 2^-23 * |z_ref|.

    The bound is derived, not measured.  Hashes, both 24-bit uniforms and the fp32 angle are the same numbers on
    both sides (integer arithmetic and exact or single fp32 products, restated in the twin), so argument rounding
    is not in the budget.  What differs: logf within 2 ulp, of which the square root passes on half (1 ulp; the
    factor -2 is exact); sqrtf, correctly rounded in this build (0.5 ulp); sinf / cosf of
    an fp32 angle in [0, 2 pi) within 2 ulp; the product r * cos, one rounding (0.5 ulp).  With 1 ulp <= 2^-23
    relative that is 4 * 2^-23; the remaining half covers the second-order terms and the difference between an
    ulp of the computed and of the exact value.  (With sqrtf taken at 2 ulp as well the sum would be 5.5 * 2^-23:
    the bound holds sqrtf to being correctly rounded.)  Where z_ref is 0 (radius 0, or sin 0) z must be 0."""
    worst = 0.0
    for off in ckm.NOISE_OFFSETS:
        z = _normals(gpu_device, ckm.NOISE_N, seed, off)
        ref = dp_normals_ref(seed, np.uint64(off) + np.arange(ckm.NOISE_N, dtype=np.uint64))
        ok = ckm.within_noise_bound(z, ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(ref != 0, np.abs(z.astype(F64) - ref) / np.abs(ref), 0.0)
        worst = max(worst, float(ratio.max()))
        print(f"[noise-twin] seed={seed} offset={off}: max |z - z_ref| / |z_ref| = {ratio.max() * 2 ** 23:.3f} * 2^-23")
        assert ok.all(), (seed, off, int(np.argmin(ok)), float(ratio.max() * 2 ** 23))
    print(f"[noise-twin] seed={seed}: worst ratio {worst * 2 ** 23:.3f} * 2^-23 (bound 4.5)")


def test_noise_stream_uses_the_whole_seed_and_odd_offsets(gpu_device):
    z = _normals(gpu_device, ckm.NOISE_N, 77, 0)
    z_hi = _normals(gpu_device, ckm.NOISE_N, 77 + 2 ** 32, 0)
    assert (z != z_hi).mean() > 0.99  # the high word of the seed selects another stream
    for off, n in ((1001, 2000), (1, 4098), (4095, 4)):  # odd offsets address the same stream
        assert np.array_equal(_normals(gpu_device, n, 77, off), z[off:off + n]), off


def test_edge_draws(gpu_device):
    """u1 = 2^-24 (h1 >> 8 == 0): the largest radius, finite and within the bound; u1 = 1 (h1 >> 8 == 0xFFFFFF):
    radius 0, so both values of the pair are 0.  The counters are pinned by test_client_oracle.py."""
    for e in ckm.EDGE_U1_MIN:
        z = _normals(gpu_device, 2, ckm.EDGE_SEED, e)
        ref = dp_normals_ref(ckm.EDGE_SEED, [e, e + 1])
        assert np.isfinite(z).all() and ckm.within_noise_bound(z, ref).all(), (e, z, ref)
        assert abs(float(np.hypot(*z.astype(F64))) - 5.768) < 1e-3
    for e in ckm.EDGE_U1_ONE:
        z = _normals(gpu_device, 2, ckm.EDGE_SEED, e)
        assert (z == 0).all(), (e, z)


# ------------------------------------------------------------------------------------------------------------------
# c. DP norm across groups and long tensors
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dp(extra=False, empties=True):
    return ckm.dp_case(extra, empties)  # read-only: tests that change values work on copies


def _clip_on_device(tab, dev, max_norm, norm_inf=False):
    from fedscale_amd import kernels as kx

    p, l = _to_dev(tab.base["p"], dev), _to_dev(tab.base["l"], dev)
    out = torch.full((3,), -1.0, dtype=torch.float32, device=dev)
    kx.dp_clip_coef(tab.device_views("p", p), tab.device_views("l", l), max_norm, norm_inf, out)
    assert same_bits(p.cpu().numpy(), tab.base["p"]) and same_bits(l.cpu().numpy(), tab.base["l"])  # inputs untouched
    return out.cpu().numpy()


def _want3(ex):
    return np.array([ex["total"], ex["coef"], 1.0 if ex["apply"] else 0.0], dtype=F32)


@pytest.mark.parametrize("max_norm", [1.0, 1e4])
def test_dp_norm_across_groups_is_exact(gpu_device, max_norm):
    """130 tensors (three launch groups; 65 workgroups at index 70, 129 at index 129; empties at 63 and 64; views
    off the 16-byte grid; some without ``last``): (total, coef, apply) bit-equal to dp_clip_exact, clipping
    (max_norm 1) and not (10^4).  Precondition on the reference alone: no fp32 rounding moves when a sum moves by
    2^-46, more than the device's fewer than 64 fp64 roundings can move it."""
    tab = _dp()
    ex = dp_clip_exact(tab.views("p"), tab.views("l"), max_norm)
    assert ckm.dp_precondition(ex) and ex["apply"] == (max_norm == 1.0)
    got = _clip_on_device(tab, gpu_device, max_norm)
    assert same_bits(got, _want3(ex)), (got, _want3(ex))


@pytest.mark.parametrize("T", [64, 65, 128, 129])
def test_dp_norm_group_count_seams(gpu_device, T):
    tab = ckm.tiny_dp_case(T)
    for max_norm in (1.0, 1e4):
        ex = dp_clip_exact(tab.views("p"), tab.views("l"), max_norm)
        assert ckm.dp_precondition(ex) and ex["apply"] == (max_norm == 1.0)
        got = _clip_on_device(tab, gpu_device, max_norm)
        assert same_bits(got, _want3(ex)), (T, got, _want3(ex))


@pytest.mark.parametrize("where", ckm.INF_PLANTS)
def test_dp_inf_norm_across_groups(gpu_device, where):
    """The inf norm over the list without its empties (130 tensors with the three extra ones): the maximum in the
    last element of the last tensor, in the last element of the 129-workgroup tensor, in the first element of
    tensor 64 and in tensor 5; a NaN in the third group gives a NaN total and no clipping.  The maximum is exact."""
    tab = ckm.plant_inf(_dp(True, False), where)
    ex = dp_clip_exact(tab.views("p"), tab.views("l"), 0.1, norm_inf=True)
    got = _clip_on_device(tab, gpu_device, 0.1, norm_inf=True)
    if where == "nan":
        assert np.isnan(ex["total"]) and np.isnan(got[0]) and np.isnan(got[1]) and got[2] == 0.0
    else:
        assert float(ex["total"]) == 1000.0
        assert same_bits(got, _want3(ex)), (got, _want3(ex))


# ------------------------------------------------------------------------------------------------------------------
# d. fa_dp_apply
# ------------------------------------------------------------------------------------------------------------------
APPLY_SEED, APPLY_SIGMA = 2 ** 63 + 9, 0.37


@pytest.mark.parametrize("clipped", [True, False])
def test_dp_apply_across_groups_is_exact(gpu_device, clipped):
    """133 tensors through kx.dp_apply with explicit counter offsets (odd ones, and beyond 2^33 and 2^40) and
    sigma != 0: recovered = last + fp32(fp32(p - last) * coef) when clipping, last + fp32(p - last) otherwise;
    buffers (no ``last``) untouched; upload = recovered + fp32(fp32(z * sigma) + 0) with z the device's own draws
    at the same counters (tied to the twin by test_noise_stream_matches_the_twin).  With write_param=False the
    uploads are the same and the parameters keep their bits.  The last three tensors have exactly one of param /
    last / upload 4 bytes off the 16-byte grid."""
    from fedscale_amd import kernels as kx

    tab = _dp(True)
    ex = dp_clip_exact(tab.views("p")[:130], tab.views("l")[:130], 1.0 if clipped else 1e4)
    assert ex["apply"] == clipped
    coef3 = (ex["total"], ex["coef"], ex["apply"])
    offs = ckm.dp_noise_offsets(tab)
    z = _draws(gpu_device, tab.n, offs, APPLY_SEED)
    assert all(np.isfinite(v).all() for v in z) and np.abs(np.concatenate(z)).max() > 3
    coef = torch.from_numpy(_want3(ex)).to(gpu_device)
    l = _to_dev(tab.base["l"], gpu_device)
    for wp in (True, False):
        want_p, want_u = ckm.dp_apply_expected(tab, coef3, APPLY_SIGMA, z, wp)
        p, u = _to_dev(tab.base["p"], gpu_device), _to_dev(tab.base["u"], gpu_device)
        kx.dp_apply(tab.device_views("p", p), tab.device_views("l", l), tab.device_views("u", u), offs, coef,
                    APPLY_SIGMA, APPLY_SEED, write_param=wp)
        got_p, got_u = p.cpu().numpy(), u.cpu().numpy()
        for t in range(tab.T):  # per tensor first, for a readable failure
            assert same_bits(tab.view("u", t, got_u), tab.view("u", t, want_u)), ("upload", t, wp)
            assert same_bits(tab.view("p", t, got_p), tab.view("p", t, want_p)), ("param", t, wp)
        assert same_bits(got_u, want_u) and same_bits(got_p, want_p)
        if not wp:
            assert same_bits(got_p, tab.base["p"])
        else:
            assert not same_bits(got_p, tab.base["p"])
    assert same_bits(l.cpu().numpy(), tab.base["l"])


def test_privatize_update_over_many_entries(gpu_device):
    """privatize_update on a module of 70 fp32 parameters, 70 fp32 buffers and 70 0-d int64 buffers (more than
    MT_MAX of each kind in every launch list), clipping, against dp_privatize fed with the device's draws.  The
    deltas are integer vectors with one non-zero entry and the threshold is a power of two, so the torch oracle's
    norms and coefficient are exact and equal to the device's: recovered and upload are bit-equal."""
    from fedscale_amd.cloud.execution.local_dp import _UploadLayout, privatize_update

    model = ckm.interleaved_module(70, seed=4).to(gpu_device)
    rng = np.random.default_rng(8)
    names = list(model.state_dict().keys())
    is_param = [n.endswith("weight") for n in names]
    state = OrderedDict((n, v.cpu().numpy().copy()) for n, v in model.state_dict().items())
    last = []
    for n in names:
        if n.endswith("weight"):
            d = np.zeros(6, F32)
            d[rng.integers(6)] = rng.integers(1, 6)
            last.append(state[n] - d.reshape(2, 3))
    clip, factor, seed = 2.0, 0.75, 2 ** 40 + 3
    lay = _UploadLayout(model)
    assert sum(d == torch.float32 for d in lay.dtypes) == 140 and sum(d == torch.int64 for d in lay.dtypes) == 70
    sigma = F32(factor * clip)
    draws = _draws(gpu_device, lay.numel, lay.noise_off, seed)
    noise = {n: (z * sigma + F32(0)).reshape(s) for n, z, s in zip(names, draws, lay.shapes)}
    rec, want_up, total = dp_privatize(state, is_param, last, clip, factor, noise=noise)
    assert total > clip
    up = privatize_update(model, [torch.from_numpy(a).to(gpu_device) for a in last], clip, factor, seed=seed)
    assert list(up.keys()) == names
    sd = model.state_dict()
    for n in names:
        got = sd[n].cpu().numpy()
        assert got.dtype == rec[n].dtype and np.array_equal(got, rec[n]), n
        assert up[n].dtype == want_up[n].dtype and up[n].shape == want_up[n].shape, n
        assert np.array_equal(up[n], want_up[n]), n
        assert up[n].dtype == (F64 if state[n].dtype == np.int64 else F32)


# ------------------------------------------------------------------------------------------------------------------
# e. fa_dp_noise_i64
# ------------------------------------------------------------------------------------------------------------------
def test_dp_noise_i64_across_groups(gpu_device):
    """66 int64 tensors (two launch groups; one of 4097 elements) with 0, -1, 2^53 + 1, INT64_MIN and INT64_MAX
    among the values: out = float64(x) + float64(fp32(fp32(z * sigma) + 0)) bit for bit, and float64(x) exactly at
    sigma = 0."""
    from fedscale_amd import kernels as kx

    xs, offs = ckm.i64_case()
    sizes = [len(x) for x in xs]
    z = _draws(gpu_device, sizes, offs, 31)
    dx = [torch.from_numpy(x).to(gpu_device) for x in xs]
    for sigma in (1.5, 0.0):
        outs = [torch.full((n,), -3.0, dtype=torch.float64, device=gpu_device) for n in sizes]
        kx.dp_noise_i64(dx, outs, offs, sigma, 31)
        for t, (x, o) in enumerate(zip(xs, outs)):
            want = x.astype(F64) + (z[t] * F32(sigma) + F32(0)).astype(F64)
            assert same_bits(o.cpu().numpy(), want), (sigma, t)
            if sigma == 0.0:
                assert same_bits(want, x.astype(F64))
    assert all(torch.equal(d.cpu(), torch.from_numpy(x)) for d, x in zip(dx, xs))


# ------------------------------------------------------------------------------------------------------------------
# f. fused SGD + FedProx across launches
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prox", [True, False])
@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("T", [49, 97])
def test_fused_sgd_across_launches_is_exact(gpu_device, T, single, fma, prox):
    """T = 49 and 97 tensors (two and three launches of SGD_MAX = 48) through kx.sgd_prox_step_groups, with scalars
    that change at 47 / 48 and 95 / 96 (lr; momentum 0.9 / 0.5 / 0 with no buffer / 0.9 nesterov; weight decay;
    dampening; first-step and later-step tensors in one launch), and through the single-group kx.sgd_prox_step.
    Three successive steps; parameters and momentum buffers bit-equal to sgd_prox_step_ref over their whole
    allocations.  First-step buffers hold NaN before the call.  Tensors 44-47 have exactly one of p / g / m / w
    4 bytes off the 16-byte grid."""
    from fedscale_amd import kernels as kx

    tab = ckm.sgd_case(T, single)
    want = ckm.sgd_expected(tab, fma, prox)
    dev = {k: _to_dev(v, gpu_device) for k, v in tab.base.items()}
    ps, ms = tab.device_views("p", dev["p"]), tab.device_views("m", dev["m"])
    ws = tab.device_views("w", dev["w"]) if prox else None
    lr, mom, damp, wd, nest = zip(*tab.cfg)
    for s in range(3):
        for t in range(T):
            if ckm.sgd_first(tab, s, t):
                ms[t].fill_(float("nan"))
        gs = tab.device_views(f"g{s}", dev[f"g{s}"])
        if single:
            kx.sgd_prox_step(ps, gs, ms, ws, lr[0], mom[0], damp[0], wd[0], bool(nest[0]), s == 0, ckm.SGD_C, fma=fma)
        else:
            kx.sgd_prox_step_groups(ps, gs, ms, ws, lr, mom, damp, wd, ckm.sgd_flags(tab, s), ckm.SGD_C, fma=fma)
        got_p, got_m = dev["p"].cpu().numpy(), dev["m"].cpu().numpy()
        for t in range(T):
            assert same_bits(tab.view("p", t, got_p), tab.view("p", t, want[s][0])), ("param", s, t, tab.cfg[t])
            if ms[t] is not None:
                assert same_bits(tab.view("m", t, got_m), tab.view("m", t, want[s][1])), ("buffer", s, t, tab.cfg[t])
        assert same_bits(got_p, want[s][0]) and same_bits(got_m, want[s][1]), s
        assert same_bits(dev[f"g{s}"].cpu().numpy(), tab.base[f"g{s}"])
    assert not np.isnan(got_p).any()
    print(f"[sgd-exact] T={T} single={single} fma={fma} prox={prox}: bit-equal to sgd_prox_step_ref over 3 steps")
