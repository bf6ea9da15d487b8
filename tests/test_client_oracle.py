"""CPU checks of the exact references for the client kernels (oracle/cpu_reference.py: ``dp_normals_ref``,
``fma_f32`` / ``sgd_prox_step_ref``, ``dp_clip_exact``) and of what tests/test_gpu_client_exact.py can see.

The second half plants one mistake at a time in a host restatement of a kernel (tests/client_kernel_models.py) and
asserts, on the inputs the device test uses, that the restatement without a mistake equals the expected result
bit for bit and that the restatement with the mistake does not.  Each such test names the device test that would
go red."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle.cpu_reference import (dp_clip_coef, dp_clip_exact, dp_noise_hashes, dp_normals_ref, fma_f32,
                                  sgd_prox_step_ref)
from tests import client_kernel_models as ckm
from tests.client_kernel_models import F32, F64, same_bits


# ------------------------------------------------------------------------------------------------------------------
# the references themselves
# ------------------------------------------------------------------------------------------------------------------
def _round_fraction_f32(q: Fraction) -> np.float32:
    """Round-to-nearest-even of an exact rational to fp32, by comparing with the candidates exactly."""
    c = F32(float(q))
    cands = {float(c), float(np.nextafter(c, F32(np.inf))), float(np.nextafter(c, F32(-np.inf)))}
    best = min(cands, key=lambda v: (abs(Fraction(v) - q), int(F32(v).view(np.uint32)) & 1))
    return F32(best)


def _fma_exact(a, x, y):
    return _round_fraction_f32(Fraction(float(y)) + Fraction(float(a)) * Fraction(float(x)))


# triples (a, x, y) whose float64 sum y + a*x is exactly the midpoint of two fp32 values while the true sum is not:
# 1 + 2^-23 - 2^-24 (1 - 2^-46) lies above the midpoint 1 + 2^-24 by 2^-70, which float64 cannot hold.  In the second
# the true sum lies below the midpoint and the tie goes down to the even neighbour anyway: two roundings are right
# there by luck.
_TIES = [(-(2.0 ** -12) * (1 + 2.0 ** -23), 2.0 ** -12 * (1 - 2.0 ** -23), 1 + 2.0 ** -23),
         (2.0 ** -12 * (1 + 2.0 ** -23), 2.0 ** -12 * (1 - 2.0 ** -23), 1.0),
         (2.0 ** -12 * (1 + 2.0 ** -23), -(2.0 ** -12) * (1 - 2.0 ** -23), -1.0 - 2.0 ** -23),
         (2.0 ** 12 * (1 + 2.0 ** -23), 2.0 ** -12 * (1 - 2.0 ** -23), 2.0 ** 24 + 2.0),
         (2.0 ** -24, 1.0, 1.0), (2.0 ** -24, 1.0, 1 + 2.0 ** -23)]  # the last two: true ties, to even


def test_fma_emulation_equals_exact_rational_arithmetic():
    rng = np.random.default_rng(1)
    n = 10000
    a, x, y = (rng.normal(size=n).astype(F32) * F32(2.0) ** rng.integers(-6, 7, size=n).astype(F32) for _ in range(3))
    y[::3] = -(a[::3] * x[::3])  # heavy cancellation: the fused result is the product's own rounding error
    got = fma_f32(a, x, y)
    want = np.array([_fma_exact(*t) for t in zip(a, x, y)], dtype=F32)
    assert same_bits(got, want)
    assert not same_bits(y + a * x, want)  # rounding the product first is a different function on these
    ta, tx, ty = (np.array(v, dtype=F32) for v in zip(*_TIES))
    assert all(float(v) == w for v, t in zip((ta, tx, ty), zip(*_TIES)) for v, w in zip(v, t))  # fp32 values
    want = np.array([_fma_exact(*t) for t in zip(ta, tx, ty)], dtype=F32)
    assert same_bits(fma_f32(ta, tx, ty), want)
    twice = (ty.astype(F64) + ta.astype(F64) * tx.astype(F64)).astype(F32)  # float64 sum, then fp32: two roundings
    assert [bool(v) for v in ckm.bits(twice) != ckm.bits(want)] == [True, False, True, True, False, False]


def test_sgd_reference_follows_torch_sgd_on_the_cpu():
    """Semantics (not bits: torch's CPU kernels may contract): weight decay, momentum with dampening, nesterov,
    first step, then FedProx, against torch.optim.SGD on the CPU within 2 fp32 ulp of the largest entry."""
    for mom, damp, wd, nest in [(0.9, 0.0, 5e-4, False), (0.5, 0.3, 0.0, False), (0.9, 0.0, 1e-3, True),
                                (0.0, 0.0, 5e-4, False)]:
        g = torch.Generator().manual_seed(5)
        p = torch.nn.Parameter(torch.randn(1001, generator=g))
        w = p.detach().clone() + 0.01
        opt = torch.optim.SGD([p], lr=0.05, momentum=mom, dampening=damp, weight_decay=wd, nesterov=nest)
        for fma in (False, True):
            mine_p, mine_m = p.detach().numpy().copy(), None
            for step in range(3):
                p.grad = torch.randn(1001, generator=g)
                flags = [(1 if nest else 0) | (2 if step == 0 else 0)]
                buf = [mine_m if mine_m is not None else np.full(1001, np.nan, F32)] if mom else [None]
                (mine_p,), (mine_m,) = sgd_prox_step_ref([mine_p], [p.grad.numpy()], buf, [w.numpy()], [0.05], [mom],
                                                         [damp], [wd], flags, 0.005, fma)
                opt.step()
                p.data += 0.05 * 0.1 * (p.data - w)
                assert np.abs(mine_p - p.detach().numpy()).max() <= 2 * 2.0 ** -23 * np.abs(mine_p).max()
                if mom:
                    mb = opt.state[p]["momentum_buffer"].numpy()
                    assert np.abs(mine_m - mb).max() <= 2 * 2.0 ** -23 * np.abs(mb).max()
            p.data.copy_(torch.randn(1001, generator=torch.Generator().manual_seed(5)))
            opt.state.clear()


def test_noise_twin_has_normal_moments_and_uses_the_whole_seed():
    n = 1 << 20
    z = dp_normals_ref(77, np.arange(n, dtype=np.uint64))
    se = 1.0 / math.sqrt(n)
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 6 * se
    assert abs(z.std() - 1.0) < 6 * se
    assert abs((np.abs(z) <= 1.0).mean() - 0.682689) < 6 * 0.47 * se
    assert abs((z ** 4).mean() - 3.0) < 6 * math.sqrt(96) * se
    assert abs((z[:-1] * z[1:]).mean()) < 6 * se
    z2 = dp_normals_ref(77 + 2 ** 32, np.arange(n, dtype=np.uint64))
    assert abs((z * z2).mean()) < 6 * se and (z != z2).mean() > 0.99
    h1, h2 = dp_noise_hashes(77, np.arange(8, dtype=np.uint64))
    assert h1.dtype == np.uint32 and (h1[0::2] == h1[1::2]).all() and len(set(h1[0::2].tolist())) == 4


def test_edge_draws_are_where_the_twin_has_them():
    """The hard-coded counters of tests/test_gpu_client_exact.py::test_edge_draws: u1 = 2^-24 gives the largest
    radius sqrt(48 ln 2), u1 = 1 gives radius 0."""
    for e in ckm.EDGE_U1_MIN:
        assert e % 2 == 0 and dp_noise_hashes(ckm.EDGE_SEED, [e])[0][0] >> 8 == 0
        z = dp_normals_ref(ckm.EDGE_SEED, [e, e + 1])
        assert abs(math.hypot(*z) - math.sqrt(48 * math.log(2))) < 1e-12 and 5.76 < math.hypot(*z) < 5.77
    for e in ckm.EDGE_U1_ONE:
        assert e % 2 == 0 and dp_noise_hashes(ckm.EDGE_SEED, [e])[0][0] >> 8 == 0xFFFFFF
        assert (dp_normals_ref(ckm.EDGE_SEED, [e, e + 1]) == 0).all()
    lo, hi = ckm.scan_edge_draws(n=1 << 22)  # the scan itself, on a range without hits of either kind
    assert lo == [] and hi == []


def test_dp_clip_exact_equals_the_torch_oracle_on_integer_input():
    """Integer-valued deltas with integer norms: every order of summation is exact, so the exactly rounded sums and
    torch's fp32 norms are the same numbers.  The thresholds are powers of two: torch evaluates ``max_norm / tensor``
    as ``tensor.reciprocal() * max_norm`` (two roundings), the kernel and ``dp_clip_exact`` divide (one); the two
    agree bit for bit when max_norm is a power of two and within one ulp otherwise, which 3.5 shows."""
    rng = np.random.default_rng(3)
    last = [rng.integers(-8, 9, size=n).astype(F32) for n in (1, 3, 4, 5, 4097, 0, 17)]
    deltas = []
    for l in last:  # one non-zero entry per tensor: its norm is that integer
        d = np.zeros_like(l)
        if len(d):
            d[rng.integers(len(d))] = rng.integers(1, 40)
        deltas.append(d)
    params = [l + d for l, d in zip(last, deltas)]
    for max_norm in (1.0, 0.5, 4.0, 2.0 ** 14):
        ex = dp_clip_exact(params, last, max_norm)
        total, coef, apply = dp_clip_coef(deltas, max_norm)
        assert (ex["total"], ex["coef"], ex["apply"]) == (total, coef, apply)
        assert ex["total"].dtype == F32 and ex["coef"].dtype == F32
    assert ex["apply"] is False and dp_clip_exact(params, last, 1.0)["apply"] is True
    ex = dp_clip_exact(params, last, 3.5)
    total, coef, apply = dp_clip_coef(deltas, 3.5)
    assert ex["total"] == total and ex["apply"] == apply
    assert ex["coef"] == F32(3.5) / (total + F32(1e-6)) and coef == F32(1) / (total + F32(1e-6)) * F32(3.5)
    assert abs(float(ex["coef"]) - float(coef)) <= float(np.spacing(coef))
    full = [rng.integers(-3, 4, size=n).astype(F32) for n in (5, 4097, 1, 300)]
    ex = dp_clip_exact(full, None, 2.0)
    assert [float(s) for s in ex["S"]] == [float((f.astype(F64) ** 2).sum()) for f in full]
    nonempty = [d for d in deltas if len(d)]
    exi = dp_clip_exact(nonempty, None, 2.0, norm_inf=True)
    total, coef, apply = dp_clip_coef(nonempty, 2.0, float("inf"))
    assert (exi["total"], exi["coef"], exi["apply"]) == (total, coef, apply)
    nan = dp_clip_exact([np.array([1, np.nan, 2], F32), np.array([3], F32)], None, 0.5, norm_inf=True)
    assert np.isnan(nan["total"]) and np.isnan(nan["coef"]) and nan["apply"] is False


def test_upload_layout_gives_disjoint_contiguous_counter_ranges():
    from fedscale_amd.cloud.execution.local_dp import _UploadLayout

    m = ckm.interleaved_module(5)
    lay = _UploadLayout(m)
    sd = m.state_dict()
    assert lay.names == list(sd.keys()) and len(lay.names) == 15
    assert [d for d in lay.dtypes[:3]] == [torch.float32, torch.float32, torch.int64]
    assert lay.numel == [max(1, v.numel()) for v in sd.values()] == [6, 3, 1] * 5
    assert lay.noise_off[0] == 0
    for i in range(1, len(lay.names)):  # each range starts where the previous one ends
        assert lay.noise_off[i] == lay.noise_off[i - 1] + lay.numel[i - 1]
    assert all(o % 4 == 0 for o in lay.f_off) and lay.f_idx == [i for i in range(15) if i % 3 != 2]


# ------------------------------------------------------------------------------------------------------------------
# planted mistakes: what the device tests can see
# ------------------------------------------------------------------------------------------------------------------
def _noise_failures(mistake):
    """The (seed, offset) cases of test_noise_stream_matches_the_twin in which the restated generator with
    ``mistake`` leaves the bound against the twin."""
    bad = set()
    for seed in ckm.NOISE_SEEDS:
        for off in ckm.NOISE_OFFSETS:
            ref = dp_normals_ref(seed, np.uint64(off) + np.arange(ckm.NOISE_N, dtype=np.uint64))
            if not ckm.within_noise_bound(ckm.model_normals(seed, off, ckm.NOISE_N, mistake), ref).all():
                bad.add((seed, off))
    return bad


def test_noise_mistakes_leave_the_bound():
    """test_gpu_client_exact.py::test_noise_stream_matches_the_twin sees: the seed's high word dropped, the pair
    counter's high word dropped, parity from the index in the read, u1 without its + 1."""
    assert _noise_failures(None) == set()
    hi_seeds = {s for s in ckm.NOISE_SEEDS if s >> 32}
    assert _noise_failures("seed_hi") == {(s, o) for s in hi_seeds for o in ckm.NOISE_OFFSETS}
    assert _noise_failures("j_hi") == {(s, o) for s in ckm.NOISE_SEEDS for o in (2 ** 33 - 3, 2 ** 40 + 1)}
    assert _noise_failures("parity_i") == {(s, o) for s in ckm.NOISE_SEEDS for o in ckm.NOISE_OFFSETS if o % 2}
    assert _noise_failures("u1_plus1") == {(s, o) for s in ckm.NOISE_SEEDS for o in ckm.NOISE_OFFSETS}
    # ... and test_edge_draws: without the + 1, u1 = 0 gives an infinite radius and u1 = 1 - 2^-24 a non-zero one
    e = ckm.EDGE_U1_MIN[0]
    assert not np.isfinite(ckm.model_normals(ckm.EDGE_SEED, e, 2, "u1_plus1")).all()
    e = ckm.EDGE_U1_ONE[0]
    assert (ckm.model_normals(ckm.EDGE_SEED, e, 2, "u1_plus1") != 0).any()
    # the odd-offset slice identity of the device test is a parity check of its own
    a = ckm.model_normals(77, 0, 64, "parity_i")
    b = ckm.model_normals(77, 7, 32, "parity_i")
    assert not np.array_equal(a[7:39], b)


@functools.lru_cache(maxsize=None)
def _dp(extra=False, empties=True):
    return ckm.dp_case(extra, empties)


DP_MISTAKES = ["part0_write", "part0_read", "tsum_t0", "norm_one_trip", "coef_one_trip"]


def test_dp_list_has_the_shape_it_is_described_with():
    tab = _dp()
    assert tab.T == 130 and tab.n[63] == tab.n[64] == 0 and set(ckm.DP_SIZES) <= set(tab.n)
    nb = [(n + ckm.MT_CHUNK - 1) // ckm.MT_CHUNK for n in tab.n]
    assert nb[70] == 65 and nb[129] == 129 and sum(nb[:64]) > 0  # part0 != 0 for the second group
    assert tab.off["p"][70] % 4 == 0 and tab.off["l"][70] % 4 == 0 and tab.off["l"][129] % 4 == 2
    assert sum(o is None for o in tab.off["l"]) >= 10 and max(tab.n) * 4 <= 2.1 * 2 ** 20
    assert any(tab.off["p"][t] % 4 and tab.n[t] >= 4096 for t in range(130))
    ex = _dp(True)
    assert [(ex.off["p"][t] % 4, ex.off["l"][t] % 4, ex.off["u"][t] % 4) for t in (130, 131, 132)] == \
        [(1, 0, 0), (0, 1, 0), (0, 0, 1)]


@pytest.mark.parametrize("max_norm", [1.0, 1e4])
def test_dp_norm_mistakes_change_the_bits(max_norm):
    """test_gpu_client_exact.py::test_dp_norm_across_groups_is_exact sees: part0 ignored by either kernel, tsum
    without t0, one trip of the k_dp_tensor_norm loop, one trip of the k_dp_coef loop.  (part0 left at 0 in both
    kernels of a group changes nothing: they agree with each other and run in stream order.)"""
    tab = _dp()
    p, l = tab.views("p"), tab.views("l")
    ex = dp_clip_exact(p, l, max_norm)
    assert ckm.dp_precondition(ex)
    assert ex["apply"] == (max_norm == 1.0)
    want = (ex["total"], ex["coef"], ex["apply"])
    assert ckm.model_dp_clip(p, l, max_norm) == want
    assert ckm.model_dp_clip(p, l, max_norm, mistake="part0_both") == want
    for m in DP_MISTAKES:
        assert ckm.model_dp_clip(p, l, max_norm, mistake=m)[0] != want[0], m


def _eq(a, b):
    return bool((np.isnan(a) and np.isnan(b)) or a == b)


def test_dp_inf_norm_mistakes_are_seen():
    """test_gpu_client_exact.py::test_dp_inf_norm_across_groups plants the maximum in five places; between them
    they see every mistake of DP_MISTAKES (each place sees those that lose its partial or its tensor)."""
    base = _dp(True, False)
    assert base.T == 130 and min(base.n) > 0
    seen = {}
    for where in ckm.INF_PLANTS:
        tab = ckm.plant_inf(base, where)
        p, l = tab.views("p"), tab.views("l")
        ex = dp_clip_exact(p, l, 0.1, norm_inf=True)
        got = ckm.model_dp_clip(p, l, 0.1, True)
        assert _eq(got[0], ex["total"]) and _eq(got[1], ex["coef"]) and got[2] == ex["apply"]
        if where == "nan":
            assert np.isnan(ex["total"]) and ex["apply"] is False
            continue
        assert float(ex["total"]) == 1000.0 and ex["apply"]
        seen[where] = {m for m in DP_MISTAKES if not _eq(ckm.model_dp_clip(p, l, 0.1, True, mistake=m)[0], ex["total"])}
    assert {"part0_write", "part0_read", "coef_one_trip"} <= seen["last"]
    assert "norm_one_trip" in seen["long_last"]
    assert {"part0_write", "coef_one_trip"} <= seen["t64"]  # (a misplaced read can still meet a maximum)
    assert "tsum_t0" in seen["t5"]
    assert set().union(*seen.values()) == set(DP_MISTAKES)


@pytest.mark.parametrize("T", [64, 65, 128, 129])
def test_tiny_dp_lists_cover_the_group_seams(T):
    """test_gpu_client_exact.py::test_dp_norm_group_count_seams: from T = 65 on there is a second group and a
    second trip of the k_dp_coef loop, at T = 129 a third of each."""
    tab = ckm.tiny_dp_case(T)
    p, l = tab.views("p"), tab.views("l")
    ex = dp_clip_exact(p, l, 1.0)
    assert ckm.dp_precondition(ex)
    want = (ex["total"], ex["coef"], ex["apply"])
    assert ckm.model_dp_clip(p, l, 1.0) == want
    seen = {m for m in DP_MISTAKES if ckm.model_dp_clip(p, l, 1.0, mistake=m)[0] != want[0]}
    # T = 64 is the last size with one group and one trip: it pins the near side of the seam
    assert seen == (set() if T == 64 else {"part0_write", "part0_read", "tsum_t0", "coef_one_trip"}), seen


def _apply_inputs(clipped):
    tab = _dp(True)
    ex = dp_clip_exact(tab.views("p")[:130], tab.views("l")[:130], 1.0 if clipped else 1e4)
    coef3 = (ex["total"], ex["coef"], ex["apply"])
    offs = ckm.dp_noise_offsets(tab)
    z = [dp_normals_ref(9, np.uint64(o) + np.arange(n, dtype=np.uint64)).astype(F32) for o, n in zip(offs, tab.n)]
    return tab, coef3, z


@pytest.mark.parametrize("clipped", [True, False])
def test_dp_apply_mistakes_change_the_result(clipped):
    """test_gpu_client_exact.py::test_dp_apply_across_groups_is_exact sees: write_param ignored, d * coef applied to
    buffers (when clipping), the vec bit without the upload pointer (under the alignment model of
    client_kernel_models), noise parity from the tensor index (odd offsets)."""
    tab, coef3, z = _apply_inputs(clipped)
    assert coef3[2] == clipped
    offs = ckm.dp_noise_offsets(tab)
    assert any(o % 2 for o in offs) and any(o >= 2 ** 33 for o in offs) and any(o >= 2 ** 40 for o in offs)
    sigma = 0.37
    for wp in (True, False):
        want = ckm.dp_apply_expected(tab, coef3, sigma, z, wp)
        got = ckm.model_dp_apply(tab, coef3, sigma, z, wp)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        if not wp:
            assert same_bits(want[0], tab.base["p"])
            bad = ckm.model_dp_apply(tab, coef3, sigma, z, wp, "write_param")
            assert not same_bits(bad[0], want[0])
        bad = ckm.model_dp_apply(tab, coef3, sigma, z, wp, "vec_upload")
        assert not same_bits(bad[1], want[1])
        t = 132  # the tensor whose upload alone is off the grid carries the difference
        assert not same_bits(tab.view("u", t, bad[1]), tab.view("u", t, want[1]))
        bad = ckm.model_dp_apply(tab, coef3, sigma, z, wp, "coef_on_buffers")
        assert same_bits(bad[1], want[1]) != clipped
    zi = [ckm.model_normals(9, o, n, "parity_i").astype(F32) for o, n in zip(offs, tab.n)]
    assert not same_bits(ckm.dp_apply_expected(tab, coef3, sigma, zi)[1], ckm.dp_apply_expected(tab, coef3, sigma, z)[1])


@functools.lru_cache(maxsize=None)
def _sgd(T, uniform):
    return ckm.sgd_case(T, uniform)


def test_sgd_lists_have_the_shape_they_are_described_with():
    for T in (49, 97):
        tab = _sgd(T, False)
        assert set(ckm.SGD_SIZES) <= set(tab.n) and tab.T == T
        assert tab.cfg[47] != tab.cfg[48] and (T < 97 or tab.cfg[95] != tab.cfg[96])
        assert all(tab.cfg[t] != tab.cfg[t - 48] for t in range(48, T))  # a slot's scalars differ across launches
        for t, name in ckm.SGD_OFFGRID.items():
            offs = {k: tab.off[{"g": "g0"}.get(k, k)][t] % 4 for k in "pgmw"}
            assert offs == {k: int(k == name) for k in "pgmw"}, (t, offs)
        fl = ckm.sgd_flags(tab, 0)[:48]
        assert any(f & ckm.FIRST for f in fl) and any(not f & ckm.FIRST and tab.cfg[t][1] for t, f in enumerate(fl))
        assert any(f & ckm.NESTEROV for f in ckm.sgd_flags(tab, 0)) == (T == 97)
        assert [o is None for o in tab.off["m"]] == [c[1] == 0 for c in tab.cfg]


@pytest.mark.parametrize("T", [49, 97])
@pytest.mark.parametrize("fma", [False, True])
def test_sgd_mistakes_change_the_result(T, fma):
    """test_gpu_client_exact.py::test_fused_sgd_across_launches_is_exact sees: scalars indexed by launch slot where
    the list position belongs and the reverse, fa_sgd_prox_step not advancing momentum_buf, a first step that reads
    its buffer, the vec bit without the momentum pointer (under the alignment model)."""
    for single in (False, True):
        tab = _sgd(T, single)
        want = ckm.sgd_expected(tab, fma, True)
        assert not np.isnan(want[-1][0]).any()
        for t in range(T):  # no NaN left in any buffer view: first steps overwrote the poison
            v = tab.view("m", t, want[-1][1])
            assert v is None or not np.isnan(v).any()

        def differs(mistake):
            got = ckm.model_sgd(tab, fma, True, single, mistake=mistake)
            return not all(same_bits(g[0], w[0]) and same_bits(g[1], w[1]) for g, w in zip(got, want))

        assert not differs(None)
        assert differs("first_reads") and differs("vec_momentum")
        if single:
            assert differs("bufs_not_advanced")
        else:
            assert differs("scalars_from_slot") and differs("scalars_to_list_pos")
