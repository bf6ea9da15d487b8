"""The kernels of the coordinate-wise trimmed mean (include/fedtrim.h) on the MI355X against the numpy restatement of
tests/trim_fixtures.py: thresholds, tie counts, means, mirror and per-row drop counts, bit for bit — no tolerance
anywhere.  Rows and thresholds have ld > P with poisons in columns [P, ld).  The shapes are the smallest at which each
loop of a kernel iterates, derived from the launch plan at the device's CU count (tests/test_trim_plan.py asserts the
plan each shape is listed for)."""
import numpy as np
import pytest
import torch

from tests import trim_fixtures as tf

pytestmark = pytest.mark.gpu

_CASES = {}
POISON_KEY, POISON_OUT = 0x5A5A5A5A, 7.0


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ld(P):
    return (P + 3) // 4 * 4 + 8  # ld > P always: columns [P, ld) hold a poison


def _case(K, P, dev, kind="ties"):
    """(rows [K, ld] on the host, the same on the device), made once per shape and never written."""
    key = (K, P, kind)
    if key not in _CASES:
        rng = np.random.default_rng(3000 + 17 * K + P % 997)
        x = (tf.tied_rows if kind == "ties" else tf.normal_rows)(rng, K, _ld(P), P)
        _CASES[key] = (x, torch.from_numpy(x).to(dev))
    return _CASES[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _u32(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def _same(got, want, what, nan_payloads=True):
    """Bit equality.  ``nan_payloads=False``, for a float result of the device against one of the host: a NaN must
    meet a NaN, whose sign and payload the contract leaves open (the CPU and the GPU propagate them differently)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    differ = _bits(got) != _bits(want)
    if not nan_payloads:
        differ &= ~(np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(differ)
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def _poisoned_thresholds(ld, dev):
    return tuple(torch.full((ld,), POISON_KEY, dtype=torch.int32, device=dev) for _ in range(3))


def _check(K, t, P, dev, kind="ties", what=""):
    """One shape through ft_select and ft_reduce, every assertion of the module's docstring."""
    from fedscale_amd import kernels as kx
    from fedscale_amd import kernels_trim as kt

    x, xd = _case(K, P, dev, kind)
    ld = x.shape[1]
    tag = (what, K, t, P, kind)
    thr = (None, None, None)
    if t > 0:
        want_lo, want_hi, want_ties = tf.select_of(x[:, :P], t)
        thr = _poisoned_thresholds(ld, dev)
        kt.select(xd, K, P, t, *thr)
        for name, got, want in zip(("lo", "hi", "ties"), thr, (want_lo, want_hi, want_ties)):
            g = _u32(got)
            _same(g[:P], want, tag + (name,))
            assert (g[P:] == POISON_KEY).all(), tag + (name, "columns [P, ld) keep the pattern")
        want_out, want_dropped, _ = tf.reduce_of(x[:, :P], t, want_lo, want_hi, want_ties)
    else:
        want_out, want_dropped, _ = tf.reduce_of(x[:, :P], 0)
    lo, hi, ties = thr
    out = torch.full((ld,), POISON_OUT, device=dev)
    mirror = torch.full((ld,), POISON_OUT).pin_memory()
    dropped = torch.zeros((K, 2), dtype=torch.int64, device=dev)
    kt.reduce_trim(xd, K, P, t, out, lo=lo, hi=hi, ties=ties, mirror=mirror, dropped=dropped)
    plain = torch.full((ld,), POISON_OUT, device=dev)
    kt.reduce_trim(xd, K, P, t, plain, lo=lo, hi=hi, ties=ties)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    _same(got[:P], want_out, tag + ("out",), nan_payloads=False)
    assert (got[P:] == POISON_OUT).all(), tag + ("out: columns [P, ld) keep the pattern",)
    _same(mirror.numpy(), got, tag + ("the pinned mirror equals out, poisons included",))
    _same(plain.cpu().numpy(), got, tag + ("the same floats with and without the drop counts",))
    assert np.array_equal(dropped.cpu().numpy(), want_dropped), tag + ("dropped",)
    assert want_dropped.sum() == 2 * t * P
    if t == 0:  # the existing unweighted FedAvg reduce on the same rows
        avg = torch.full((ld,), POISON_OUT, device=dev)
        kx.reduce(xd, K, P, avg, denom=float(np.float32(K)), finalize=True)
        _same(avg.cpu().numpy()[:P], got[:P], tag + ("t = 0 is kernels.reduce's FedAvg",), nan_payloads=False)
        _same(got[:P], tf.fedavg_of(x[:, :P]), tag + ("t = 0 is the FedAvg chain",), nan_payloads=False)


def test_every_row_case_at_small_widths(gpu_device):
    """K = 1, 2 (t = 0), 3 (t = 1); every depth T at t = T and T - 1 with K = 2t + 1 and 2t + 2; K past every
    rows-ahead depth — at a width below one float4, one with a ragged float4, and one with two level-2 tiles."""
    for K, t in tf.row_cases():
        for P in (3, 257, 1025):
            _check(K, t, P, gpu_device)


def test_every_small_width(gpu_device):
    """P = 1 .. 257 and one tile of each level +- 1, at the deepest selection of each geometry and at t = 0."""
    for P in tf.SMALL_P:
        for K, t in ((5, 0), (9, 4), (33, 16)):
            _check(K, t, P, gpu_device)


def test_standard_normals(gpu_device):
    for K, t in ((2, 0), (3, 1), (10, 2), (17, 8), (34, 16)):
        for P in (5, 1025):
            _check(K, t, P, gpu_device, kind="normal")


def _shape(name):
    return next(s for s in tf.shapes(_cus()) if s[0] == name)


@pytest.mark.parametrize("name", [s[0] for s in tf.shapes(256)])
def test_plan_shapes(gpu_device, name):
    """Every depth T at a level-1 + level-2 plan (two launches) and at a level-0 plan with a ragged last tile, and a
    capped grid whose workgroups walk two tiles, once per geometry.  The plan is asserted first."""
    from fedscale_amd import kernels_trim as kt

    _, K, t, P, tag = _shape(name)
    launches = kt.plan(_cus(), K, P, t)
    assert launches == tf.plan(_cus(), K, P, t)
    sel = tf.of_kernel(launches, "select")
    assert {l["T"] for l in sel} == {tf.depth_of(t)}
    if name.startswith("two_levels"):
        assert len(sel) == 2
    elif name.startswith("capped"):
        assert len(sel) == 1 and sel[0]["tiles"] == 2 * sel[0]["grid"]
    else:
        assert len(sel) == 1 and sel[0]["tiles"] == sel[0]["grid"]
    _check(K, t, P, gpu_device, what=name)
    _CASES.clear()  # (the wide cases are not shared; free them)


def test_drop_counts_past_the_lds_table(gpu_device):
    """K above the rows a workgroup gathers in LDS: the counts go straight to the table."""
    K = tf.LDS_ROWS + 1
    for t in (1, 16):
        _check(K, t, 5, gpu_device)
    _CASES.clear()


def test_drop_counts_accumulate(gpu_device):
    """The table is added to, not overwritten (the caller zeroes it)."""
    from fedscale_amd import kernels_trim as kt

    K, t, P = 9, 2, 257
    x, xd = _case(K, P, gpu_device)
    thr = kt.thresholds(P, gpu_device)
    kt.select(xd, K, P, t, *thr)
    out = torch.empty(_ld(P), device=gpu_device)
    dropped = torch.full((K, 2), 1000, dtype=torch.int64, device=gpu_device)
    for _ in range(2):
        kt.reduce_trim(xd, K, P, t, out, lo=thr[0], hi=thr[1], ties=thr[2], dropped=dropped)
    _, want = tf.trimmed_mean(x[:, :P], t)
    assert np.array_equal(dropped.cpu().numpy(), 1000 + 2 * want)


def test_refused_operands_launch_nothing(gpu_device):
    from fedscale_amd import _native_trim as nt
    from fedscale_amd import kernels_trim as kt
    from fedscale_amd._native import FedAggError, ptr

    K, t, P = 9, 2, 257
    dev = gpu_device
    x, xd = _case(K, P, dev)
    ld = x.shape[1]
    lo, hi, ties = _poisoned_thresholds(ld, dev)
    out = torch.full((ld,), POISON_OUT, device=dev)
    dropped = torch.full((K, 2), -5, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def sel(**kw):
        a = dict(x=ptr(xd), ld=ld, K=K, P=P, t=t, lo=ptr(lo), hi=ptr(hi), ties=ptr(ties))
        a.update(kw)
        return nt.call("ft_select", a["x"], a["ld"], a["K"], a["P"], a["t"], a["lo"], a["hi"], a["ties"], s)

    def red(**kw):
        a = dict(x=ptr(xd), ld=ld, K=K, P=P, t=t, lo=ptr(lo), hi=ptr(hi), ties=ptr(ties), out=ptr(out), mirror=None,
                 dropped=ptr(dropped))
        a.update(kw)
        return nt.call("ft_reduce", a["x"], a["ld"], a["K"], a["P"], a["t"], a["lo"], a["hi"], a["ties"], a["out"],
                       a["mirror"], a["dropped"], s)

    short = torch.empty(64, dtype=torch.int32, device=dev)
    pageable = torch.empty(ld)
    bad = [dict(K=-1), dict(P=-1), dict(t=-1), dict(t=5), dict(K=4), dict(t=17, K=100), dict(ld=P - 1), dict(ld=ld + 2),
           dict(x=None), dict(x=ptr(xd) + 4), dict(lo=None), dict(hi=ptr(hi) + 4), dict(ties=ptr(ties) + 8)]
    for kw in bad + [dict(t=0)]:
        with pytest.raises(FedAggError, match="ft_select.*nothing was launched"):
            sel(**kw)
    for kw in bad + [dict(out=None), dict(out=ptr(out) + 4), dict(mirror=ptr(out) + 8), dict(dropped=ptr(dropped) + 4),
                     dict(t=0), dict(t=0, lo=None, hi=None), dict(hi=None), dict(mirror=pageable.data_ptr())]:
        with pytest.raises(FedAggError, match="ft_reduce.*nothing was launched"):
            red(**kw)
    with pytest.raises(ValueError, match="2t < K"):
        kt.select(xd, 4, P, 2, lo, hi, ties)
    with pytest.raises(ValueError, match="no thresholds"):
        kt.reduce_trim(xd, K, P, 0, out, lo=lo, hi=hi, ties=ties)
    with pytest.raises(ValueError, match="needs lo, hi and ties"):
        kt.reduce_trim(xd, K, P, t, out)
    with pytest.raises(TypeError, match="lo"):
        kt.select(xd, K, P, t, lo.float(), hi, ties)
    with pytest.raises(ValueError, match="lo: has 64 elements"):  # the typed wrappers check every operand's size
        kt.select(xd, K, P, t, short, hi, ties)
    with pytest.raises(ValueError, match="out: has 64 elements"):
        kt.reduce_trim(xd, K, P, t, short.view(torch.float32), lo=lo, hi=hi, ties=ties)
    with pytest.raises(ValueError, match="dropped: has 2 elements"):
        kt.reduce_trim(xd, K, P, t, out, lo=lo, hi=hi, ties=ties, dropped=dropped[:1])
    with pytest.raises(ValueError, match="K=10 > rows 9"):
        kt.select(xd, K + 1, P, t, lo, hi, ties)
    torch.cuda.synchronize()
    for v in (lo, hi, ties):
        assert (_u32(v) == POISON_KEY).all()
    assert bool((out == POISON_OUT).all()) and bool((dropped == -5).all())
    assert sel(P=0) == 0 and red(P=0) == 0  # nothing to do is not an error — and writes nothing
    torch.cuda.synchronize()
    assert (_u32(lo) == POISON_KEY).all() and bool((out == POISON_OUT).all())
