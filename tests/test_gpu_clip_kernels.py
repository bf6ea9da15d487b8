"""The kernels of norm-clipped aggregation (include/fedclip.h) on the MI355X against the numpy restatement of
tests/clip_fixtures.py.  The squared norms meet the bound derived from their fp64 adds (and are bit-exact where every
order of adds is); everything after them — coefficients, chain, finish — is bit-identical to the restatement, no
tolerance anywhere.  The shapes are the smallest at which each loop of a kernel iterates, derived from the launch
plans at the device's CU count (tests/test_clip_plan.py asserts the plan each shape is listed for)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import clip_fixtures as cf

pytestmark = pytest.mark.gpu

_CASES = {}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ld(P):
    return (P + 3) // 4 * 4 + 8  # ld > P always: columns [P, ld) hold a poison


def _case(K, P, dev, seed=0, ints=False):
    """(last [ld], rows [K, ld]) on the host and on the device, made once per shape and never written.  Columns
    [P, ld) of the rows AND of last hold nonzero poisons."""
    key = (K, P, seed, ints)
    if key not in _CASES:
        ld = _ld(P)
        rng = np.random.default_rng(2000 + seed + P % 991)
        if ints:  # small integers: every difference, square and partial sum is exact in any order
            last = rng.integers(-64, 65, size=ld).astype(np.float32)
            x = np.broadcast_to(last, (K, ld)) + rng.integers(-8, 9, size=(K, ld)).astype(np.float32)
            x = np.ascontiguousarray(x, dtype=np.float32)
        else:
            last = rng.standard_normal(ld, dtype=np.float32)
            x = cf.random_rows(rng, K, ld, P, last)
            # row k's update is (1 + k) times as long: a bound at the median norm clips some rows and not others
            x[:, :P] = last[:P] + (x[:, :P] - last[:P]) * (1 + np.arange(K, dtype=np.float32))[:, None]
        last[P:] = -7.0e3
        x[:, P:] = 3.0e4
        _CASES[key] = (last, x, torch.from_numpy(last).to(dev), torch.from_numpy(x).to(dev))
    return _CASES[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


def _sqnorms(xd, n, P, lastd):
    from fedscale_amd import kernels_clip as kc

    sq = torch.full((n,), -1.0, dtype=torch.float64, device=xd.device)
    kc.row_sqnorms(xd, n, P, lastd, sq, kc.workspace(n, P, xd.device))
    return sq


def _coefs(xd, n, P, lastd, M):
    """(device coefficients from the device's own norms, their host copy, the rejected count)."""
    from fedscale_amd import kernels_clip as kc

    sq = _sqnorms(xd, n, P, lastd)
    c = torch.full((n,), -1.0, dtype=torch.float32, device=xd.device)
    rej = torch.zeros(1, dtype=torch.int32, device=xd.device)
    kc.clip_coefs(sq, n, M, c, rej)
    ch = c.cpu().numpy()
    _same_bits(ch, cf.coefs_of(sq.cpu().numpy(), M), ("coefficients", n, P, M))
    return c, ch, int(rej.cpu()[0])


def _median_norm(x, last, P):
    with np.errstate(all="ignore"):
        n = np.sqrt(((x[:, :P] - last[:P]).astype(np.float64) ** 2).sum(axis=1))
    return float(np.median(n[np.isfinite(n)]))


# ---- norms ---------------------------------------------------------------------------------------------------------
def _check_norms(K, P, dev, ns):
    last, x, lastd, xd = _case(K, P, dev)
    exact = [cf.sq_exact(x[k, :P], last[:P]) for k in range(K)]
    singles = [_sqnorms(xd[k:k + 1], 1, P, lastd).cpu().numpy()[0] for k in range(K)]
    for n in ns:
        got = _sqnorms(xd, n, P, lastd).cpu().numpy()
        again = _sqnorms(xd, n, P, lastd).cpu().numpy()
        _same_bits(again, got, ("the same call twice", n, P))
        _same_bits(got, np.asarray(singles[:n]), ("one call over n rows = n calls of one row", n, P))
        for k in range(n):
            # fewer than P roundings of at most 2^-53 relative each on non-negative partial sums
            assert abs(got[k] - exact[k]) <= P * 2.0 ** -52 * exact[k], (n, P, k, got[k], exact[k])
            assert exact[k] > 0


def test_norms_small_widths(gpu_device):
    """P = 1 .. 4099 and the narrowest width at which a lane of the partial-sum launch adds two partials (65 wave
    tiles, the last ragged, three columns past the last float4); n = 1, 2, 5; poisons in x[:, P:] and last[P:]."""
    for P in cf.SMALL_P + (cf.P_NORM_TWO_PARTIALS,):
        _check_norms(5, P, gpu_device, (1, 2, 5))


@pytest.mark.parametrize("P", [cf.P_NORM_NARROW_MAX, cf.P_NORM_WIDE])
def test_norms_either_side_of_the_geometry_threshold(gpu_device, P):
    """The widest bucket of the narrow geometry, and the narrowest of the wide one: its capped grid's waves walk two
    tiles, the last tile ragged, one column past the last float4.  The plan is asserted first."""
    from fedscale_amd import kernels_clip as kc

    cus = _cus()
    plan = kc.norm_plan(cus, P)
    assert plan == cf.norm_plan(cus, P)
    if P == cf.P_NORM_WIDE:
        assert plan["tile_cols"] == 4096 and plan["grid"] * plan["waves"] < plan["tiles"] == 1025
    else:
        assert plan["tile_cols"] == 2048 and plan["tiles"] == 2048
    _check_norms(2, P, gpu_device, (2,))


def test_norms_are_exact_on_small_integers(gpu_device):
    """Differences in [-8, 8] on integer models: every square and every partial sum is an integer below 2^53, so any
    order of adds gives the exact value — the kernel must, bit for bit."""
    for P, K in [(p, 5) for p in cf.SMALL_P] + [(cf.P_NORM_TWO_PARTIALS, 5), (cf.P_NORM_NARROW_MAX, 2),
                                                      (cf.P_NORM_WIDE, 2)]:
        last, x, lastd, xd = _case(K, P, gpu_device, ints=True)
        d = (x[:, :P] - last[:P]).astype(np.int64)
        want = (d * d).sum(axis=1).astype(np.float64)
        for n in sorted({1, 2, K}):
            _same_bits(_sqnorms(xd, n, P, lastd), want[:n], ("integers", n, P))


# ---- coefficients --------------------------------------------------------------------------------------------------
def test_coefficients_straddle_the_bound(gpu_device):
    """Norms just below M (c = 1.0 exactly), just above, 1000 x above; an inf and a NaN upload give c = 0 and are
    counted.  Bit-equal to the host's fp64 M / (sqrt(sq) + 1e-6) rounded to fp32, from the device's own sq."""
    P, M = 257, 3.0
    last, x, lastd, xd = _case(5, P, gpu_device, seed=3)
    x = x.copy()
    u = (x[0, :P] - last[:P]).astype(np.float64)
    u /= np.sqrt((u * u).sum())
    for k, norm in enumerate((M * (1 - 1e-3), M * (1 + 1e-3), M * 1000.0)):
        x[k, :P] = last[:P] + (u * norm).astype(np.float32)
    x[3, 5] = np.inf
    x[4, P - 1] = np.nan
    xd = torch.from_numpy(x).to(gpu_device)
    c, ch, rejected = _coefs(xd, 5, P, lastd, M)  # (asserts the bits against the host formula)
    sq = _sqnorms(xd, 5, P, lastd).cpu().numpy()
    assert np.isinf(sq[3]) and np.isnan(sq[4]) and rejected == 2
    assert ch[0] == 1.0 and 0.99 < ch[1] < 1.0 and abs(ch[2] - 1e-3) < 1e-5 and ch[3] == 0.0 and ch[4] == 0.0
    assert math.sqrt(sq[0]) < M < math.sqrt(sq[1])


def test_coefficients_of_given_norms(gpu_device):
    from fedscale_amd import kernels_clip as kc

    M = 0.75
    vals = np.asarray([0.0, 1e-300, 1e-12, M * M, np.nextafter(M * M, 0), np.nextafter(M * M, 1), 0.5625, 2.0, 1e10,
                       1e300, np.inf, np.nan, 4.9e-324] + list(np.random.default_rng(1).uniform(0, 4, 300)))
    sq = torch.from_numpy(vals).to(gpu_device)
    c = torch.full((vals.size,), -1.0, dtype=torch.float32, device=gpu_device)
    rej = torch.full((1,), 10, dtype=torch.int32, device=gpu_device)
    kc.clip_coefs(sq, vals.size, M, c, rej)
    _same_bits(c, cf.coefs_of(vals, M), "given norms")
    assert int(rej.cpu()[0]) == 12  # the counter accumulates: 10 + inf + NaN
    assert (c.cpu().numpy() < 1).sum() > 100 and (c.cpu().numpy() == 1).sum() > 10


# ---- the chain -----------------------------------------------------------------------------------------------------
def _check_chain(K, P, dev, split=None, what=""):
    from fedscale_amd import kernels_clip as kc

    last, x, lastd, xd = _case(K, P, dev)
    ld = x.shape[1]
    M = _median_norm(x, last, P)
    c, ch, rejected = _coefs(xd, K, P, lastd, M)
    assert rejected == 0 and (K < 2 or ((ch < 1).any() and (ch == 1).any()))  # clipped and unclipped rows both
    want = cf.chain_of(x[:, :P], last[:P], ch)
    out = torch.full((ld,), 7.0, device=dev)
    kc.reduce_clip(xd, K, P, lastd, c, out)
    _same_bits(out[:P], want, (what, K, P, "one call"))
    assert bool((out[P:] == 7.0).all()), (what, K, P, "columns [P, ld) keep the pattern")
    if split:
        acc = torch.full((ld,), 7.0, device=dev)
        kc.reduce_clip(xd, split, P, lastd, c, acc)
        _same_bits(acc[:P], cf.chain_of(x[:split, :P], last[:P], ch[:split]), (what, K, P, "first chunk"))
        kc.reduce_clip(xd[split:], K - split, P, lastd, c[split:], acc, acc_in=acc)  # in place
        _same_bits(acc[:P], want, (what, K, P, "two chunks, aliasing"))
        assert bool((acc[P:] == 7.0).all())


def test_chain_small_widths(gpu_device):
    for P in cf.SMALL_P:
        _check_chain(5, P, gpu_device, split=3, what="small")


@pytest.mark.parametrize("shape", ["level2", "two_levels", "level0"])
def test_chain_every_k_loop_of_every_variant(gpu_device, shape):
    """K in {1, 2, U-1, U, U+1, 2U+1} for the U of each variant, at the narrowest width that takes the variant."""
    from fedscale_amd import kernels_clip as kc

    cus = _cus()
    P, want_plan = cf.expected_plans(cus)[shape]
    assert kc.reduce_clip_plan(cus, 3, P) == want_plan
    ks = cf.ks_for(want_plan[0]["U"])
    Kmax = max(ks)
    last, x, lastd, xd = _case(Kmax, P, gpu_device)
    c, ch, _ = _coefs(xd, Kmax, P, lastd, _median_norm(x, last, P))
    chain = np.zeros(P, dtype=np.float32)
    for k in range(Kmax):  # one restated chain; its value after K rows is the K-row call's
        chain = cf.chain_of(x[k:k + 1, :P], last[:P], ch[k:k + 1], acc=chain)
        if k + 1 in ks:
            out = torch.full((x.shape[1],), 7.0, device=gpu_device)
            kc.reduce_clip(xd, k + 1, P, lastd, c, out)
            _same_bits(out[:P], chain, (shape, k + 1))
            assert bool((out[P:] == 7.0).all())


@pytest.mark.parametrize("shape", ["two_levels", "capped"])
def test_chain_long_widths(gpu_device, shape):
    """Two plan levels in one call; the capped grid whose workgroups each walk two tiles, the last one ragged: one
    call, and two chunks whose second continues the first in place.  The plan is asserted first, so a change of the
    kernel's constants fails here instead of thinning what is covered."""
    from fedscale_amd import kernels_clip as kc

    cus = _cus()
    P, want_plan = cf.expected_plans(cus)[shape]
    assert kc.reduce_clip_plan(cus, 3, P) == want_plan
    _check_chain(3, P, gpu_device, split=2, what=shape)


@pytest.mark.parametrize("where", [0, 2, 4])
def test_a_rejected_row_never_reaches_the_chain(gpu_device, where):
    from fedscale_amd import kernels_clip as kc

    K, P = 5, cf.P_LEVEL2
    last, x, lastd, _ = _case(K, P, gpu_device)
    x = x.copy()
    x[where, 17] = np.nan
    x[where, 300:400] = np.inf
    x[where, 4000] = -np.inf
    xd = torch.from_numpy(x).to(gpu_device)
    M = _median_norm(x, last, P)
    c, ch, rejected = _coefs(xd, K, P, lastd, M)
    assert rejected == 1 and ch[where] == 0.0 and (np.delete(ch, where) != 0).all()
    out = torch.full((x.shape[1],), 7.0, device=gpu_device)
    kc.reduce_clip(xd, K, P, lastd, c, out)
    got = out[:P].cpu().numpy()
    assert np.isfinite(got).all()
    keep = [k for k in range(K) if k != where]
    _same_bits(got, cf.chain_of(x[keep][:, :P], last[:P], ch[keep]), ("the chain over the other rows", where))
    _same_bits(got, cf.chain_of(x[:, :P], last[:P], ch), ("the restatement's own skip", where))


# ---- finish --------------------------------------------------------------------------------------------------------
def _guarded(P, dev=None, fill=9.0):
    """A buffer of exactly P floats between two 256-byte guards: (whole, the P floats)."""
    whole = torch.full((64 + P + 64,), fill, dtype=torch.float32)
    whole = whole.to(dev) if dev is not None else whole.pin_memory()
    return whole, whole[64:64 + P]


def _guards_intact(whole, P, fill=9.0):
    return bool((whole[:64] == fill).all()) and bool((whole[64 + P:] == fill).all())


@pytest.mark.parametrize("sigma", [0.0, 0.0375])
def test_finish(gpu_device, sigma):
    """out = last + (chain / K [+ sigma z]) bit for bit, z being the device's own draws of fa_dp_normals at the same
    seed and offset; mean_delta_out and a pinned mirror; outputs end exactly at P between 256-byte guards."""
    from fedscale_amd import kernels as kx
    from fedscale_amd import kernels_clip as kc

    dev, seed, offset = gpu_device, 1234567, 1000
    for P in (1, 3, 4, 5, 257, cf.P_LEVEL2):
        rng = np.random.default_rng(P)
        cols = (P + 3) // 4 * 4
        chain = rng.standard_normal(cols, dtype=np.float32) * 5
        last = rng.standard_normal(cols, dtype=np.float32)
        chain[P:], last[P:] = 1e30, -1e30
        z = None
        if sigma > 0:
            z = torch.empty(cols, dtype=torch.float32, device=dev)
            kx.dp_normals(z, seed, offset)
            zh = z.cpu().numpy()
            assert abs(float(zh.mean())) < 1 and (P < 100 or 0.8 < float(zh[:P].std()) < 1.2)
        want, want_m = cf.finish_of(chain[:P], last[:P], 7, sigma, None if z is None else zh[:P])
        ow, out = _guarded(P, dev)
        mw, md = _guarded(P, dev)
        hw, mirror = _guarded(P)
        kc.finish(torch.from_numpy(chain).to(dev), torch.from_numpy(last).to(dev), P, float(np.float32(7)), out, z=z,
                  sigma=sigma, mean_delta_out=md, mirror=mirror)
        torch.cuda.synchronize()
        _same_bits(out, want, ("out", P, sigma))
        _same_bits(md, want_m, ("mean_delta_out", P, sigma))
        _same_bits(mirror.numpy(), want, ("mirror", P, sigma))
        assert _guards_intact(ow, P) and _guards_intact(mw, P) and _guards_intact(hw, P), P
        if sigma > 0:
            plain, _ = cf.finish_of(chain[:P], last[:P], 7)
            assert P < 100 or (want != plain).sum() > P // 2  # the noise is really in the result
        # without the optional outputs
        ow2, out2 = _guarded(P, dev)
        kc.finish(torch.from_numpy(chain).to(dev), torch.from_numpy(last).to(dev), P, 7.0, out2, z=z, sigma=sigma)
        _same_bits(out2, want, ("out alone", P, sigma))
        assert _guards_intact(ow2, P)


# ---- the ABI's refusals --------------------------------------------------------------------------------------------
def test_operands_are_checked_before_anything_is_queued(gpu_device):
    """FA_E_ARG, the operand named, "nothing was launched", outputs untouched: misaligned and pageable operands, a
    short workspace, no rows, ld < P, unknown flags."""
    from fedscale_amd import _native_clip as nc

    lib = nc.load()
    dev = gpu_device
    n, LD, P = 4, 128, 100
    x = torch.ones(n * LD + 64, dtype=torch.float32, device=dev)
    last = torch.zeros(LD, device=dev)
    out = torch.full((LD,), 7.0, device=dev)
    sq = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    c = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    rej = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.zeros(64, dtype=torch.float64, device=dev)
    z = torch.zeros(LD, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    pageable = np.zeros(1 << 16, dtype=np.float32)
    pinned = torch.zeros(1 << 16, dtype=torch.float32).pin_memory()
    err = lambda: lib.fa_last_error_string().decode()  # noqa: E731

    def norms(xp=x.data_ptr(), ld=LD, rows=n, p=P, lp=last.data_ptr(), sp=sq.data_ptr(), wp=ws.data_ptr(), wb=512):
        return lib.fcl_row_sqnorms(xp, ld, rows, p, lp, sp, wp, wb, st), err()

    def coefs(sp=sq.data_ptr(), rows=n, M=1.0, cp=c.data_ptr(), rp=rej.data_ptr()):
        return lib.fcl_clip_coefs(sp, rows, M, cp, rp, st), err()

    def reduce(xp=x.data_ptr(), ld=LD, rows=n, p=P, lp=last.data_ptr(), cp=c.data_ptr(), ap=None, op=out.data_ptr(),
               flags=0):
        return lib.fcl_reduce(xp, ld, rows, p, lp, cp, ap, op, flags, st), err()

    def finish(chp=x.data_ptr(), lp=last.data_ptr(), zp=None, sigma=0.0, den=4.0, p=P, op=out.data_ptr(), mp=None,
               hp=None):
        return lib.fcl_finish(chp, lp, zp, sigma, den, p, op, mp, hp, st), err()

    refused = [
        (norms(xp=x.data_ptr() + 4), "fcl_row_sqnorms", "x "),
        (norms(lp=last.data_ptr() + 8), "fcl_row_sqnorms", "last"),
        (norms(sp=sq.data_ptr() + 4), "fcl_row_sqnorms", "sq "),
        (norms(xp=pageable.ctypes.data), "fcl_row_sqnorms", "x is pageable"),
        (norms(xp=pinned.data_ptr()), "fcl_row_sqnorms", "x is pinned host memory"),
        (norms(lp=pageable.ctypes.data), "fcl_row_sqnorms", "last is pageable"),
        (norms(sp=pageable.ctypes.data), "fcl_row_sqnorms", "sq is pageable"),
        (norms(wp=pageable.ctypes.data), "fcl_row_sqnorms", "workspace is pageable"),
        (norms(wb=0), "fcl_row_sqnorms", "workspace of 0 bytes"),
        (norms(p=8192, ld=8192, rows=1, wb=24), "fcl_row_sqnorms", "workspace of 24 bytes, needs 32"),
        (norms(rows=0), "fcl_row_sqnorms", "n=0"),
        (norms(ld=96), "fcl_row_sqnorms", "ld=96 < P=100"),
        (norms(ld=LD + 2), "fcl_row_sqnorms", "multiple of 4"),
        (coefs(rows=0), "fcl_clip_coefs", "n=0"),
        (coefs(M=0.0), "fcl_clip_coefs", "max_norm"),
        (coefs(M=float("nan")), "fcl_clip_coefs", "max_norm"),
        (coefs(sp=pageable.ctypes.data), "fcl_clip_coefs", "sq is pageable"),
        (coefs(cp=pageable.ctypes.data), "fcl_clip_coefs", "c is pageable"),
        (coefs(rp=pageable.ctypes.data), "fcl_clip_coefs", "rejected is pageable"),
        (coefs(cp=c.data_ptr() + 2), "fcl_clip_coefs", "aligned"),
        (reduce(xp=x.data_ptr() + 8), "fcl_reduce", "x "),
        (reduce(op=out.data_ptr() + 4), "fcl_reduce", "out"),
        (reduce(xp=pageable.ctypes.data), "fcl_reduce", "x is pageable"),
        (reduce(xp=pinned.data_ptr()), "fcl_reduce", "x is pinned host memory"),
        (reduce(lp=pageable.ctypes.data), "fcl_reduce", "last is pageable"),
        (reduce(cp=pageable.ctypes.data), "fcl_reduce", "c is pageable"),
        (reduce(op=pageable.ctypes.data), "fcl_reduce", "out is pageable"),
        (reduce(ap=pageable.ctypes.data, flags=1), "fcl_reduce", "acc_in is pageable"),
        (reduce(flags=1), "fcl_reduce", "acc_in"),
        (reduce(rows=0), "fcl_reduce", "n=0"),
        (reduce(ld=96), "fcl_reduce", "ld=96 < P=100"),
        (reduce(flags=2), "fcl_reduce", "flags"),
        (reduce(flags=8), "fcl_reduce", "flags"),
        (finish(chp=pageable.ctypes.data), "fcl_finish", "chain is pageable"),
        (finish(op=pageable.ctypes.data), "fcl_finish", "out is pageable"),
        (finish(mp=pageable.ctypes.data), "fcl_finish", "mean_delta_out is pageable"),
        (finish(hp=pageable.ctypes.data), "fcl_finish", "mirror is pageable"),
        (finish(mp=pinned.data_ptr()), "fcl_finish", "mean_delta_out is pinned host memory"),
        (finish(sigma=0.5), "fcl_finish", "without z"),
        (finish(sigma=0.5, zp=pageable.ctypes.data), "fcl_finish", "z is pageable"),
        (finish(sigma=-1.0, zp=z.data_ptr()), "fcl_finish", "sigma"),
        (finish(den=0.0), "fcl_finish", "denom"),
        (finish(op=out.data_ptr() + 4), "fcl_finish", "out"),
    ]
    for (rc, msg), entry, word in refused:
        assert rc == -1 and entry in msg and word in msg and "nothing was launched" in msg, (rc, msg, entry, word)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((sq == 7.0).all()) and bool((c == 7.0).all()) and int(rej.cpu()[0]) == 0
    # rows that would run past their allocation (a hipMalloc of its own: torch's allocator hands out slices)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    short = ctypes.c_void_p()
    nbytes = ((n - 1) * LD + 96) * 4
    assert hip.hipMalloc(ctypes.byref(short), nbytes) == 0
    try:
        assert hip.hipMemset(short, 0, nbytes) == 0
        for rc, msg in (norms(xp=short.value), reduce(xp=short.value)):  # the last row needs 100 columns, has 96
            assert rc == -1 and "x extends" in msg and "past the end of its allocation" in msg, msg
        rc, msg = norms(xp=short.value, p=96)
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert bool((sq == 0.0).all())
    finally:
        torch.cuda.synchronize()
        hip.hipFree(short)
    # and the valid calls go through: rows of ones against a model of zeros, M = 1
    assert norms()[0] == 0 and coefs()[0] == 0 and reduce()[0] == 0
    assert finish(chp=out.data_ptr(), op=z.data_ptr(), hp=pinned.data_ptr())[0] == 0
    torch.cuda.synchronize()
    assert bool((sq == 100.0).all()) and int(rej.cpu()[0]) == 0
    ck = np.float32(1.0 / (10.0 + 1e-6))
    assert bool((c == float(ck)).all())
    chain = np.float32(0)
    for _ in range(n):
        chain = np.float32(chain + ck * np.float32(1.0))
    assert bool((out[:P] == float(chain)).all()) and bool((out[P:] == 7.0).all())
    assert bool((z[:P] == float(chain / np.float32(4))).all()) and bool((z[P:] == 0).all())
    assert bool((pinned[:P] == z[:P].cpu()).all()) and bool((pinned[P:] == 0).all())
