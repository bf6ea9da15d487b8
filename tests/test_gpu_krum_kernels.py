"""The kernels of Krum / Multi-Krum selection (include/fedkrum.h) on the MI355X against the numpy restatement of
tests/krum_fixtures.py.  The Gram matrix is exact (every bit) on integer-valued data and within the derived any-order
summation bound of the fsum reference otherwise; everything after it — scores, selection, finish — is bit for bit.  Rows
have ld > P with NaN in columns [P, ld).  K <= 200 and P <= 20 000 throughout, except fk_scores' row widths, which take
a host-made G (tests/test_krum_plan.py asserts the conditions each shape is listed for)."""
import numpy as np
import pytest
import torch

from tests import krum_fixtures as kf

pytestmark = pytest.mark.gpu

GUARD = 256
F32, F64 = np.float32, np.float64


def _ld(P):
    return (P + 3) // 4 * 4 + 8  # ld > P always: columns [P, ld) hold NaN


def _bits64(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _gram(xd, K, P, Ld, dev):
    from fedscale_amd import kernels_krum as kk

    out = torch.full((K * K,), 7.0, dtype=torch.float64, device=dev)
    ws = kk.gram_workspace(K, P, dev)
    ws.fill_(float("nan"))  # nothing of the workspace is read before it is written
    kk.gram(xd, K, P, Ld, out, ws)
    return out.cpu().numpy().reshape(K, K)


def _assert_plan(K, P):
    """The conditions a shape is run for, from fk_gram_plan itself."""
    from fedscale_amd import kernels_krum as kk

    p = kk.gram_plan(K, P)
    assert p == kf.plan(K, P)
    if K == max(kf.GRAM_K):
        assert p["tiles"] >= 6  # three row tiles: an off-diagonal tile with both indices above 0
    if P in (kf.STEP - 1, kf.STEP, kf.STEP + 1):
        assert p["step_cols"] == kf.STEP and -(-P // p["step_cols"]) == (1 if P <= kf.STEP else 2)
    if P == kf.P_SPLIT:
        assert p["nsplit"] >= 2 and 2 <= p["last_steps"] < p["split_cols"] // p["step_cols"]
    return p


# ---- fk_gram ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", kf.GRAM_K)
def test_gram_is_exact_on_integer_data(gpu_device, K):
    for P in kf.GRAM_P:
        _assert_plan(K, P)
        rng = np.random.default_rng(1000 * K + P)
        x, L = kf.int_rows(rng, K, P, _ld(P))
        assert np.isnan(x[:, P:]).all() and np.isnan(L[P:]).all()
        d = kf.diffs(x, L, P)
        want = kf.gram_exact(d)
        got = _gram(torch.from_numpy(x).to(gpu_device), K, P, torch.from_numpy(L).to(gpu_device), gpu_device)
        bad = np.argwhere(_bits64(got) != _bits64(want))
        assert bad.size == 0, (K, P, bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
        assert np.array_equal(_bits64(got), _bits64(got.T)), (K, P, "symmetric")


def test_gram_of_non_integer_data_is_within_the_derived_bound_and_repeats(gpu_device):
    K, P = kf.NONINT_SHAPE
    p = _assert_plan(K, P)
    assert p["nsplit"] >= 2 and p["split_cols"] // p["step_cols"] >= 2  # the splits and the step loop iterate
    x, L = kf.normal_rows(np.random.default_rng(77), K, P, _ld(P))
    x[:, P:] = np.nan
    d = kf.diffs(x, L, P)
    want, bound = kf.gram_fsum(d), kf.gram_bound(d)
    xd, Ld = torch.from_numpy(x).to(gpu_device), torch.from_numpy(L).to(gpu_device)
    got = _gram(xd, K, P, Ld, gpu_device)
    err = np.abs(got - want)
    print("gram error / bound, max:", float((err / bound).max()), "max error:", float(err.max()))
    assert (err <= bound).all(), (float((err / bound).max()),)
    assert np.array_equal(_bits64(got), _bits64(got.T))
    again = _gram(xd, K, P, Ld, gpu_device)
    assert np.array_equal(_bits64(got), _bits64(again))  # the same bits on a second run


def test_non_finite_rows_stay_in_their_rows_and_columns(gpu_device):
    K, P = 20, kf.P_SPLIT
    _assert_plan(K, P)
    x, L = kf.normal_rows(np.random.default_rng(5), K, P, _ld(P))
    x[:, 40] = L[40]  # a column where every row's d is 0 ...
    clean = _gram(torch.from_numpy(x).to(gpu_device), K, P, torch.from_numpy(L).to(gpu_device), gpu_device)
    assert np.isfinite(clean).all()
    bad = x.copy()
    bad[3, 7] = np.inf
    bad[9, 200] = np.nan
    bad[14, 40] = -np.inf  # ... so this inf meets only zeros: inf * 0
    got = _gram(torch.from_numpy(bad).to(gpu_device), K, P, torch.from_numpy(L).to(gpu_device), gpu_device)
    rows = [3, 9, 14]
    keep = np.ones(K, dtype=bool)
    keep[rows] = False
    assert np.array_equal(_bits64(got[np.ix_(keep, keep)]), _bits64(clean[np.ix_(keep, keep)]))
    assert not np.isfinite(got[rows][:, rows].diagonal()).any()
    # and every case of v leads to dist2 = +inf, score = +inf for exactly those rows
    from fedscale_amd import kernels_krum as kk

    sc = torch.zeros(K, dtype=torch.float64, device=gpu_device)
    kk.scores(torch.from_numpy(got.reshape(-1)).to(gpu_device), K, 3, sc)
    s = sc.cpu().numpy()
    assert np.isposinf(s[rows]).all() and np.isfinite(s[keep]).all()
    assert np.array_equal(_bits64(s), _bits64(kf.scores_of(got, 3)))


# ---- fk_scores -------------------------------------------------------------------------------------------------------
def _host_gram(rng, K):
    """A symmetric K x K matrix (not a true Gram: v goes negative) with ties, NaN and inf entries."""
    g = rng.integers(0, 6, size=(K, K)).astype(F64)  # small integers: many equal distances
    g = g + g.T
    g[np.arange(K), np.arange(K)] = rng.integers(0, 4, size=K)  # small diagonals: (gii + gjj) - 2 gij < 0 often
    if K >= 9:  # non-integers in the later rows and columns, so that the order of the adds matters
        frac = rng.random((K, K))
        late = np.arange(K) >= K // 2
        g = g + (frac + frac.T) * (late[:, None] | late[None, :])
    if K >= 5:
        g[1, 3] = g[3, 1] = np.nan
        g[K - 1, K - 1] = np.inf  # an infinite row: dist2 = +inf to everyone
    return g


@pytest.mark.parametrize("K", kf.SCORE_K)
def test_scores_are_bit_exact_at_every_width(gpu_device, K):
    from fedscale_amd import kernels_krum as kk

    rng = np.random.default_rng(K)
    g = _host_gram(rng, K)
    with np.errstate(invalid="ignore"):
        v = (np.diag(g)[:, None] + np.diag(g)[None, :]) - 2.0 * g
    assert K < 5 or ((v < 0).any() and np.isnan(v).any())
    gd = torch.from_numpy(g.reshape(-1).copy()).to(gpu_device)
    fmax = (K - 3) // 2
    for f in sorted({0, 1 if fmax >= 1 else 0, fmax // 2, fmax}):
        sc = torch.full((K,), -1.0, dtype=torch.float64, device=gpu_device)
        kk.scores(gd, K, f, sc)
        got, want = sc.cpu().numpy(), kf.scores_of(g, f)
        bad = np.flatnonzero(_bits64(got) != _bits64(want))
        assert bad.size == 0, (K, f, bad[:5], got[bad[:5]], want[bad[:5]])
        if K >= 5:
            assert np.isposinf(got[K - 1]) and np.isfinite(got[:K - 1]).any()


# ---- fk_select -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,m", [(3, 1), (7, 3), (7, 4), (7, 7), (200, 150), (1500, 700), (4096, 4096)])
def test_select(gpu_device, K, m):
    from fedscale_amd import kernels_krum as kk

    rng = np.random.default_rng(K + m)
    if K == 7:
        sc = np.asarray([2.0, 1.0, 2.0, np.inf, 1.0, 0.5, np.inf])  # ties, and fewer finite scores than m = 7
    else:
        sc = rng.integers(0, max(2, K // 3), size=K).astype(F64)  # every score several times
        sc[rng.integers(0, K, size=max(1, K // 10))] = np.inf
    c = torch.full((K + 4,), 9.0, dtype=torch.float32, device=gpu_device)
    n = torch.full((2,), -5, dtype=torch.int32, device=gpu_device)
    kk.select(torch.from_numpy(sc).to(gpu_device), K, m, c, n)
    want_c, want_n = kf.select_of(sc, m)
    got_c, got_n = c.cpu().numpy(), n.cpu().numpy()
    assert np.array_equal(_bits32(got_c[:K]), _bits32(want_c)) and (got_c[K:] == 9.0).all()
    assert got_n[0] == want_n and got_n[1] == -5
    assert want_n == min(m, int(np.isfinite(sc).sum())) and not (want_c[~np.isfinite(sc)] != 0).any()
    allinf = torch.full((K,), float("inf"), dtype=torch.float64, device=gpu_device)
    kk.select(allinf, K, m, c, n)
    assert int(n.cpu()[0]) == 0 and (c.cpu().numpy()[:K] == 0).all()


# ---- fk_finish -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3, 4, 5, 1023, 4097])
def test_finish(gpu_device, P):
    from fedscale_amd import kernels_krum as kk

    rng = np.random.default_rng(P)
    ld = _ld(P)
    chain = np.full(ld, np.nan, dtype=F32)
    L = np.full(ld, np.nan, dtype=F32)
    chain[:P] = rng.standard_normal(P).astype(F32) * 5
    L[:P] = rng.standard_normal(P).astype(F32)
    L[0] = -0.0
    cd, Ld = torch.from_numpy(chain).to(gpu_device), torch.from_numpy(L).to(gpu_device)
    for n_sel in (0, 1, 3, 8):
        out = torch.full((ld,), 7.0, dtype=torch.float32, device=gpu_device)
        pinned = torch.full((ld,), 7.0, dtype=torch.float32).pin_memory()
        dmirror = torch.full((ld,), 7.0, dtype=torch.float32, device=gpu_device)
        nd = torch.tensor([n_sel], dtype=torch.int32, device=gpu_device)
        kk.finish(cd, Ld, nd, P, out, mirror=pinned)
        kk.finish(cd, Ld, nd, P, dmirror.clone(), mirror=dmirror)
        torch.cuda.synchronize()
        want = kf.finish_of(chain[:P], L[:P], n_sel)
        if n_sel == 0:
            assert np.array_equal(_bits32(want), _bits32(L[:P]))  # the bits of L, -0 included
        for name, got in (("out", out.cpu().numpy()), ("pinned", pinned.numpy()), ("mirror", dmirror.cpu().numpy())):
            assert np.array_equal(_bits32(got[:P]), _bits32(want)), (P, n_sel, name)
            assert (got[P:] == 7.0).all(), (P, n_sel, name, "columns >= P are not written")


# ---- refusals and extents ------------------------------------------------------------------------------------------
def test_refused_calls_launch_nothing(gpu_device):
    from fedscale_amd import _native_krum as nk
    from fedscale_amd._native import FedAggError
    from fedscale_amd.kernels import _stream

    K, P = 5, 40
    ld = _ld(P)
    x = torch.zeros((K, ld), dtype=torch.float32, device=gpu_device)
    L = torch.zeros(ld, dtype=torch.float32, device=gpu_device)
    g = torch.full((K * K,), 7.0, dtype=torch.float64, device=gpu_device)
    big = torch.full((64,), 7.0, dtype=torch.float64, device=gpu_device)
    sc = torch.full((K,), 7.0, dtype=torch.float64, device=gpu_device)
    c = torch.full((K,), 7.0, dtype=torch.float32, device=gpu_device)
    n = torch.full((1,), 7, dtype=torch.int32, device=gpu_device)
    need = nk.call("fk_gram_workspace_bytes", K, P)
    ws = torch.full((need // 8 + 2,), 7.0, dtype=torch.float64, device=gpu_device)
    st = _stream(g)
    p = lambda t: t.data_ptr()  # noqa: E731
    cases = [
        ("fk_gram", (p(x), ld, nk.MAX_K + 1, P, p(L), p(g), p(ws), 1 << 40, st), "FK_MAX_K"),
        ("fk_gram", (p(x) + 4, ld, K, P, p(L), p(g), p(ws), need, st), "16-byte aligned"),
        ("fk_gram", (p(x), ld, K, P, p(L), p(g), p(ws), need - 1, st), "workspace"),
        ("fk_gram", (p(x), ld - 1, K, P, p(L), p(g), p(ws), need, st), "multiple of 4"),
        ("fk_gram", (p(x), P - 4, K, P, p(L), p(g), p(ws), need, st), "ld="),
        ("fk_scores", (p(big), nk.MAX_K + 1, 0, p(sc), st), "FK_MAX_K"),
        ("fk_scores", (p(g), K, 2, p(sc), st), r"2f \+ 3 <= K"),
        ("fk_scores", (p(g), K, -1, p(sc), st), r"2f \+ 3 <= K"),
        ("fk_select", (p(sc), K, 0, p(c), p(n), st), "1 <= m <= K"),
        ("fk_select", (p(sc), K, K + 1, p(c), p(n), st), "1 <= m <= K"),
        ("fk_select", (p(sc), nk.MAX_K + 1, 1, p(c), p(n), st), "FK_MAX_K"),
        ("fk_finish", (p(L) + 4, p(L), p(n), P, p(x), None, st), "16-byte aligned"),
    ]
    for name, args, match in cases:
        with pytest.raises(FedAggError, match=f"{name}.*{match}.*nothing was launched"):
            nk.call(name, *args)
    torch.cuda.synchronize()
    for t in (g, big, sc, c, ws):
        assert (t.cpu().numpy() == 7.0).all()
    assert int(n.cpu()[0]) == 7 and (x.cpu().numpy() == 0).all()


class _Guarded:
    """``nbytes`` of device memory with GUARD bytes of 0xA5 before and after it (and 0xA5 inside, to begin with)."""

    def __init__(self, dev, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def check(self, ctx, dtype):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == 0xA5).all(), f"{ctx}: written before its start"
        assert (b[GUARD + self.nbytes:] == 0xA5).all(), f"{ctx}: written past its declared extent"
        return b[GUARD:GUARD + self.nbytes].copy().view(dtype)


def test_kernels_leave_memory_past_the_declared_extents_alone(gpu_device):
    """K = 67 (a ragged second row tile), P = 301 (a ragged float4 and a ragged step): every output sits between guards
    and ends exactly at the extent include/fedkrum.h declares — nsplit * K * K doubles of workspace, K * K of the Gram,
    K scores, K coefficients, one count, P floats of out and mirror."""
    from fedscale_amd import _native_krum as nk
    from fedscale_amd.kernels import _stream

    K, P, f, m = 67, kf.P_SPLIT, 5, 40
    ld = _ld(P)
    x, L = kf.int_rows(np.random.default_rng(9), K, P, ld)
    xd, Ld = torch.from_numpy(x).to(gpu_device), torch.from_numpy(L).to(gpu_device)
    st = _stream(xd)
    need = int(nk.call("fk_gram_workspace_bytes", K, P))
    assert need == kf.workspace_bytes(K, P)
    g_ws, g_gram = _Guarded(gpu_device, need), _Guarded(gpu_device, K * K * 8)
    g_sc, g_c, g_n = _Guarded(gpu_device, K * 8), _Guarded(gpu_device, K * 4), _Guarded(gpu_device, 16)
    g_out, g_mir = _Guarded(gpu_device, P * 4 + (-P * 4) % 16), _Guarded(gpu_device, P * 4 + (-P * 4) % 16)
    nk.call("fk_gram", xd.data_ptr(), ld, K, P, Ld.data_ptr(), g_gram.ptr, g_ws.ptr, need, st)
    nk.call("fk_scores", g_gram.ptr, K, f, g_sc.ptr, st)
    nk.call("fk_select", g_sc.ptr, K, m, g_c.ptr, g_n.ptr, st)
    chain = torch.ones(ld, dtype=torch.float32, device=gpu_device)
    nk.call("fk_finish", chain.data_ptr(), Ld.data_ptr(), g_n.ptr, P, g_out.ptr, g_mir.ptr, st)
    torch.cuda.synchronize()
    g_ws.check("workspace", F64)
    G = g_gram.check("gram_out", F64).reshape(K, K)
    want = kf.krum_round(x, L, P, f, m)
    assert np.array_equal(_bits64(G), _bits64(want["G"]))
    assert np.array_equal(_bits64(g_sc.check("score_out", F64)), _bits64(want["score"]))
    assert np.array_equal(_bits32(g_c.check("c_out", F32)), _bits32(want["c"]))
    cnt = g_n.check("n_sel_out", np.int32)
    assert cnt[0] == want["n_sel"] == m and (cnt[1:].view(np.uint32) == 0xA5A5A5A5).all()
    fin = kf.finish_of(np.ones(P, dtype=F32), L[:P], m)
    for name, gd in (("out", g_out), ("mirror", g_mir)):
        got = gd.check(name, F32)
        assert np.array_equal(_bits32(got[:P]), _bits32(fin)), name
        assert (got[P:].view(np.uint32) == 0xA5A5A5A5).all(), (name, "columns >= P are not written")
    assert np.isnan(xd.cpu().numpy()[:, P:]).all()  # the rows were only read
