"""The kernels of geometric-median aggregation (include/fedgeomed.h) on the MI355X against the numpy restatement of
tests/geomed_fixtures.py, bit for bit: the start weights, an iteration's weights and objective, the distances in Gram
space (host-made symmetric matrices, so K runs to 4096 without a Gram of real rows) and the finish.  Every K and P is
a boundary of the 64-lane sum, of the 256 chunk / j block, of the 1024-thread workgroup or of the float4 column
(tests/test_geomed_plan.py asserts the lists)."""
import numpy as np
import pytest
import torch

from tests import geomed_fixtures as gf

pytestmark = pytest.mark.gpu

GUARD = 256
F32, F64 = np.float32, np.float64
NU = 1e-6


def _bits64(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _same64(got, want, what):
    bad = np.flatnonzero(_bits64(got) != _bits64(want))
    assert bad.size == 0, (what, bad[:5], np.asarray(got)[bad[:5]], np.asarray(want)[bad[:5]])


def _outputs(K, dev):
    """w, c, obj, n_valid with sentinels and slack past K."""
    return (torch.full((K + 3,), 7.0, dtype=torch.float64, device=dev),
            torch.full((K + 3,), 7.0, dtype=torch.float32, device=dev),
            torch.full((2,), 7.0, dtype=torch.float64, device=dev),
            torch.full((2,), -5, dtype=torch.int32, device=dev))


# ---- fgm_weights -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", gf.WEIGHTS_K)
def test_weights_are_bit_exact(gpu_device, K):
    from fedscale_amd import kernels_geomed as kg

    rng = np.random.default_rng(K)
    for name, q in (("crafted", gf.crafted_q(rng, K, NU)), ("plain", (rng.random(K) * 3 + 0.1) ** 2),
                    ("invalid", np.where(np.arange(K) % 2 == 0, np.nan, np.inf))):
        w, c, obj, n = _outputs(K, gpu_device)
        kg.weights(torch.from_numpy(q).to(gpu_device), K, NU, w, c, obj, n)
        ww, wc, wobj, wn = gf.weights_of(q, NU)
        gw, gc, gobj, gn = w.cpu().numpy(), c.cpu().numpy(), obj.cpu().numpy(), n.cpu().numpy()
        _same64(gw[:K], ww, (K, name, "w"))
        assert np.array_equal(_bits32(gc[:K]), _bits32(wc)), (K, name, "c")
        assert _bits64(gobj[:1])[0] == _bits64([wobj])[0], (K, name, gobj[0], wobj)
        assert gn[0] == wn and gn[1] == -5 and gobj[1] == 7.0 and (gw[K:] == 7.0).all() and (gc[K:] == 7.0).all()
        if name == "invalid":
            assert wn == 0 and (gw[:K] == 0).all() and not np.signbit(gw[:K]).any() and gobj[0] == 0.0
        elif K >= 3:
            assert 0 < wn <= K and abs(gw[:K].sum() - 1) < 1e-12 and (gw[:K][~np.isfinite(q)] == 0).all()


# ---- fgm_start -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", gf.WEIGHTS_K)
def test_start_is_bit_exact_at_both_strides(gpu_device, K):
    from fedscale_amd import kernels_geomed as kg

    rng = np.random.default_rng(100 + K)
    q0 = (rng.random(K) * 5) ** 2
    if K >= 8:
        q0[rng.permutation(K)[:4]] = (np.nan, np.inf, -np.inf, 0.0)
        q0[K // 2] = q0[K // 3] = q0[K - 1]  # ties, possibly at the median
        big = rng.permutation(K)[:max(1, K // 5)]
        q0[big] = q0[big] * 2.0 ** 100  # a minority far above the median norm
    ww, wc, wn = gf.start_of(q0)
    for stride in (1, K + 1):
        if stride == 1:
            src = q0.copy()
        else:  # the diagonal of a K x K matrix whose other entries must not be read as norms
            src = np.full((K, K), -3.0)
            src[np.arange(K), np.arange(K)] = q0
            src = src.reshape(-1)
        w, c, _, n = _outputs(K, gpu_device)
        kg.start(torch.from_numpy(src).to(gpu_device), K, w, c, n, stride=stride)
        gw, gc, gn = w.cpu().numpy(), c.cpu().numpy(), n.cpu().numpy()
        _same64(gw[:K], ww, (K, stride, "w"))
        assert np.array_equal(_bits32(gc[:K]), _bits32(wc)), (K, stride, "c")
        assert gn[0] == wn and gn[1] == -5 and (gw[K:] == 7.0).all() and (gc[K:] == 7.0).all()
    assert wn == int(np.isfinite(q0).sum()) and (ww[~np.isfinite(q0)] == 0).all()
    allbad = torch.full((K,), float("nan"), dtype=torch.float64, device=gpu_device)
    w, c, _, n = _outputs(K, gpu_device)
    kg.start(allbad, K, w, c, n)
    assert int(n.cpu()[0]) == 0 and (w.cpu().numpy()[:K] == 0).all() and (c.cpu().numpy()[:K] == 0).all()


# ---- fgm_gram_dist2 --------------------------------------------------------------------------------------------------
def _dist2(gd, K, wd, dev):
    from fedscale_amd import kernels_geomed as kg

    q = torch.full((K + 3,), 7.0, dtype=torch.float64, device=dev)
    ws = kg.dist2_workspace(K, dev)
    ws.fill_(float("nan"))  # nothing of the workspace is read before it is written
    kg.gram_dist2(gd, K, wd, q, ws)
    got = q.cpu().numpy()
    assert (got[K:] == 7.0).all()
    return got[:K]


@pytest.mark.parametrize("K", gf.DIST2_K)
def test_gram_dist2_is_bit_exact(gpu_device, K):
    rng = np.random.default_rng(200 + K)
    for integer in (True, False):
        g = gf.symmetric(rng, K, integer)
        if integer:
            w = rng.integers(0, 4, size=K).astype(F64) / 64.0  # dyadic, many exact zeros, far from summing to 1
        else:
            w = rng.random(K) / K * 0.7
            w[rng.random(K) < 0.2] = 0.0
        bad = []
        if not integer and K >= 5:  # two non-finite rows and columns; their weight is 0, as in every round
            bad = [1, K - 2]
            g[1, :] = g[:, 1] = np.nan
            g[K - 2, :] = g[:, K - 2] = np.inf
            g[K - 2, K - 2] = -np.inf
            w[bad] = 0.0
        want = gf.gram_dist2_of(g, w)
        gd, wd = torch.from_numpy(g.reshape(-1).copy()).to(gpu_device), torch.from_numpy(w).to(gpu_device)
        got = _dist2(gd, K, wd, gpu_device)
        keep = np.ones(K, dtype=bool)
        keep[bad] = False
        _same64(got[keep], want[keep], (K, integer))
        assert np.isfinite(got[keep]).all() and not np.isfinite(got[~keep]).any()
        if integer:  # and the exact route: sum over j, k of w_j G_jk w_k is exact in any order here
            b = float(w @ g @ w)
            assert np.array_equal(got, (np.diag(g) - 2.0 * (g @ w)) + b)
        else:
            again = _dist2(gd, K, wd, gpu_device)
            assert np.array_equal(_bits64(got), _bits64(again))  # the same bits on a second run


# ---- fgm_finish ------------------------------------------------------------------------------------------------------
def _ld(P):
    return (P + 3) // 4 * 4 + 8


@pytest.mark.parametrize("P", gf.FINISH_P)
def test_finish(gpu_device, P):
    from fedscale_amd import kernels_geomed as kg

    rng = np.random.default_rng(P)
    ld = _ld(P)
    chain = np.full(ld, np.nan, dtype=F32)
    L = np.full(ld, np.nan, dtype=F32)
    chain[:P] = rng.standard_normal(P).astype(F32) * 5
    L[:P] = rng.standard_normal(P).astype(F32)
    L[0] = -0.0
    cd, Ld = torch.from_numpy(chain).to(gpu_device), torch.from_numpy(L).to(gpu_device)
    for n_valid in (0, 1, 8):
        out = torch.full((ld,), 7.0, dtype=torch.float32, device=gpu_device)
        plain = torch.full((ld,), 7.0, dtype=torch.float32, device=gpu_device)
        pinned = torch.full((ld,), 7.0, dtype=torch.float32).pin_memory()
        dmirror = torch.full((ld,), 7.0, dtype=torch.float32, device=gpu_device)
        nd = torch.tensor([n_valid], dtype=torch.int32, device=gpu_device)
        kg.finish(cd, Ld, nd, P, plain)
        kg.finish(cd, Ld, nd, P, out, mirror=pinned)
        kg.finish(cd, Ld, nd, P, dmirror.clone(), mirror=dmirror)
        torch.cuda.synchronize()
        want = gf.finish_of(chain[:P], L[:P], n_valid)
        if n_valid == 0:
            assert np.array_equal(_bits32(want), _bits32(L[:P]))  # the bits of L, -0 included
        for name, got in (("no mirror", plain.cpu().numpy()), ("out", out.cpu().numpy()), ("pinned", pinned.numpy()),
                          ("mirror", dmirror.cpu().numpy())):
            assert np.array_equal(_bits32(got[:P]), _bits32(want)), (P, n_valid, name)
            assert (got[P:] == 7.0).all(), (P, n_valid, name, "columns >= P are not written")


# ---- refusals and extents ------------------------------------------------------------------------------------------
def test_refused_calls_launch_nothing(gpu_device):
    from fedscale_amd import _native_geomed as ng
    from fedscale_amd._native import FedAggError
    from fedscale_amd.kernels import _stream

    K, P = 5, 40
    ld = _ld(P)
    g = torch.full((K * K,), 7.0, dtype=torch.float64, device=gpu_device)
    q = torch.full((K + 1,), 7.0, dtype=torch.float64, device=gpu_device)
    w = torch.full((K + 1,), 7.0, dtype=torch.float64, device=gpu_device)
    obj = torch.full((2,), 7.0, dtype=torch.float64, device=gpu_device)
    c = torch.full((K + 1,), 7.0, dtype=torch.float32, device=gpu_device)
    n = torch.full((2,), 7, dtype=torch.int32, device=gpu_device)
    L = torch.full((ld,), 7.0, dtype=torch.float32, device=gpu_device)
    out = torch.full((ld,), 7.0, dtype=torch.float32, device=gpu_device)
    need = int(ng.call("fgm_dist2_workspace_bytes", K))
    ws = torch.full((need // 8 + 2,), 7.0, dtype=torch.float64, device=gpu_device)
    st = _stream(g)
    p = lambda t: t.data_ptr()  # noqa: E731
    cases = [
        ("fgm_start", (p(q), 1, 0, p(w), p(c), p(n), st), "K=0"),
        ("fgm_start", (p(q), 1, ng.MAX_K + 1, p(w), p(c), p(n), st), "FGM_MAX_K"),
        ("fgm_start", (p(q), 0, K, p(w), p(c), p(n), st), "stride=0"),
        ("fgm_start", (None, 1, K, p(w), p(c), p(n), st), "NULL"),
        ("fgm_start", (p(q) + 4, 1, K, p(w), p(c), p(n), st), "aligned"),
        ("fgm_start", (p(q), 1, K, p(w), p(c) + 2, p(n), st), "aligned"),
        ("fgm_weights", (p(q), 0, NU, p(w), p(c), p(obj), p(n), st), "K=0"),
        ("fgm_weights", (p(q), ng.MAX_K + 1, NU, p(w), p(c), p(obj), p(n), st), "FGM_MAX_K"),
        ("fgm_weights", (p(q), K, 0.0, p(w), p(c), p(obj), p(n), st), "nu="),
        ("fgm_weights", (p(q), K, -1e-6, p(w), p(c), p(obj), p(n), st), "nu="),
        ("fgm_weights", (p(q), K, float("nan"), p(w), p(c), p(obj), p(n), st), "nu="),
        ("fgm_weights", (p(q), K, float("inf"), p(w), p(c), p(obj), p(n), st), "nu="),
        ("fgm_weights", (p(q), K, NU, p(w), p(c), None, p(n), st), "NULL"),
        ("fgm_weights", (p(q), K, NU, p(w) + 4, p(c), p(obj), p(n), st), "aligned"),
        ("fgm_gram_dist2", (p(g), 0, p(w), p(q), p(ws), need, st), "K=0"),
        ("fgm_gram_dist2", (p(g), ng.MAX_K + 1, p(w), p(q), p(ws), 1 << 40, st), "FGM_MAX_K"),
        ("fgm_gram_dist2", (p(g), K, p(w), p(q), p(ws), need - 1, st), "workspace"),
        ("fgm_gram_dist2", (p(g), K, p(w), p(q), None, need, st), "NULL"),
        ("fgm_gram_dist2", (p(g) + 4, K, p(w), p(q), p(ws), need, st), "aligned"),
        ("fgm_finish", (p(L) + 4, p(L), p(n), P, p(out), None, st), "16-byte aligned"),
        ("fgm_finish", (p(L), p(L), p(n), P, p(out) + 4, None, st), "16-byte aligned"),
        ("fgm_finish", (p(L), p(L), None, P, p(out), None, st), "NULL"),
        ("fgm_finish", (p(L), p(L), p(n), -1, p(out), None, st), "negative P"),
    ]
    for name, args, match in cases:
        with pytest.raises(FedAggError, match=f"{name}.*{match}.*nothing was launched"):
            ng.call(name, *args)
    torch.cuda.synchronize()
    for t in (g, q, w, obj, c, L, out, ws):
        assert (t.cpu().numpy() == 7.0).all()
    assert (n.cpu().numpy() == 7).all()


def test_a_stream_of_another_device_than_the_output_is_refused(gpu_device):
    from fedscale_amd import _native_geomed as ng
    from fedscale_amd._native import FedAggError

    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU to make a stream on another device than the output's")
    K, P = 5, 40
    q = torch.full((K * K,), 7.0, dtype=torch.float64, device=gpu_device)
    w = torch.full((K,), 7.0, dtype=torch.float64, device=gpu_device)
    obj = torch.full((1,), 7.0, dtype=torch.float64, device=gpu_device)
    c = torch.full((K,), 7.0, dtype=torch.float32, device=gpu_device)
    n = torch.full((1,), 7, dtype=torch.int32, device=gpu_device)
    L = torch.full((_ld(P),), 7.0, dtype=torch.float32, device=gpu_device)
    out = torch.full((_ld(P),), 7.0, dtype=torch.float32, device=gpu_device)
    ws = torch.full((K,), 7.0, dtype=torch.float64, device=gpu_device)
    st = torch.cuda.Stream(device=1).cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731
    for name, args in (("fgm_start", (p(q), 1, K, p(w), p(c), p(n), st)),
                       ("fgm_weights", (p(q), K, NU, p(w), p(c), p(obj), p(n), st)),
                       ("fgm_gram_dist2", (p(q), K, p(w), p(q), p(ws), K * 8, st)),
                       ("fgm_finish", (p(L), p(L), p(n), P, p(out), None, st))):
        with pytest.raises(FedAggError, match=f"{name}.*stream belongs to device 1"):
            ng.call(name, *args)
    torch.cuda.synchronize()
    for t in (q, w, obj, c, L, out, ws):
        assert (t.cpu().numpy() == 7.0).all()
    assert int(n.cpu()[0]) == 7


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
    """K = 300 (two ragged chunks and j blocks, a ragged row of the 64-lane sum), P = 301 (a ragged float4): every
    output sits between guards and ends exactly at the extent include/fedgeomed.h declares — ceil(K / 256) * K doubles
    of workspace, K doubles of w and q, K floats of c, one count, one objective, P floats of out and mirror."""
    from fedscale_amd import _native_geomed as ng
    from fedscale_amd.kernels import _stream

    K, P = 300, 301
    ld = _ld(P)
    rng = np.random.default_rng(9)
    g = gf.symmetric(rng, K, integer=False)
    gd = torch.from_numpy(g.reshape(-1).copy()).to(gpu_device)
    st = _stream(gd)
    need = int(ng.call("fgm_dist2_workspace_bytes", K))
    assert need == 2 * K * 8
    g_ws, g_w, g_q = _Guarded(gpu_device, need), _Guarded(gpu_device, K * 8), _Guarded(gpu_device, K * 8)
    g_c, g_n, g_obj = _Guarded(gpu_device, K * 4), _Guarded(gpu_device, 16), _Guarded(gpu_device, 16)
    g_out, g_mir = _Guarded(gpu_device, P * 4 + (-P * 4) % 16), _Guarded(gpu_device, P * 4 + (-P * 4) % 16)
    ng.call("fgm_start", gd.data_ptr(), K + 1, K, g_w.ptr, g_c.ptr, g_n.ptr, st)
    torch.cuda.synchronize()
    w0, c0, n0 = gf.start_of(np.diag(g))
    _same64(g_w.check("w (start)", F64), w0, "start w")
    assert np.array_equal(_bits32(g_c.check("c (start)", F32)), _bits32(c0))
    assert g_n.check("n_valid (start)", np.int32)[0] == n0 == K
    ng.call("fgm_gram_dist2", gd.data_ptr(), K, g_w.ptr, g_q.ptr, g_ws.ptr, need, st)
    ng.call("fgm_weights", g_q.ptr, K, NU, g_w.ptr, g_c.ptr, g_obj.ptr, g_n.ptr, st)
    chain = torch.ones(ld, dtype=torch.float32, device=gpu_device)
    L = np.full(ld, np.nan, dtype=F32)
    L[:P] = rng.standard_normal(P).astype(F32)
    Ld = torch.from_numpy(L).to(gpu_device)
    ng.call("fgm_finish", chain.data_ptr(), Ld.data_ptr(), g_n.ptr, P, g_out.ptr, g_mir.ptr, st)
    torch.cuda.synchronize()
    g_ws.check("workspace", F64)
    q1 = gf.gram_dist2_of(g, w0)
    w1, c1, obj1, n1 = gf.weights_of(q1, NU)
    _same64(g_q.check("q_out", F64), q1, "q")
    _same64(g_w.check("w", F64), w1, "w")
    assert np.array_equal(_bits32(g_c.check("c", F32)), _bits32(c1))
    cnt, ob = g_n.check("n_valid", np.int32), g_obj.check("obj_out", F64)
    assert cnt[0] == n1 == K and (cnt[1:].view(np.uint32) == 0xA5A5A5A5).all()
    assert _bits64(ob[:1])[0] == _bits64([obj1])[0] and ob[1:].view(np.uint64)[0] == 0xA5A5A5A5A5A5A5A5
    fin = gf.finish_of(np.ones(P, dtype=F32), L[:P], K)
    for name, gdd in (("out", g_out), ("mirror", g_mir)):
        got = gdd.check(name, F32)
        assert np.array_equal(_bits32(got[:P]), _bits32(fin)), name
        assert (got[P:].view(np.uint32) == 0xA5A5A5A5).all(), (name, "columns >= P are not written")
    assert np.array_equal(_bits64(gd.cpu().numpy()), _bits64(g.reshape(-1)))  # the matrix was only read
