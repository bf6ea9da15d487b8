"""fs_reduce, fs_row_offsets and fs_check_rows on the MI355X against the numpy restatement of the contract
(tests/sparse_fixtures.py), bit for bit: the order and the continuation of the chain at widths around every tile
seam and on a capped grid, columns no row names, what lies outside the declared extents, the rows fs_check_rows
flags, a flagged row skipped whole, and the operands the ABI refuses.  Every row fed to fs_reduce unflagged is well
formed."""
import numpy as np
import pytest
import torch

from tests import sparse_fixtures as sf

pytestmark = pytest.mark.gpu

T = sf.TILE
KS = (5, 33)
WIDTHS = (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5)
_ROWS = {}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, ctx):
    g, w = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), ctx
    assert np.array_equal(_bits(g)[~nan], _bits(w)[~nan]), ctx


class Staged:
    """Device arrays of the rows, with everything a reduction must never count poisoned: pairs in [nnz, ldk) hold
    index 0xFFFFFFFF and a NaN, and ``extra`` rows past n hold only such pairs under a count of ldk."""

    def __init__(self, rows, P, dev, extra=0, index=True):
        from fedscale_amd import kernels_sparse as ks

        n = len(rows)
        self.n, self.P = n, P
        ldk = ks.row_stride(max([len(i) for i, _ in rows] + [1]) + 3)  # ldk > nnz always
        idx = np.full((n + extra, ldk), 0xFFFFFFFF, dtype=np.uint32)
        val = np.full((n + extra, ldk), np.nan, dtype=np.float32)
        nnz = np.full(n + extra, ldk, dtype=np.int32)
        for k, (i, v) in enumerate(rows):
            idx[k, :len(i)] = i
            val[k, :len(i)] = v
            nnz[k] = len(i)
        self.idx = torch.from_numpy(idx.view(np.int32)).to(dev)
        self.val = torch.from_numpy(val).to(dev)
        self.nnz = torch.from_numpy(nnz).to(dev)
        self.off = torch.full((ks.boundaries(P), n + extra), -7, dtype=torch.int32, device=dev)
        self.flags = torch.full((n + extra,), -7, dtype=torch.int32, device=dev)
        if index:
            ks.row_offsets(self.idx, self.nnz, n, P, self.off)
            ks.check_rows(self.idx, self.nnz, n, P, self.flags)

    def reduce(self, out, n=None, row0=0, acc_in=None):
        from fedscale_amd import kernels_sparse as ks

        return ks.reduce_sparse(self.idx, self.val, self.nnz, self.off, self.flags, self.n if n is None else n,
                                self.P, out, acc_in=acc_in, row0=row0)


def _rows(K, P):
    """The shared rows of (K, P), made once; the tests leave them unchanged.  Row 0 is empty, row 1 has one pair,
    row 2 is fully dense (small P) or sits on the first and last column of every tile, the rest are random with up to
    min(P, 4096) pairs; the last three rows hit one column with (1e8, 1, -1e8); the last row also carries a subnormal,
    a -0, an infinity and a NaN in columns of its own."""
    if (K, P) in _ROWS:
        return _ROWS[(K, P)]
    rng = np.random.default_rng(1000 * K + P % 9973)
    rows = [(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32)),
            (np.asarray([P - 1], dtype=np.uint32), np.asarray([0.75], dtype=np.float32))]
    if P <= 65:
        rows.append(sf.random_row(rng, P, P))
    else:
        nt = sf.tiles(P)  # (the first and last two tiles: all of them at the widths around a seam)
        seams = sorted({c for t in {0, 1, nt - 2, nt - 1} if 0 <= t < nt for c in (t * T, min(P, (t + 1) * T) - 1)})
        rows.append((np.asarray(seams, dtype=np.uint32), rng.standard_normal(len(seams)).astype(np.float32)))
    while len(rows) < K:
        rows.append(sf.random_row(rng, P, int(rng.integers(1, min(P, 4096) + 1))))
    rows[3] = sf.random_row(rng, P, min(P, 40))  # a short row: inside one tile when P <= T
    col = P // 2
    for k, v in zip((K - 3, K - 2, K - 1), (1e8, 1.0, -1e8)):
        i, x = rows[k]
        keep = i != col
        i, x = np.append(i[keep], np.uint32(col)), np.append(x[keep], np.float32(v))
        order = np.argsort(i, kind="stable")
        rows[k] = (i[order].astype(np.uint32), x[order].astype(np.float32))
    i, x = rows[K - 1]
    x = x.copy()
    for j, v in zip(np.flatnonzero(i != col)[:4], (1e-40, -0.0, np.inf, np.nan)):
        x[j] = np.float32(v)
    rows[K - 1] = (i, x)
    _ROWS[(K, P)] = rows
    return rows


def test_order_changes_the_sum_the_test_plants():
    """(1e8 + 1) - 1e8 is 0 in fp32 and (1e8 - 1e8) + 1 is 1: the planted column tells the orders apart."""
    f = np.float32
    assert f(f(f(0) + f(1e8)) + f(1)) + f(-1e8) == 0.0 and f(f(f(0) + f(1e8)) + f(-1e8)) + f(1) == 1.0
    c = sf.chain([(np.asarray([32], np.uint32), np.asarray([v], np.float32)) for v in (1e8, 1.0, -1e8)], 65)
    assert c[32] == 0.0


@pytest.mark.parametrize("K", KS)
def test_chain_order_continuation_and_aliasing(gpu_device, K):
    """Bit-equal to the restatement; a call split at chunk sizes 1, 2 and K - 1 with FA_ACCUMULATE equals the one-shot
    call; out aliasing acc_in equals the non-aliased call; rows >= n, pairs in [nnz, ldk) and out beyond P — all
    poisoned — change nothing."""
    dev = gpu_device
    for P in WIDTHS:
        rows = _rows(K, P)
        want = sf.chain(rows, P)
        st = Staged(rows, P, dev, extra=2)
        assert not st.flags[:K].any().item(), (K, P)
        out = torch.full((P + 68,), 7.0, dtype=torch.float32, device=dev)
        st.reduce(out)
        got = out.cpu().numpy()
        _same(got[:P], want, (K, P))
        assert (got[P:] == 7.0).all(), (K, P)  # out is written in [0, P) only
        for chunk in sorted({1, 2, K - 1}):
            acc = torch.zeros(P + 4, dtype=torch.float32, device=dev)
            other = torch.zeros(P + 4, dtype=torch.float32, device=dev)
            k0 = 0
            while k0 < K:
                n = min(chunk, K - k0)
                if k0 == 0:
                    st.reduce(acc, n=n)
                elif (k0 // chunk) % 2:  # out aliases acc_in ...
                    st.reduce(acc, n=n, row0=k0, acc_in=acc)
                else:  # ... or does not
                    st.reduce(other, n=n, row0=k0, acc_in=acc)
                    acc, other = other, acc
                k0 += n
            _same(acc.cpu().numpy()[:P], want, (K, P, chunk))
        # continuing a chain that is not +0 (every third column -0: a column no row names keeps it)
        start = (np.random.default_rng(P).standard_normal(P) * 1e-3).astype(np.float32)
        start[::3] = -0.0
        acc = torch.zeros(P + 4, dtype=torch.float32, device=dev)
        acc[:P] = torch.from_numpy(start).to(dev)
        st.reduce(acc, acc_in=acc)
        want_acc = sf.chain(rows, P, acc_in=start)
        _same(acc.cpu().numpy()[:P], want_acc, (K, P, "acc"))


def test_subnormals_and_negative_zero(gpu_device):
    """Subnormal values add exactly; -0 onto a +0 chain gives +0, onto a -0 chain -0; an unnamed column of a -0 chain
    stays -0 (no added zero)."""
    dev, P = gpu_device, 65
    u = np.uint32
    rows = [(np.asarray([3, 5, 7], u), np.asarray([-0.0, 1e-40, -1e-45], np.float32)),
            (np.asarray([5, 9], u), np.asarray([1e-40, -0.0], np.float32)),
            (np.asarray([9, 64], u), np.asarray([-0.0, 2e-45], np.float32))]
    st = Staged(rows, P, dev)
    out = torch.full((P + 3,), 7.0, dtype=torch.float32, device=dev)
    st.reduce(out)
    got = out.cpu().numpy()[:P]
    _same(got, sf.chain(rows, P), "from +0")
    assert _bits(got)[3] == 0 and _bits(got)[9] == 0 and got[5] == np.float32(1e-40) + np.float32(1e-40) != 0
    assert _bits(got)[7] == 0x80000001 and _bits(got)[64] == 1
    neg = np.full(P, -0.0, dtype=np.float32)
    acc = torch.from_numpy(np.append(neg, np.zeros(3, np.float32))).to(dev)
    st.reduce(acc, acc_in=acc)
    got = acc.cpu().numpy()[:P]
    _same(got, sf.chain(rows, P, acc_in=neg), "from -0")
    assert _bits(got)[3] == 0x80000000 and _bits(got)[9] == 0x80000000 and _bits(got)[0] == 0x80000000


def test_nan_and_inf_stay_in_their_own_columns(gpu_device):
    dev, P, K = gpu_device, 2 * T + 5, 5
    rows = _rows(K, P)
    i, x = rows[K - 1]
    bad = i[~np.isfinite(x)].astype(np.int64)
    assert bad.size == 2
    st = Staged(rows, P, dev)
    out = torch.empty(P, dtype=torch.float32, device=dev)
    st.reduce(out)
    got = out.cpu().numpy()
    mask = np.zeros(P, dtype=bool)
    mask[bad] = True
    assert np.isfinite(got[~mask]).all() and not np.isfinite(got[mask]).any()


def test_a_workgroup_walks_more_than_one_tile(gpu_device):
    """K = 5 at a width just past the grid cap of this GPU: the plan gives a workgroup two tiles; at most 4096 pairs
    per row keep the test small."""
    from fedscale_amd import kernels_sparse as ks

    dev, cus, K = gpu_device, _cus(), 5
    P = (cus * sf.WG_PER_CU + 3) * T + 5
    (l,) = ks.reduce_sparse_plan(cus, K, P)
    assert l["per"] == 2 and l["grid"] < l["tiles"]
    rows = _rows(K, P)
    assert max(len(i) for i, _ in rows) <= 4096
    last = l["tiles"] - 1  # pairs in the last tile: the second tile of its workgroup
    assert any((i.astype(np.int64) // T == last).any() for i, _ in rows)
    st = Staged(rows, P, dev)
    out = torch.full((P + 4,), 7.0, dtype=torch.float32, device=dev)
    st.reduce(out)
    got = out.cpu().numpy()
    _same(got[:P], sf.chain(rows, P), P)
    assert (got[P:] == 7.0).all()


def test_row_offsets_are_the_lower_bounds(gpu_device):
    dev, K = gpu_device, 5
    for P in (1, T, T + 1, 2 * T + 5):
        rows = _rows(K, P)
        st = Staged(rows, P, dev, extra=1)
        off = st.off.cpu().numpy()
        for k, (i, _) in enumerate(rows):
            want = np.searchsorted(i.astype(np.int64), np.arange(sf.tiles(P) + 1) * T, side="left")
            assert np.array_equal(off[:, k], want), (P, k)
        assert (off[:, K] == -7).all()  # rows >= n are not written


def test_check_rows_flags_exactly_the_malformed_rows(gpu_device):
    from fedscale_amd import kernels_sparse as ks

    dev, P = gpu_device, 3 * T
    rng = np.random.default_rng(8)
    u = np.uint32
    long_ok = np.sort(rng.choice(P, size=8200, replace=False)).astype(u)
    seam_desc = long_ok.copy()  # a descending pair across the 4096-pair seam of two checking workgroups
    seam_desc[4095], seam_desc[4096] = seam_desc[4096], seam_desc[4095]
    last_eq = long_ok.copy()
    last_eq[-1] = last_eq[-2]
    cases = [
        (np.asarray([1, 5, 9], u), 0),
        (np.asarray([1, 9, 5], u), 1),            # a descending pair
        (np.asarray([1, 5, 5, 9], u), 1),         # an equal pair
        (np.asarray([1, 5, P], u), 1),            # an index = P
        (np.asarray([0xFFFFFFFF], u), 1),         # a lone index far past P
        (np.asarray([P - 1], u), 0),
        (np.zeros(0, u), 0),                      # an empty row
        (long_ok, 0),
        (seam_desc, 1),
        (last_eq, 1),
        (np.arange(P, dtype=u)[:9000], 0),        # consecutive columns
    ]
    rows = [(i, np.ones(len(i), np.float32)) for i, _ in cases]
    st = Staged(rows, P, dev, extra=1)
    flags = st.flags.cpu().numpy()
    assert ((flags[:len(cases)] != 0).astype(int) == np.asarray([w for _, w in cases])).all(), flags
    assert flags[len(cases)] == -7  # rows >= n are not written
    # a count outside [0, ldk] is flagged too (and nothing past ldk is read)
    nnz = st.nnz.clone()
    nnz[0], nnz[5] = st.idx.shape[1] + 1, -1
    f2 = torch.zeros_like(st.flags)
    ks.check_rows(st.idx, nnz, len(cases), P, f2)
    f2 = f2.cpu().numpy()
    assert f2[0] != 0 and f2[5] != 0 and f2[6] == 0 and f2[7] == 0


def test_a_flagged_row_is_skipped_whole(gpu_device):
    """A valid row flagged by hand contributes nothing: the result is the chain without it, in one call and across a
    fold."""
    dev, K = gpu_device, 5
    for P in (65, 2 * T + 5):
        rows = _rows(K, P)
        st = Staged(rows, P, dev)
        assert not st.flags.any().item()
        st.flags[K - 2] = 1
        want = sf.chain(rows[:K - 2] + rows[K - 1:], P)
        out = torch.empty(P, dtype=torch.float32, device=dev)
        st.reduce(out)
        _same(out.cpu().numpy(), want, P)
        assert not np.array_equal(_bits(want), _bits(sf.chain(rows, P)))
        acc = torch.zeros(P + 4, dtype=torch.float32, device=dev)
        st.reduce(acc, n=2)
        st.reduce(acc, n=K - 2, row0=2, acc_in=acc)
        _same(acc.cpu().numpy()[:P], want, (P, "fold"))


def test_operands_are_checked_before_anything_is_queued(gpu_device):
    from fedscale_amd import _native_sparse as ns

    lib = ns.load()
    dev = gpu_device
    n, LDK, P = 4, 16, 100
    NB = 2
    idx = torch.zeros(n * LDK + 16, dtype=torch.int32, device=dev)
    val = torch.zeros(n * LDK + 16, dtype=torch.float32, device=dev)
    nnz = torch.zeros(n + 4, dtype=torch.int32, device=dev)
    off = torch.zeros(NB * n + 4, dtype=torch.int32, device=dev)
    rfl = torch.zeros(n + 4, dtype=torch.int32, device=dev)
    out = torch.full((128,), 7.0, device=dev)
    acc = torch.zeros(128, device=dev)
    x = torch.zeros(128, device=dev)
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    pageable = np.zeros(1 << 16, dtype=np.uint8)
    pinned = torch.zeros(1 << 16, dtype=torch.uint8).pin_memory()
    err = lambda: lib.fa_last_error_string().decode()  # noqa: E731

    def reduce(ip=idx.data_ptr(), vp=val.data_ptr(), ldk=LDK, np_=nnz.data_ptr(), fp=off.data_ptr(), ldo=n,
               rp=rfl.data_ptr(), rows=n, p=P, ap=None, op=out.data_ptr(), flags=0, stream=st):
        return lib.fs_reduce(ip, vp, ldk, np_, fp, ldo, rp, rows, p, ap, op, flags, stream), err()

    def offsets(ip=idx.data_ptr(), ldk=LDK, np_=nnz.data_ptr(), rows=n, p=P, fp=off.data_ptr(), ldo=n):
        return lib.fs_row_offsets(ip, ldk, np_, rows, p, fp, ldo, st), err()

    def check(ip=idx.data_ptr(), ldk=LDK, np_=nnz.data_ptr(), rows=n, p=P, fp=rfl.data_ptr()):
        return lib.fs_check_rows(ip, ldk, np_, rows, p, fp, st), err()

    def topk(xp=x.data_ptr(), bp=None, rp=None, p=P, k=5, wp=ws.data_ptr(), ip=idx.data_ptr(), vp=val.data_ptr(),
             op=None):
        return lib.fs_topk_row(xp, bp, rp, p, k, wp, ip, vp, op, st), err()

    refused = [
        (reduce(ip=idx.data_ptr() + 8), "fs_reduce", "idx"),
        (reduce(vp=val.data_ptr() + 4), "fs_reduce", "val"),
        (reduce(op=out.data_ptr() + 4), "fs_reduce", "out"),
        (reduce(ap=acc.data_ptr() + 8, flags=1), "fs_reduce", "acc_in"),
        (reduce(ldk=LDK + 2), "fs_reduce", "multiple of 4"),
        (reduce(ldo=n - 1), "fs_reduce", "ldo=3 < n=4"),
        (reduce(np_=pageable.ctypes.data), "fs_reduce", "nnz is pageable"),
        (reduce(ip=pageable.ctypes.data), "fs_reduce", "idx is pageable"),
        (reduce(ip=pinned.data_ptr()), "fs_reduce", "idx is pinned host memory"),
        (reduce(vp=pageable.ctypes.data), "fs_reduce", "val is pageable"),
        (reduce(rp=pageable.ctypes.data), "fs_reduce", "row_flags is pageable"),
        (reduce(op=pageable.ctypes.data), "fs_reduce", "out is pageable"),
        (reduce(ap=pageable.ctypes.data, flags=1), "fs_reduce", "acc_in is pageable"),
        (reduce(flags=1), "fs_reduce", "acc_in"),
        (reduce(rows=0), "fs_reduce", "n=0"),
        (reduce(flags=2), "fs_reduce", "flags"),
        (offsets(ip=idx.data_ptr() + 4), "fs_row_offsets", "aligned"),
        (offsets(ldo=2), "fs_row_offsets", "ldo=2 < n=4"),
        (offsets(fp=pinned.data_ptr()), "fs_row_offsets", "offsets is pinned host memory"),
        (offsets(ip=pageable.ctypes.data), "fs_row_offsets", "idx is pageable"),
        (check(fp=pageable.ctypes.data), "fs_check_rows", "flags is pageable"),
        (check(np_=pinned.data_ptr()), "fs_check_rows", "nnz is pinned host memory"),
        (topk(xp=x.data_ptr() + 4), "fs_topk_row", "aligned"),
        (topk(k=0), "fs_topk_row", "k=0"),
        (topk(xp=pageable.ctypes.data), "fs_topk_row", "x is pageable"),
        (topk(bp=pageable.ctypes.data), "fs_topk_row", "base is pageable"),
        (topk(rp=pinned.data_ptr()), "fs_topk_row", "r_in is pinned host memory"),
        (topk(op=pageable.ctypes.data), "fs_topk_row", "r_out is pageable"),
    ]
    for (rc, msg), entry, word in refused:
        assert rc == -1 and entry in msg and word in msg and "nothing was launched" in msg, (rc, msg, entry, word)
    rc, msg = reduce(p=1 << 31)
    assert rc < 0 and "fs_reduce" in msg and "2^31" in msg, msg
    if torch.cuda.device_count() > 1:  # a stream of another GPU than the output's
        other = torch.cuda.Stream(device=1)
        rc, msg = reduce(stream=other.cuda_stream)
        assert rc == -1 and "fs_reduce" in msg and "stream belongs to device 1" in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((off == 0).all()) and bool((rfl == 0).all()) and bool((idx == 0).all())
