"""fsa_mask_sum, fsa_reduce, fsa_encode_row and fsa_finish on the MI355X against the numpy restatement of the contract
(tests/secagg_fixtures.py), bit for bit: the mask stream's known answers, widths around every block, tile and sweep
seam, key counts around the wave width with both signs, wrap-around mod 2^32, aliasing, what lies outside the declared
extents, and the operands the ABI refuses."""
import numpy as np
import pytest
import torch

from tests import secagg_fixtures as sf

pytestmark = pytest.mark.gpu

NONCE = (0x1234, 0xFFFFFFFF, 7)
GUARD = 64  # words of 0xA5A5A5A5 on either side of every output
_A5 = np.uint32(0xA5A5A5A5)
_STREAMS = {}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev32(a, dev):
    """A uint32 numpy array as the int32 device tensor of the same bits."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(dev)


def _host32(t):
    return t.cpu().numpy().view(np.uint32)


def _guarded(P, dev):
    """(buffer, the 16-byte aligned view of P words inside it): guard words all around."""
    buf = torch.from_numpy(np.full(GUARD + P + GUARD, _A5, dtype=np.uint32).view(np.int32)).to(dev)
    view = buf[GUARD:GUARD + P]
    assert view.data_ptr() % 16 == 0
    return buf, view


def _guards_intact(buf, P):
    b = _host32(buf)
    return bool((b[:GUARD] == _A5).all() and (b[GUARD + P:] == _A5).all())


def _keys(M, seed=5):
    return np.asarray(sf.make_keys(np.random.default_rng(seed), M), dtype=np.uint32).reshape(M, 8)


def _streams(M, P):
    """uint32 [M, P]: the keystreams of _keys(M) under NONCE over columns [0, P), made once and left unchanged."""
    have = _STREAMS.get(M)
    if have is None or have.shape[1] < P:
        have = _STREAMS[M] = sf.streams(_keys(M), NONCE, 0, P)
    return have[:, :P]


def _want(acc, M, n_add, P):
    s = _streams(M, P).astype(np.uint64)
    tot = acc.astype(np.uint64) + s[:n_add].sum(axis=0) - s[n_add:].sum(axis=0)
    return (tot & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# ---- fsa_mask_sum -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kat", sf.KATS, ids=["rfc8439-2.3.2", "zero-key", "counter-crosses-2^31"])
def test_mask_stream_known_answers(gpu_device, kat):
    from fedscale_amd import kernels_secagg as ks

    dev, P = gpu_device, kat["P"]
    keys = _dev32(np.asarray(kat["key"], dtype=np.uint32).reshape(1, 8), dev)
    zero = torch.zeros(P, dtype=torch.int32, device=dev)
    buf, out = _guarded(P, dev)
    ks.mask_sum(keys, 1, 0, kat["nonce"], P, zero, out, col0=kat["col0"])
    assert np.array_equal(_host32(out)[kat["lo"]:], sf.kat_words(kat)) and _guards_intact(buf, P)
    ks.mask_sum(keys, 0, 1, kat["nonce"], P, out, out, col0=kat["col0"])  # subtracting it again: zero, in place
    assert not _host32(out).any()


def test_mask_sum_widths_around_every_block_tile_and_sweep_seam(gpu_device):
    """Three keys (+, +, -) over an accumulator of 0xFFFFFFFF words, so every sum wraps; widths around a block of 16,
    a strip of 1024, one workgroup's tile and the whole grid's first sweep."""
    from fedscale_amd import _native_secagg as ns
    from fedscale_amd import kernels_secagg as ks

    dev = gpu_device
    sweep = _cus() * ns.MASK_GRID_PER_CU * ns.MASK_TILE
    widths = (1, 15, 16, 17, 1023, 1024, 1025, ns.MASK_TILE + 1, 2 * ns.MASK_TILE + 17, sweep + 1)
    for P in widths:
        M, n_add = (3, 2) if P < 1 << 20 else (1, 1)  # (the sweep's width: one key keeps the restatement quick)
        keys = _dev32(_keys(M), dev)
        acc = np.full(P, 0xFFFFFFFF, dtype=np.uint32)
        acc[::3] = np.arange(0, P, 3, dtype=np.uint32)
        buf, out = _guarded(P, dev)
        ks.mask_sum(keys, n_add, M - n_add, NONCE, P, _dev32(acc, dev), out)
        assert np.array_equal(_host32(out), _want(acc, M, n_add, P)), P
        assert _guards_intact(buf, P), P


@pytest.mark.parametrize("M", [0, 1, 2, 63, 64, 65, 1000])
def test_mask_sum_key_counts_with_both_signs_and_aliasing(gpu_device, M):
    from fedscale_amd import kernels_secagg as ks

    dev, P = gpu_device, 4097
    rng = np.random.default_rng(M)
    acc = rng.integers(0, 1 << 32, P, dtype=np.uint64).astype(np.uint32)
    keys = _dev32(_keys(M), dev) if M else None
    for n_add in sorted({0, M // 3, M}):
        want = _want(acc, M, n_add, P)
        buf, out = _guarded(P, dev)
        ks.mask_sum(keys, n_add, M - n_add, NONCE, P, _dev32(acc, dev), out)
        assert np.array_equal(_host32(out), want) and _guards_intact(buf, P), (M, n_add)
        buf, io = _guarded(P, dev)  # out aliasing acc_in
        io.copy_(_dev32(acc, dev))
        ks.mask_sum(keys, n_add, M - n_add, NONCE, P, io, io)
        assert np.array_equal(_host32(io), want) and _guards_intact(buf, P), (M, n_add)


# ---- fsa_reduce -------------------------------------------------------------------------------------------------------
def _stage(rows, P, dev, extra_rows=1):
    """Device [n + extra, ld] of the rows; words in [P, ld) and the rows >= n are garbage a sum must never count."""
    n, ld = len(rows), (P + 63) // 64 * 64 + 64
    y = np.full((n + extra_rows, ld), 0xDEADBEEF, dtype=np.uint32)
    y[:n, :P] = rows
    return _dev32(y, dev)


def _rows(rng, n, P):
    rows = rng.integers(0, 1 << 32, (n, P), dtype=np.uint64).astype(np.uint32)
    rows[:, ::5] = 0xFFFFFFFF  # every fifth column wraps n - 1 times
    return rows


@pytest.mark.parametrize("n", [1, 2, 3, 33])
def test_reduce_sums_mod_2_32_with_continuation_and_aliasing(gpu_device, n):
    from fedscale_amd import kernels_secagg as ks

    dev = gpu_device
    rng = np.random.default_rng(100 + n)
    for P in (1, 3, 4, 5, 255, 256, 257, 1023, 1025, 2049):
        rows = _rows(rng, n, P)
        y = _stage(rows, P, dev)
        want = sf.reduce(rows)
        buf, out = _guarded(P, dev)
        ks.reduce32(y, n, P, out)
        assert np.array_equal(_host32(out), want) and _guards_intact(buf, P), (n, P)
        acc = np.full((P + 3) // 4 * 4, 0xFFFFFFFF, dtype=np.uint32)
        want2 = sf.reduce(rows, acc[:P])
        buf, out = _guarded(P, dev)
        ks.reduce32(y, n, P, out, acc_in=_dev32(acc, dev))  # FA_ACCUMULATE, not aliased
        assert np.array_equal(_host32(out), want2) and _guards_intact(buf, P), (n, P)
        io = _dev32(acc, dev)
        ks.reduce32(y, n, P, io, acc_in=io)  # aliased
        got = _host32(io)
        assert np.array_equal(got[:P], want2) and (got[P:] == 0xFFFFFFFF).all(), (n, P)
        ks.reduce32(None, 0, P, io, acc_in=io)  # no rows: the accumulator as it is
        assert np.array_equal(_host32(io)[:P], want2), (n, P)


def test_reduce_at_the_plans_seams(gpu_device):
    """n = 3 at one width just past each level and tile seam fsa_reduce_plan reports for the two-level and the
    level-0 plans of this GPU, a capped grid included (the restated plan equals the library's:
    tests/test_secagg_plan.py)."""
    from fedscale_amd import kernels_secagg as ks

    dev, cus, n = gpu_device, _cus(), 3
    n1 = (cus + 1) // 2
    span0, span1 = (sf.WAVES * v for v, _ in sf.LEVELS[:2])
    cap = max(1, cus * sf.CAP_PCT // 100)
    t0 = (cap * 85 + 99) // 100
    two_levels = (span1 * n1 + 3) * sf.STRIP + 77
    level0 = (span0 * t0 - 3) * sf.STRIP - 5
    capped = span0 * cap * sf.STRIP + 1
    assert [l["V"] for l in ks.reduce32_plan(cus, n, two_levels)] == [sf.LEVELS[1][0], sf.LEVELS[2][0]]
    assert [l["V"] for l in ks.reduce32_plan(cus, n, level0)] == [sf.LEVELS[0][0]]
    (l,) = ks.reduce32_plan(cus, n, capped)
    assert l["grid"] < l["tiles"]
    widths = {two_levels, level0, capped, span1 * n1 * sf.STRIP + 1}
    widths |= set(sf.seam_widths(ks.reduce32_plan(cus, n, two_levels)))
    rng = np.random.default_rng(9)
    for P in sorted(widths):
        rows = _rows(rng, n, P)
        buf, out = _guarded(P, dev)
        ks.reduce32(_stage(rows, P, dev), n, P, out)
        assert np.array_equal(_host32(out), sf.reduce(rows)) and _guards_intact(buf, P), P


# ---- fsa_encode_row ---------------------------------------------------------------------------------------------------
def test_encode_row_on_the_crafted_values_and_at_partial_widths(gpu_device):
    from fedscale_amd import kernels_secagg as ks

    dev = gpu_device
    x, base, q, n_clamped, n_nan = sf.crafted_encode_case()
    for xs, bs in ((x, base), (np.tile(x, 50)[:1023], np.tile(base, 50)[:1023])):
        P = xs.size
        want, cl, nn = sf.encode(xs, bs, 16, 20)
        buf, out = _guarded(P, dev)
        stats = torch.full((2,), -1, dtype=torch.int64, device=dev)
        ks.encode_row(torch.from_numpy(xs).to(dev), torch.from_numpy(bs).to(dev), P, 16, 20, out, stats)
        assert np.array_equal(_host32(out), want) and _guards_intact(buf, P), P
        assert stats.tolist() == [cl, nn] and cl > 0 and nn > 0
    assert np.array_equal(sf.encode(x, base, 16, 20)[0].view(np.int32), q)  # (the hand-written answers)
    # base = NULL encodes x itself; other specs; widths with a partial float4
    rng = np.random.default_rng(12)
    for P, f, b in ((1, 0, 1), (5, 30, 30), (4099, 10, 12), (1025, 16, 20)):
        xs = (rng.standard_normal(P) * 4).astype(np.float32)
        want, cl, nn = sf.encode(xs, np.zeros(P, np.float32), f, b)
        buf, out = _guarded(P, dev)
        stats = torch.zeros(2, dtype=torch.int64, device=dev)
        ks.encode_row(torch.from_numpy(xs).to(dev), None, P, f, b, out, stats)
        assert np.array_equal(_host32(out), want) and _guards_intact(buf, P) and stats.tolist() == [cl, nn], (P, f, b)


def test_device_and_host_paths_of_compress_secagg_agree(gpu_device):
    from collections import OrderedDict

    from fedscale_amd.cloud.execution.secagg_upload import compress_secagg, encode_update
    from fedscale_amd.secagg_round import SecAggSpec

    dev = gpu_device
    torch.manual_seed(4)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                              torch.nn.Linear(4 * 26 * 26, 3))
    base = OrderedDict((k, v.clone()) for k, v in net.state_dict().items())
    sd = OrderedDict((k, v + 0.01 * torch.randn_like(v) if v.dtype == torch.float32 else v + 5)
                     for k, v in base.items())
    sd["3.bias"][2] = float("nan")
    sd["3.bias"][1] = 1e30
    on_dev = OrderedDict((k, v.to(dev)) for k, v in sd.items())
    keys = sf.make_keys(np.random.default_rng(6), 5)
    kw = dict(self_key=keys[0], add_keys=keys[1:3], sub_keys=keys[3:], nonce=(9, 8, 7), return_stats=True)
    spec = SecAggSpec(14, 18)
    host, hstats = compress_secagg(sd, list(base.values()), spec, **kw)
    devd, dstats = compress_secagg(on_dev, list(base.values()), spec, **kw)
    assert hstats == dstats == (1, 1) and list(host) == list(devd) == list(sd)
    for k in host:
        assert host[k].dtype == devd[k].dtype and host[k].shape == devd[k].shape, k
        assert np.array_equal(host[k], devd[k]), k
    h, hs = encode_update(sd, base, spec)
    d, ds = encode_update(on_dev, base, spec)
    assert hs == ds == (1, 1) and all(np.array_equal(h[k], d[k]) for k in h)


# ---- fsa_finish -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 7])
def test_finish_on_the_crafted_sums_with_mirror_and_counter(gpu_device, n):
    from fedscale_amd import kernels_secagg as ks

    dev = gpu_device
    crafted, _ = sf.crafted_finish_case(n)
    rng = np.random.default_rng(n)
    for P in (crafted.size, 5, 1023, 4099):
        total = np.resize(crafted, (P + 3) // 4 * 4)
        last = rng.standard_normal(total.size).astype(np.float32)
        want, bad = sf.finish(total[:P], last[:P], 16, 20, n)
        assert bad > 0
        buf = torch.from_numpy(np.full(GUARD + P + GUARD, _A5, dtype=np.uint32).view(np.float32).copy()).to(dev)
        out = buf[GUARD:GUARD + P]
        mirror = torch.from_numpy(np.full(P + 8, _A5, dtype=np.uint32).view(np.float32).copy()).pin_memory()
        oor = torch.full((1,), -5, dtype=torch.int64, device=dev)
        ks.finish(_dev32(total, dev), torch.from_numpy(last).to(dev), P, 16, 20, n, out, oor, mirror=mirror)
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[GUARD:GUARD + P], want.view(np.uint32)), (n, P)
        assert (got[:GUARD] == _A5).all() and (got[GUARD + P:] == _A5).all(), (n, P)
        m = mirror.numpy().view(np.uint32)
        assert np.array_equal(m[:P], want.view(np.uint32)) and (m[P:] == _A5).all(), (n, P)
        assert int(oor.item()) == bad, (n, P)
        dmirror = torch.zeros(P, dtype=torch.float32, device=dev)  # a device mirror, and none
        ks.finish(_dev32(total, dev), torch.from_numpy(last).to(dev), P, 16, 20, n, out, oor, mirror=dmirror)
        assert torch.equal(dmirror, out) and int(oor.item()) == bad


# ---- operands ---------------------------------------------------------------------------------------------------------
def test_operands_are_checked_before_anything_is_queued(gpu_device):
    from fedscale_amd import _native_secagg as ns

    lib = ns.load()
    dev = gpu_device
    n, LD, P = 4, 128, 100
    y = torch.zeros(n * LD + 64, dtype=torch.int32, device=dev)
    out = torch.full((LD,), 7, dtype=torch.int32, device=dev)
    acc = torch.zeros(LD, dtype=torch.int32, device=dev)
    x = torch.zeros(LD, dtype=torch.float32, device=dev)
    fout = torch.full((LD,), 7.0, dtype=torch.float32, device=dev)
    keys = torch.zeros(16, dtype=torch.int32, device=dev)
    cnt = torch.full((2,), 7, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    pageable = np.zeros(1 << 16, dtype=np.uint8)
    pinned = torch.zeros(1 << 16, dtype=torch.uint8).pin_memory()
    err = lambda: lib.fa_last_error_string().decode()  # noqa: E731

    def reduce(yp=y.data_ptr(), ld=LD, rows=n, p=P, ap=None, op=out.data_ptr(), flags=0, stream=st):
        return lib.fsa_reduce(yp, ld, rows, p, ap, op, flags, stream), err()

    def mask(kp=keys.data_ptr(), n_add=1, n_sub=1, col0=0, p=P, ap=acc.data_ptr(), op=out.data_ptr(), stream=st):
        return lib.fsa_mask_sum(kp, n_add, n_sub, 1, 2, 3, col0, p, ap, op, stream), err()

    def encode(xp=x.data_ptr(), bp=None, p=P, f=16, b=20, op=out.data_ptr(), sp=cnt.data_ptr()):
        return lib.fsa_encode_row(xp, bp, p, f, b, op, sp, st), err()

    def finish(sp=acc.data_ptr(), lp=x.data_ptr(), p=P, f=16, b=20, rows=n, op=fout.data_ptr(), mp=None,
               cp=cnt.data_ptr()):
        return lib.fsa_finish(sp, lp, p, f, b, rows, op, mp, cp, st), err()

    refused = [
        (reduce(yp=None), "fsa_reduce", "y is NULL"),
        (reduce(op=None), "fsa_reduce", "out is NULL"),
        (reduce(yp=y.data_ptr() + 8), "fsa_reduce", "y must be 16-byte aligned"),
        (reduce(op=out.data_ptr() + 4), "fsa_reduce", "out"),
        (reduce(ap=acc.data_ptr() + 8, flags=1), "fsa_reduce", "acc_in"),
        (reduce(ld=96), "fsa_reduce", "ld=96 < P=100"),
        (reduce(ld=LD + 32), "fsa_reduce", "multiple of 64"),
        (reduce(yp=pageable.ctypes.data), "fsa_reduce", "y is pageable"),
        (reduce(yp=pinned.data_ptr()), "fsa_reduce", "y is pinned host memory"),
        (reduce(op=pageable.ctypes.data), "fsa_reduce", "out is pageable"),
        (reduce(ap=pageable.ctypes.data, flags=1), "fsa_reduce", "acc_in is pageable"),
        (reduce(flags=1), "fsa_reduce", "acc_in"),
        (reduce(rows=0), "fsa_reduce", "n=0"),
        (reduce(flags=2), "fsa_reduce", "flags"),
        (mask(kp=None), "fsa_mask_sum", "keys is NULL"),
        (mask(ap=None), "fsa_mask_sum", "acc_in or out is NULL"),
        (mask(op=None), "fsa_mask_sum", "acc_in or out is NULL"),
        (mask(kp=keys.data_ptr() + 2), "fsa_mask_sum", "keys must be 4-byte aligned"),
        (mask(ap=acc.data_ptr() + 4), "fsa_mask_sum", "16-byte aligned"),
        (mask(op=out.data_ptr() + 8), "fsa_mask_sum", "16-byte aligned"),
        (mask(ap=out.data_ptr() + 16), "fsa_mask_sum", "overlaps"),
        (mask(col0=8), "fsa_mask_sum", "col0=8 must be a multiple of 16"),
        (mask(col0=-16), "fsa_mask_sum", "col0=-16"),
        (mask(col0=(1 << 36) - 96), "fsa_mask_sum", "exceeds 2^36"),
        (mask(n_add=ns.MAX_KEYS, n_sub=1), "fsa_mask_sum", "FSA_MAX_KEYS"),
        (mask(n_add=-1), "fsa_mask_sum", "negative"),
        (mask(kp=pageable.ctypes.data), "fsa_mask_sum", "keys is pageable"),
        (mask(ap=pageable.ctypes.data), "fsa_mask_sum", "acc_in is pageable"),
        (mask(op=pinned.data_ptr()), "fsa_mask_sum", "out is pinned host memory"),
        (encode(xp=None), "fsa_encode_row", "NULL"),
        (encode(sp=None), "fsa_encode_row", "stats is NULL"),
        (encode(xp=x.data_ptr() + 4), "fsa_encode_row", "aligned"),
        (encode(sp=cnt.data_ptr() + 4), "fsa_encode_row", "8-byte aligned"),
        (encode(f=31), "fsa_encode_row", "frac_bits=31"),
        (encode(b=0), "fsa_encode_row", "mag_bits=0"),
        (encode(xp=pageable.ctypes.data), "fsa_encode_row", "x is pageable"),
        (encode(bp=pageable.ctypes.data), "fsa_encode_row", "base is pageable"),
        (encode(op=pageable.ctypes.data), "fsa_encode_row", "out_u32 is pageable"),
        (encode(sp=pinned.data_ptr()), "fsa_encode_row", "pinned host memory"),
        (finish(sp=None), "fsa_finish", "NULL"),
        (finish(cp=None), "fsa_finish", "out_of_range is NULL"),
        (finish(lp=x.data_ptr() + 4), "fsa_finish", "aligned"),
        (finish(mp=fout.data_ptr() + 4), "fsa_finish", "aligned"),
        (finish(f=-1), "fsa_finish", "frac_bits=-1"),
        (finish(rows=0), "fsa_finish", "n=0"),
        (finish(rows=2049), "fsa_finish", "n=2049"),
        (finish(sp=pageable.ctypes.data), "fsa_finish", "sum is pageable"),
        (finish(op=pinned.data_ptr()), "fsa_finish", "out is pinned host memory"),
        (finish(mp=pageable.ctypes.data), "fsa_finish", "mirror is pageable"),
        (finish(cp=pinned.data_ptr()), "fsa_finish", "pinned host memory"),
    ]
    for (rc, msg), entry, word in refused:
        assert rc == -1 and entry in msg and word in msg and "nothing was launched" in msg, (rc, msg, entry, word)
    assert mask(col0=(1 << 36) - 112)[0] == 0  # the last columns of a stream are taken
    out.fill_(7)
    if torch.cuda.device_count() > 1:  # a stream of another GPU than the output's
        other = torch.cuda.Stream(device=1)
        for rc, msg in (reduce(stream=other.cuda_stream), mask(stream=other.cuda_stream)):
            assert rc == -1 and "stream belongs to device 1" in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((fout == 7.0).all()) and bool((cnt == 7).all()) and bool((y == 0).all())
