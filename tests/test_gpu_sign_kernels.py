"""fsg_reduce and fsg_sign_row on the MI355X against the numpy restatement of the contract (tests/sign_fixtures.py),
bit for bit: every byte value at every byte position of a lane's load under scales of every kind, the order and the
continuation of the chain at widths around every block, strip, tile and level seam, what lies outside the declared
extents, the operands the ABI refuses, and the encoder on the contract's edge cases."""
import numpy as np
import pytest
import torch

from tests import sign_fixtures as sg

pytestmark = pytest.mark.gpu

U = sg.U  # rows the kernel keeps in flight: the row loop's unrolled body, then its tail
KS = (1, U - 1, U, U + 1, 2 * U + 1)
SMALL_P = (1, 31, 32, 33, 255, 256, 257, sg.STRIP - 1, sg.STRIP, sg.STRIP + 1)
_ROWS = {}
F32 = np.float32


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _stage(rows, P, dev, extra_rows=0):
    """Device (bits [n + extra, ldb + 16], scales [n + extra, lds + 4]) of the rows; everything a reduction must never
    count — the last byte's bits past P, bytes in [ceil(P / 8), stride), scales past ceil(P / 256), rows >= n — is
    0xFF bits (every sign set) and NaN scales."""
    n, PB, NB = len(rows), sg.bit_bytes(P), sg.blocks(P)
    b = np.full((n + extra_rows, sg.bit_stride(P) + 16), 0xFF, dtype=np.uint8)
    s = np.full((n + extra_rows, sg.scale_stride(P) + 4), np.nan, dtype=F32)
    for k, (bits, sc) in enumerate(rows):
        b[k, :PB] = bits
        if P % 8:
            b[k, PB - 1] |= np.uint8((0xFF << (P % 8)) & 0xFF)
        s[k, :NB] = sc
    return torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev)


def _rows(K, P):
    """The shared rows of (K, P), made once; the tests leave them unchanged."""
    if (K, P) not in _ROWS:
        _ROWS[(K, P)] = sg.random_rows(np.random.default_rng(1000 * K + P % 9973), K, P)
    return _ROWS[(K, P)]


def _ld(P):
    return (P + 3) // 4 * 4 + 64


# ---- dequantisation: every byte value at every byte position, under every kind of scale ------------------------------
def test_every_byte_value_stands_at_every_byte_position_of_a_lanes_load(gpu_device):
    """One row of 1024 dwords (128 blocks), n = 1: dword 256 b + v holds the byte value v at byte position b and random
    bytes elsewhere.  Eight calls rotate the scales over the blocks: a subnormal, FLT_MAX, -0.0, a NaN, +0.0, a
    negative value (its columns' signs are flipped), the smallest subnormal and an ordinary one.  Bit-equal to the
    sign flip of the scale; NaN exactly where the scale is."""
    from fedscale_amd import kernels_sign as kg

    dev = gpu_device
    rng = np.random.default_rng(77)
    words = rng.integers(0, 256, (4, 256, 4)).astype(np.uint8)
    for b in range(4):
        words[b, :, b] = np.arange(256)
    bits = words.reshape(-1)
    P = bits.size * 8
    kinds = np.asarray([2.0 ** -140, np.finfo(F32).max, -0.0, np.nan, 0.0, -2.5, 2.0 ** -149, 1.5], dtype=F32)
    tb = torch.from_numpy(bits.reshape(1, -1)).to(dev)
    for rot in range(8):
        sc = np.roll(np.tile(kinds, sg.blocks(P) // 8), rot)
        want = sg.dequantize(bits, sc, P)
        assert np.isnan(want).sum() == P // 8
        out = torch.full((P,), 7.0, dtype=torch.float32, device=dev)
        kg.reduce_sign(tb, torch.from_numpy(sc.reshape(1, -1)).to(dev), 1, P, out)
        # the chain starts from +0: +0 + deq (a -0 becomes +0; every other value is unchanged)
        with np.errstate(invalid="ignore"):
            sg.same(out.cpu().numpy(), (np.zeros(P, dtype=F32) + want).astype(F32), rot)
        # ... and from -0, which keeps a -0: the dequantised bits themselves
        acc = torch.full((P,), -0.0, dtype=torch.float32, device=dev)
        kg.reduce_sign(tb, torch.from_numpy(sc.reshape(1, -1)).to(dev), 1, P, acc, acc_in=acc)
        sg.same(acc.cpu().numpy(), want, (rot, "-0"))


# ---- the chain -------------------------------------------------------------------------------------------------------
def _check_chain(dev, K, P, chunks=()):
    from fedscale_amd import kernels_sign as kg

    rows = _rows(K, P)
    want = sg.chain(rows, P=P)
    b, s = _stage(rows, P, dev, extra_rows=2)
    out = torch.full((_ld(P),), 7.0, dtype=torch.float32, device=dev)
    kg.reduce_sign(b, s, K, P, out)
    got = out.cpu().numpy()
    sg.same(got[:P], want, (K, P))
    assert (got[P:] == 7.0).all(), (K, P)  # out is written in [0, P) only
    for chunk in chunks:
        acc = torch.zeros(_ld(P), dtype=torch.float32, device=dev)
        other = torch.zeros(_ld(P), dtype=torch.float32, device=dev)
        k0 = 0
        while k0 < K:
            n = min(chunk, K - k0)
            if k0 == 0:
                kg.reduce_sign(b[k0:], s[k0:], n, P, acc)
            elif (k0 // chunk) % 2:  # out aliases acc_in ...
                kg.reduce_sign(b[k0:], s[k0:], n, P, acc, acc_in=acc)
            else:  # ... or does not
                kg.reduce_sign(b[k0:], s[k0:], n, P, other, acc_in=acc)
                acc, other = other, acc
            k0 += n
        sg.same(acc.cpu().numpy()[:P], want, (K, P, chunk))
    return rows, b, s


@pytest.mark.parametrize("K", KS)
def test_chain_order_continuation_and_aliasing(gpu_device, K):
    """Bit-equal to the restatement at K around the kernel's rows in flight; a call split into chunks with
    FA_ACCUMULATE equals the one-shot call; out aliasing acc_in equals the non-aliased call; n == 0 with FA_ACCUMULATE
    copies the chain; rows >= n, bits past P and scales past ceil(P / 256) — all set, all NaN — change nothing."""
    from fedscale_amd import kernels_sign as kg

    dev = gpu_device
    for P in SMALL_P + (sg.STRIP * sg.WAVES * 2 + 5,):
        rows, b, s = _check_chain(dev, K, P, chunks=sorted({1, 2, max(1, K - 1)}))
        # continuing a chain that is not +0: the restatement's chain over acc
        start = (np.random.default_rng(P).standard_normal(P) * 1e-3).astype(F32)
        acc = torch.zeros(_ld(P), dtype=torch.float32, device=dev)
        acc[:P] = torch.from_numpy(start).to(dev)
        kg.reduce_sign(b, s, K, P, acc, acc_in=acc)
        sg.same(acc.cpu().numpy()[:P], sg.chain(rows, acc=start, P=P), (K, P, "acc"))
        # n == 0 with FA_ACCUMULATE: out <- acc_in, aliased or not
        src = torch.full((_ld(P),), 3.0, dtype=torch.float32, device=dev)
        src[:P] = torch.from_numpy(start).to(dev)
        dst = torch.full((_ld(P),), 7.0, dtype=torch.float32, device=dev)
        kg.reduce_sign(None, None, 0, P, dst, acc_in=src)
        kg.reduce_sign(None, None, 0, P, src, acc_in=src)
        g = dst.cpu().numpy()
        sg.same(g[:P], start, (P, "n=0"))
        assert (g[P:] == 7.0).all() and torch.equal(src[:P], dst[:P]) and bool((src[P:] == 3.0).all())


def test_level_and_tile_seams_of_the_plans(gpu_device):
    """K = U + 1 at one column short of, at, and one column past every seam fsg_reduce_plan reports for the two-level
    and the level-0 plans of this GPU, a capped grid among them (the restated plan equals the library's:
    tests/test_sign_plan.py)."""
    from fedscale_amd import kernels_sign as kg

    dev, cus, K = gpu_device, _cus(), U + 1
    n1 = (cus + 1) // 2
    span0, span1 = (sg.WAVES * v for v, _ in sg.LEVELS[:2])
    cap = max(1, cus * sg.CAP_PCT // 100)
    t0 = (cap * 85 + 99) // 100
    two_levels = (span1 * n1 + 1) * sg.STRIP + 77
    level0 = (span0 * t0 - 3) * sg.STRIP - 5
    capped = span0 * cap * sg.STRIP + 1
    plan2 = kg.reduce_sign_plan(cus, K, two_levels)
    assert plan2 == sg.plan(cus, K, two_levels) and len(plan2) == 2 and plan2[1]["col0"] == span1 * n1 * sg.STRIP
    (l0,) = kg.reduce_sign_plan(cus, K, level0)
    assert l0["grid"] == l0["tiles"] == t0
    (lc,) = kg.reduce_sign_plan(cus, K, capped)
    assert lc["grid"] < lc["tiles"]
    widths = set(sg.seam_widths(plan2, two_levels)) | {two_levels}
    for P in sorted(widths):
        _check_chain(dev, K, P)
    for P in (level0, capped - 2, capped - 1, capped):  # the long rows: three rows keep the restatement quick
        _check_chain(dev, 3, P)


# ---- bounds -----------------------------------------------------------------------------------------------------------
GUARD = 256


def test_out_is_written_inside_its_declared_extent_only(gpu_device):
    """Guard bands of 0xA5 around out (P floats exactly) are intact after the call, at widths with a partial float4
    column, a partial byte, a partial dword and a partial block."""
    from fedscale_amd import _native_sign as ns

    dev, K = gpu_device, 5
    lib = ns.load()
    st = torch.cuda.current_stream().cuda_stream
    for P in (1, 7, 33, 255, 257, 2047, 2049, 8195):
        rows = _rows(K, P)
        b, s = _stage(rows, P, dev, extra_rows=1)
        buf = torch.full((GUARD + 4 * P + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        ptr = buf.data_ptr() + GUARD
        assert ptr % 16 == 0
        rc = lib.fsg_reduce(b.data_ptr(), s.data_ptr(), b.shape[1], s.shape[1], K, P, None, ptr, 0, st)
        assert rc == 0, lib.fa_last_error_string().decode()
        g = buf.cpu().numpy()
        assert (g[:GUARD] == 0xA5).all() and (g[GUARD + 4 * P:] == 0xA5).all(), P
        sg.same(g[GUARD:GUARD + 4 * P].copy().view(F32), sg.chain(rows, P=P), P)


# ---- operands ---------------------------------------------------------------------------------------------------------
def test_operands_are_checked_before_anything_is_queued(gpu_device):
    from fedscale_amd import _native_sign as ns

    lib = ns.load()
    dev = gpu_device
    n, P = 4, 1000
    LDB, LDS = sg.bit_stride(P), sg.scale_stride(P)
    b = torch.zeros(n * LDB + 64, dtype=torch.uint8, device=dev)
    s = torch.full((n * LDS + 64,), 1.5, dtype=torch.float32, device=dev)
    out = torch.full((1024,), 7.0, device=dev)
    acc = torch.zeros(1024, device=dev)
    x = torch.zeros(1024, device=dev)
    res = torch.full((1024,), 9.0, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    pageable = np.zeros(1 << 16, dtype=np.uint8)
    pinned = torch.zeros(1 << 16, dtype=torch.uint8).pin_memory()
    err = lambda: lib.fa_last_error_string().decode()  # noqa: E731

    def reduce(bp=b.data_ptr(), sp=s.data_ptr(), ldb=LDB, lds=LDS, rows=n, p=P, ap=None, op=out.data_ptr(), flags=0,
               stream=st):
        return lib.fsg_reduce(bp, sp, ldb, lds, rows, p, ap, op, flags, stream), err()

    def sign(xp=x.data_ptr(), lp=None, rp=None, p=P, bp=b.data_ptr(), sp=s.data_ptr(), op=None):
        return lib.fsg_sign_row(xp, lp, rp, p, bp, sp, op, st), err()

    refused = [
        (reduce(bp=b.data_ptr() + 8), "fsg_reduce", "bits"),
        (reduce(sp=s.data_ptr() + 4), "fsg_reduce", "scales"),
        (reduce(op=out.data_ptr() + 4), "fsg_reduce", "out"),
        (reduce(ap=acc.data_ptr() + 8, flags=1), "fsg_reduce", "acc_in"),
        (reduce(ldb=112), "fsg_reduce", "ldb=112 < ceil(P / 8)=125"),
        (reduce(ldb=LDB + 8), "fsg_reduce", "multiple of 16"),
        (reduce(lds=3), "fsg_reduce", "lds=3"),
        (reduce(rows=-1), "fsg_reduce", "negative"),
        (reduce(p=-1), "fsg_reduce", "negative"),
        (reduce(bp=None), "fsg_reduce", "bits or scales is NULL"),
        (reduce(sp=None), "fsg_reduce", "bits or scales is NULL"),
        (reduce(op=None), "fsg_reduce", "out is NULL"),
        (reduce(bp=pageable.ctypes.data), "fsg_reduce", "bits is pageable"),
        (reduce(bp=pinned.data_ptr()), "fsg_reduce", "bits is pinned host memory"),
        (reduce(sp=pageable.ctypes.data), "fsg_reduce", "scales is pageable"),
        (reduce(op=pageable.ctypes.data), "fsg_reduce", "out is pageable"),
        (reduce(ap=pageable.ctypes.data, flags=1), "fsg_reduce", "acc_in is pageable"),
        (reduce(flags=1), "fsg_reduce", "acc_in"),
        (reduce(rows=0), "fsg_reduce", "n=0"),
        (reduce(flags=2), "fsg_reduce", "flags"),
        (sign(p=-1), "fsg_sign_row", "negative"),
        (sign(xp=None), "fsg_sign_row", "NULL"),
        (sign(bp=b.data_ptr() + 8), "fsg_sign_row", "16-byte aligned"),
        (sign(xp=x.data_ptr() + 2), "fsg_sign_row", "4-byte aligned"),
        (sign(xp=pageable.ctypes.data), "fsg_sign_row", "x is pageable"),
        (sign(lp=pageable.ctypes.data), "fsg_sign_row", "base is pageable"),
        (sign(rp=pageable.ctypes.data), "fsg_sign_row", "residual is pageable"),
        (sign(bp=pageable.ctypes.data), "fsg_sign_row", "bits is pageable"),
        (sign(sp=pinned.data_ptr()), "fsg_sign_row", "scales is pinned host memory"),
        (sign(op=pageable.ctypes.data), "fsg_sign_row", "residual_out is pageable"),
        (sign(op=res.data_ptr() + 2), "fsg_sign_row", "4-byte aligned"),
    ]
    for (rc, msg), entry, word in refused:
        assert rc == -1 and entry in msg and word in msg and "nothing was launched" in msg, (rc, msg, entry, word)
    if torch.cuda.device_count() > 1:  # a stream of another GPU than the output's
        other = torch.cuda.Stream(device=1)
        rc, msg = reduce(stream=other.cuda_stream)
        assert rc == -1 and "fsg_reduce" in msg and "stream belongs to device 1" in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((b == 0).all()) and bool((s == 1.5).all()) and bool((res == 9.0).all())


# ---- the encoder ------------------------------------------------------------------------------------------------------
def test_sign_row_equals_the_restatement_on_the_contracts_cases(gpu_device):
    """fsg_sign_row with and without base, with and without a residual, and with residual_out aliasing residual, byte
    for byte: bits (the padding bits of the last block 0), scales and residual_out; nothing past the extents."""
    from fedscale_amd import kernels_sign as kg

    dev = gpu_device
    cases = sg.contract_cases()
    rng = np.random.default_rng(11)
    x0 = rng.standard_normal(4099).astype(F32)
    cases["real_base"] = x0
    for name, x in cases.items():
        P, NB = x.size, sg.blocks(x.size)
        base0 = (x0 + rng.standard_normal(4099).astype(F32) * F32(1e-3)).astype(F32) if name == "real_base" else None
        res0 = (rng.standard_normal(P) * 0.3 * float(np.nanmedian(np.abs(x)) + 1e-30)).astype(F32)
        if name in ("nan_block_between_finite_blocks", "inf_block"):
            res0[:] = 0.25
        for base in ([base0] if base0 is not None else [None, np.zeros_like(x)]):
            for res, alias in ((None, False), (res0, False), (res0, True)):
                want_b, want_s, want_r = sg.encode_fast(sg.delta(x, base, res))
                tx = torch.from_numpy(x).to(dev)
                tb = None if base is None else torch.from_numpy(base).to(dev)
                tr = None if res is None else torch.from_numpy(res).to(dev)
                bits = torch.full((NB * 32 + 32,), 0xA5, dtype=torch.uint8, device=dev)
                sc = torch.full((NB + 16,), 5.0, dtype=torch.float32, device=dev)
                ro = tr if alias else torch.full((P + 16,), 5.0, dtype=torch.float32, device=dev)
                kg.sign_row(tx, tb, tr, P, bits, sc, ro)
                gb, gs, gr = bits.cpu().numpy(), sc.cpu().numpy(), ro.cpu().numpy()
                ctx = (name, base is not None, res is not None, alias)
                assert np.array_equal(gb[:sg.bit_bytes(P)], want_b), ctx
                assert not gb[sg.bit_bytes(P):NB * 32].any(), ctx  # padding bits of the last block
                assert np.array_equal(gs[:NB].view(np.uint32), want_s.view(np.uint32)), ctx
                assert np.array_equal(gr[:P].view(np.uint32), want_r.view(np.uint32)), ctx
                assert (gb[NB * 32:] == 0xA5).all() and (gs[NB:] == 5.0).all(), ctx  # nothing past the extents
                if not alias:
                    assert (gr[P:] == 5.0).all(), ctx
                    if res is not None:
                        assert np.array_equal(tr.cpu().numpy().view(np.uint32), res.view(np.uint32)), ctx
                kg.sign_row(tx, tb, torch.from_numpy(res).to(dev) if res is not None else None, P, bits, sc, None)
                assert np.array_equal(bits.cpu().numpy()[:sg.bit_bytes(P)], want_b), ctx  # residual_out NULL


def test_device_and_host_paths_of_compress_sign_agree(gpu_device):
    from collections import OrderedDict

    from fedscale_amd.cloud.execution.sign_upload import BITS_KEY, SCALES_KEY, compress_sign

    dev = gpu_device
    torch.manual_seed(4)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                              torch.nn.Linear(4 * 26 * 26, 10))
    base = OrderedDict((k, v.clone()) for k, v in net.state_dict().items())
    sd = OrderedDict((k, v + 0.01 * torch.randn_like(v) if v.dtype == torch.float32 else v + 5)
                     for k, v in base.items())
    sd["3.bias"][2] = float("nan")  # a NaN block
    P = sum(v.numel() for v in sd.values() if v.dtype == torch.float32)
    r_host = None
    r_dev = None
    for rnd in range(2):  # the second round feeds the first one's residual back, on each side
        host, r_host = compress_sign(sd, list(base.values()), residual=r_host, residual_out=True)
        on_dev, r_dev = compress_sign(OrderedDict((k, v.to(dev)) for k, v in sd.items()), list(base.values()),
                                      residual=r_dev, residual_out=True)
        assert list(host) == list(on_dev) and list(host)[-2:] == [BITS_KEY, SCALES_KEY]
        for k in host:
            assert host[k].dtype == on_dev[k].dtype and host[k].shape == on_dev[k].shape, k
            assert np.array_equal(host[k].view(np.uint8) if k == SCALES_KEY else host[k],
                                  on_dev[k].view(np.uint8) if k == SCALES_KEY else on_dev[k]), k
        assert np.isnan(host[SCALES_KEY]).sum() == 1
        assert r_dev.is_cuda and r_dev.shape == (P,) and r_host.shape == (P,)
        assert np.array_equal(r_dev.cpu().numpy().view(np.uint32), r_host.view(np.uint32))
