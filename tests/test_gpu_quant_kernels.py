"""fq_reduce and fq_quantize_row on the MI355X against the numpy restatement of the contract
(tests/quant_fixtures.py), bit for bit: every code against every scale byte, the order and the continuation of the
chain at widths around every block, strip, tile and level seam, what lies outside the declared extents, the
operands the ABI refuses, and the quantiser on the contract's edge cases."""
import numpy as np
import pytest
import torch

from tests import quant_fixtures as qf

pytestmark = pytest.mark.gpu

KS = (5, 33)
SMALL_P = (1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025)
_ROWS = {}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ld(P):
    return (P + 63) // 64 * 64 + 64  # ld > P always: codes in [P, ld) hold a NaN code


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, ctx):
    g, w = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), ctx
    assert np.array_equal(_bits(g)[~nan], _bits(w)[~nan]), ctx


def _stage(rows, P, dev, extra_rows=0):
    """Device (q8 [n + extra, ld], scales [n + extra, lds]) of the rows; everything a reduction must never count —
    codes in [P, ld), scale bytes past ceil(P / 32), rows >= n — is 0x7F / 0xFF (NaN codes, the NaN scale)."""
    n, ld = len(rows), _ld(P)
    lds, NB = (ld // 32 + 15) // 16 * 16, qf.blocks(P)  # (a multiple of 16: every row's scale bytes start aligned)
    q = np.full((n + extra_rows, ld), 0x7F, dtype=np.uint8)
    s = np.full((n + extra_rows, lds), 0xFF, dtype=np.uint8)
    for k, (codes, sc) in enumerate(rows):
        q[k, :P] = codes[:P]
        s[k, :NB] = sc
    return torch.from_numpy(q).to(dev), torch.from_numpy(s).to(dev)


def _rows(K, P):
    """The shared rows of (K, P), made once; the tests leave them unchanged."""
    if (K, P) not in _ROWS:
        _ROWS[(K, P)] = qf.random_rows(np.random.default_rng(1000 * K + P % 9973), K, P)
    return _ROWS[(K, P)]


# ---- dequantisation: every code against every scale byte -----------------------------------------------------------
def test_every_code_meets_every_scale_byte(gpu_device):
    """8 rows of 256 blocks x 32 columns, n = 1, one call per row: row r, block b holds codes 32 r .. 32 r + 31 under
    scale byte b.  Bit-equal to the table product; NaN for the codes 0x7F / 0xFF and for scale 255; 247..254 follow
    the rounded product (inf where it overflows)."""
    from fedscale_amd import kernels_quant as kq

    dev = gpu_device
    P = 256 * 32
    sc = np.arange(256, dtype=np.uint8)
    for r in range(8):
        codes = np.tile(np.arange(32 * r, 32 * r + 32, dtype=np.uint8), 256)
        want = qf.dequantize(codes, sc)
        q = torch.from_numpy(codes.reshape(1, P)).to(dev)
        s = torch.from_numpy(sc.reshape(1, 256)).to(dev)
        out = torch.full((P,), 7.0, dtype=torch.float32, device=dev)
        kq.reduce8(q, s, 1, P, out)
        got = out.cpu().numpy()
        # the chain starts from +0: +0 + deq (a -0 product becomes +0; every other value is unchanged)
        _same(got, (np.zeros(P, dtype=np.float32) + want).astype(np.float32), f"row {r}")
        blk = want.reshape(256, 32)
        assert np.isnan(blk[255]).all()
        if r == 3:
            assert np.isnan(blk[:, 31]).all() and np.isinf(blk[254, 30])  # 0x7F; 448 x 2^127 overflows
        if r == 0:
            assert blk[0, 1] == np.float32(2.0 ** -136) and blk[10, 1] == np.float32(2.0 ** -126)  # subnormal fp32


# ---- the chain -------------------------------------------------------------------------------------------------------
def _widths(K):
    from fedscale_amd import kernels_quant as kq

    cus = _cus()
    out = list(SMALL_P)
    for P in (qf.STRIP * qf.WAVES * 2 + 5, ):  # a few level-2 tiles
        out.append(P)
    for P0 in (3 * qf.STRIP + 7, ):
        out += [p for p in qf.seam_widths(kq.reduce8_plan(cus, K, P0), P0) if p <= (1 << 16)]
    return sorted(set(out))


@pytest.mark.parametrize("K", KS)
def test_chain_order_continuation_and_aliasing(gpu_device, K):
    """Bit-equal to the restatement; a call split at chunk sizes 1, 2 and K - 1 with FA_ACCUMULATE equals the one-shot
    call; out aliasing acc_in equals the non-aliased call; rows >= n, codes in [P, ld) and scale bytes past
    ceil(P / 32) — all NaN — change nothing."""
    from fedscale_amd import kernels_quant as kq

    dev = gpu_device
    for P in _widths(K):
        rows = _rows(K, P)
        want = qf.chain(rows, P=P)
        q, s = _stage(rows, P, dev, extra_rows=2)
        out = torch.full((_ld(P),), 7.0, dtype=torch.float32, device=dev)
        kq.reduce8(q, s, K, P, out)
        got = out.cpu().numpy()
        _same(got[:P], want, (K, P))
        assert (got[P:] == 7.0).all(), (K, P)  # out is written in [0, P) only
        for chunk in sorted({1, 2, K - 1}):
            acc = torch.zeros(_ld(P), dtype=torch.float32, device=dev)
            other = torch.zeros(_ld(P), dtype=torch.float32, device=dev)
            k0 = 0
            while k0 < K:
                n = min(chunk, K - k0)
                if k0 == 0:
                    kq.reduce8(q[k0:], s[k0:], n, P, acc)
                elif (k0 // chunk) % 2:  # out aliases acc_in ...
                    kq.reduce8(q[k0:], s[k0:], n, P, acc, acc_in=acc)
                else:  # ... or does not
                    kq.reduce8(q[k0:], s[k0:], n, P, other, acc_in=acc)
                    acc, other = other, acc
                k0 += n
            _same(acc.cpu().numpy()[:P], want, (K, P, chunk))
        # continuing a chain that is not +0: the restatement's chain over acc
        start = (np.random.default_rng(P).standard_normal(P) * 1e-3).astype(np.float32)
        acc = torch.zeros(_ld(P), dtype=torch.float32, device=dev)
        acc[:P] = torch.from_numpy(start).to(dev)
        kq.reduce8(q, s, K, P, acc, acc_in=acc)
        _same(acc.cpu().numpy()[:P], qf.chain(rows, acc=start, P=P), (K, P, "acc"))


def test_level_and_tile_seams_of_the_wide_plans(gpu_device):
    """K = 5 at one width just past each seam fq_reduce_plan reports for the two-level and the level-0 plans of this
    GPU (the restated plan equals the library's: tests/test_quant_plan.py)."""
    from fedscale_amd import kernels_quant as kq

    dev, cus, K = gpu_device, _cus(), 5
    n1 = (cus + 1) // 2
    span0, span1 = (qf.WAVES * v for v, _ in qf.LEVELS[:2])
    cap = max(1, cus * qf.CAP_PCT // 100)
    t0 = (cap * 85 + 99) // 100
    two_levels = (span1 * n1 + 3) * qf.STRIP + 77
    level0 = (span0 * t0 - 3) * qf.STRIP - 5
    assert [l["V"] for l in kq.reduce8_plan(cus, K, two_levels)] == [4, 1]
    assert [l["V"] for l in kq.reduce8_plan(cus, K, level0)] == [8]
    widths = {two_levels, level0, span1 * n1 * qf.STRIP + 1, span0 * cap * qf.STRIP + 1}  # the last: a capped grid
    (l,) = kq.reduce8_plan(cus, K, span0 * cap * qf.STRIP + 1)
    assert l["grid"] < l["tiles"]
    for P in sorted(widths):
        rows = _rows(K, P)
        q, s = _stage(rows, P, dev)
        out = torch.empty(_ld(P), dtype=torch.float32, device=dev)
        kq.reduce8(q, s, K, P, out)
        _same(out.cpu().numpy()[:P], qf.chain(rows, P=P), P)


# ---- bounds -----------------------------------------------------------------------------------------------------------
GUARD = 256


def test_out_is_written_inside_its_declared_extent_only(gpu_device):
    """Guard bands of 0xA5 around out (P floats exactly) are intact after the call, at widths with a partial float4
    column, a partial 16-byte load and a partial block."""
    from fedscale_amd import _native_quant as nq

    dev, K = gpu_device, 5
    lib = nq.load()
    st = torch.cuda.current_stream().cuda_stream
    for P in (1, 17, 33, 1023, 1025, 4099):
        rows = _rows(K, P)
        q, s = _stage(rows, P, dev, extra_rows=1)
        buf = torch.full((GUARD + 4 * P + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        ptr = buf.data_ptr() + GUARD
        assert ptr % 16 == 0
        rc = lib.fq_reduce(q.data_ptr(), s.data_ptr(), q.shape[1], s.shape[1], K, P, None, ptr, 0, st)
        assert rc == 0, lib.fa_last_error_string().decode()
        b = buf.cpu().numpy()
        assert (b[:GUARD] == 0xA5).all() and (b[GUARD + 4 * P:] == 0xA5).all(), P
        _same(b[GUARD:GUARD + 4 * P].copy().view(np.float32), qf.chain(rows, P=P), P)


# ---- operands ---------------------------------------------------------------------------------------------------------
def test_operands_are_checked_before_anything_is_queued(gpu_device):
    from fedscale_amd import _native_quant as nq

    lib = nq.load()
    dev = gpu_device
    n, LD, P = 4, 128, 100
    LDS = LD // 32
    q = torch.zeros(n * LD + 64, dtype=torch.uint8, device=dev)
    s = torch.full((n * LDS + 64,), 127, dtype=torch.uint8, device=dev)
    out = torch.full((LD,), 7.0, device=dev)
    acc = torch.zeros(LD, device=dev)
    x = torch.zeros(LD, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    pageable = np.zeros(1 << 16, dtype=np.uint8)
    pinned = torch.zeros(1 << 16, dtype=torch.uint8).pin_memory()
    err = lambda: lib.fa_last_error_string().decode()  # noqa: E731

    def reduce(qp=q.data_ptr(), sp=s.data_ptr(), ld=LD, lds=LDS, rows=n, p=P, ap=None, op=out.data_ptr(), flags=0,
               stream=st):
        return lib.fq_reduce(qp, sp, ld, lds, rows, p, ap, op, flags, stream), err()

    def quant(xp=x.data_ptr(), bp=None, p=P, qp=q.data_ptr(), sp=s.data_ptr()):
        return lib.fq_quantize_row(xp, bp, p, qp, sp, st), err()

    refused = [
        (reduce(qp=q.data_ptr() + 8), "fq_reduce", "q8"),
        (reduce(sp=s.data_ptr() + 4), "fq_reduce", "scales"),
        (reduce(op=out.data_ptr() + 4), "fq_reduce", "out"),
        (reduce(ap=acc.data_ptr() + 8, flags=1), "fq_reduce", "acc_in"),
        (reduce(ld=96), "fq_reduce", "ld=96 < P=100"),
        (reduce(ld=LD + 32), "fq_reduce", "multiple of 64"),
        (reduce(lds=3), "fq_reduce", "lds=3"),
        (reduce(qp=pageable.ctypes.data), "fq_reduce", "q8 is pageable"),
        (reduce(qp=pinned.data_ptr()), "fq_reduce", "q8 is pinned host memory"),
        (reduce(sp=pageable.ctypes.data), "fq_reduce", "scales is pageable"),
        (reduce(op=pageable.ctypes.data), "fq_reduce", "out is pageable"),
        (reduce(ap=pageable.ctypes.data, flags=1), "fq_reduce", "acc_in is pageable"),
        (reduce(flags=1), "fq_reduce", "acc_in"),
        (reduce(rows=0), "fq_reduce", "n=0"),
        (reduce(flags=2), "fq_reduce", "flags"),
        (quant(xp=x.data_ptr() + 4), "fq_quantize_row", "aligned"),
        (quant(xp=pageable.ctypes.data), "fq_quantize_row", "x is pageable"),
        (quant(bp=pageable.ctypes.data), "fq_quantize_row", "base is pageable"),
        (quant(qp=pageable.ctypes.data), "fq_quantize_row", "q8 is pageable"),
        (quant(sp=pinned.data_ptr()), "fq_quantize_row", "scales is pinned host memory"),
    ]
    for (rc, msg), entry, word in refused:
        assert rc == -1 and entry in msg and word in msg and "nothing was launched" in msg, (rc, msg, entry, word)
    if torch.cuda.device_count() > 1:  # a stream of another GPU than the output's
        other = torch.cuda.Stream(device=1)
        rc, msg = reduce(stream=other.cuda_stream)
        assert rc == -1 and "fq_reduce" in msg and "stream belongs to device 1" in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((q == 0).all()) and bool((s == 127).all())


# ---- the quantiser ----------------------------------------------------------------------------------------------------
def test_quantize_row_equals_the_restatement_on_the_contracts_cases(gpu_device):
    """fq_quantize_row with base (x - base is the case's delta exactly: base = +0) and with NULL, byte for byte;
    scale bytes everywhere, codes wherever the contract specifies them, the padding codes 0; and a real base."""
    from fedscale_amd import kernels_quant as kq

    dev = gpu_device
    cases = qf.contract_cases()
    rng = np.random.default_rng(11)
    x0 = rng.standard_normal(4099).astype(np.float32)
    b0 = (x0 + rng.standard_normal(4099).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
    cases["real_base"] = None
    for name, d in cases.items():
        if d is None:
            xs, bases, d = x0, [b0], (x0 - b0).astype(np.float32)
        else:
            xs, bases = d, [None, np.zeros_like(d)]
        P, NB = d.size, qf.blocks(d.size)
        want_codes, want_s = qf.quantize(d)
        keep = np.repeat(want_s != 255, 32)
        for base in bases:
            x = torch.from_numpy(xs).to(dev)
            b = None if base is None else torch.from_numpy(base).to(dev)
            q8 = torch.full((NB * 32 + 32,), 0xA5, dtype=torch.uint8, device=dev)
            sc = torch.full((NB + 16,), 0xA5, dtype=torch.uint8, device=dev)
            kq.quantize_row(x, b, P, q8, sc)
            gq, gs = q8.cpu().numpy(), sc.cpu().numpy()
            assert np.array_equal(gs[:NB], want_s), name
            assert np.array_equal(gq[:NB * 32][keep], want_codes[keep]), name
            assert (gq[NB * 32:] == 0xA5).all() and (gs[NB:] == 0xA5).all(), name  # nothing past the extents


def test_device_and_host_paths_of_compress_delta_agree(gpu_device):
    from collections import OrderedDict

    from fedscale_amd.cloud.execution.quant_upload import SCALES_KEY, compress_delta

    dev = gpu_device
    torch.manual_seed(4)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                              torch.nn.Linear(4 * 26 * 26, 10))
    base = OrderedDict((k, v.clone()) for k, v in net.state_dict().items())
    sd = OrderedDict((k, v + 0.01 * torch.randn_like(v) if v.dtype == torch.float32 else v + 5)
                     for k, v in base.items())
    sd["3.bias"][2] = float("nan")  # a NaN block: scale 255, and both paths write the same codes
    host = compress_delta(sd, list(base.values()))
    on_dev = compress_delta(OrderedDict((k, v.to(dev)) for k, v in sd.items()), list(base.values()))
    assert list(host) == list(on_dev) and list(host)[-1] == SCALES_KEY
    for k in host:
        assert host[k].dtype == on_dev[k].dtype and host[k].shape == on_dev[k].shape, k
        assert np.array_equal(host[k], on_dev[k]), k
    assert (host[SCALES_KEY] == 255).sum() == 1
