"""fq4_reduce and fq4_quantize_row on the MI355X, bit for bit against tests/quant4_fixtures.py."""
import functools

import numpy as np
import pytest
import torch

from tests import quant4_fixtures as q4f

pytestmark = pytest.mark.gpu

SMALL_P = (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049)
WAVES, STRIP = 4, 2048
POISON = (0, 1, 253, 254, 255)


def _ld(P):
    return (P + 63) // 64 * 64 + 64  # ld > P always


def _same(got, want, ctx):
    g, w = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), ctx
    assert np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan]), ctx


def _stage(rows, P, dev, extra_rows=0):
    """Device (q4, scales) of the rows; codes in [P, ld), scale bytes past ceil(P / 32) and rows >= n are poison."""
    n, ld = len(rows), _ld(P)
    lds, NB = (ld // 32 + 15) // 16 * 16, q4f.blocks(P)
    c = np.full((n + extra_rows, ld), 0xF, dtype=np.uint8)
    s = np.full((n + extra_rows, lds), 0xFF, dtype=np.uint8)
    for k, (codes, sc) in enumerate(rows):
        c[k, :P] = codes[:P]
        s[k, :NB] = sc
    return torch.from_numpy(q4f.pack(c.reshape(-1)).reshape(-1, ld // 2)).to(dev), torch.from_numpy(s).to(dev)


@functools.lru_cache(maxsize=None)
def _rows(K, P):
    """The shared rows of (K, P): scales over 40 binades (order matters), one poisoned block in the middle row."""
    rng, NB = np.random.default_rng(1000 * K + P % 9973), q4f.blocks(P)
    rows = [(rng.integers(0, 16, NB * 32).astype(np.uint8), rng.integers(107, 147, NB).astype(np.uint8))
            for _ in range(K)]
    rows[K // 2][1][NB // 2] = POISON[P % 5]
    return rows


def test_every_code_meets_every_scale_byte(gpu_device):
    """One row of 256 blocks, n = 1: block b holds the 16 codes twice under scale byte b.  Bit-equal to the table for
    the bytes 2..252 (+0 + deq: a -0 becomes +0); every column of the other five blocks is NaN."""
    from fedscale_amd import kernels_quant4 as kq4

    P = 256 * 32
    codes, sc = np.tile(np.arange(16, dtype=np.uint8), 2 * 256), np.arange(256, dtype=np.uint8)
    want = q4f.dequantize(codes, sc)
    out = torch.full((P,), 7.0, dtype=torch.float32, device=gpu_device)
    kq4.reduce4(torch.from_numpy(q4f.pack(codes).reshape(1, P // 2)).to(gpu_device),
                torch.from_numpy(sc.reshape(1, 256)).to(gpu_device), 1, P, out)
    _same(out.cpu().numpy(), np.zeros(P, dtype=np.float32) + want, "table")
    blk = want.reshape(256, 32)
    assert np.isnan(blk[list(POISON)]).all() and not np.isnan(np.delete(blk, POISON, axis=0)).any()
    assert blk[2, 1] == np.float32(2.0 ** -126) and blk[252, 7] == np.float32(6 * 2.0 ** 125)


@pytest.mark.parametrize("K", (5, 33))
def test_chain_order_continuation_and_aliasing(gpu_device, K):
    """Bit-equal to the restatement at the small widths and just past every seam of a few-strip plan, the poisoned
    block's 32 columns NaN; split calls, aliased or not, and a non-zero start equal the one-shot chain."""
    from fedscale_amd import kernels_quant4 as kq4

    dev = gpu_device
    widths = set(SMALL_P) | {STRIP * WAVES * 2 + 5}
    for l in kq4.reduce4_plan(torch.cuda.get_device_properties(0).multi_processor_count, K, 3 * STRIP + 7):
        widths |= {c + 1 for c in (l["col0"], l["col0"] + WAVES * l["sw"] * STRIP, l["col0"] + STRIP) if c > 0}
    for P in sorted(widths):
        rows = _rows(K, P)
        want = q4f.chain(rows, P=P)
        b = q4f.blocks(P) // 2
        assert np.isnan(want[32 * b:32 * b + 32]).all() and np.isnan(want).sum() == min(32, P - 32 * b)
        q, s = _stage(rows, P, dev, extra_rows=2)
        out = torch.full((_ld(P),), 7.0, dtype=torch.float32, device=dev)
        kq4.reduce4(q, s, K, P, out)
        got = out.cpu().numpy()
        _same(got[:P], want, (K, P))
        assert (got[P:] == 7.0).all(), (K, P)
        for chunk in sorted({1, 2, K - 1}):
            acc, other = (torch.zeros(_ld(P), dtype=torch.float32, device=dev) for _ in range(2))
            for i, k0 in enumerate(range(0, K, chunk)):
                dst = acc if i % 2 else other  # out aliases acc_in on the odd calls
                kq4.reduce4(q[k0:], s[k0:], min(chunk, K - k0), P, dst, acc_in=acc if i else None)
                if dst is other:
                    acc, other = other, acc
            _same(acc.cpu().numpy()[:P], want, (K, P, chunk))
        start = (np.random.default_rng(P).standard_normal(P) * 1e-3).astype(np.float32)
        acc = torch.zeros(_ld(P), dtype=torch.float32, device=dev)
        acc[:P] = torch.from_numpy(start).to(dev)
        kq4.reduce4(q, s, K, P, acc, acc_in=acc)
        _same(acc.cpu().numpy()[:P], q4f.chain(rows, acc=start, P=P), (K, P, "acc"))


def test_level_and_tile_seams_of_the_wide_plans(gpu_device):
    """K = 5 at one width just past the two-level and the level-0 seams of this GPU's own plan, and one capped grid."""
    from fedscale_amd import kernels_quant4 as kq4

    dev, cus, K = gpu_device, torch.cuda.get_device_properties(0).multi_processor_count, 5
    cap, span0, span1 = max(1, cus * 75 // 100), WAVES * 4, WAVES * 2
    two_levels = (span1 * ((cus + 1) // 2) + 3) * STRIP + 77
    level0, capped = (span0 * ((cap * 85 + 99) // 100) - 3) * STRIP - 5, span0 * cap * STRIP + 1
    assert [l["V"] for l in kq4.reduce4_plan(cus, K, two_levels)] == [2, 1]
    assert [l["V"] for l in kq4.reduce4_plan(cus, K, level0)] == [4]
    (l,) = kq4.reduce4_plan(cus, K, capped)
    assert l["grid"] < l["tiles"]
    for P in (two_levels, level0, capped):
        rows = _rows(K, P)
        q, s = _stage(rows, P, dev)
        out = torch.empty(_ld(P), dtype=torch.float32, device=dev)
        kq4.reduce4(q, s, K, P, out)
        _same(out.cpu().numpy()[:P], q4f.chain(rows, P=P), P)


def test_operands_are_checked_before_anything_is_queued(gpu_device):
    from fedscale_amd import _native_quant4 as nq4

    lib, dev = nq4.load(), gpu_device
    n, LD, P = 4, 128, 100
    q = torch.zeros(n * LD // 2 + 64, dtype=torch.uint8, device=dev)
    s = torch.full((n * 4 + 64,), 127, dtype=torch.uint8, device=dev)
    out, x = torch.full((LD,), 7.0, device=dev), torch.zeros(LD, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    page, pin = np.zeros(1 << 16, dtype=np.uint8).ctypes.data, torch.zeros(1 << 16, dtype=torch.uint8).pin_memory()
    R = [q.data_ptr(), s.data_ptr(), LD, 4, n, P, None, out.data_ptr(), 0, st]  # fq4_reduce's arguments
    Q = [x.data_ptr(), None, None, P, q.data_ptr(), s.data_ptr(), None, st]      # fq4_quantize_row's
    cases = [(R, {0: R[0] + 8}, "q4"), (R, {1: R[1] + 4}, "scales"), (R, {7: R[7] + 4}, "out"),
             (R, {6: R[7] + 8, 8: 1}, "acc_in"), (R, {2: 96}, "ld=96 < P=100"), (R, {2: LD + 32}, "multiple of 64"),
             (R, {3: 3}, "lds=3"), (R, {0: page}, "q4 is pageable"), (R, {1: pin.data_ptr()}, "scales is pinned"),
             (R, {7: page}, "out is pageable"), (R, {6: page, 8: 1}, "acc_in is pageable"), (R, {8: 1}, "acc_in"),
             (R, {4: 0}, "n=0"), (R, {8: 2}, "flags"), (Q, {0: Q[0] + 4}, "aligned"), (Q, {0: page}, "x is pageable"),
             (Q, {1: page}, "base is pageable"), (Q, {2: pin.data_ptr()}, "residual is pinned"),
             (Q, {4: page}, "q4 is pageable"), (Q, {5: page}, "scales is page"), (Q, {6: page}, "residual_out is page")]
    for base, change, word in cases:
        entry = "fq4_reduce" if base is R else "fq4_quantize_row"
        rc = getattr(lib, entry)(*[change.get(i, v) for i, v in enumerate(base)])
        msg = lib.fa_last_error_string().decode()
        assert rc == -1 and entry in msg and word in msg and "nothing was launched" in msg, (rc, msg, entry, word)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((q == 0).all()) and bool((s == 127).all())


@pytest.mark.parametrize("with_residual", (False, True))
def test_quantize_row_equals_the_restatement_on_the_contracts_cases(gpu_device, with_residual):
    """Byte for byte, with a NULL base, a +0 base and a real one; nothing past the extents is written."""
    from fedscale_amd import kernels_quant4 as kq4

    dev = gpu_device
    rng = np.random.default_rng(11)
    x0 = rng.standard_normal(4099).astype(np.float32)
    b0 = (x0 + rng.standard_normal(4099).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
    cases = dict(q4f.contract_cases(), real_base=None)
    for name, d in cases.items():
        xs, bases = (x0, [b0]) if d is None else (d, [None, np.zeros_like(d)])
        d = (x0 - b0).astype(np.float32) if d is None else d
        P, NB = d.size, q4f.blocks(d.size)
        r_in = (rng.standard_normal(P) * np.abs(d).clip(0, 1e30) * 0.3).astype(np.float32) if with_residual else None
        with np.errstate(invalid="ignore", over="ignore"):
            want_c, want_s, want_r = q4f.quantize(d if r_in is None else d + r_in)
        for base in bases:
            t = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
            q = torch.full((NB * 16 + 32,), 0xA5, dtype=torch.uint8, device=dev)
            sc = torch.full((NB + 16,), 0xA5, dtype=torch.uint8, device=dev)
            ro = torch.full((P + 8,), 7.0, dtype=torch.float32, device=dev) if with_residual else None
            kq4.quantize_row4(t(xs), t(base), t(r_in), P, q, sc, ro)
            gq, gs = q.cpu().numpy(), sc.cpu().numpy()
            assert np.array_equal(gs[:NB], want_s), name
            assert np.array_equal(gq[:NB * 16], q4f.pack(want_c)), name
            assert (gq[NB * 16:] == 0xA5).all() and (gs[NB:] == 0xA5).all(), name
            if with_residual:
                gr = ro.cpu().numpy()
                assert np.array_equal(gr[:P].view(np.uint32), want_r.view(np.uint32)) and (gr[P:] == 7.0).all(), name


def test_device_and_host_paths_of_compress_delta4_agree(gpu_device):
    from fedscale_amd.cloud.execution.quant4_upload import SCALES_KEY, compress_delta4

    torch.manual_seed(4)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                              torch.nn.Linear(4 * 26 * 26, 10))
    base = {k: v.clone() for k, v in net.state_dict().items()}
    sd = {k: v + 0.01 * torch.randn_like(v) if v.dtype == torch.float32 else v + 5 for k, v in base.items()}
    sd["3.bias"][2] = float("nan")
    P = sum(v.numel() for v in sd.values() if v.dtype == torch.float32)
    r_in = (0.003 * torch.randn(P)).numpy()
    host, hr = compress_delta4(sd, list(base.values()), residual=r_in)
    on_dev, dr = compress_delta4({k: v.to(gpu_device) for k, v in sd.items()}, list(base.values()),
                                 residual=torch.from_numpy(r_in).to(gpu_device))
    assert list(host) == list(on_dev) and list(host)[-1] == SCALES_KEY
    for k in host:
        assert host[k].dtype == on_dev[k].dtype and np.array_equal(host[k], on_dev[k]), k
    assert (host[SCALES_KEY] == 255).sum() == 1
    assert np.array_equal(hr.view(np.uint32), dr.cpu().numpy().view(np.uint32))
