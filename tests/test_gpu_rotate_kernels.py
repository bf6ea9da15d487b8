"""frt_rotate and frt_unrotate on the GPU against the numpy restatement of include/fedrotate.h
(tests/rotate_fixtures.py), bit for bit: sizes on either side of a block, more blocks than CUs, with and without a
base, both extreme seeds, a 4-byte aligned x, out aliasing y, the inputs on which a wrong pairing, a wrong stage
order, a negated difference or a flushed denormal shows, the padding and the extents, host against device encoding,
and the argument refusals."""
import numpy as np
import pytest
import torch

from tests import rotate_fixtures as rf

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = (1, 63, 4095, 4096, 4097, 3 * 4096 + 257, 257 * 4096 + 1)
SEEDS = (0, (1 << 64) - 1)
GUARD = 256


def _vec(P, seed=0):
    """Values over 30 binades, so that a butterfly's rounding depends on the stage order."""
    rng = np.random.default_rng(1000 + P + seed % 97)
    return (rng.standard_normal(P) * np.ldexp(1.0, rng.integers(-15, 15, P))).astype(F32)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rotate(dev, x, base, seed):
    from fedscale_amd import kernels_rotate as kr

    P = x.size
    y = torch.full((rf.padded(P),), 7.0, dtype=torch.float32, device=dev)
    kr.rotate(_dev(x, dev), None if base is None else _dev(base, dev), P, seed, y)
    return y.cpu().numpy()


def _unrotate(dev, y, P, seed):
    from fedscale_amd import kernels_rotate as kr

    out = torch.full((P,), 7.0, dtype=torch.float32, device=dev)
    kr.unrotate(_dev(y, dev), P, seed, out)
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def reference():
    """(x, base, y, back) per (P, seed, with base): computed once, read by the tests."""
    ref = {}
    for P in SIZES:
        for seed in SEEDS:
            for with_base in (False, True):
                if P > 4 * 4096 and (seed != 0 or not with_base):
                    continue  # the long row once: its point is the grid, not the variants
                x = _vec(P, seed)
                base = _vec(P, seed + 1) if with_base else None
                y = rf.rotate(x, base, seed)
                ref[(P, seed, with_base)] = (x, base, y, rf.unrotate(y, P, seed))
    return ref


def test_padded_is_the_contracts():
    from fedscale_amd import kernels_rotate as kr

    for P in (0, 1, 4095, 4096, 4097, 25_000_000):
        assert kr.padded(P) == rf.padded(P)


def test_rotate_and_unrotate_equal_the_restatement_at_every_size(gpu_device, reference):
    for (P, seed, with_base), (x, base, y, back) in reference.items():
        got = _rotate(gpu_device, x, base, seed)
        rf.same(got, y, ("rotate", P, seed, with_base))  # all P' columns, the padding's included
        rf.same(_unrotate(gpu_device, y, P, seed), back, ("unrotate", P, seed, with_base))


def test_x_at_a_four_byte_aligned_address_and_out_aliasing_y(gpu_device, reference):
    from fedscale_amd import kernels_rotate as kr

    dev = gpu_device
    for P in (4097, 3 * 4096 + 257):
        x, base, y, back = reference[(P, 0, True)]
        for off in (1, 2, 3):
            xb = torch.zeros(P + 4, dtype=torch.float32, device=dev)
            bb = torch.zeros(P + 4, dtype=torch.float32, device=dev)
            xs, bs = xb[off:off + P], bb[(off + 1) % 4:(off + 1) % 4 + P]
            xs.copy_(_dev(x, dev))
            bs.copy_(_dev(base, dev))
            assert xs.data_ptr() % 16 != 0
            out = torch.empty(rf.padded(P), dtype=torch.float32, device=dev)
            kr.rotate(xs, bs, P, 0, out)
            rf.same(out.cpu().numpy(), y, (P, off))
        yy = _dev(y, dev)
        kr.unrotate(yy, P, 0, yy)  # in place: columns [0, P) are the model's, the padding keeps the rotated values
        g = yy.cpu().numpy()
        rf.same(g[:P], back, P)
        rf.same(g[P:], y[P:], P)


def test_integer_inputs_are_exact_and_round_trip(gpu_device):
    rng = np.random.default_rng(7)
    x = rng.integers(-2047, 2048, 2 * 4096).astype(F32)
    for seed in SEEDS:
        y = _rotate(gpu_device, x, None, seed)
        want = np.concatenate([rf.dense(x[:4096], seed), _dense_block(x[4096:], seed, 1)])
        assert np.array_equal(y.astype(np.float64), want)
        back = _unrotate(gpu_device, y, x.size, seed)
        assert np.array_equal(back, x)  # by value: a zero column comes back as +0.0 xor d[p]
        assert np.array_equal(back.view(np.uint32), rf.unrotate(y, x.size, seed).view(np.uint32))
        nz = x != 0
        assert np.array_equal(back.view(np.uint32)[nz], x.view(np.uint32)[nz])


def _dense_block(x, seed, b):
    """rf.dense for block b: the diagonal's columns start at 4096 b."""
    H = np.array([[1.0]])
    while H.shape[0] < 4096:
        H = np.block([[H, H], [H, -H]])
    d = 1.0 - 2.0 * rf.diag(seed, 4096 * (b + 1))[4096 * b:].astype(np.float64)
    return H @ (d * x.astype(np.float64)) / 64.0


def test_signed_zeros_denormals_and_one_hot_columns(gpu_device):
    """A constant block and an all-zero block (every difference is a zero whose sign the encoder reads), 1e-40 beside
    1 (sums and results that are subnormal), and one-hot columns at every index bit (a wrong pairing moves them)."""
    cases = {}
    c = np.full(3 * 4096, 0.75, dtype=F32)
    c[4096:2 * 4096] = 0.0
    c[4096 + 5] = -0.0
    cases["constant_and_zero_blocks"] = c
    t = np.zeros(4096 + 100, dtype=F32)
    t[::2] = F32(1e-40)
    t[1::64] = 1.0
    t[4096:] = F32(-1e-40)
    cases["denormals"] = t
    tiny = np.full(4096, F32(1e-40), dtype=F32)
    tiny[7] = F32(-3e-39)
    cases["all_denormal"] = tiny
    hot = np.zeros(13 * 4096, dtype=F32)
    for k in range(12):
        hot[k * 4096 + (1 << k)] = 1.0 + k
    hot[12 * 4096 + 4095] = -2.0
    cases["one_hot"] = hot
    for name, x in cases.items():
        for seed in SEEDS:
            y = rf.rotate(x, None, seed)
            got = _rotate(gpu_device, x, None, seed)
            assert np.array_equal(got.view(np.uint32), y.view(np.uint32)), (name, seed)
            back = _unrotate(gpu_device, y, x.size, seed)
            assert np.array_equal(back.view(np.uint32), rf.unrotate(y, x.size, seed).view(np.uint32)), (name, seed)


def test_a_nan_and_an_infinity_poison_their_own_blocks_only(gpu_device):
    """Every column of a block that holds a NaN or an infinity is non-finite after either transform (NaN, or for a
    lone infinity +-inf), and no other block is touched."""
    P = 5 * 4096 + 10
    x = _vec(P)
    x[4096 + 17] = np.nan
    x[3 * 4096 + 4000] = -np.inf
    y = rf.rotate(x, None, 3)
    got = _rotate(gpu_device, x, None, 3)
    rf.same(got, y)
    for b in range(6):
        blk = got[b * 4096:(b + 1) * 4096]
        assert (~np.isfinite(blk)).all() if b in (1, 3) else np.isfinite(blk).all(), b
    back = _unrotate(gpu_device, y, P, 3)
    rf.same(back, rf.unrotate(y, P, 3))
    for b in range(6):
        blk = back[b * 4096:min(P, (b + 1) * 4096)]
        assert (~np.isfinite(blk)).all() if b in (1, 3) else np.isfinite(blk).all(), b


def test_the_inverse_writes_inside_its_extent_only(gpu_device):
    """Guard bands of 0xA5 around out (P floats exactly) are intact after frt_unrotate, at widths with a partial
    float4 and a partial block; the forward transform writes exactly P' floats."""
    from fedscale_amd import _native_rotate as nr

    dev = gpu_device
    lib = nr.load()
    st = torch.cuda.current_stream().cuda_stream
    for P in (1, 4, 63, 4095, 4097, 2 * 4096 + 6):
        x = _vec(P)
        y = rf.rotate(x, None, 9)
        buf = torch.full((GUARD + 4 * P + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        ptr = buf.data_ptr() + GUARD
        assert ptr % 16 == 0
        rc = lib.frt_unrotate(_keep(y, dev).data_ptr(), P, 9, ptr, st)
        assert rc == 0, lib.fa_last_error_string().decode()
        g = buf.cpu().numpy()
        assert (g[:GUARD] == 0xA5).all() and (g[GUARD + 4 * P:] == 0xA5).all(), P
        rf.same(g[GUARD:GUARD + 4 * P].copy().view(F32), rf.unrotate(y, P, 9), P)
        Pp = rf.padded(P)
        buf = torch.full((GUARD + 4 * Pp + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        rc = lib.frt_rotate(_keep(x, dev).data_ptr(), None, P, 9, buf.data_ptr() + GUARD, st)
        assert rc == 0, lib.fa_last_error_string().decode()
        g = buf.cpu().numpy()
        assert (g[:GUARD] == 0xA5).all() and (g[GUARD + 4 * Pp:] == 0xA5).all(), P
        rf.same(g[GUARD:GUARD + 4 * Pp].copy().view(F32), y, P)


_KEPT = []


def _keep(a, dev):
    """A device copy that outlives the asynchronous call that reads it."""
    t = _dev(a, dev)
    _KEPT.append(t)
    del _KEPT[:-8]
    return t


def _model_state(rng, dev=None):
    st = {"emb.weight": rng.standard_normal((3, 4096)).astype(F32), "steps": np.array(11, dtype=np.int64),
          "fc.weight": rng.standard_normal((19, 41)).astype(F32), "fc.bias": rng.standard_normal(19).astype(F32)}
    st["emb.weight"][1:] = 0.0  # rows no token touched
    if dev is not None:
        return {k: torch.from_numpy(v).to(dev) for k, v in st.items()}
    return st


def test_device_and_host_paths_of_compress_sign_rotated_agree(gpu_device):
    """Two rounds with the residual carried, on a device state and on the same host state: the same bits, scales and
    residual, which are the restatement's; rerotate gives the same vector on both sides."""
    from fedscale_amd.cloud.execution import rotate_upload as ru
    from fedscale_amd.cloud.execution.sign_upload import BITS_KEY, SCALES_KEY

    dev = gpu_device
    rng = np.random.default_rng(5)
    base = _model_state(rng)
    seed = 0xC0FFEE1234567
    r_h = r_d = r_f = None
    for rnd in range(2):
        state = {k: (v + (rng.standard_normal(v.shape) * 0.01).astype(F32) if v.dtype == F32 else v + 1)
                 for k, v in base.items()}
        up_h, r_h = ru.compress_sign_rotated(state, base, seed, residual=r_h, residual_out=True)
        up_d, r_d = ru.compress_sign_rotated({k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in state.items()},
                                             {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in base.items()},
                                             seed, residual=r_d, residual_out=True)
        flat = lambda s: np.concatenate([np.asarray(v).reshape(-1) for v in s.values() if v.dtype == F32])  # noqa: E731
        bits, scales, r_f = rf.encode(flat(state), flat(base), seed, r_f)
        P = flat(state).size
        for up in (up_h, up_d):
            assert list(up) == ["steps", BITS_KEY, SCALES_KEY, ru.ROTATE_KEY]
            assert up[BITS_KEY].shape == (rf.padded(P) // 8,) and up[SCALES_KEY].shape == (rf.padded(P) // 256,)
            assert np.array_equal(up[BITS_KEY], bits), rnd
            assert np.array_equal(up[SCALES_KEY].view(np.uint32), scales.view(np.uint32)), rnd
            assert up[ru.ROTATE_KEY].dtype == np.uint64 and int(up[ru.ROTATE_KEY][0]) == seed
            assert int(up["steps"]) == 12
        rf.same(r_h, r_f, rnd)
        rf.same(r_d.cpu().numpy(), r_f, rnd)
    want = rf.rotate(rf.unrotate(r_f, r_f.size, seed), None, 77)
    rf.same(ru.rerotate(r_h, seed, 77), want)
    rf.same(ru.rerotate(r_d, seed, 77).cpu().numpy(), want)


def test_operands_are_checked_before_anything_is_queued(gpu_device):
    from fedscale_amd import _native_rotate as nr

    lib = nr.load()
    dev = gpu_device
    P = 5000
    x = torch.zeros(8192, device=dev)
    base = torch.zeros(8192, device=dev)
    y = torch.full((8192,), 7.0, device=dev)
    out = torch.full((8192,), 9.0, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    pageable = np.zeros(1 << 16, dtype=np.uint8)
    pinned = torch.zeros(1 << 16, dtype=torch.uint8).pin_memory()
    err = lambda: lib.fa_last_error_string().decode()  # noqa: E731

    def rot(xp=x.data_ptr(), lp=None, p=P, yp=y.data_ptr()):
        return lib.frt_rotate(xp, lp, p, 1, yp, st), err()

    def unrot(yp=y.data_ptr(), p=P, op=out.data_ptr()):
        return lib.frt_unrotate(yp, p, 1, op, st), err()

    refused = [
        (rot(p=-1), "frt_rotate", "negative"),
        (rot(xp=None), "frt_rotate", "NULL"),
        (rot(yp=None), "frt_rotate", "NULL"),
        (rot(xp=x.data_ptr() + 2), "frt_rotate", "4-byte aligned"),
        (rot(lp=base.data_ptr() + 1), "frt_rotate", "4-byte aligned"),
        (rot(yp=y.data_ptr() + 4), "frt_rotate", "16-byte aligned"),
        (rot(xp=pageable.ctypes.data), "frt_rotate", "x is pageable"),
        (rot(lp=pageable.ctypes.data), "frt_rotate", "base is pageable"),
        (rot(yp=pinned.data_ptr()), "frt_rotate", "y is pinned host memory"),
        (unrot(p=-1), "frt_unrotate", "negative"),
        (unrot(yp=None), "frt_unrotate", "NULL"),
        (unrot(op=None), "frt_unrotate", "NULL"),
        (unrot(yp=y.data_ptr() + 8), "frt_unrotate", "16-byte aligned"),
        (unrot(op=out.data_ptr() + 4), "frt_unrotate", "16-byte aligned"),
        (unrot(yp=pageable.ctypes.data), "frt_unrotate", "y is pageable"),
        (unrot(op=pageable.ctypes.data), "frt_unrotate", "out is pageable"),
    ]
    for (rc, msg), entry, word in refused:
        assert rc == -1 and entry in msg and word in msg and "nothing was launched" in msg, (rc, msg, entry, word)
    assert lib.frt_padded(-1) == -1 and "frt_padded" in err()
    assert lib.frt_rotate(None, None, 0, 1, None, st) == 0 and lib.frt_unrotate(None, 0, 1, None, st) == 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((out == 9.0).all())
