"""fh_reduce on the MI355X against the CPU oracle applied to the widened rows (oracle.cpu_reference.fedavg_flat /
fedbuff_flat on ``x.astype(float32)``): bit-identical, no tolerance anywhere.  The shapes are the smallest at which
each loop of the kernel iterates, derived from the launch plan at the device's CU count (tests/half_fixtures.py;
tests/test_half_reduce_plan.py asserts the plan each shape is listed for)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.cpu_reference import fedavg_flat, fedbuff_flat
from tests import half_fixtures as hf

pytestmark = pytest.mark.gpu

DTYPES = ("float16", "bfloat16")
_ROWS = {}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _to_dev(a: np.ndarray, dtype: str, dev):
    if dtype == "float16":
        return torch.from_numpy(a).to(dev)
    return torch.from_numpy(a.view(np.int16)).to(dev).view(torch.bfloat16)


def _rows(dtype, K, P, dev, seed=0):
    """(host rows [K, ld], widened fp32 [K, P], device rows), made once per shape and never written."""
    key = (dtype, K, P, seed)
    if key not in _ROWS:
        ld = (P + 63) // 64 * 64
        h = hf.random_rows(np.random.default_rng(1000 + seed + P % 977), K, ld, P, dtype)
        _ROWS[key] = (h, hf.widen(h[:, :P], dtype), _to_dev(h, dtype, dev))
    return _ROWS[key]


def _weights(K):
    return [1 / (1 + (3 * j) % 5) ** 0.5 for j in range(K)]  # FedBuff's 1/sqrt(1 + staleness), Python floats


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got: torch.Tensor, want: np.ndarray, P: int, what):
    g = got[:P].cpu().numpy()
    assert g.dtype == np.float32 and want.dtype == np.float32
    bad = np.flatnonzero(_bits(g) != _bits(want[:P]))
    assert bad.size == 0, (what, bad[:5], g[bad[:5]], want[bad[:5]])


def _run_forms(dtype, K, P, dev, forms=("plain", "weighted", "chunks"), split=None):
    from fedscale_amd import kernels_half as kh

    h, w32, x = _rows(dtype, K, P, dev)
    ld = x.shape[1]
    if "plain" in forms:
        out = torch.full((ld,), 7.0, device=dev)
        kh.reduce16(x, K, P, out, denom=float(np.float32(K)), finalize=True)
        _same_bits(out, fedavg_flat(w32), P, (dtype, K, P, "plain"))
    if "weighted" in forms:
        s = _weights(K)
        a = torch.from_numpy(np.asarray([np.float32(v) for v in s], dtype=np.float32)).to(dev)
        den = s[0]
        for v in s[1:]:
            den += v
        out = torch.full((ld,), 7.0, device=dev)
        kh.reduce16(x, K, P, out, a=a, denom=float(np.float32(den)), finalize=True)
        _same_bits(out, fedbuff_flat(w32, s), P, (dtype, K, P, "weighted"))
    if "chunks" in forms and K >= 2:
        k1 = split or (K + 1) // 2
        acc = torch.full((ld,), 7.0, device=dev)
        kh.reduce16(x, k1, P, acc)  # the raw chain of the first chunk
        want1 = w32[0]
        for k in range(1, k1):
            want1 = want1 + w32[k]
        _same_bits(acc, want1, P, (dtype, K, P, "first chunk"))
        # the second chunk continues it, out aliasing acc_in, against ONE oracle chain over all rows
        kh.reduce16(x[k1:], K - k1, P, acc, acc_in=acc, denom=float(np.float32(K)), finalize=True)
        _same_bits(acc, fedavg_flat(w32), P, (dtype, K, P, "chunks"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_widths(gpu_device, dtype):
    """P = 1 .. 513 with K = 5 and ld = round_up(P, 64): masks of the 16-byte loads and the float4 stores."""
    for P in hf.SMALL_P:
        _run_forms(dtype, 5, P, gpu_device)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["level2", "two_levels", "level0"])
def test_every_k_loop_of_every_variant(gpu_device, dtype, shape):
    """K in {1, 2, U-1, U, U+1, 2U+1} for the U of each variant, at the narrowest width that takes the variant:
    the rows-ahead loop runs 0, 1 and 2 times, with and without the single-row remainder."""
    from fedscale_amd import kernels_half as kh

    cus = _cus()
    P, want_plan = hf.expected_plans(cus)[shape]
    assert kh.reduce16_plan(cus, 3, P) == want_plan and kh.reduce16_launches(3, P) == len(want_plan)
    U = want_plan[0]["U"]
    ks = hf.ks_for(U)
    h, w32, x = _rows(dtype, max(ks), P, gpu_device)
    chain, means = w32[0], {}
    for k in range(1, max(ks) + 1):  # one oracle chain; the mean after k rows is chain / fp32(k)
        if k in ks:
            means[k] = np.divide(chain, np.float32(k))
        if k < max(ks):
            chain = chain + w32[k]
    assert np.array_equal(_bits(means[max(ks)]), _bits(fedavg_flat(w32)))
    for K in ks:
        out = torch.full((x.shape[1],), 7.0, device=gpu_device)
        kh.reduce16(x, K, P, out, denom=float(np.float32(K)), finalize=True)
        _same_bits(out, means[K], P, (dtype, shape, K))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["two_levels", "level0", "capped"])
def test_long_widths_in_three_forms(gpu_device, dtype, shape):
    """Two plan levels in one call; one workgroup per level-0 tile with a ragged last tile; the capped grid whose
    workgroups each walk two tiles, the last one ragged.  Unweighted, FedBuff-weighted, and as two chunks whose
    second continues the first (FA_ACCUMULATE, out aliasing acc_in).  Columns [P, ld) hold a poison."""
    from fedscale_amd import kernels_half as kh

    cus = _cus()
    P, want_plan = hf.expected_plans(cus)[shape]
    assert kh.reduce16_plan(cus, 3, P) == want_plan
    h, _, _ = _rows(dtype, 3, P, gpu_device)
    assert h.shape[1] > P and (hf.widen(h[:, P:], dtype) == 3.0).all()
    _run_forms(dtype, 3, P, gpu_device, split=2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mirror_copy_in_pinned_host_memory_equals_out(gpu_device, dtype):
    from fedscale_amd import kernels_half as kh

    for P in (513, hf.P_LEVEL2, hf.p_two_levels(_cus())):
        h, w32, x = _rows(dtype, 3, P, gpu_device)
        ld = x.shape[1]
        out = torch.full((ld,), 7.0, device=gpu_device)
        mirror = torch.full((ld,), 9.0).pin_memory()
        kh.reduce16(x, 3, P, out, denom=float(np.float32(3)), finalize=True, mirror=mirror)
        torch.cuda.synchronize()
        _same_bits(out, fedavg_flat(w32), P, (dtype, P, "out"))
        assert np.array_equal(_bits(mirror[:P].numpy()), _bits(out[:P].cpu().numpy()))
        P4 = (P + 3) // 4 * 4
        assert (mirror[P4:] == 9.0).all() and bool((out[P4:] == 7.0).all())  # nothing past ceil(P/4) float4


def _specials(dtype):
    """16-bit patterns: +-0, the smallest and largest subnormals, the largest finite value, +-inf, NaN."""
    if dtype == "float16":
        return np.asarray([0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x7bff, 0xfbff, 0x7c00, 0xfc00, 0x7e00,
                           0x7c01, 0x0400, 0x3c00], dtype=np.uint16)
    return np.asarray([0x0000, 0x8000, 0x0001, 0x8001, 0x007f, 0x807f, 0x7f7f, 0xff7f, 0x7f80, 0xff80, 0x7fc0,
                       0x7f81, 0x0080, 0x3f80], dtype=np.uint16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(gpu_device, dtype):
    """Subnormals of the 16-bit format and of fp32 survive (bfloat16's subnormals ARE fp32 subnormals), +-inf and
    NaN pass through: finite results bit-equal to the oracle's, NaN in the same positions."""
    from fedscale_amd import kernels_half as kh

    sp = _specials(dtype)
    K, P = 6, 2000
    ld = 2048
    rng = np.random.default_rng(5)
    bits = hf.random_rows(rng, K, ld, P, dtype).view(np.uint16).copy()
    # every special value meets every other one somewhere down a column, and ordinary values elsewhere
    for k in range(K):
        for j in range(0, P - len(sp), 3 * len(sp)):
            bits[k, j:j + len(sp)] = np.roll(sp, k * (1 + j // (3 * len(sp))))
    bits[1:, 40:60] = 0  # columns that keep a single subnormal / special to the end of the chain
    h = bits.view(np.float16) if dtype == "float16" else bits
    w32 = hf.widen(h[:, :P], dtype)
    x = _to_dev(h, dtype, gpu_device)
    for weighted in (False, True):
        out = torch.empty(ld, device=gpu_device)
        with np.errstate(all="ignore"):
            if weighted:
                s = [1.0, 0.5, 2.0 ** -20, 1 / 3 ** 0.5, 1.0, 0.25]
                a = torch.tensor(s, dtype=torch.float32, device=gpu_device)
                den = s[0]
                for v in s[1:]:
                    den += v
                kh.reduce16(x, K, P, out, a=a, denom=float(np.float32(den)), finalize=True)
                want = fedbuff_flat(w32, s)
            else:
                kh.reduce16(x, K, P, out)  # the raw chain: subnormal sums are not divided away
                want = w32[0]
                for k in range(1, K):
                    want = want + w32[k]
        got = out[:P].cpu().numpy()
        nan = np.isnan(want)
        assert nan.any() and (~nan).sum() > P // 2
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])
        if not weighted:
            fin = want[~nan]
            if dtype == "bfloat16":  # fp32 subnormal results are among those compared
                assert ((np.abs(fin) < np.finfo(np.float32).tiny) & (fin != 0)).any()
            else:  # and so is the smallest float16 subnormal, carried alone to the end of a chain
                assert (np.abs(fin) == np.float32(2.0 ** -24)).any()
            assert np.isinf(fin).any()


def test_operands_are_checked_before_anything_is_queued(gpu_device):
    """FA_E_ARG, the operand named, nothing launched: a misaligned x16, ld not a multiple of 64, an unknown
    row_dtype, a pageable out, rows in pinned host memory (x16 is device memory only), rows shorter than K x ld.
    (The stream-of-another-device half of the check needs two GPUs; tests/test_abi_operands.py covers DevScope's
    device checks on the CPU.)"""
    from fedscale_amd import _native_half as nh

    lib = nh.load()
    dev = gpu_device
    K, LD, P = 4, 128, 100
    x = torch.ones(K * LD + 64, dtype=torch.float16, device=dev)
    out = torch.full((LD,), 7.0, device=dev)
    acc = torch.zeros(LD, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    den = ctypes.c_float(4.0)

    def call(x16=x.data_ptr(), dt=0, ld=LD, k=K, p=P, a=None, acc_in=None, o=out.data_ptr(), mirror=None, flags=2):
        rc = lib.fh_reduce(x16, dt, ld, k, p, a, acc_in, o, mirror, den, flags, st)
        return rc, lib.fa_last_error_string().decode()

    pageable = np.zeros(1 << 16, dtype=np.float32)
    pinned = torch.zeros(1 << 16, dtype=torch.float16).pin_memory()
    refused = [
        (call(x16=x.data_ptr() + 2), "x16"),
        (call(x16=x.data_ptr() + 8), "16-byte"),
        (call(ld=LD + 8, p=P), "multiple of 64"),
        (call(ld=96, p=90), "multiple of 64"),
        (call(dt=2), "row_dtype"),
        (call(dt=-1), "row_dtype"),
        (call(o=pageable.ctypes.data), "out"),
        (call(x16=pageable.ctypes.data), "x16"),
        (call(x16=pinned.data_ptr()), "x16"),
        (call(a=pageable.ctypes.data), "a "),
        (call(acc_in=pageable.ctypes.data, flags=3), "acc_in"),
        (call(mirror=pageable.ctypes.data), "mirror"),
        (call(mirror=acc.data_ptr(), flags=0), "mirror"),
        (call(flags=1), "acc_in"),
        (call(k=0, flags=2), "K == 0"),
        (call(ld=64, p=100), "ld < P"),
        (call(flags=8), "flags"),
    ]
    for (rc, msg), word in refused:
        assert rc == -1 and "fh_reduce" in msg and word in msg, (rc, msg, word)
    for (rc, msg), word in refused[6:12]:
        assert "nothing was launched" in msg, msg
    assert "pageable" in refused[6][0][1] and "pinned host memory" in refused[8][0][1]
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # rows that would run past their allocation (a hipMalloc of its own: torch's allocator hands out slices)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    short = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(short), (K - 1) * LD * 2 + 96 * 2) == 0
    try:
        assert hip.hipMemset(short, 0, (K - 1) * LD * 2 + 96 * 2) == 0
        rc, msg = call(x16=short.value)  # needs (K-1)*ld + round_up(P, 8) = 104 elements in the last row, has 96
        assert rc == -1 and "x16" in msg and "past the end of its allocation" in msg, msg
        rc, msg = call(x16=short.value, p=96)
        assert rc == 0, msg
        torch.cuda.synchronize()
        assert bool((out[:96] == 0.0).all()) and bool((out[96:] == 7.0).all())
    finally:
        torch.cuda.synchronize()
        hip.hipFree(short)
    # and the valid call goes through, with and without a pinned mirror
    mirror = torch.zeros(LD).pin_memory()
    rc, msg = call(mirror=mirror.data_ptr())
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert bool((out[:P] == 1.0).all()) and bool((mirror[:P] == 1.0).all()) and bool((out[P:] == 7.0).all())
