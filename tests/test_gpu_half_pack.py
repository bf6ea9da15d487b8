"""fh_pack_row on the MI355X: seven separately placed fp32 tensors rounded into one 16-bit row, bit-equal to numpy's
``astype(float16)`` and to torch's CPU ``to(bfloat16)``; and ``compress_update`` of a state on the GPU against the
same state on the CPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = ("float16", "bfloat16")
SIZES = (1, 3, 8, 1027, 4101, 16, 100)  # T = 7; 4101 spans three workgroups of 2048 elements
SRC_OFF = (1, 4, 10, 20, 1051, 5156, 5176)  # fp32 element offsets in one buffer: 4-byte and 16-byte alignments
DST_OFF = (3, 8, 21, 40, 1070, 5180, 5201)  # 16-bit element offsets: 2-, 4- and 16-byte alignments, with gaps
ROW = 5400


def _specials():
    f = np.float32
    one = f(1.0)
    return np.asarray([
        one + f(2.0 ** -11), one + f(3 * 2.0 ** -11),      # float16 ties: to even, down and up
        one + f(2.0 ** -8), one + f(3 * 2.0 ** -8),        # bfloat16 ties: down and up
        -(one + f(2.0 ** -11)), -(one + f(3 * 2.0 ** -8)),
        np.nextafter(f(65520.0), f(0)), f(65520.0), np.nextafter(f(65520.0), f(1e9)), f(-65520.0),  # float16 overflow
        f(2.0 ** -25), np.nextafter(f(2.0 ** -25), one), f(3 * 2.0 ** -25), f(1e-7), f(-6e-8), f(2.0 ** -14),
        f(5.9e-8), f(1e-10),                                # float16 subnormal range and below it
        f(3.3895314e38), f(3.4028235e38), f(-3.4028235e38),  # bfloat16: the largest finite fp32 rounds to inf
        f(np.inf), f(-np.inf), f(np.nan), f(0.0), f(-0.0), f(1e-40), f(-1e-45),
    ], dtype=np.float32)


def _inputs():
    rng = np.random.default_rng(11)
    sp = _specials()
    buf = rng.standard_normal(5300, dtype=np.float32) * np.float32(10.0) ** rng.integers(-9, 5, 5300).astype(np.float32)
    pos = 0
    for t, (n, o) in enumerate(zip(SIZES, SRC_OFF)):
        m = min(n, len(sp))
        buf[o:o + m] = np.roll(sp, -pos)[:m]  # a tensor of one element gets one special, the large ones all
        pos += m
    return buf


def _reference(a: np.ndarray, dtype: str) -> np.ndarray:
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16).view(np.uint16)
    return torch.from_numpy(a.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_row_rounds_as_numpy_and_torch_do(gpu_device, dtype):
    from fedscale_amd import kernels_half as kh

    for a, b, n in zip(SRC_OFF, SRC_OFF[1:], SIZES):
        assert a + n <= b
    for a, b, n in zip(DST_OFF, DST_OFF[1:] + (ROW,), SIZES):
        assert a + n < b  # a gap after every tensor
    assert {o % 4 for o in SRC_OFF} >= {0, 1, 2} and {o % 8 for o in DST_OFF} >= {0, 3, 5, 4}
    host = _inputs()
    buf = torch.from_numpy(host).to(gpu_device)
    assert buf.data_ptr() % 16 == 0
    tensors = [buf[o:o + n] for o, n in zip(SRC_OFF, SIZES)]
    tdt = torch.float16 if dtype == "float16" else torch.bfloat16
    row = torch.full((ROW,), 0x5555, dtype=torch.int16, device=gpu_device).view(tdt)
    kh.pack_row16(tensors, DST_OFF, row)
    got = row.view(torch.int16).cpu().numpy().view(np.uint16)
    touched = np.zeros(ROW, dtype=bool)
    for o, so, n in zip(DST_OFF, SRC_OFF, SIZES):
        src = host[so:so + n]
        want = _reference(src, dtype)
        g = got[o:o + n]
        nan = np.isnan(src)
        assert np.array_equal(g[~nan], want[~nan]), (dtype, n, np.flatnonzero(g != want)[:5])
        if dtype == "float16":
            assert np.isnan(g[nan].view(np.float16)).all()
        else:
            assert ((g[nan] & 0x7f80) == 0x7f80).all() and ((g[nan] & 0x007f) != 0).all()
        touched[o:o + n] = True
    assert touched.sum() == sum(SIZES) and (got[~touched] == 0x5555).all()  # the rest of the row is untouched


@pytest.mark.parametrize("dtype", DTYPES)
def test_compress_update_on_the_gpu_equals_the_cpu_path(gpu_device, dtype):
    from fedscale_amd.cloud.execution.half_upload import compress_update

    torch.manual_seed(5)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                              torch.nn.Linear(4 * 26 * 26, 10))
    sd = net.state_dict()
    sd["0.weight"].reshape(-1)[:28] = torch.from_numpy(_specials())
    cpu = compress_update(sd, dtype)
    dev = compress_update({k: v.to(gpu_device) for k, v in sd.items()}, dtype)
    assert list(dev) == list(cpu) == list(sd)
    spans = []
    for k in cpu:
        assert dev[k].dtype == cpu[k].dtype and dev[k].shape == cpu[k].shape, k
        if cpu[k].dtype == np.int64:
            assert np.array_equal(dev[k], cpu[k])
            continue
        c, d = cpu[k].reshape(-1).view(np.uint16), dev[k].reshape(-1).view(np.uint16)
        nan = np.isnan(sd[k].reshape(-1).numpy())
        assert np.array_equal(c[~nan], d[~nan]), k
        assert not dev[k].flags.owndata
        a0 = dev[k].__array_interface__["data"][0]
        spans.append((a0, a0 + dev[k].nbytes))
    # views of the one host buffer the single D2H filled: every entry 16-byte aligned inside one row-sized span
    total = sum((cpu[k].size + 7) // 8 * 8 for k in cpu if cpu[k].dtype != np.int64)
    lo = min(a for a, _ in spans)
    assert max(b for _, b in spans) - lo <= 2 * total and all((a - lo) % 16 == 0 for a, _ in spans)
