"""fa_qfed_accumulate (k_qfed_accum and the gather kernels) against its numpy restatement (tests/qfed_fixtures.py), bit
for bit in delta, chain and the squared norms, at every shape the fixtures list: each tile width of the plain and the
chain launches, full and ragged windows, both gather forms, the K edges as one call and as a continued second call,
integer data (exact in any order), denormal / huge / infinite / NaN entries at three learning rates, and non-zero padding
columns.  The workspace holds NaN before every call, the rows are longer than the columns the kernel may touch (NaN
there in x and last, a sentinel in delta and chain that must survive), and the norms start from non-zero values.

Wall time on an MI355X: the whole file 6 s; a K-edge case 0.01-0.07 s, the full-window and two-window shapes
0.12-0.24 s, the eight-window shape 0.45 s (making the rows and the restatement dominate)."""
import numpy as np
import pytest
import torch

from tests import qfed_fixtures as qf

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENTINEL = -7.5  # delta and chain past the 4 ceil(P / 4) columns
GUARD = 256  # bytes of 0xA5 on either side of a guarded operand


@pytest.fixture(scope="module", autouse=True)
def _free_device_memory():
    yield
    torch.cuda.empty_cache()


def _run(case, x, last, alpha, sq0, chain, dev):
    """The calls of a case on device rows x (calls, K, ld): after each call (delta, chain, sqnorm) on the host; the
    workspace is NaN before each call and the sentinels past the columns must survive."""
    from fedscale_amd import kernels as kx

    K, P, ld = case["K"], case["P"], x.shape[2]
    C = qf.round_up4(P)
    delta = torch.full((ld,), SENTINEL, device=dev)
    ch = torch.full((ld,), SENTINEL, device=dev) if chain else None
    sq = torch.from_numpy(np.ascontiguousarray(sq0)).to(dev)
    ws = torch.empty(qf.ws_bytes_of(case) // 8, dtype=torch.float64, device=dev)
    outs = []
    for i in range(case["calls"]):
        ws.fill_(float("nan"))
        kx.qfed_accumulate(x[i], K, P, last=last, alpha=alpha[i], lr=case["lr"], delta=delta, sqnorm=sq, workspace=ws,
                           accumulate=i > 0, chain=ch)
        outs.append((delta[:C].cpu().numpy(), ch[:C].cpu().numpy() if chain else None, sq.cpu().numpy()))
    assert bool((delta[C:] == SENTINEL).all()) and (ch is None or bool((ch[C:] == SENTINEL).all())), case["name"]
    return outs


@pytest.mark.parametrize("name", [c["name"] for c in qf.SHAPES])
def test_every_shape_bit_for_bit(gpu_device, name):
    """delta, chain and sqnorm equal the restatement after every call of the case; a second run gives the same bits in
    all three; the launch kind the case does not name (plain for a chain case and the reverse) gives the same delta."""
    c = qf.BY_NAME[name]
    d = qf.make(c)
    want = qf.reference(c, d)
    x, last = torch.from_numpy(d["x"]).to(gpu_device), torch.from_numpy(d["last"]).to(gpu_device)
    alpha = torch.from_numpy(d["alpha"]).to(gpu_device)
    got = _run(c, x, last, alpha, d["sqnorm0"], c["chain"], gpu_device)
    for i, ((gd, gc, gs), (wd, wc, ws)) in enumerate(zip(got, want)):
        assert qf.same_bits(gs, ws), (name, i, "sqnorm", gs[:8], ws[:8])
        assert qf.same_bits(gd, wd), (name, i, "delta")
        assert gc is None or qf.same_bits(gc, wc), (name, i, "chain")
    again = _run(c, x, last, alpha, d["sqnorm0"], c["chain"], gpu_device)
    other = _run(c, x, last, alpha, d["sqnorm0"], not c["chain"], gpu_device)
    for i in range(c["calls"]):
        assert all(a is None or qf.same_bits(a, b) for a, b in zip(again[i], got[i])), (name, i, "second run")
        assert qf.same_bits(other[i][0], got[i][0]), (name, i, "plain and chain launches: delta")
    if c["kind"] == "integer":
        assert np.array_equal(got[-1][2], qf.integer_norms(c, d)), name
    if c["kind"] == "specials":
        sq = got[0][2]
        assert np.isfinite(sq[0]) and np.isinf(sq[2]) and np.isnan(sq[3]), sq
        # the other clients of the call move no client's norm, and the poked entries no other column
        for k in (0, 1, 4):
            solo = dict(c, K=1)
            (_, _, s1), = _run(solo, x[:, k:k + 1], last, alpha[:, k:k + 1], d["sqnorm0"][k:k + 1], c["chain"],
                               gpu_device)
            assert qf.same_bits(s1, sq[k:k + 1]), (name, k)
        (cd, cc, _), = _run(c, torch.from_numpy(d["clean"]).to(gpu_device), last, alpha, d["sqnorm0"], c["chain"],
                            gpu_device)
        cols = np.ones(cd.size, dtype=bool)
        cols[[col for pokes in qf.SPECIAL_AT.values() for col, _ in pokes]] = False
        assert qf.same_bits(got[0][0][cols], cd[cols]) and (cc is None or qf.same_bits(got[0][1][cols], cc[cols]))


class Guarded:
    """``nbytes`` of device memory between GUARD bytes of 0xA5."""

    def __init__(self, dev, nbytes, init):
        self.nbytes = nbytes
        self.buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 0
        self.buf[GUARD:GUARD + nbytes] = torch.from_numpy(np.ascontiguousarray(init).view(np.uint8).ravel()).to(dev)

    def check(self, what, dtype):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == 0xA5).all(), f"{what}: written before its start"
        assert (b[GUARD + self.nbytes:] == 0xA5).all(), f"{what}: written past its declared extent"
        return b[GUARD:GUARD + self.nbytes].copy().view(dtype)


def _guarded_operands(c, d, dev, ws_bytes):
    K, C = c["K"], qf.round_up4(c["P"])
    return dict(alpha=Guarded(dev, 4 * K, d["alpha"][0]), sqnorm=Guarded(dev, 8 * K, d["sqnorm0"]),
                workspace=Guarded(dev, ws_bytes, np.full(ws_bytes // 8, np.nan)),
                delta=Guarded(dev, 4 * C, np.full(C, SENTINEL, dtype=F32)),
                chain=Guarded(dev, 4 * C, np.full(C, SENTINEL, dtype=F32)))


def _call(c, x, last, g, K, ws_bytes, flags=0):
    from fedscale_amd import _native
    from fedscale_amd.state import raw_stream

    _native.call("fa_qfed_accumulate", x.data_ptr(), x.shape[-1], K, c["P"], last.data_ptr(), g["alpha"].ptr,
                 c["lr"], g["delta"].ptr, g["chain"].ptr, g["sqnorm"].ptr, g["workspace"].ptr, ws_bytes, flags,
                 raw_stream(0))
    torch.cuda.synchronize()


def test_nothing_is_written_outside_the_declared_extents(gpu_device):
    """K = 257, P = 1025, a chain launch, the workspace of fa_qfed_workspace_bytes(K, ld, P): K floats of alpha, K
    doubles of sqnorm, the workspace and 4 ceil(P / 4) floats of delta and chain each sit between guards of 0xA5; the
    guards are intact after the call, x, last and alpha are unchanged, and the outputs are the restatement's."""
    c = qf.BY_NAME["k257_p1025_chain"]
    d = qf.make(c)
    (wd, wc, wsq) = qf.reference(c, d)[0]
    x, last = torch.from_numpy(d["x"][0]).to(gpu_device), torch.from_numpy(d["last"]).to(gpu_device)
    ws_bytes = qf.workspace_bytes(c["K"], qf.ld_of(c), c["P"])
    g = _guarded_operands(c, d, gpu_device, ws_bytes)
    _call(c, x, last, g, c["K"], ws_bytes)
    assert qf.same_bits(g["delta"].check("delta", F32), wd)
    assert qf.same_bits(g["chain"].check("chain", F32), wc)
    assert qf.same_bits(g["sqnorm"].check("sqnorm", F64), wsq)
    g["workspace"].check("workspace", F64)
    assert np.array_equal(g["alpha"].check("alpha", np.uint32), d["alpha"][0].view(np.uint32))
    assert np.array_equal(x.cpu().numpy().view(np.uint32), d["x"][0].view(np.uint32))
    assert np.array_equal(last.cpu().numpy().view(np.uint32), d["last"].view(np.uint32))


def test_refusals_touch_nothing(gpu_device):
    """K = 2049 (one past fa_qfed_max_chunk) and a workspace one byte short of fa_qfed_workspace_bytes(K, 0, 0) are
    refused before anything is queued: delta, chain, sqnorm and the workspace keep every byte."""
    from fedscale_amd._native import FedAggError

    c = dict(qf.BY_NAME["k2048_p257_chain"], calls=1)
    d = qf.make(c)
    x = torch.zeros((2049, qf.ld_of(c)), device=gpu_device)
    last = torch.from_numpy(d["last"]).to(gpu_device)
    for K, ws_bytes, word in ((2049, qf.workspace_bytes(2049), "K=2049"),
                              (2048, qf.workspace_bytes(2048) - 1, "workspace")):
        g = _guarded_operands(c, d, gpu_device, qf.workspace_bytes(2049))
        before = {n: o.buf.cpu().numpy() for n, o in g.items()}
        with pytest.raises(FedAggError, match=word):
            _call(c, x, last, g, K, ws_bytes)
        torch.cuda.synchronize()
        for n, o in g.items():
            assert np.array_equal(o.buf.cpu().numpy(), before[n]), (word, n)
