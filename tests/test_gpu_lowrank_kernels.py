"""flr_reduce on the MI355X against the float64 reference of tests/lowrank_fixtures.py: exact on integer data at every
tile edge, chain offset, stage tail and rank; inside the any-order bound on random data; bit-identical however the
round is chunked and whichever tile the plan picks; a NaN confined to its output row; and the operands the ABI
refuses."""
import numpy as np
import pytest
import torch

from tests import lowrank_fixtures as lf

pytestmark = pytest.mark.gpu

# a 3-element entry first (every later chain offset is odd), both edges partial on the small tile, several large tiles
# with partial last ones, O < 32, a matrix too small to factor at r >= 3 (a dense tile), a 1-D entry last
SHAPES = [(3,), (33, 95), (130, 260), (8, 40), (4, 5), (7,)]
RANKS = (1, 3, 8, 64)
CHUNKS = (1, 3, 7)  # n * r2 below, equal to and not a multiple of the stage depth 8
P = sum(int(np.prod(s)) for s in SHAPES)
SENTINEL = np.float32(-12345.5)
FA_E_ARG = -1
_DATA = {}


def _uploads(rank, kind):
    """Seven clients' uploads, made once per (rank, kind) and left unchanged; and an accumulator."""
    key = (rank, kind)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * rank + (kind == "int"))
        draw = ((lambda s: rng.integers(-8, 9, size=s).astype(np.float32)) if kind == "int"
                else (lambda s: rng.standard_normal(s).astype(np.float32)))
        ups = [[draw((rank, sum(lf.matrix_dims(s)))) if lf.factored(s, rank) else draw(s) for s in SHAPES]
               for _ in range(7)]
        _DATA[key] = (ups, draw(P))
    return _DATA[key]


def _reduce(ups, rank, acc=None, force=0, chunks=None):
    """The bucket (and the 16 floats after it) after flr_reduce over ``ups``, in one chunk or in ``chunks``."""
    from fedscale_amd import kernels_lowrank as kl

    dev = torch.device("cuda", 0)
    table = kl.TileTable(kl.entry_dims(SHAPES, rank), rank, dev, force)
    rows, _ = lf.pack_rows(ups, SHAPES, rank)
    assert rows.shape[1] == table.ldf and table.P == P
    staged = torch.from_numpy(rows).to(dev)
    out = torch.full((P + 16,), float(SENTINEL), dtype=torch.float32, device=dev)
    a = None if acc is None else torch.from_numpy(acc).to(dev)
    k = 0
    for c in chunks or (len(ups),):
        kl.reduce_lowrank(staged, c, table, out, acc_in=a, row0=k)
        a, k = out, k + c
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("with_acc", (False, True))
@pytest.mark.parametrize("n", CHUNKS)
@pytest.mark.parametrize("rank", RANKS)
def test_exact_on_integers(rank, n, with_acc):
    ups, acc = _uploads(rank, "int")
    acc = acc if with_acc else None
    got = _reduce(ups[:n], rank, acc)
    want = lf.ref64(ups[:n], SHAPES, rank, acc).astype(np.float32)  # |partial sums| < 2^24: any order is exact
    assert np.array_equal(_bits(got[:P]), _bits(want)), np.flatnonzero(got[:P] != want)[:8]
    assert np.all(got[P:] == SENTINEL)


@pytest.mark.parametrize("n", CHUNKS)
@pytest.mark.parametrize("rank", RANKS)
def test_bounded_on_random_data(rank, n):
    ups, acc = _uploads(rank, "normal")
    got = _reduce(ups[:n], rank, acc)[:P].astype(np.float64)
    err = np.abs(got - lf.ref64(ups[:n], SHAPES, rank, acc))
    lim = lf.bound(ups[:n], SHAPES, rank, acc)
    print(f"rank {rank} n {n}: max err / bound = {np.max(err / lim):.3f}")
    assert np.all(err <= lim), np.flatnonzero(err > lim)[:8]


@pytest.mark.parametrize("rank", RANKS)
def test_order_is_the_datas_alone(rank):
    ups, acc = _uploads(rank, "normal")
    one = _reduce(ups, rank, acc)
    assert np.array_equal(_bits(one), _bits(_reduce(ups, rank, acc, chunks=(3, 3, 1))))
    small, large = _reduce(ups, rank, acc, force=64), _reduce(ups, rank, acc, force=128)
    assert np.array_equal(_bits(small), _bits(large)) and np.array_equal(_bits(one), _bits(small))


@pytest.mark.parametrize("force", (64, 128))
def test_a_nan_stays_in_its_row(force):
    rank, e, o = 3, 2, 77  # entry (130, 260), output row 77
    ups, _ = _uploads(rank, "normal")
    clean = _reduce(ups, rank, force=force)
    bad = [[a.copy() for a in u] for u in ups]
    bad[2][e][1, o] = np.nan  # client 2's Ut[1, 77]
    got = _reduce(bad, rank, force=force)
    p0 = sum(int(np.prod(s)) for s in SHAPES[:e]) + o * SHAPES[e][1]
    row = np.zeros(P + 16, dtype=bool)
    row[p0:p0 + SHAPES[e][1]] = True
    assert np.all(np.isnan(got[row])) and np.array_equal(_bits(got[~row]), _bits(clean[~row]))


@pytest.mark.parametrize("what", ("rank 0", "rank 65", "misaligned out", "a table of other shapes"))
def test_refusals(what):
    from fedscale_amd import _native_lowrank as NL
    from fedscale_amd import kernels_lowrank as kl

    dev, rank = torch.device("cuda", 0), 3
    dims = kl.entry_dims(SHAPES, rank)
    table = kl.TileTable(dims, rank, dev)
    other = kl.TileTable(kl.entry_dims(SHAPES[:-1] + [(9,)], rank), rank, dev)
    staged = torch.zeros(2, table.ldf, dtype=torch.float32, device=dev)
    out = torch.full((P + 16,), float(SENTINEL), dtype=torch.float32, device=dev)
    use = other if what == "a table of other shapes" else table
    rc = NL.load().flr_reduce(staged.data_ptr(), table.ldf, 2, {"rank 0": 0, "rank 65": 65}.get(what, rank),
                              len(SHAPES), dims.ctypes.data, 0, use.dev.data_ptr(), use.host.ctypes.data,
                              use.host.size, None, out.data_ptr() + (4 if what == "misaligned out" else 0), 0,
                              torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert rc == FA_E_ARG and bool((out == float(SENTINEL)).all())
