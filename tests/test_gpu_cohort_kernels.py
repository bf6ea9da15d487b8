"""The cohort kernels (fedscale_amd/csrc/cohort_sig.hip) against plain numpy at the shapes where their code paths
differ from what the fixtures of tests/test_gpu_cohort_signature.py reach: several steps of ``k_gram_partial``'s
main loop per workgroup, short last splits and ragged ends; both reduction levels of ``fc_center``'s sum of squares
and a second block along K; the row loops of ``fc_signature`` / ``fc_normalize`` past gridDim.y; several launches of
``fc_signature`` (more than SG_MAX segments) and its full grid of source / destination / ``last`` alignments.

Criteria.  No tolerance of its own: every numeric assertion is bit equality against a host reference (integer or
float64 arithmetic that is exact for the inputs, or numpy's own order of operations where that is the contract of
include/fedcohort.h), or one of the bounds tests/test_gpu_cohort_signature.py states (D * 2^-52 for the fp64 sums of
squares, D * 2^-24 * sqrt(G_ii G_jj) for a Gram of non-integer data).  Outputs are compared over their whole
allocation where the test owns it: what a kernel is not to write keeps the pattern the test put there.

Conditions on the inputs are asserted on the host before any device call (they say that the test can see the
mistake it is for): the Gram shapes really iterate (from ``fc_gram_workspace_bytes``), and the crafted columns of
the centring tests give a different float16 mean under every other summation order / division."""
import numpy as np
import pytest
import torch

from tests.test_cohort_kernel_plans import CT_SEG, GK, center_plan, gram_plan
from tests.test_gpu_cohort_signature import _bits_equal, _gram_check, _gram_matrix

pytestmark = pytest.mark.gpu

F16, F32, F64 = np.float16, np.float32, np.float64
NAN16 = float("nan")
FILL = 0x5A5A  # bit pattern of every float16 a kernel is not to write (203.25: not zero, not NaN)


def _round_up(a, b):
    return (a + b - 1) // b * b


def _layouts(mat: np.ndarray, dev, pad=NAN16):
    """``mat`` ([K, D] float16) in the three layouts of include/fedcohort.h, as [K, ld] device tensors whose first D
    columns hold it and whose other columns hold ``pad``:
      odd stride      ld odd: element-wise loads and stores everywhere
      aligned padded  16-byte aligned base, ld a multiple of 8 greater than D: the 16-byte path
      base 2 off      the same stride from a base 2 bytes past a 16-byte boundary: element-wise again"""
    K, D = mat.shape
    src = torch.tensor(mat, device=dev)  # (a copy: the shared inputs are read-only arrays)
    ld_odd = D if D % 2 else D + 1
    ld8 = _round_up(D + 1, 8)
    odd = torch.full((K, ld_odd), pad, dtype=torch.float16, device=dev)
    vec = torch.full((K, ld8), pad, dtype=torch.float16, device=dev)
    off = torch.full((K * ld8 + 1,), pad, dtype=torch.float16, device=dev)[1:].view(K, ld8)
    assert vec.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 2 and odd.stride(0) % 2 == 1
    for t in (odd, vec, off):
        t[:, :D] = src
    return [("odd stride", odd), ("aligned padded", vec), ("base 2 bytes off", off)]


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ----------------------------------------------------------------------------------------------------------------
# 1. fc_gram
# ----------------------------------------------------------------------------------------------------------------
# (K, D, least number of columns every split but the last must hold)
#   256: four or more 64-column steps per workgroup; 128: two or three; None: a one-step shape, listed for its edges
GRAM_SHAPES = [
    (129, 65701, 256),   # 6 tiles, 342 splits reduced to 257, 4 steps each, a short last split, 37 ragged columns
    (65, 131395, 256),   # 3 tiles, 4 steps per split
    (3, 200000, 128),    # one tile, 2 steps per split, 1563 splits
    (200, 70000, 256),   # 10 tiles, 6 steps per split
    (4096, 130, 128),    # 2080 tiles: the whole triangular tile decode at FC_GRAM_MAX_K; a single split of 3 steps
    (4096, 8, None),     # 2080 tiles, one partial step
    (64, 128, None),     # D an exact multiple of the step
    (130, 43776, 128),   # 6 tiles, 2 steps per split, D = 342 * 128: no short last split
]
GRAM_THREE_LAYOUTS = {(129, 65701), (65, 131395), (3, 200000)}


def _assert_gram_iterates(K, D, min_cols):
    """The number of splits, read from the library: every split but the last holds dchunk >= D / nsplit columns, and
    dchunk is a whole number, so ceil(D / nsplit) >= 128 proves a second step of the main loop (the register prefetch
    under the MFMAs, the barrier before the LDS image is overwritten, the ``dk + GK < d1`` edge) and >= 256 a fourth.
    (D / nsplit itself is 255.6 at K = 129, D = 65701 because the last split is short, and 128 at the two-step
    shapes; the bound is on the whole columns per split, which is what the loop runs.)  A change of the tile
    constants that turns these shapes into one-step cases fails here, and so does one that leaves the restated plan
    of tests/test_cohort_kernel_plans.py behind."""
    from fedscale_amd import _native_cohort as nc

    nsplit = nc.load().fc_gram_workspace_bytes(K, D) // (4 * K * K)
    tiles, want_nsplit, per = gram_plan(K, D)
    assert nsplit == want_nsplit and nsplit >= 1, (K, D, nsplit, want_nsplit)
    if min_cols is not None:
        cols = -(-D // nsplit)
        assert cols >= min_cols and per * GK >= min_cols and per >= 2, \
            f"K={K} D={D}: {nsplit} splits of {cols} columns no longer iterate"
    return nsplit, per


def _int_matrix(K, D, seed):
    return np.random.default_rng(seed).integers(-4, 5, size=(K, D)).astype(F16)


@pytest.mark.parametrize("K,D,min_cols", GRAM_SHAPES)
def test_gram_of_integer_matrices_is_exact(gpu_device, K, D, min_cols):
    """float16 matrices of integers in -4..4: every product and every partial sum is an integer below 2^24
    (|G_ij| <= 16 D < 2.2 M), so fp32 accumulation is exact in any order and the Gram must equal the integer Gram
    bit for bit — a dropped, doubled or stale 64-column step, or one column at a split seam, changes it."""
    from fedscale_amd import cohort_signature as cs

    nsplit, per = _assert_gram_iterates(K, D, min_cols)
    c = _int_matrix(K, D, 7 * K + D)
    c64 = c.astype(F64)
    want = (c64 @ c64.T).astype(F32)
    assert np.abs(want).max() < 2.0 ** 24 and np.count_nonzero(c[:, -1]) > 0
    if (K, D) in GRAM_THREE_LAYOUTS:
        layouts = [("contiguous", torch.from_numpy(c).to(gpu_device))] + _layouts(c, gpu_device)[1:]
    else:
        layouts = [("contiguous", torch.from_numpy(c).to(gpu_device))]
    first = None
    for name, t in layouts:
        ctx = f"gram K={K} D={D} ({nsplit} splits of {per} steps) {name}"
        got = cs.gram(t, K, D).cpu().numpy()
        assert got.dtype == F32 and got.shape == (K, K), ctx
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, f"{ctx}: {bad.size} of {K * K} elements differ from the integer Gram, first at " \
                              f"{divmod(int(bad[0]), K)}: {got.flat[bad[0]]} != {want.flat[bad[0]]}"
        assert np.array_equal(got, got.T), f"{ctx}: not exactly symmetric"
        assert _same_bits(cs.gram(t, K, D).cpu().numpy(), got), f"{ctx}: second call differs"
        if first is None:
            first = got
        assert _same_bits(got, first), f"{ctx}: differs from the contiguous layout"


def test_gram_of_non_integer_data_at_an_iterating_shape(gpu_device):
    """Rows of different magnitude, K = 129, D = 65701 (4 steps per split): the any-order bound of
    tests/test_gpu_cohort_signature.py, whose share ``_gram_check`` prints."""
    from fedscale_amd import cohort_signature as cs

    K, D = 129, 65701
    _assert_gram_iterates(K, D, 256)
    c = _gram_matrix(K, D, 1000 * K + D)
    t = torch.from_numpy(c).to(gpu_device)
    got = cs.gram(t).cpu().numpy()
    _gram_check(c, got, False, f"gram K={K} D={D}")
    assert _same_bits(cs.gram(t).cpu().numpy(), got), "second call differs"
    pad = _layouts(c, gpu_device)[1][1]
    assert _same_bits(cs.gram(pad, K, D).cpu().numpy(), got), "the 16-byte path differs from the element-wise one"


def test_gram_refuses_more_than_max_k_rows_and_writes_nothing(gpu_device):
    from fedscale_amd import _native_cohort as nc
    from fedscale_amd import cohort_signature as cs
    from fedscale_amd._native import FedAggError

    K, D = nc.GRAM_MAX_K + 1, 8
    c = torch.ones(K, D, dtype=torch.float16, device=gpu_device)
    with pytest.raises(ValueError, match="at most 4096"):
        cs.gram(c)
    with pytest.raises(ValueError, match="at most 4096"):
        cs.gram(c, K, D)
    assert nc.load().fc_gram_workspace_bytes(K, D) == 0
    out = torch.full((K * K,), 7.25, dtype=torch.float32, device=gpu_device)  # (room for K x K: nothing can land outside)
    ws = torch.full((K * K,), 7.25, dtype=torch.float32, device=gpu_device)
    with pytest.raises(FedAggError, match="at most 4096"):
        nc.call("fc_gram", c.data_ptr(), D, K, D, out.data_ptr(), ws.data_ptr(), cs._handle(c))
    torch.cuda.synchronize()
    assert bool((out == 7.25).all()) and bool((ws == 7.25).all()) and bool((c == 1).all())


# ----------------------------------------------------------------------------------------------------------------
# 2. fc_center
# ----------------------------------------------------------------------------------------------------------------
def _chain(a32: np.ndarray) -> np.ndarray:
    """The contract of include/fedcohort.h: an fp32 accumulator that starts from row 0 and adds the rows in order."""
    acc = a32[0].copy()
    for k in range(1, a32.shape[0]):
        acc = acc + a32[k]
    return acc


def _tree(a32: np.ndarray) -> np.ndarray:
    if a32.shape[0] == 1:
        return a32[0]
    h = a32.shape[0] // 2
    return _tree(a32[:h]) + _tree(a32[h:])


def _center_ref(sig: np.ndarray):
    """fp32 chain from row 0, / float32(K), one rounding to float16, centre in fp32, one rounding to float16."""
    K = sig.shape[0]
    with np.errstate(all="ignore"):
        avg = (_chain(sig.astype(F32)) / F32(K)).astype(F16)
        cen = (sig.astype(F32) - avg.astype(F32)).astype(F16)
    return avg, cen


def _other_means(sig: np.ndarray):
    """The float16 mean under the orders of operations a rewrite might choose instead."""
    K = sig.shape[0]
    a = sig.astype(F32)
    fk = F32(K)
    alts = {
        "reversed chain": (_chain(a[::-1]) / fk).astype(F16),
        "pairwise tree": (_tree(a) / fk).astype(F16),
        "fp64 sum": (a.astype(F64).sum(axis=0).astype(F32) / fk).astype(F16),
        "multiply by 1/K": (_chain(a) * (F32(1) / fk)).astype(F16),
    }
    if K >= 8:  # numpy's own pairwise sum (8 accumulators) runs along a contiguous axis only
        alts["np.add.reduce"] = (np.add.reduce(np.ascontiguousarray(a.T), axis=1) / fk).astype(F16)
    return alts


_DIV, _RCP = {}, {}


def _reciprocal_can_differ(K: int) -> bool:
    """Whether ANY fp32 sum acc gives a different float16 for acc / K than for acc * (1 / K).  The two fp32 quotients
    are at most an ulp apart, so the float16 results differ only where they lie on or astride a float16 tie m: every
    tie of a binade (the rest follows by scaling with powers of two) and of the subnormal range, and the fp32
    neighbours of m * K.  For K = 9, 10, 17 and 300 there is none (1 / K rounds to fp32 with a relative error below
    2^-25, which moves no quotient across a tie): a reciprocal multiply gives the same bits as the division for
    every input there, and no test can tell them apart.  K = 7 and K = 1000 have such sums, which is why the centring
    tests run them."""
    if K not in _RCP:
        fk = F32(K)
        rcp = F32(1) / fk
        odd = 2.0 * np.arange(1024) + 1
        hits = 0
        for m in (1 + odd * 2.0 ** -11, odd * 2.0 ** -25):
            base = (m * K).astype(F32)
            for j in range(-4, 5):
                acc = base.copy()
                for _ in range(abs(j)):
                    acc = np.nextafter(acc, F32(np.inf if j > 0 else -np.inf))
                hits += int(((acc / fk).astype(F16).view(np.uint16) != (acc * rcp).astype(F16).view(np.uint16)).sum())
        _RCP[K] = hits > 0
    return _RCP[K]


def _division_columns(K: int, n: int) -> np.ndarray:
    """[K, n] float16 columns (three non-zero rows each) whose fp32 sum acc gives a different float16 for acc / K
    than for acc * (1 / K): a seeded search over sums of three random float16 of independent magnitude, once per K."""
    if K not in _DIV:
        rng = np.random.default_rng(9000 + K)
        fk = F32(K)
        rcp = F32(1) / fk
        found = []
        have = 0
        for _ in range(60):
            v = (rng.normal(0, 1, size=(3, 1 << 19)) * 10.0 ** rng.uniform(-2, 2, size=(3, 1 << 19))).astype(F16)
            acc = (v[0].astype(F32) + v[1].astype(F32)) + v[2].astype(F32)
            hit = (acc / fk).astype(F16).view(np.uint16) != (acc * rcp).astype(F16).view(np.uint16)
            found.append(v[:, hit])
            have += int(hit.sum())
            if have >= 96:
                break
        _DIV[K] = np.concatenate(found, axis=1)
        assert _DIV[K].shape[1] >= 96, f"K={K}: the search found {_DIV[K].shape[1]} division columns"
    v = _DIV[K][:, :n]
    rng = np.random.default_rng(K)
    out = np.zeros((K, v.shape[1]), dtype=F16)
    for j in range(v.shape[1]):
        out[np.sort(rng.choice(K, size=3, replace=False)), j] = v[:, j]
    return out


def _cancellation_columns(K: int, n: int, seed: int) -> np.ndarray:
    """[K, n] float16: +B in one row, -B in a later one (B = 32768), s = 2^-10 everywhere else.  The fp32 chain
    loses the s that follow +B (a quarter of an ulp each) and keeps those after -B; a tree, a reversed chain or an
    fp64 accumulator keeps others."""
    rng = np.random.default_rng(seed)
    pairs = [(p, q) for p in range(K) for q in range(p + 1, K)]
    if len(pairs) > n:
        keep = {(0, 1), (0, K - 1), (K - 2, K - 1), (1, K - 2), (K // 2, K // 2 + 1), (3, K - 1), (2, K - 3)}
        rest = [pq for pq in pairs if pq not in keep]
        pairs = sorted(pq for pq in keep if pq[0] < pq[1]) + [rest[i] for i in rng.permutation(len(rest))]
    out = np.full((K, n), 2.0 ** -10, dtype=F16)
    for j in range(n):
        p, q = pairs[j % len(pairs)]
        out[p, j], out[q, j] = 32768.0, -32768.0
    return out


_CENTER_IN = {}


def _center_input(K: int, D: int) -> np.ndarray:
    """Random columns of different magnitude with the crafted ones scattered among them (so they fall on every lane
    and both sides of a workgroup boundary); for D < 512 as many crafted ones as fit."""
    if (K, D) in _CENTER_IN:
        return _CENTER_IN[(K, D)]
    rng = np.random.default_rng(100 * K + D)
    sig = (rng.normal(0, 1, size=(K, D)) * 10.0 ** rng.uniform(-4, 1, size=(1, D))).astype(F16)
    ncan = min(160, (D + 1) // 2) if K >= 2 else 0
    ndiv = min(96, D - ncan) if K >= 3 and _reciprocal_can_differ(K) else 0
    cols = rng.permutation(D)[:ncan + ndiv]
    if ncan:
        sig[:, cols[:ncan]] = _cancellation_columns(K, ncan, K)
    if ndiv:
        sig[:, cols[ncan:]] = _division_columns(K, ndiv)
    sig.setflags(write=False)
    _CENTER_IN[(K, D)] = sig
    return sig


def _assert_orders_differ(sig: np.ndarray, avg: np.ndarray):
    """A property of the inputs, checked against the references only: every other order of operations gives a
    different float16 mean in at least 64 columns.  It can hold only where orders differ at all: K >= 3 (K = 1 and
    K = 2 have one order; every listed K above 2 is at least 7), at least 64 crafted columns of each kind (D >= 511),
    and for the reciprocal a K at which it can differ from the division at all (``_reciprocal_can_differ``: of the
    listed K, 7 and 1000)."""
    K, D = sig.shape
    if K < 3 or D < 511:
        return
    for name, alt in _other_means(sig).items():
        if name == "multiply by 1/K" and not _reciprocal_can_differ(K):
            assert _same_bits(alt, avg)
            continue
        ndiff = int((alt.view(np.uint16) != avg.view(np.uint16)).sum())
        assert ndiff >= 64, f"K={K} D={D}: '{name}' differs from the chain in {ndiff} columns only"


def _check_center(dev, sig: np.ndarray, exact_sumsq=None, finite=True, crafted=True):
    from fedscale_amd import cohort_signature as cs

    K, D = sig.shape
    avg, cen = _center_ref(sig)
    if crafted:
        _assert_orders_differ(sig, avg)
    c64 = cen.astype(F64)
    with np.errstate(all="ignore"):
        want = (c64 * c64).sum(axis=1)
    first = None
    for name, t in _layouts(sig, dev):
        ctx = f"center K={K} D={D} {name}"
        a, c, ss = cs.center(t, K, D)
        assert tuple(a.shape) == (D,) and tuple(ss.shape) == (K,) and c.shape[0] == K and c.shape[1] >= D
        _bits_equal(a.cpu().numpy(), avg, f"{ctx} mean")
        _bits_equal(c[:K, :D].cpu().numpy(), cen, f"{ctx} centred")
        got = ss.cpu().numpy()
        assert got.dtype == F64
        if finite:
            rel = np.abs(got - want) / np.where(want > 0, want, 1.0)
            print(f"{ctx}: sumsq max rel err {rel.max():.3g} (bound {D * 2.0 ** -52:.3g})")
            assert (np.abs(got - want) <= D * 2.0 ** -52 * want).all(), ctx
        else:
            assert np.array_equal(np.isnan(got), np.isnan(want)), f"{ctx}: sumsq NaN placement"
            assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]), f"{ctx}: sumsq inf placement"
        if exact_sumsq is not None:
            assert _same_bits(got, exact_sumsq), f"{ctx}: sumsq {got} is not the exact {exact_sumsq}"
        if first is None:
            first = got
        assert _same_bits(got, first), f"{ctx}: sumsq differs between layouts"  # (fixed order: the same bits)


CENTER_SHAPES = [(K, 513) for K in (1, 2, 7, 8, 9, 10, 16, 17, 300, 1000)] + \
    [(9, D) for D in (1, 8, 511, 512, 16385, 36003)] + [(300, 16385)]


@pytest.mark.parametrize("K,D", CENTER_SHAPES)
def test_center_in_numpys_order_with_crafted_columns(gpu_device, K, D):
    """Mean and centred matrix bit-exact in the order of operations include/fedcohort.h states, on columns built so
    that a reversed, pairwise or fp64 accumulation each change the float16 mean, and at K = 7 and K = 1000 (the listed
    K at which it can) a multiply by 1 / K; K - 1 takes the remainders 0, 1, 6, 7 of the 8-way unrolled loop; D = 16385 and 36003 give ``k_center_seg`` 2 and 3 partial rows
    per segment (36003: a short last one, empty ones after it), K = 300 a second block along K."""
    nrows, per, blocks = center_plan(K, D)
    if D == 16385:
        assert (nrows, per) == (33, 2)
    if D == 36003:
        assert (nrows, per) == (71, 3) and nrows % per and nrows < CT_SEG * per
    if K >= 300:
        assert blocks == (K + 255) // 256 >= 2
    _check_center(gpu_device, _center_input(K, D))


@pytest.mark.parametrize("K", [8, 16])
def test_center_sumsq_is_exact_on_integer_input(gpu_device, K):
    """Integers in -8..8, K = 8 or 16: the mean is a multiple of 1 / K, every centred value a multiple of 1 / 16
    below 32, every square a multiple of 2^-8 below 2^10 and every fp64 partial sum exact in any order — so the
    device's sums of squares must equal the exact ones bit for bit.  D = 36003: 71 partial rows, 3 per segment; a
    dropped or doubled partial row shows."""
    D = 36003
    assert center_plan(K, D)[:2] == (71, 3)
    sig = np.random.default_rng(K).integers(-8, 9, size=(K, D)).astype(F16)
    ints = sig.astype(np.int64)
    cen_k = ints * K - ints.sum(axis=0)  # K * (v - mean): integers
    exact = (cen_k * cen_k).sum(axis=1).astype(F64) / F64(K * K)  # (integer below 2^53, power-of-two divisor)
    avg, cen = _center_ref(sig)
    assert np.array_equal(cen.astype(F64) * K, cen_k.astype(F64)) and (exact > 0).all()
    _check_center(gpu_device, sig, exact_sumsq=exact, crafted=False)


def test_center_special_values(gpu_device):
    """+inf, +inf with -inf (NaN mean, a NaN column), float16 subnormals, -0.0, and columns whose fp32 sum leaves
    the float16 range while the mean does not (an accumulator narrower than fp32 would give inf; the mean of finite
    float16 values cannot itself overflow — it is +-inf only where a column holds an infinity).  NaN where numpy has
    NaN, every other bit equal."""
    K, D = 9, 513
    rng = np.random.default_rng(77)
    sig = (rng.normal(0, 1, size=(K, D)) * 10.0 ** rng.uniform(-4, 1, size=(1, D))).astype(F16)
    sub = 2.0 ** -24
    cols = rng.permutation(D)
    for i, j in enumerate(cols[:40]):
        sig[i % K, j] = np.inf if i % 3 else -np.inf                    # one infinity: the mean is +-inf
    for i, j in enumerate(cols[40:80]):
        sig[i % K, j], sig[(i + 1 + i % 5) % K, j] = np.inf, -np.inf    # both: the mean and the column are NaN
    for i, j in enumerate(cols[80:120]):
        sig[:, j] = (rng.integers(-1023, 1024, size=K) * sub).astype(F16)  # subnormals only
    for i, j in enumerate(cols[120:150]):
        sig[:, j] = -0.0
        if i % 2:
            sig[i % K, j] = 0.0
    for i, j in enumerate(cols[150:190]):
        sig[:, j] = (60000.0 + 32 * rng.integers(0, 100, size=K)) * (1 if i % 2 else -1)  # |sum| ~ 5.4e5
    for i, j in enumerate(cols[190:210]):
        sig[:, j] = 65504.0 if i % 2 else -65504.0
    avg, cen = _center_ref(sig)
    assert np.isnan(avg.astype(F32)).sum() == 40 and np.isinf(avg.astype(F32)).sum() == 40
    assert np.isnan(cen.astype(F32)).all(axis=0).sum() == 40
    assert (np.abs(avg[cols[150:210]].astype(F32)) >= 60000).all() and np.isfinite(avg[cols[150:210]].astype(F32)).all()
    _check_center(gpu_device, sig, finite=False, crafted=False)


# ----------------------------------------------------------------------------------------------------------------
# 3. fc_normalize
# ----------------------------------------------------------------------------------------------------------------
def _normalize_ref(c: np.ndarray, norms: np.ndarray) -> np.ndarray:
    n = norms.copy()
    n[n == 0.0] = 1.0
    return (c.astype(F32) / n.astype(F32)[:, None]).astype(F16)


def _normalize_input(K, D, seed):
    rng = np.random.default_rng(seed)
    c = (rng.normal(0, 1, size=(K, D)) * 10.0 ** rng.uniform(-3, 0, size=(K, 1))).astype(F16)
    zero = np.arange(K) % 3 == 1 if K > 2 else np.zeros(K, dtype=bool)
    zero[-1] = K > 1
    c[zero] = 0
    norms = np.sqrt((c.astype(F64) ** 2).sum(axis=1))  # (0 for the zero rows)
    assert (norms[zero] == 0).all() and (norms[~zero] > 0).all()
    return c, norms, zero


def test_normalize_more_rows_than_grid_rows(gpu_device):
    """K = 65540 > 65535 = gridDim.y: the kernel's row loop takes the last five rows (one of them a zero row)."""
    from fedscale_amd import cohort_signature as cs

    K, D = 65540, 5
    c, norms, zero = _normalize_input(K, D, 3)
    assert zero[-1] and not zero[-2]
    got = cs.normalize(torch.from_numpy(c).to(gpu_device), K, D, torch.from_numpy(norms).to(gpu_device)).cpu().numpy()
    _bits_equal(got, _normalize_ref(c, norms), "normalize K=65540")
    assert not got[zero].any()


@pytest.mark.parametrize("D", [2047, 2048, 2049, 6151])
def test_normalize_around_the_workgroup_width(gpu_device, D):
    """2048 columns per workgroup: one short, exact, one over, and three workgroups with a ragged end; the three
    layouts, and in place (normalized_out == centered, which include/fedcohort.h allows).  Whole buffers are
    compared: the padding columns keep their bits."""
    from fedscale_amd import _native_cohort as nc
    from fedscale_amd import cohort_signature as cs

    K = 3
    c, norms, zero = _normalize_input(K, D, D)
    want = _normalize_ref(c, norms)
    nd = torch.from_numpy(norms).to(gpu_device)
    for name, t in _layouts(c, gpu_device, pad=3.0):
        ctx = f"normalize D={D} {name}"
        got = cs.normalize(t, K, D, nd)[:, :D].cpu().numpy()
        _bits_equal(got, want, ctx)
        assert not got[zero].any(), ctx
        ld = t.stride(0)
        nc.call("fc_normalize", t.data_ptr(), ld, K, D, nd.data_ptr(), t.data_ptr(), cs._handle(t))  # in place
        after = t.cpu().numpy()
        _bits_equal(np.ascontiguousarray(after[:, :D]), want, f"{ctx} in place")
        assert (after[:, D:] == F16(3.0)).all(), f"{ctx} in place: padding columns were written"


# ----------------------------------------------------------------------------------------------------------------
# 4. fc_signature through hand-made segment tables
# ----------------------------------------------------------------------------------------------------------------
def _signature_case(dev, n, ld, ldd, segs, isegs, x, last, xi=None, last_i=None, last_off=0, ctx=""):
    """Run fc_signature on a sig_out filled with FILL and compare ALL of it: the covered elements with
    half((last - x) in fp32) / half(float64(wrapping int64 difference)), every other element with FILL."""
    from fedscale_amd import cohort_signature as cs

    D = max([d + l for _, d, l in segs if l > 0] + [d + 1 for _, d in isegs])
    assert D <= ldd and x.shape == (n, ld) and last.shape == (ld,)
    cover = np.zeros(ldd, dtype=np.int64)
    want = np.full((n, ldd), FILL, dtype=np.uint16).view(F16)
    with np.errstate(all="ignore"):
        for s, d, l in segs:
            assert 0 <= s and s + l <= ld and 0 <= d and d + l <= D
            cover[d:d + l] += 1
            want[:, d:d + l] = (last[s:s + l][None, :] - x[:, s:s + l]).astype(F16)
        for q, d in isegs:
            cover[d] += 1
            want[:, d] = (last_i[q] - xi[:, q]).astype(F64).astype(F16)
    assert cover.max() == 1 and (cover == 0).any(), "the table must leave part of the row uncovered, and not overlap"
    plan = cs.SignaturePlan(10 * D, D, segs, isegs)
    out = torch.full((n, ldd), FILL, dtype=torch.int16, device=dev).view(torch.float16)
    lbuf = torch.zeros(ld + last_off, dtype=torch.float32, device=dev)
    lbuf[last_off:] = torch.from_numpy(last).to(dev)
    xd = torch.from_numpy(x).to(dev)
    xid = torch.from_numpy(xi).to(dev) if xi is not None else None
    lid = torch.from_numpy(last_i).to(dev) if last_i is not None else None
    cs.signature(xd, xid, n, lbuf[last_off:], lid, plan, out)
    got = out.cpu().numpy()
    _bits_equal(got, want, ctx)
    return got


SIG_LENS = (1, 2, 3, 7, 8, 9, 11, 2047, 2048, 2049, 4101)
SIG_DST_MODS = (0, 1, 2, 4, 6, 7)


@pytest.mark.parametrize("ld_mod4,last_off", [(2, 0), (1, 0), (2, 1), (3, 3)])
def test_signature_alignment_and_length_grid(gpu_device, ld_mod4, last_off):
    """Every (length, source offset mod 4, destination offset mod 8) in one call of 264 segments (five launches):
    lengths around the 8-element group and the 2048-element chunk, the scalar prefix 0..3, the 16- / 4- / 2-byte
    store branches.  With ld odd the prefix and (with ldd odd) the store branch differ from row to row; ``last``
    starts 0, 4 or 12 bytes past a 16-byte boundary, so its 16-byte loads are taken for some segments and rows and
    not for others."""
    n = 5
    segs, s, d = [], 0, 0
    for i, (ln, sm, dm) in enumerate((ln, sm, dm) for ln in SIG_LENS for sm in range(4) for dm in SIG_DST_MODS):
        s += (sm - s) % 4
        d += (dm - d) % 8 + (8 if i % 3 == 0 else 0)
        segs.append((s, d, ln))
        s, d = s + ln, d + ln
    assert len(segs) == 264
    ld = s + (ld_mod4 - s) % 4
    ldd = _round_up(d + 1, 8) + (ld_mod4 % 2)
    assert ld % 4 == ld_mod4 and ldd % 2 == ld % 2
    rng = np.random.default_rng(ld_mod4 * 10 + last_off)
    x = rng.normal(0, 0.05, size=(n, ld)).astype(F32)
    last = rng.normal(0, 0.05, size=ld).astype(F32)
    _signature_case(gpu_device, n, ld, ldd, segs, [], x, last, last_off=last_off, ctx=f"grid ld%4={ld_mod4}")


def test_signature_more_segments_than_one_launch_takes(gpu_device):
    """130 non-empty short segments (three launches of at most 64) with zero-length entries among them, out of
    source order, and 130 int64 entries (three launches): every segment lands, nothing else is written."""
    n, nseg = 5, 130
    rng = np.random.default_rng(130)
    lens = rng.integers(1, 21, size=nseg)
    segs, s, d = [], 0, 0
    for i, ln in enumerate(lens.tolist()):
        if i % 13 == 5:
            segs.append((s, d, 0))  # an empty entry: skipped, and it does not count towards a launch's 64
        s += int(rng.integers(0, 6))
        d += int(rng.integers(0, 4))
        segs.append((s, d, ln))
        s, d = s + ln, d + ln
    segs.append((s, d, 0))
    assert sum(1 for seg in segs if seg[2] > 0) == nseg and sum(1 for seg in segs if seg[2] == 0) >= 10
    order = rng.permutation(len(segs))
    segs = [segs[i] for i in order]  # the binary search runs over workgroup starts, not over src or dst
    ldq = 150
    isegs = [(int(q), d + 1 + 2 * j) for j, q in enumerate(rng.permutation(ldq)[:130])]
    ld, ldd = s + 3, d + 1 + 2 * 130 + 5
    x = rng.normal(0, 0.05, size=(n, ld)).astype(F32)
    last = rng.normal(0, 0.05, size=ld).astype(F32)
    xi = rng.integers(-3000, 3000, size=(n, ldq)).astype(np.int64)
    last_i = rng.integers(-3000, 3000, size=ldq).astype(np.int64)
    _signature_case(gpu_device, n, ld, ldd, segs, isegs, x, last, xi, last_i, ctx="130 segments")


def test_signature_more_rows_than_grid_rows(gpu_device):
    """n = 65540 > 65535 = gridDim.y: the row loop of ``k_signature``; the int64 kernel indexes rows flat."""
    n, ld, ldd, ldq = 65540, 16, 16, 3
    rng = np.random.default_rng(65540)
    x = rng.normal(0, 0.05, size=(n, ld)).astype(F32)
    last = rng.normal(0, 0.05, size=ld).astype(F32)
    xi = rng.integers(-3000, 3000, size=(n, ldq)).astype(np.int64)
    last_i = rng.integers(-3000, 3000, size=ldq).astype(np.int64)
    got = _signature_case(gpu_device, n, ld, ldd, [(3, 1, 11)], [(0, 13), (2, 0)], x, last, xi, last_i, ctx="65540 rows")
    assert (got[-5:, 12].view(np.uint16) == FILL).all() and (got[-5:, 1:12].view(np.uint16) != FILL).all()


def test_signature_special_values(gpu_device):
    """What tests/golden/auxo_sig_values_k6 holds (subnormals, ties at the bottom, exact ties, the float16 range and
    beyond) and more: differences that round up to the smallest subnormal and down to zero, +-65520 (the first
    value that overflows), int64 differences of +-2^24 and +-(2^24 + 1) (not exact in fp32), int64 ties, and a
    wrapping int64 subtraction."""
    sub = 2.0 ** -24
    vals = np.asarray([
        sub, 3 * sub, 0.5 * sub, 1.5 * sub, 2.5 * sub, 1023 * sub,
        -sub, -0.5 * sub, 0.49 * sub, 2.0 ** -14, 2.0 ** -14 - sub, 2.0 ** -15,
        1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2048 + 1, 2048 + 3, 0.1,
        1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -24, 1e-3, -1e-3, 3.1415927, -2.7182817,
        65504.0, 65519.996, 65520.0, 1e5, -65520.0, -7e4,
        -65519.996, 3e38, -3e38, 65536.0, 4e4, -4e4,
        0.5 * sub * (1 + 2.0 ** -23), 0.5 * sub * (1 - 2.0 ** -24), -0.5 * sub * (1 + 2.0 ** -23), 0.51 * sub,
        -1.5 * sub, -2.5 * sub, 1023.5 * sub, 1024 * sub - 0.5 * sub, 0.0, -0.0,
        4096 + 2, 4096 + 6, -(4096 + 2), 32768 + 16, 32768 + 48, 65504 + 15.996,
    ], dtype=F64).astype(F32)
    n, M = 6, len(vals)
    x = np.stack([-np.roll(vals, k) for k in range(n)])           # last = 0: the difference is vals, exactly
    x = np.concatenate([x, x - F32(1.0)], axis=1).astype(F32)     # last = -1 there: (-1) - (x - 1), one rounding
    last = np.concatenate([np.zeros(M, dtype=F32), np.full(M, -1.0, dtype=F32)])
    with np.errstate(all="ignore"):
        want0 = (last[None, :M] - x[:, :M]).astype(F16)
    assert np.isinf(want0.astype(F32)).any() and (want0.view(np.uint16) == 1).any() and (want0 == 0).any()
    assert not np.isnan(want0.astype(F32)).any()
    di = np.asarray([1 << 24, -(1 << 24), (1 << 24) + 1, -(1 << 24) - 1, 2049, 2051, -2049, -2051, 2048, 0, 1, -1,
                     65504, 65519, 65520, -65520, (1 << 62), -(1 << 63)], dtype=np.int64)
    Q = len(di)
    last_i = np.asarray([0, 5, -7, 100000, (1 << 63) - 1, -(1 << 63)] * 3, dtype=np.int64)[:Q]
    xi = np.stack([last_i - np.roll(di, k) for k in range(n)])    # wraps where last_i - di leaves the int64 range
    assert ((last_i[None, :] - xi) == np.stack([np.roll(di, k) for k in range(n)])).all()
    segs = [(0, 3, M), (M, 3 + M + 2, M)]
    isegs = [(q, 3 + 2 * M + 4 + q) for q in range(Q)]
    ld, ldd = 2 * M, 3 + 2 * M + 4 + Q + 3
    _signature_case(gpu_device, n, ld, ldd, segs, isegs, x, last, xi, last_i, ctx="special values")


# ----------------------------------------------------------------------------------------------------------------
# 5. guards past the declared extent
# ----------------------------------------------------------------------------------------------------------------
GUARD = 256


class _Guarded:
    """``nbytes`` of device memory with GUARD bytes of 0xA5 before and after it (and 0xA5 inside, to begin with)."""

    def __init__(self, dev, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def check(self, ctx, dtype):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == 0xA5).all(), f"{ctx}: written before its start"
        assert (b[GUARD + self.nbytes:] == 0xA5).all(), f"{ctx}: written past its declared extent"
        return b[GUARD:GUARD + self.nbytes].copy().view(dtype)


def test_kernels_leave_memory_past_the_declared_extents_alone(gpu_device):
    """K = 7, D = 203, row stride 203 (element-wise paths, nothing aligned): every output of fc_center,
    fc_normalize and fc_gram sits between guards and ends exactly at the extent include/fedcohort.h declares —
    ((K - 1) * ldd + D) float16, D for avg16_out, K doubles for sumsq_out, K * K floats for the Gram."""
    from fedscale_amd import _native_cohort as nc
    from fedscale_amd import cohort_signature as cs

    K, D = 7, 203
    ldd = D
    rng = np.random.default_rng(12)
    sig = (rng.normal(0, 1, size=(K, D)) * 10.0 ** rng.uniform(-4, 1, size=(1, D))).astype(F16)
    avg, cen = _center_ref(sig)
    lib = nc.load()
    sd = torch.from_numpy(sig).to(gpu_device)
    st = cs._handle(sd)
    mbytes = ((K - 1) * ldd + D) * 2
    g_avg, g_cen, g_ss = _Guarded(gpu_device, D * 2), _Guarded(gpu_device, mbytes), _Guarded(gpu_device, K * 8)
    ws = torch.empty(lib.fc_center_workspace_bytes(K, D) // 8, dtype=torch.float64, device=gpu_device)
    nc.call("fc_center", sd.data_ptr(), ldd, K, D, g_avg.ptr, g_cen.ptr, g_ss.ptr, ws.data_ptr(), st)
    torch.cuda.synchronize()
    _bits_equal(g_avg.check("avg16_out", F16), avg, "guarded mean")
    got_cen = g_cen.check("centered_out", F16).reshape(K, D)
    _bits_equal(got_cen, cen, "guarded centred")
    want_ss = (cen.astype(F64) ** 2).sum(axis=1)
    got_ss = g_ss.check("sumsq_out", F64)
    assert (np.abs(got_ss - want_ss) <= D * 2.0 ** -52 * want_ss).all()

    norms = np.sqrt(got_ss)
    nd = torch.from_numpy(norms).to(gpu_device)
    g_nrm = _Guarded(gpu_device, mbytes)
    nc.call("fc_normalize", g_cen.ptr, ldd, K, D, nd.data_ptr(), g_nrm.ptr, st)
    torch.cuda.synchronize()
    _bits_equal(g_nrm.check("normalized_out", F16).reshape(K, D), _normalize_ref(cen, norms), "guarded normalized")
    g_cen.check("centered (read only)", F16)

    g_gram = _Guarded(gpu_device, K * K * 4)
    wsg = torch.empty(max(4, lib.fc_gram_workspace_bytes(K, D) // 4), dtype=torch.float32, device=gpu_device)
    nc.call("fc_gram", g_cen.ptr, ldd, K, D, g_gram.ptr, wsg.data_ptr(), st)
    torch.cuda.synchronize()
    _gram_check(cen, g_gram.check("gram_out", F32).reshape(K, K), True, "guarded gram")
    g_cen.check("c (read only)", F16)
