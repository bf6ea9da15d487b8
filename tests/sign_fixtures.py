"""A numpy restatement of the 1-bit sign delta-upload contract (include/fedsign.h), written from the contract's text
and independent of the product code: the encode with its fixed fp64 add order (block by block, lane by lane), the
exact dequantisation, the in-order fp32 chain, the finish, and fsg_reduce's launch plan.  Test infrastructure, shared
by the CPU and GPU tests of the path.  All parity against it is bit for bit."""
import numpy as np

BLOCK = 256
F32 = np.float32
NAN_SCALE_BITS = 0x7FC00000


def blocks(P: int) -> int:
    return (int(P) + BLOCK - 1) // BLOCK


def bit_bytes(P: int) -> int:
    return (int(P) + 7) // 8


def bit_stride(P: int) -> int:
    return (bit_bytes(P) + 15) // 16 * 16


def scale_stride(P: int) -> int:
    return (blocks(P) + 3) // 4 * 4


def delta(x, L=None, r=None) -> np.ndarray:
    """Step 1: e = (x - L) + r in fp32, two roundings; either of L and r may be missing."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.asarray(x, dtype=F32)
        if L is not None:
            e = (e - np.asarray(L, dtype=F32)).astype(F32)
        if r is not None:
            e = (e + np.asarray(r, dtype=F32)).astype(F32)
    return e.copy()


def block_scale(blk: np.ndarray) -> np.float32:
    """Step 3 for one block of n_b = blk.size existing columns: python floats are fp64, every + is one IEEE add."""
    n_b = blk.size
    a = [0.0] * BLOCK
    for i in range(n_b):
        a[i] = abs(float(blk[i]))
    t = [((a[l] + a[l + 64]) + a[l + 128]) + a[l + 192] for l in range(64)]
    for m in (32, 16, 8, 4, 2, 1):
        t = [t[l] + t[l ^ m] for l in range(64)]
    return F32(t[0] / float(n_b))


def encode(e: np.ndarray):
    """(bits uint8 [ceil(P / 8)], scales float32 [ceil(P / 256)], residual_out float32 [P]) of the float32 vector e:
    steps 2 to 5."""
    e = np.ascontiguousarray(e, dtype=F32)
    P, NB = e.size, blocks(e.size)
    u = e.view(np.uint32)
    bits = np.zeros(bit_bytes(P), dtype=np.uint8)
    scales = np.zeros(NB, dtype=F32)
    res = np.zeros(P, dtype=F32)
    for b in range(NB):
        lo, hi = b * BLOCK, min(P, (b + 1) * BLOCK)
        blk = e[lo:hi]
        if not np.isfinite(blk).all():
            scales[b:b + 1].view(np.uint32)[0] = NAN_SCALE_BITS
            continue  # all-zero bits, +0.0 residual
        s = block_scale(blk)
        scales[b] = s
        for p in range(lo, hi):
            neg = (int(u[p]) >> 31) & 1
            if neg:
                bits[p // 8] |= np.uint8(1 << (p % 8))
            deq = -s if neg else s
            with np.errstate(over="ignore"):
                res[p] = F32(e[p] - deq)
    return bits, scales, res


def encode_fast(e: np.ndarray):
    """``encode`` for large vectors: the same steps over whole arrays (checked against ``encode`` by the CPU tests)."""
    e = np.ascontiguousarray(e, dtype=F32)
    P, NB = e.size, blocks(e.size)
    pad = np.zeros(NB * BLOCK, dtype=F32)
    pad[:P] = e
    neg = (pad.view(np.uint32) >> 31).astype(np.uint8)
    a = np.abs(pad.astype(np.float64)).reshape(NB, 4, 64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]
        for m in (32, 16, 8, 4, 2, 1):
            t = t + t[:, np.arange(64) ^ m]
        n_b = np.full(NB, 256.0)
        if NB:
            n_b[-1] = P - BLOCK * (NB - 1)
        scales = (t[:, 0] / n_b).astype(F32)
    bad = ~np.isfinite(pad.reshape(NB, BLOCK)).all(axis=1)
    scales.view(np.uint32)[bad] = NAN_SCALE_BITS
    neg[np.repeat(bad, BLOCK)] = 0
    sc = np.repeat(scales, BLOCK)[:P]
    with np.errstate(invalid="ignore", over="ignore"):
        res = (e - np.where(neg[:P] != 0, -sc, sc)).astype(F32)
    res[np.repeat(bad, BLOCK)[:P]] = 0.0
    return np.packbits(neg, bitorder="little")[:bit_bytes(P)], scales, res


def dequantize(bits: np.ndarray, scales: np.ndarray, P: int) -> np.ndarray:
    """float32 [P]: the block's scale with its sign bit xor the column's bit — exact, NaN scales included."""
    bit = np.unpackbits(np.asarray(bits, dtype=np.uint8), bitorder="little")[:P].astype(np.uint32)
    sb = np.repeat(np.ascontiguousarray(scales, dtype=F32).view(np.uint32), BLOCK)[:P]
    return (sb ^ (bit << np.uint32(31))).view(F32)


def chain(rows, acc=None, P: int = None) -> np.ndarray:
    """acc (or +0) + deq_0 + deq_1 + ... in fp32, in order; ``rows``: (bits, scales) pairs."""
    rows = list(rows)
    c = np.zeros(P, dtype=F32) if acc is None else np.asarray(acc[:P], dtype=F32).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for bits, scales in rows:
            c = (c + dequantize(bits, scales, P)).astype(F32)
    return c


def finish(L: np.ndarray, c: np.ndarray, K: int) -> np.ndarray:
    """L + chain / float(K), fp32."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (L.astype(F32) + (c / F32(K)).astype(F32)).astype(F32)


def same(got, want, ctx=None):
    """Bit equality; where the expectation is NaN, a NaN (its payload is the adder's)."""
    g, w = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    assert g.shape == w.shape, ctx
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), ctx
    assert np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan]), ctx


# ---- the contract's edge cases, as update vectors -------------------------------------------------------------------
def contract_cases() -> dict:
    """name -> float32 vector e: the cases the contract lists."""
    rng = np.random.default_rng(20261)
    c = {}
    exps = np.arange(-140, 120, 7)
    with np.errstate(under="ignore"):
        c["random_binades"] = (rng.standard_normal((exps.size, BLOCK)) * np.ldexp(1.0, exps)[:, None]).astype(
            F32).reshape(-1)
    z = rng.standard_normal(2 * BLOCK).astype(F32)
    z[5], z[BLOCK + 9] = -0.0, -0.0
    z[6] = 0.0
    c["negative_zero"] = z
    zb = rng.standard_normal(3 * BLOCK).astype(F32)
    zb[BLOCK:2 * BLOCK] = 0.0
    zb[BLOCK + 3] = -0.0
    c["zero_block"] = zb
    nan = rng.standard_normal(3 * BLOCK).astype(F32)
    nan[BLOCK + 200] = np.nan
    c["nan_block_between_finite_blocks"] = nan
    inf = rng.standard_normal(3 * BLOCK).astype(F32)
    inf[2 * BLOCK + 255] = -np.inf
    c["inf_block"] = inf
    big = (rng.uniform(-1, 1, BLOCK) * 3e38).astype(F32)
    big[0], big[255] = np.finfo(F32).max, -np.finfo(F32).max
    c["flt_max"] = big
    tiny = np.zeros(BLOCK, dtype=F32)
    tiny[3], tiny[70], tiny[255] = F32(2.0 ** -149), F32(-2.0 ** -140), F32(2.0 ** -130)
    c["subnormal_scale"] = tiny
    for P in (1, 7, 8, 9, 255, 256, 257, BLOCK + 1, 2 * BLOCK + 255):
        c[f"P={P}"] = (rng.standard_normal(P) * 10.0 ** rng.uniform(-3, 3)).astype(F32)
    return c


# ---- fsg_reduce's launch plan, restated (strip_plan of fedscale_amd/csrc/fa_common.h with FSG_GEO of sign_reduce.hip)
WAVES = 4
LEVELS = ((1, 8), (1, 8), (1, 8))  # (V, U) of levels 0, 1, 2
U = 8
CAP_PCT = 600
STRIP = 2048  # columns of one strip: 64 lanes x 32 columns


def strips(P: int) -> int:
    return ((P + 31) // 32 + 63) // 64


def plan(cus: int, K: int, P: int) -> list:
    """The launches of fsg_reduce at (K, P) on ``cus`` compute units: dicts V, U, col0, tiles, sw, grid."""
    if P <= 0 or cus <= 0:
        return []
    S = strips(P)
    cap = max(1, cus * CAP_PCT // 100)
    span = [WAVES * v for v, _ in LEVELS]

    def launch(level, strip0, tiles, grid):
        v, u = LEVELS[level]
        return dict(V=v, U=u, col0=strip0 * STRIP, tiles=tiles, sw=v, grid=grid)

    t0 = (S + span[0] - 1) // span[0]
    if t0 * 100 >= cap * 85:
        rounds = (t0 + cap - 1) // cap
        return [launch(0, 0, t0, (t0 + rounds - 1) // rounds)]
    out, s = [], 0
    n1 = S // span[1]
    if n1 > 0 and 2 * n1 >= cus:
        out.append(launch(1, 0, n1, n1))
        s = n1 * span[1]
    if s < S:
        t2 = (S - s + span[2] - 1) // span[2]
        out.append(launch(2, s, t2, t2))
    return out


def seam_widths(launches, P: int) -> list:
    """Widths one column short of, at, and one column past each tile or level seam of a plan: the first column of
    every launch after the first, of the second tile of every launch, and of the second strip."""
    out = set()
    for l in launches:
        tile = WAVES * l["sw"] * STRIP
        for seam in (l["col0"], l["col0"] + tile, l["col0"] + STRIP):
            if seam > 0:
                out |= {seam - 1, seam, seam + 1}
    return sorted(out)


def random_rows(rng, K: int, P: int, binades: int = 40):
    """K rows of (bits [ceil(P / 8)], scales [ceil(P / 256)]) whose block scales are mixed over ``binades`` binades,
    so that the fp32 sum of a column depends on the order; finite scales; the last byte's padding bits are 0."""
    NB, PB = blocks(P), bit_bytes(P)
    rows = []
    for _ in range(K):
        bits = rng.integers(0, 256, PB).astype(np.uint8)
        if P % 8:
            bits[-1] &= np.uint8((1 << (P % 8)) - 1)
        s = (rng.uniform(1.0, 2.0, NB) * np.ldexp(1.0, rng.integers(-binades // 2, binades // 2, NB))).astype(F32)
        rows.append((bits, s))
    return rows
