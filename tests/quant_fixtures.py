"""A numpy restatement of the MXFP8 delta-upload contract (include/fedquant.h), written from the format's definition
and independent of the product code: the 256-entry e4m3fn table, the scale rule on integer bit fields, rounding by
comparison against the sorted table (not torch's cast), the exact dequantisation, the in-order fp32 chain and the
finish.  Test infrastructure, shared by the CPU and GPU tests of the path."""
import numpy as np

BLOCK = 32
F32 = np.float32


def _e4m3_value(code: int) -> float:
    """OCP e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities; S.1111.111 is NaN."""
    sign = -1.0 if code & 0x80 else 1.0
    e, m = (code >> 3) & 0xF, code & 0x7
    if e == 0xF and m == 0x7:
        return float("nan")
    if e == 0:
        return sign * (m / 8.0) * 2.0 ** -6
    return sign * (1.0 + m / 8.0) * 2.0 ** (e - 7)


#: value of every code, float64 (exact)
TABLE = np.asarray([_e4m3_value(c) for c in range(256)], dtype=np.float64)
#: the non-negative finite values in code order 0x00 .. 0x7E: strictly increasing, 0 .. 448
POS = TABLE[:0x7F].copy()
assert POS[0] == 0.0 and POS[1] == 2.0 ** -9 and POS[-1] == 448.0 and np.all(np.diff(POS) > 0)
_MID = (POS[:-1] + POS[1:]) / 2.0  # exact in float64


def blocks(P: int) -> int:
    return (int(P) + BLOCK - 1) // BLOCK


def scale_bytes(d: np.ndarray) -> np.ndarray:
    """The scale byte of every block of the float32 vector ``d`` (the last block may be partial), on bit fields."""
    P = d.size
    NB = blocks(P)
    bits = np.zeros(NB * BLOCK, dtype=np.uint32)
    bits[:P] = np.ascontiguousarray(d, dtype=F32).view(np.uint32) & 0x7FFFFFFF
    out = np.zeros(NB, dtype=np.uint8)
    for b in range(NB):
        am = int(bits[b * BLOCK:(b + 1) * BLOCK].max())
        E, M = am >> 23, am & 0x7FFFFF
        if E == 0xFF:  # an infinity (M == 0) or a NaN in the block
            out[b] = 255
        else:
            out[b] = min(max(E - 8 + (1 if M > 0x600000 else 0), 10), 246)
    return out


def round_e4m3(v: np.ndarray) -> np.ndarray:
    """Codes of the finite float32 values ``v`` in [-448, 448]: nearest table value, ties to the even code, the sign
    bit kept (so -0 and a negative value that rounds to zero give 0x80)."""
    a = np.abs(v.astype(np.float64))
    assert np.all(a <= 448.0)
    lo = np.searchsorted(_MID, a, side="left")  # a <= _MID[lo]: candidates lo (below the midpoint) and lo + 1
    idx = lo.copy()
    tie = (lo < _MID.size) & (a == _MID[np.minimum(lo, _MID.size - 1)])
    idx[tie] = lo[tie] + (lo[tie] & 1)  # of lo and lo + 1, the even one
    return (idx.astype(np.uint8) | (np.signbit(v).astype(np.uint8) << 7)).astype(np.uint8)


def quantize(d: np.ndarray):
    """(codes uint8 [round_up(P, 32)], scales uint8 [ceil(P / 32)]) of the float32 delta vector ``d``.  Codes of a
    block with scale 255 are unspecified by the contract; 0 here."""
    d = np.ascontiguousarray(d, dtype=F32)
    P, NB = d.size, blocks(d.size)
    s = scale_bytes(d)
    pad = np.zeros(NB * BLOCK, dtype=F32)
    pad[:P] = d
    codes = np.zeros(NB * BLOCK, dtype=np.uint8)
    for b in range(NB):
        if s[b] == 255:
            continue
        mul = np.ldexp(F32(1.0), 127 - int(s[b]))  # a normal fp32 for s in 10..246
        assert mul.dtype == F32
        with np.errstate(under="ignore"):
            v = pad[b * BLOCK:(b + 1) * BLOCK] * mul  # fp32 product
        v = np.minimum(np.maximum(v, F32(-448.0)), F32(448.0))
        codes[b * BLOCK:(b + 1) * BLOCK] = round_e4m3(v)
    return codes, s


def dequantize(codes: np.ndarray, s: np.ndarray, P: int = None) -> np.ndarray:
    """float32 [P]: value(code) * 2^(s - 127) as the fp32 product rounded to nearest (float64 holds the product
    exactly; the cast rounds once); scale 255 makes the block NaN."""
    n = codes.size if P is None else P
    sb = np.repeat(s.astype(np.int64), BLOCK)[:n]
    prod = TABLE[codes[:n]] * np.ldexp(1.0, sb - 127)
    prod[sb == 255] = np.nan
    with np.errstate(over="ignore", invalid="ignore"):
        return prod.astype(F32)


def chain(rows, acc=None, P: int = None) -> np.ndarray:
    """acc (or +0) + deq_0 + deq_1 + ... in fp32, in order; ``rows``: (codes, scales) pairs."""
    rows = list(rows)
    P = P if P is not None else (acc.size if acc is not None else rows[0][0].size)
    c = np.zeros(P, dtype=F32) if acc is None else acc[:P].astype(F32).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for codes, s in rows:
            c = (c + dequantize(codes, s, P)).astype(F32)
    return c


def finish(L: np.ndarray, c: np.ndarray, K: int) -> np.ndarray:
    """L + chain / float(K), fp32."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (L.astype(F32) + (c / F32(K)).astype(F32)).astype(F32)


def error_bound_holds(d: np.ndarray, codes: np.ndarray, s: np.ndarray) -> bool:
    """|deq - d| <= max(|d| 2^-4, 2^(s - 137)) on every element of a block with s < 246 (half an e4m3 ulp of a
    normal code is at most 2^-4 of the value; half the subnormal spacing 2^-9 at scale s is 2^(s - 137))."""
    P = d.size
    sb = np.repeat(s.astype(np.int64), BLOCK)[:P]
    keep = sb < 246
    deq = dequantize(codes, s, P).astype(np.float64)
    dd = d.astype(np.float64)
    bound = np.maximum(np.abs(dd) * 2.0 ** -4, np.ldexp(1.0, sb - 137))
    return bool(np.all(np.abs(deq - dd)[keep] <= bound[keep]))


# ---- the contract's edge cases, as delta vectors ---------------------------------------------------------------------
def _with_amax(vals, amax=448.0):
    """Blocks of 32 holding ``vals`` in order, each block's first element ``amax`` (which pins the block's scale)."""
    vals = np.asarray(vals, dtype=np.float64)
    out = []
    for i in range(0, vals.size, BLOCK - 1):
        blk = np.zeros(BLOCK)
        blk[0] = amax
        part = vals[i:i + BLOCK - 1]
        blk[1:1 + part.size] = part
        out.append(blk)
    return np.concatenate(out).astype(F32)


def contract_cases() -> dict:
    """name -> float32 delta vector: the cases the contract lists."""
    rng = np.random.default_rng(20260)
    c = {}
    exps = np.arange(-140, 125)
    with np.errstate(under="ignore"):
        c["random_binades"] = (rng.standard_normal((exps.size, BLOCK)) * np.ldexp(1.0, exps)[:, None]).astype(
            F32).reshape(-1)
    c["zero_block"] = np.zeros(BLOCK, dtype=F32)
    c["negative_zero_block"] = np.full(BLOCK, -0.0, dtype=F32)
    top = F32(448.0 * 2.0 ** -20)
    small = (rng.uniform(-1, 1, BLOCK) * float(top) * 0.9).astype(F32)
    a, b = small.copy(), small.copy()
    a[5], b[7] = top, -np.nextafter(top, F32(np.inf))
    c["amax_at_448_threshold"] = a
    c["amax_just_above_448_threshold"] = b
    c["ties"] = _with_amax(np.concatenate([_MID, -_MID]))
    c["subnormal_codes"] = _with_amax(np.concatenate([np.arange(0, 17) * 2.0 ** -10, -np.arange(0, 17) * 2.0 ** -10,
                                                      rng.uniform(-2.0 ** -6, 2.0 ** -6, 60)]))
    tiny = np.zeros(BLOCK, dtype=F32)
    tiny[3], tiny[9], tiny[10] = F32(1.5 * 2.0 ** -128), F32(-2.0 ** -130), F32(2.0 ** -149)
    c["amax_below_2^-127"] = tiny
    big = (rng.uniform(-1, 1, BLOCK) * 1e38).astype(F32)
    big[0], big[1] = np.finfo(F32).max, -np.finfo(F32).max
    c["amax_flt_max"] = big
    nan = rng.standard_normal(3 * BLOCK).astype(F32)
    nan[BLOCK + 4] = np.nan
    c["nan_block_between_finite_blocks"] = nan
    inf = rng.standard_normal(3 * BLOCK).astype(F32)
    inf[2 * BLOCK + 31] = -np.inf
    c["inf_block"] = inf
    for P in (1, 31, 32, 33, 95):
        c[f"P={P}"] = (rng.standard_normal(P) * 10.0 ** rng.uniform(-3, 3)).astype(F32)
    return c


# ---- fq_reduce's launch plan, restated (strip_plan of fedscale_amd/csrc/fa_common.h with FQ_GEO of quant_reduce.hip) --
WAVES = 4
LEVELS = ((8, 4), (4, 4), (1, 8))  # (V, U) of levels 0, 1, 2
CAP_PCT = 75
STRIP = 1024  # columns of one strip: 64 lanes x 16 columns


def strips(P: int) -> int:
    return ((P + 15) // 16 + 63) // 64


def plan(cus: int, K: int, P: int) -> list:
    """The launches of fq_reduce at (K, P) on ``cus`` compute units: dicts V, U, col0, tiles, sw, grid."""
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
    """One width just past each tile or level seam of a plan: the first column of every launch after the first, of the
    second tile of every launch, and of the second strip — plus one, so that a lone column sits past the seam."""
    out = set()
    for l in launches:
        tile = WAVES * l["sw"] * STRIP
        for seam in (l["col0"], l["col0"] + tile, l["col0"] + STRIP):
            if seam > 0:
                out.add(seam + 1)
    return sorted(out)


def random_rows(rng, K: int, P: int, binades: int = 40):
    """K rows of (codes [round_up(P, 32)], scales [ceil(P / 32)]) whose block magnitudes are mixed over ``binades``
    binades, so that the fp32 sum of a column depends on the order; finite codes only."""
    NB = blocks(P)
    rows = []
    for _ in range(K):
        codes = rng.integers(0, 256, NB * BLOCK).astype(np.uint8)
        codes[(codes & 0x7F) == 0x7F] = 0x3A  # no NaN codes
        s = rng.integers(127 - binades // 2, 127 + binades // 2, NB).astype(np.uint8)
        rows.append((codes, s))
    return rows
