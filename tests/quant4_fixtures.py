"""A numpy restatement of the MXFP4 delta-upload contract (include/fedquant4.h), independent of the product code.
Codes are kept one per column here; ``pack`` gives the wire's two-to-a-byte layout."""
import numpy as np

BLOCK = 32
F32 = np.float32
POS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])  # magnitudes of codes 0..7: s eem
TABLE = np.concatenate([POS, -POS])                        # value of every code (code 8 is -0), float64
MID = (POS[:-1] + POS[1:]) / 2.0                           # the seven tie points


def blocks(P: int) -> int:
    return (int(P) + BLOCK - 1) // BLOCK


def pack(codes: np.ndarray) -> np.ndarray:
    """Column 2i in the low nibble of byte i, column 2i + 1 in its high nibble."""
    return (codes[0::2] | (codes[1::2] << 4)).astype(np.uint8)


def quantize(d: np.ndarray):
    """(codes [round_up(P, 32)], scales [ceil(P / 32)], residual [P]) of ``d``, the update plus any residual."""
    d = np.ascontiguousarray(d, dtype=F32)
    P, NB = d.size, blocks(d.size)
    pad = np.zeros(NB * BLOCK, dtype=F32)
    pad[:P] = d
    codes, s = np.zeros(NB * BLOCK, dtype=np.uint8), np.zeros(NB, dtype=np.uint8)
    res = np.zeros(NB * BLOCK, dtype=F32)
    for b in range(NB):
        blk = pad[b * BLOCK:(b + 1) * BLOCK]
        am = int((blk.view(np.uint32) & 0x7FFFFFFF).max())
        E, M = am >> 23, am & 0x7FFFFF
        if E == 0xFF:  # an infinity or a NaN: the block is poisoned, its codes and residual are 0
            s[b] = 255
            continue
        s[b] = min(max(E - 2 + (1 if M > 0x400000 else 0), 2), 252)
        with np.errstate(under="ignore", over="ignore"):
            v = np.clip(blk * np.ldexp(F32(1.0), 127 - int(s[b])), F32(-6.0), F32(6.0))  # fp32 product
        a = np.abs(v.astype(np.float64))
        lo = np.searchsorted(MID, a, side="left")  # a <= MID[lo]: below the midpoint lo, at it the even of lo, lo + 1
        tie = (lo < MID.size) & (a == MID[np.minimum(lo, MID.size - 1)])
        lo[tie] += lo[tie] & 1
        c = (lo | (np.signbit(v) << 3)).astype(np.uint8)
        codes[b * BLOCK:(b + 1) * BLOCK] = c
        res[b * BLOCK:(b + 1) * BLOCK] = blk - (TABLE[c] * np.ldexp(1.0, int(s[b]) - 127)).astype(F32)
    return codes, s, res[:P]


def dequantize(codes: np.ndarray, s: np.ndarray, P: int = None) -> np.ndarray:
    """float32 [P]: value(code) * 2^(s - 127), exact for s in 2..252; any other scale byte makes the block NaN."""
    n = codes.size if P is None else P
    sb = np.repeat(s.astype(np.int64), BLOCK)[:n]
    prod = TABLE[codes[:n]] * np.ldexp(1.0, sb - 127)
    prod[(sb < 2) | (sb > 252)] = np.nan
    out = prod.astype(F32)
    assert np.array_equal(out.astype(np.float64)[~np.isnan(prod)], prod[~np.isnan(prod)])  # exact
    return out


def chain(rows, acc=None, P: int = None) -> np.ndarray:
    """acc (or +0) + deq_0 + deq_1 + ... as sequential np.float32 adds; ``rows``: (codes, scales) pairs."""
    P = P if P is not None else (acc.size if acc is not None else rows[0][0].size)
    c = np.zeros(P, dtype=F32) if acc is None else acc[:P].astype(F32).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for codes, s in rows:
            c = (c + dequantize(codes, s, P)).astype(F32, copy=False)
    return c


def contract_cases() -> dict:
    """name -> float32 delta vector: the cases the contract lists."""
    rng = np.random.default_rng(20264)
    c = {}
    ties = np.concatenate([[6.0], MID, -MID, [0.0, -0.0], np.zeros(BLOCK - 17)]).astype(F32)  # amax 6: scale 127
    up, down = ties.copy(), ties.copy()
    up[1:15], down[1:15] = np.nextafter(ties[1:15], F32(np.inf)), np.nextafter(ties[1:15], F32(-np.inf))
    c["ties"] = np.concatenate([ties, up, down, ties * F32(2.0 ** 40), ties * F32(2.0 ** -90)])
    small = (rng.uniform(-1, 1, BLOCK) * 0.7 * 2.0 ** -20).astype(F32)
    a, b = small.copy(), small.copy()
    a[5], b[7] = F32(1.5 * 2.0 ** -20), -np.nextafter(F32(1.5 * 2.0 ** -20), F32(np.inf))
    c["amax_at_1.5"], c["amax_one_ulp_above_1.5"] = a, b
    tiny = np.zeros(BLOCK, dtype=F32)
    tiny[[3, 9, 10, 11, 12]] = [1.5 * 2.0 ** -126, -2.0 ** -127, 2.0 ** -149, 3 * 2.0 ** -128, -0.0]
    c["low_clamp"] = tiny
    big = (rng.uniform(-1, 1, BLOCK) * 3e38).astype(F32)
    big[0], big[1] = np.finfo(F32).max, -np.finfo(F32).max
    c["high_clamp"] = big
    for name, at, v in (("nan_block_between_finite_blocks", BLOCK + 4, np.nan), ("inf_block", 3 * BLOCK - 1, -np.inf)):
        c[name] = rng.standard_normal(3 * BLOCK).astype(F32)
        c[name][at] = v
    exps = np.arange(-140, 127, 3)
    with np.errstate(under="ignore"):
        c["random_binades"] = (rng.standard_normal((exps.size, BLOCK)) * np.ldexp(1.0, exps)[:, None]).astype(
            F32).reshape(-1)
    for P in (1, 31, 33, 4099):  # no multiples of 32 or 8
        c[f"P={P}"] = (rng.standard_normal(P) * 10.0 ** rng.uniform(-3, 3)).astype(F32)
    return c
