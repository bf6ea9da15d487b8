"""Shared by the trimmed-mean tests: the arithmetic of include/fedtrim.h restated in numpy (order keys, selection,
the kept rule walked in arrival order, chain, mean, per-row drop counts), ``ft_plan`` restated in Python (strip_plan
of fedscale_amd/csrc/fa_common.h with the two geometries of trim_reduce.hip), and the shapes the GPU tests run as a
function of the CU count, with the plan each is meant to hit."""
import numpy as np

# constants of trim_reduce.hip
WAVES = 4
STRIP = 256  # columns of one strip: 64 lanes x 4 columns
DEPTHS = (1, 2, 4, 8, 16)  # the instantiated selection depths T
MAX_TRIM = 16
NARROW = dict(levels=((4, 2), (2, 4), (1, 8)), cap_pct=200)  # (V, U) of levels 0, 1, 2: T <= 4 and the reduce
DEEP = dict(levels=((1, 4), (1, 4), (1, 4)), cap_pct=300)    # T >= 8
LDS_ROWS = 4096  # above it the drop counts go straight to the table


# ---- the arithmetic ------------------------------------------------------------------------------------------------
def keys_of(x: np.ndarray) -> np.ndarray:
    """The unsigned order key of every fp32 value."""
    assert x.dtype == np.float32
    b = np.ascontiguousarray(x).view(np.uint32)
    k = np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(x)] = np.uint32(0xFFFFFFFF)
    return k


def select_of(x: np.ndarray, t: int):
    """(lo, hi, ties) of the [K, P] rows, uint32 each: the t-th smallest and largest key of every column and
    n_lo | n_hi << 16, the rows EQUAL to lo / hi that are dropped."""
    K = x.shape[0]
    assert 1 <= t and 2 * t < K
    key = keys_of(x)
    lo = np.partition(key, t - 1, axis=0)[t - 1]
    hi = np.partition(key, K - t, axis=0)[K - t]
    n_lo = t - (key < lo).sum(axis=0)
    n_hi = t - (key > hi).sum(axis=0)
    assert n_lo.min(initial=1) >= 1 and n_lo.max(initial=1) <= t and n_hi.min(initial=1) >= 1 and \
        n_hi.max(initial=1) <= t
    return lo, hi, (n_lo | (n_hi << 16)).astype(np.uint32)


def reduce_of(x: np.ndarray, t: int, lo=None, hi=None, ties=None):
    """(out, dropped, kept): the trimmed mean of every column (fp32), the int64 [K, 2] per-row drop counts, and the
    bool [K, P] kept set — the kept rule walked over the rows in arrival order."""
    assert x.dtype == np.float32
    K, P = x.shape
    kept = np.ones((K, P), dtype=bool)
    dropped = np.zeros((K, 2), dtype=np.int64)
    chain = np.zeros(P, dtype=np.float32)
    started = np.zeros(P, dtype=bool)
    if t > 0:
        key = keys_of(x)
        n_lo = (ties & 0xFFFF).astype(np.int64)
        n_hi = (ties >> 16).astype(np.int64)
    with np.errstate(all="ignore"):
        for k in range(K):
            if t > 0:
                tie_lo = (key[k] == lo) & (n_lo > 0)
                low = (key[k] < lo) | tie_lo
                n_lo -= tie_lo
                tie_hi = ~low & (key[k] == hi) & (n_hi > 0)
                high = ~low & ((key[k] > hi) | tie_hi)
                n_hi -= tie_hi
                kept[k] = ~low & ~high
                dropped[k] = (low.sum(), high.sum())
            chain = np.where(kept[k], np.where(started, chain + x[k], x[k]), chain)
            started |= kept[k]
        out = np.divide(chain, np.float32(K - 2 * t))
    assert out.dtype == np.float32
    return out, dropped, kept


def trimmed_mean(x: np.ndarray, t: int):
    """(out, dropped) of the whole operation: selection, then the reduction."""
    if t == 0:
        out, dropped, _ = reduce_of(x, 0)
    else:
        out, dropped, _ = reduce_of(x, t, *select_of(x, t))
    return out, dropped


def fedavg_of(x: np.ndarray) -> np.ndarray:
    """The unweighted FedAvg round on the same rows: the chain starts from client 0 and is divided by fp32(K)."""
    chain = x[0].copy()
    with np.errstate(all="ignore"):
        for k in range(1, x.shape[0]):
            chain = chain + x[k]
        return np.divide(chain, np.float32(x.shape[0]))


SPECIALS = np.asarray([0.0, -0.0, np.inf, -np.inf, 1e15, -1e15], dtype=np.float32)
NANS = np.asarray([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)


def tied_rows(rng, K: int, ld: int, P: int, nan_share: float = 0.03, poison: float = 3.0e4) -> np.ndarray:
    """[K, ld] fp32 rows of small integers (heavy ties) with planted +-0, +-inf, +-1e15 and NaNs of both sign bits
    in [:P], and a poison in columns [P, ld) that no output or count may see."""
    v = rng.integers(-3, 4, size=(K, ld)).astype(np.float32)
    r = rng.random((K, ld))
    sp = r < 0.10
    v[sp] = SPECIALS[rng.integers(0, SPECIALS.size, size=int(sp.sum()))]
    nn = (r >= 0.10) & (r < 0.10 + nan_share)
    v[nn] = NANS[rng.integers(0, NANS.size, size=int(nn.sum()))]
    v[:, P:] = poison
    return v


def normal_rows(rng, K: int, ld: int, P: int, poison: float = 3.0e4) -> np.ndarray:
    v = rng.standard_normal((K, ld), dtype=np.float32)
    v[:, P:] = poison
    return v


# ---- the plan ------------------------------------------------------------------------------------------------------
def depth_of(t: int) -> int:
    return next(T for T in DEPTHS if t <= T)


def strips(P: int) -> int:
    return ((P + 3) // 4 + 63) // 64


def strip_plan(cus: int, P: int, geo: dict) -> list:
    """[(level, first strip, tiles, grid)] of strip_plan over the strips of P columns."""
    S = strips(P)
    if S <= 0 or cus <= 0:
        return []
    cap = max(1, cus * geo["cap_pct"] // 100)
    span = [WAVES * v for v, _ in geo["levels"]]
    t0 = (S + span[0] - 1) // span[0]
    if t0 * 100 >= cap * 85:
        rounds = (t0 + cap - 1) // cap
        return [(0, 0, t0, (t0 + rounds - 1) // rounds)]
    out, s = [], 0
    n1 = S // span[1]
    if n1 > 0 and 2 * n1 >= cus:
        out.append((1, 0, n1, n1))
        s = n1 * span[1]
    if s < S:
        t2 = (S - s + span[2] - 1) // span[2]
        out.append((2, s, t2, t2))
    return out


def plan(cus: int, K: int, P: int, t: int) -> list:
    """The launches of ft_select (none at t = 0) and then ft_reduce: dicts kernel, T, V, U, col0, tiles, grid."""
    out = []
    for kernel in (("select", "reduce") if t > 0 else ("reduce",)):
        T = depth_of(t) if kernel == "select" else 0
        geo = DEEP if T >= 8 else NARROW
        for level, s0, tiles, grid in strip_plan(cus, P, geo):
            v, u = geo["levels"][level]
            out.append(dict(kernel=kernel, T=T, V=v, U=u, col0=s0 * STRIP, tiles=tiles, grid=grid))
    return out


def of_kernel(launches: list, kernel: str) -> list:
    return [l for l in launches if l["kernel"] == kernel]


# ---- the shapes ----------------------------------------------------------------------------------------------------
#: the narrow widths every test of small P runs: 1 .. 257, and one tile of each level of the narrow geometry
#: (1024, 2048 and 4096 columns) +- 1 — at these widths the plan is level 2 alone, with 1 .. 5 tiles
SMALL_P = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)


def row_cases() -> list:
    """(K, t): K = 1, 2 (t = 0), 3 (t = 1); for every depth T both t = T and t = T - 1 at K = 2t + 1 and 2t + 2; and
    one K past every rows-ahead depth U in {2, 4, 8} (U, U + 1, 2U + 1) at t = 1 and, where it exists, t = 0."""
    out = [(1, 0), (2, 0), (3, 1)]
    for T in DEPTHS:
        for t in (T - 1, T):
            if t >= 1:
                out += [(2 * t + 1, t), (2 * t + 2, t)]
    for U in (2, 4, 8):
        for K in (U, U + 1, 2 * U + 1):
            out.append((K, 0))
            if K >= 3:
                out.append((K, 1))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


def _cap(cus: int, geo: dict) -> int:
    return max(1, cus * geo["cap_pct"] // 100)


def p_two_levels(cus: int, geo: dict) -> int:
    """Just enough whole level-1 tiles to cover half the CUs, then a ragged rest for level 2."""
    n1 = (cus + 1) // 2
    span1 = WAVES * geo["levels"][1][0]
    return (span1 * n1 + max(1, span1 // 4)) * STRIP + 77


def p_level0(cus: int, geo: dict) -> int:
    """The narrowest width that is one level-0 launch: ceil(0.85 cap) tiles, one per workgroup, the last ragged."""
    t0 = (_cap(cus, geo) * 85 + 99) // 100
    span0 = WAVES * geo["levels"][0][0]
    return (span0 * t0 - max(1, span0 // 4)) * STRIP - 5


def p_capped(cus: int, geo: dict) -> int:
    """A width at which the capped grid's workgroups each walk exactly two level-0 tiles, the last tile ragged."""
    span0 = WAVES * geo["levels"][0][0]
    return (span0 * 2 * _cap(cus, geo) - max(1, span0 // 4)) * STRIP - 3


def expected_launches(cus: int, geo: dict) -> dict:
    """name -> (P, [(V, U, col0, tiles, grid)]) of one kernel under ``geo`` on a GPU of ``cus`` CUs (cus >= 16)."""
    cap = _cap(cus, geo)
    n1 = (cus + 1) // 2
    t0 = (cap * 85 + 99) // 100
    (v0, u0), (v1, u1), (v2, u2) = geo["levels"]
    return {
        "two_levels": (p_two_levels(cus, geo), [(v1, u1, 0, n1, n1), (v2, u2, WAVES * v1 * n1 * STRIP, 1, 1)]),
        "level0": (p_level0(cus, geo), [(v0, u0, 0, t0, t0)]),
        "capped": (p_capped(cus, geo), [(v0, u0, 0, 2 * cap, cap)]),
    }


def shapes(cus: int) -> list:
    """(name, K, t, P, geometry the width is derived from): every depth T at a level-1 + level-2 plan and at a
    level-0 plan of its own geometry (at the narrow widths the reduce takes the same levels; at the deep ones it
    takes whatever the narrow geometry gives that width), and a grid that walks two tiles once per geometry."""
    out = []
    for T in DEPTHS:
        geo = DEEP if T >= 8 else NARROW
        K, t = (2 * T + 1, T) if T <= 4 else (2 * (T // 2 + 1) + 1, T // 2 + 1)
        tag = "deep" if T >= 8 else "narrow"
        out.append((f"two_levels_T{T}", K, t, p_two_levels(cus, geo), tag))
        out.append((f"level0_T{T}", K, t, p_level0(cus, geo), tag))
    out.append(("capped_T1", 3, 1, p_capped(cus, NARROW), "narrow"))
    out.append(("capped_T8", 11, 5, p_capped(cus, DEEP), "deep"))
    return out
