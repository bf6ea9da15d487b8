"""Shared by the norm-clipped aggregation tests: the arithmetic of include/fedclip.h restated in numpy (with
``math.fsum`` for the exact squared norm), ``fcl_reduce``'s and ``fcl_row_sqnorms``' launch plans restated in Python
(strip_plan of fedscale_amd/csrc/fa_common.h with FCL_GEO, norm_tiles / norm_grid of clip_reduce.hip), and the
shapes the GPU tests run as a function of the CU count, with the plan each is meant to hit."""
import math

import numpy as np

# constants of clip_reduce.hip
WAVES = 4
LEVELS = ((16, 1), (8, 4), (2, 8))  # (V, U) of levels 0, 1, 2
CAP_PCT = 75
STRIP = 256  # columns of one strip: 64 lanes x 4 columns
# the norm pass's two geometries, chosen by P alone: wave tile in columns (64 lanes x V float4), waves per
# workgroup, grid cap in workgroups per 100 CUs
NORM_NARROW = dict(tile=2048, waves=2, pct=400)
NORM_WIDE = dict(tile=4096, waves=4, pct=75)
NORM_WIDE_MIN_P = 4 << 20
NORM_TILE = NORM_NARROW["tile"]


# ---- the arithmetic ------------------------------------------------------------------------------------------------
def sq_exact(x: np.ndarray, last: np.ndarray) -> float:
    """The exactly summed (then once-rounded) fp64 squared norm of the fp32 difference x - last."""
    assert x.dtype == np.float32 and last.dtype == np.float32
    with np.errstate(all="ignore"):
        d = (x - last).astype(np.float64)
        return math.fsum((d * d).tolist())  # an fp32 square is exact in fp64


def coef_of(sq: float, M: float) -> np.float32:
    """c_k of one fp64 squared norm (clip_norm.py:57-60 in fp64, rounded once to fp32)."""
    sq = np.float64(sq)
    if not np.isfinite(sq):
        return np.float32(0.0)
    r = np.float64(M) / (np.sqrt(sq) + np.float64(1e-6))
    return np.float32(r) if r < 1 else np.float32(1.0)


def coefs_of(sq, M: float) -> np.ndarray:
    return np.asarray([coef_of(s, M) for s in np.asarray(sq, dtype=np.float64)], dtype=np.float32)


def coef_is_stable(sq: float, M: float) -> bool:
    """float(r_k) is the same number for sq_k (1 +- 2^-40): the device's last-bits freedom in sq_k cannot move it."""
    if not np.isfinite(sq):
        return True
    e = 2.0 ** -40
    return coef_of(sq * (1 - e), M) == coef_of(sq, M) == coef_of(sq * (1 + e), M)


def chain_of(x: np.ndarray, last: np.ndarray, c: np.ndarray, acc: np.ndarray = None) -> np.ndarray:
    """chain = acc (or +0); chain = chain + c_k * (x_k - last) for k in order with c_k != 0; all fp32."""
    assert x.dtype == np.float32 and last.dtype == np.float32 and c.dtype == np.float32
    chain = np.zeros(last.shape, dtype=np.float32) if acc is None else acc.astype(np.float32, copy=True)
    with np.errstate(all="ignore"):
        for k in range(x.shape[0]):
            if c[k] != 0:
                chain = chain + c[k] * (x[k] - last)
    assert chain.dtype == np.float32
    return chain


def finish_of(chain: np.ndarray, last: np.ndarray, denom, sigma: float = 0.0, z: np.ndarray = None):
    """(out, m): m = chain / fp32(denom) [+ fp32(sigma) * z]; out = last + m."""
    with np.errstate(all="ignore"):
        m = np.divide(chain, np.float32(denom))
        if sigma > 0:
            m = m + np.float32(sigma) * z
        out = last + m
    assert m.dtype == np.float32 and out.dtype == np.float32
    return out, m


# ---- the plans -----------------------------------------------------------------------------------------------------
def strips(P: int) -> int:
    return ((P + 3) // 4 + 63) // 64


def plan(cus: int, K: int, P: int) -> list:
    """The launches of fcl_reduce at (K, P) on ``cus`` compute units: dicts V, U, col0, tiles, sw, grid."""
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


def norm_plan(cus: int, P: int) -> dict:
    """fcl_row_sqnorms' launches at P columns: wave tiles over the whole float4 columns, the first launch's grid."""
    g = NORM_WIDE if P >= NORM_WIDE_MIN_P else NORM_NARROW
    tiles = (P // 4 * 4 + g["tile"] - 1) // g["tile"]
    grid = min((tiles + g["waves"] - 1) // g["waves"], max(1, cus * g["pct"] // 100))
    return dict(launches=2 if tiles else 1, tiles=tiles, grid=grid, waves=g["waves"], tile_cols=g["tile"])


def ks_for(U: int) -> list:
    """K at which the U-rows-ahead loop runs 0, 1 and 2 times, with and without a remainder."""
    return sorted({1, 2, max(1, U - 1), U, U + 1, 2 * U + 1})


#: the narrow widths every test of small P runs
SMALL_P = (1, 3, 4, 5, 255, 256, 257, 4099)
#: a width of a few thousand columns: level 2 alone, three tiles, the last one ragged
P_LEVEL2 = 4099
#: the narrowest width at which one lane of the partial-sum launch adds two partials (65 wave tiles), the last ragged
P_NORM_TWO_PARTIALS = 64 * NORM_TILE + 4 * 77 + 3


#: either side of the threshold between the norm pass's geometries: the widest narrow bucket, and the narrowest wide
#: one with a ragged last tile and one column past the last float4 (1025 tiles of 4096 columns: with fewer than 342
#: CUs the capped grid's waves walk two tiles, and a lane of the partial-sum launch adds 17 partials)
P_NORM_NARROW_MAX = NORM_WIDE_MIN_P - 1
P_NORM_WIDE = NORM_WIDE_MIN_P + 4 * 77 + 1


def p_two_levels(cus: int) -> int:
    """The smallest kind of width that takes two plan levels in one call: just enough whole level-1 tiles to cover
    half the CUs, then 6 strips for level 2, the last strip ragged."""
    n1 = (cus + 1) // 2
    return (32 * n1 + 5) * STRIP + 77


def p_level0(cus: int) -> int:
    """The narrowest width that is one level-0 launch: ceil(0.85 cap) tiles, one per workgroup, the last tile ragged
    (54 of its 64 strips, the last strip short)."""
    cap = max(1, cus * CAP_PCT // 100)
    t0 = (cap * 85 + 99) // 100
    return (64 * t0 - 10) * STRIP - 5


def p_capped(cus: int) -> int:
    """A width at which the capped grid's workgroups each walk exactly two level-0 tiles and the last tile is
    ragged (at 256 CUs: 192 workgroups, 384 tiles, 6.29 M columns)."""
    cap = max(1, cus * CAP_PCT // 100)
    return (64 * 2 * cap - 20) * STRIP - 3


def expected_plans(cus: int) -> dict:
    """name -> (P, the plan the shape is listed for) on a GPU of ``cus`` CUs (cus >= 8)."""
    cap = cus * CAP_PCT // 100
    n1 = (cus + 1) // 2
    t0 = (cap * 85 + 99) // 100
    return {
        "level2": (P_LEVEL2, [dict(V=2, U=8, col0=0, tiles=3, sw=2, grid=3)]),
        "two_levels": (p_two_levels(cus), [dict(V=8, U=4, col0=0, tiles=n1, sw=8, grid=n1),
                                           dict(V=2, U=8, col0=32 * n1 * STRIP, tiles=1, sw=2, grid=1)]),
        "level0": (p_level0(cus), [dict(V=16, U=1, col0=0, tiles=t0, sw=16, grid=t0)]),
        "capped": (p_capped(cus), [dict(V=16, U=1, col0=0, tiles=2 * cap, sw=16, grid=cap)]),
    }


def random_rows(rng, K: int, ld: int, P: int, last: np.ndarray, scale: float = 0.01,
                poison: float = 3.0e4) -> np.ndarray:
    """[K, ld] fp32 rows: last + N(0, scale^2) in [:P], a nonzero poison in columns [P, ld) that no sum may count."""
    v = rng.standard_normal((K, ld), dtype=np.float32) * np.float32(scale)
    v[:, :P] += last[:P]
    v[:, P:] = poison
    return v
