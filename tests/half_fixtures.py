"""Shared by the 16-bit upload tests: ``fh_reduce``'s launch plan restated in Python (strip_plan of
fedscale_amd/csrc/fa_common.h with FH_GEO of reduce_half.hip), the shapes the GPU tests run as a function of the CU
count, with the plan each is meant to hit, and exact widening of 16-bit arrays on the host."""
import numpy as np

# constants of reduce_half.hip
WAVES = 4
LEVELS = ((16, 2), (8, 4), (2, 8))  # (V, U) of levels 0, 1, 2
CAP_PCT = 75
STRIP = 512  # columns of one strip: 64 lanes x 8 columns


def strips(P: int) -> int:
    return ((P + 7) // 8 + 63) // 64


def plan(cus: int, K: int, P: int, weighted: bool = False) -> list:
    """The launches of fh_reduce at (K, P) on ``cus`` compute units: dicts V, U, col0, tiles, sw, grid."""
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


def ks_for(U: int) -> list:
    """K at which the U-rows-ahead loop runs 0, 1 and 2 times, with and without a remainder."""
    return sorted({1, 2, max(1, U - 1), U, U + 1, 2 * U + 1})


#: the narrow widths every test of small P runs (K = 5, ld = round_up(P, 64))
SMALL_P = (1, 4, 5, 7, 8, 9, 511, 513)
#: a width of a few thousand columns: level 2 alone, two tiles, the last one ragged
P_LEVEL2 = 4099


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
    ragged (at 256 CUs: 192 workgroups, 384 tiles, 12.57 M columns)."""
    cap = max(1, cus * CAP_PCT // 100)
    return (64 * 2 * cap - 20) * STRIP - 3


def expected_plans(cus: int) -> dict:
    """name -> (P, the plan the shape is listed for) on a GPU of ``cus`` CUs (cus >= 8)."""
    cap = cus * CAP_PCT // 100
    n1 = (cus + 1) // 2
    t0 = (cap * 85 + 99) // 100
    return {
        "level2": (P_LEVEL2, [dict(V=2, U=8, col0=0, tiles=2, sw=2, grid=2)]),
        "two_levels": (p_two_levels(cus), [dict(V=8, U=4, col0=0, tiles=n1, sw=8, grid=n1),
                                           dict(V=2, U=8, col0=32 * n1 * STRIP, tiles=1, sw=2, grid=1)]),
        "level0": (p_level0(cus), [dict(V=16, U=2, col0=0, tiles=t0, sw=16, grid=t0)]),
        "capped": (p_capped(cus), [dict(V=16, U=2, col0=0, tiles=2 * cap, sw=16, grid=cap)]),
    }


def widen(a: np.ndarray, dtype_name: str) -> np.ndarray:
    """The exact fp32 values of a float16 array, or of a uint16 array of bfloat16 bits."""
    if dtype_name == "float16":
        assert a.dtype == np.float16
        return a.astype(np.float32)
    assert a.dtype == np.uint16
    return (a.astype(np.uint32) << 16).view(np.float32)


def random_rows(rng, K: int, ld: int, P: int, dtype_name: str, poison: float = 3.0) -> np.ndarray:
    """[K, ld] 16-bit rows (float16, or uint16 bfloat16 bits): ordinary values in [:P], a nonzero poison in
    columns [P, ld), which a reduction must never count."""
    v = rng.standard_normal((K, ld), dtype=np.float32)
    v[:, P:] = poison
    if dtype_name == "float16":
        return v.astype(np.float16)
    return (v.view(np.uint32) >> 16).astype(np.uint16)  # truncation: any bfloat16 will do as an input
