"""CPU checks of the cohort kernels' host-side plans (fedscale_amd/csrc/cohort_sig.hip): ``gram_plan`` and
``center_rows`` restated in Python, against the library's host-only workspace queries.  The GPU tests
(tests/test_gpu_cohort_kernels.py) derive from these sizes that a shape really runs the code path it is listed
for: several steps of ``k_gram_partial``'s main loop per workgroup, a short last split, more than one partial
row per segment of ``k_center_seg``."""
import pytest

from fedscale_amd import _native_cohort as nc

# constants of cohort_sig.hip
GB, GK = 64, 64
G_TARGET_WGS = 2048
G_MAX_WS = 512 << 20
CW_COLS = 512
CT_SEG = 32


def gram_plan(K: int, D: int):
    """(tiles, nsplit, steps per split) of fc_gram: ``gram_plan`` of cohort_sig.hip."""
    T = (K + GB - 1) // GB
    tiles = T * (T + 1) // 2
    steps = (D + GK - 1) // GK if D > 0 else 1
    ns = min((G_TARGET_WGS + tiles - 1) // tiles, steps)
    one = K * K * 4
    while ns > 1 and ns * one > G_MAX_WS:
        ns -= 1
    per = (steps + ns - 1) // ns
    return tiles, (steps + per - 1) // per, per


def center_rows(D: int) -> int:
    return (D + CW_COLS - 1) // CW_COLS


def center_plan(K: int, D: int):
    """(partial rows, rows per first-level segment, blocks along K) of fc_center."""
    nrows = center_rows(D)
    return nrows, (nrows + CT_SEG - 1) // CT_SEG, (K + 255) // 256


# (K, D, tiles, nsplit, steps per split, columns of the last split): the shapes of the GPU Gram tests
GRAM_SHAPES = [
    (129, 65701, 6, 257, 4, 165),    # 342 splits reduced to 257; the last split holds 2 whole steps and 37 columns
    (65, 131395, 3, 514, 4, 67),
    (3, 200000, 1, 1563, 2, 64),
    (200, 70000, 10, 183, 6, 112),
    (4096, 130, 2080, 1, 3, 130),
    (4096, 8, 2080, 1, 1, 8),
    (64, 128, 1, 2, 1, 64),
    (130, 43776, 6, 342, 2, 128),    # D = 342 * 128: no short last split
]
# (K, D, partial rows, rows per segment, blocks along K): the shapes of the GPU fc_center tests
CENTER_SHAPES = [(K, 513, 2, 1, (K + 255) // 256) for K in (1, 2, 7, 8, 9, 10, 16, 17, 300, 1000)] + \
    [(9, 1, 1, 1, 1), (9, 8, 1, 1, 1), (9, 511, 1, 1, 1), (9, 512, 1, 1, 1), (9, 16385, 33, 2, 1),
     (9, 36003, 71, 3, 1), (300, 16385, 33, 2, 2), (8, 36003, 71, 3, 1), (16, 36003, 71, 3, 1), (7, 203, 1, 1, 1)]

_GRID_K = [1, 2, 3, 5, 63, 64, 65, 128, 129, 130, 200, 1000, 4095, 4096]
_GRID_D = [0, 1, 7, 8, 63, 64, 65, 128, 130, 4097, 20001, 43776, 65701, 70000, 131395, 200000, 1119126]


def test_listed_gram_shapes_have_the_plan_they_are_listed_for():
    for K, D, tiles, nsplit, per, last in GRAM_SHAPES:
        assert gram_plan(K, D) == (tiles, nsplit, per), (K, D, gram_plan(K, D))
        assert D - (nsplit - 1) * per * GK == last and 0 < last <= per * GK, (K, D)
    assert (G_TARGET_WGS + 6 - 1) // 6 == 342  # K = 129: the split count before it is reduced to 257
    assert 65701 % GK == 37


def test_listed_center_shapes_have_the_plan_they_are_listed_for():
    for K, D, nrows, per, blocks in CENTER_SHAPES:
        assert center_plan(K, D) == (nrows, per, blocks), (K, D, center_plan(K, D))
    nrows, per, _ = center_plan(9, 36003)
    assert nrows - 23 * per == 2  # segment 23 is the last that holds rows, and it is short; 24..31 are empty


def test_workspace_queries_equal_the_restated_plans():
    lib = nc.load()
    shapes = {(K, D) for K in _GRID_K for D in _GRID_D}
    shapes |= {(K, D) for K, D, *_ in GRAM_SHAPES} | {(K, D) for K, D, *_ in CENTER_SHAPES}
    shapes |= {(65540, 5), (33, 20001), (10, 2449)}
    for K, D in sorted(shapes):
        want_c = (center_rows(D) + CT_SEG) * K * 8
        assert lib.fc_center_workspace_bytes(K, D) == want_c, (K, D)
        if K <= nc.GRAM_MAX_K:
            _, nsplit, per = gram_plan(K, D)
            got = lib.fc_gram_workspace_bytes(K, D)
            assert got == nsplit * K * K * 4, (K, D, got)
            assert got <= max(G_MAX_WS, K * K * 4), (K, D)
            assert nsplit >= 1 and (nsplit - 1) * per * GK < max(D, 1) <= nsplit * per * GK, (K, D)  # covers [0, D)
        else:
            assert lib.fc_gram_workspace_bytes(K, D) == 0, (K, D)


@pytest.mark.parametrize("K,D", [(0, 8), (-1, 8), (-2147483648, 8), (5, -1), (5, -(1 << 40)), (0, -1)])
def test_workspace_queries_return_zero_for_bad_shapes(K, D):
    lib = nc.load()
    assert lib.fc_center_workspace_bytes(K, D) == 0
    assert lib.fc_gram_workspace_bytes(K, D) == 0


def test_gram_workspace_query_refuses_more_than_max_k_rows():
    lib = nc.load()
    assert nc.GRAM_MAX_K == 4096
    for D in (0, 1, 64, 130, 70000):
        assert lib.fc_gram_workspace_bytes(nc.GRAM_MAX_K, D) > 0
        assert lib.fc_gram_workspace_bytes(nc.GRAM_MAX_K + 1, D) == 0
        assert lib.fc_gram_workspace_bytes(2147483647, D) == 0
        assert lib.fc_center_workspace_bytes(nc.GRAM_MAX_K + 1, D) > 0  # fc_center has no such limit
