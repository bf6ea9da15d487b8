"""CPU checks of fh_reduce's launch plan (fedscale_amd/csrc/reduce_half.hip): the plan restated in Python
(tests/half_fixtures.py) against the library's host-only ``fh_reduce_plan``, over a grid that straddles every
boundary of the plan, and the shapes the GPU tests run with the plan each is listed for."""
import numpy as np
import pytest

from fedscale_amd import _native_half as nh
from fedscale_amd import kernels_half as kh
from tests import half_fixtures as hf

CUS = (1, 2, 8, 104, 256, 304)


def _widths(cus):
    """Widths on either side of every boundary of the plan at this CU count."""
    cap = max(1, cus * hf.CAP_PCT // 100)
    S = {1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65}
    t0 = (cap * 85 + 99) // 100  # first tile count that takes the single level-0 launch
    S |= {64 * (t0 - 1), 64 * (t0 - 1) + 1, 64 * t0, 64 * t0 + 1}
    for rounds in (1, 2, 3):  # capped grid: tiles on either side of a whole number of rounds
        S |= {64 * rounds * cap - 1, 64 * rounds * cap, 64 * rounds * cap + 1, 64 * rounds * cap + 64}
    n1 = (cus + 1) // 2  # first level-1 tile count that covers half the CUs
    S |= {32 * n1 - 1, 32 * n1, 32 * n1 + 1, 32 * (n1 - 1), 32 * n1 + 8, 32 * n1 + 9}
    P = {0, 1, 7, 8, 9, 511, 512, 513}
    for s in S:
        if s > 0:
            P |= {s * hf.STRIP - 8, s * hf.STRIP - 7, s * hf.STRIP - 1, s * hf.STRIP, s * hf.STRIP + 1}
    return sorted(p for p in P if p >= 0)


def test_abi_version_and_symbols():
    lib = nh.load()
    assert lib.fh_abi_version() == nh.ABI_VERSION == 1
    for name in nh.SIGNATURES:
        assert hasattr(lib, name)


@pytest.mark.parametrize("cus", CUS)
def test_library_plan_equals_the_restated_plan(cus):
    for P in _widths(cus):
        for K, weighted in ((1, False), (3, True), (1000, False)):
            got = kh.reduce16_plan(cus, K, P, weighted)
            want = hf.plan(cus, K, P, weighted)
            assert got == want, (cus, K, P, got, want)


@pytest.mark.parametrize("cus", CUS)
def test_every_plan_covers_each_column_once(cus):
    for P in _widths(cus):
        launches = hf.plan(cus, 5, P)
        col = 0
        for l in launches:
            assert l["col0"] == col and l["col0"] % hf.STRIP == 0
            assert 1 <= l["grid"] <= l["tiles"] and l["sw"] == l["V"]
            assert (l["V"], l["U"]) in hf.LEVELS
            col += l["tiles"] * hf.WAVES * l["sw"] * hf.STRIP
        if P > 0:
            last = launches[-1]
            span = hf.WAVES * last["sw"] * hf.STRIP
            assert col - span < P <= col, (cus, P, launches)  # all of [0, P), and no empty last tile
            for l in launches[:-1]:  # only the last launch has a ragged tile
                assert l["col0"] + l["tiles"] * hf.WAVES * l["sw"] * hf.STRIP <= P
        else:
            assert launches == []
        # a capped grid gives every workgroup the same number of tiles, give or take one
        for l in launches:
            if l["grid"] < l["tiles"]:
                assert l["V"] == 16 and l["grid"] <= max(1, cus * hf.CAP_PCT // 100)
                rounds = -(-l["tiles"] // l["grid"])
                assert l["grid"] * (rounds - 1) < l["tiles"] <= l["grid"] * rounds


@pytest.mark.parametrize("cus", (104, 256, 304))
def test_gpu_test_shapes_have_the_plan_they_are_listed_for(cus):
    for name, (P, want) in hf.expected_plans(cus).items():
        assert kh.reduce16_plan(cus, 3, P) == want, (name, cus, P, kh.reduce16_plan(cus, 3, P))
    exp = hf.expected_plans(cus)
    # "capped": every workgroup walks exactly two tiles, and the last tile is ragged
    P, (l,) = exp["capped"]
    assert l["tiles"] == 2 * l["grid"] and P < l["tiles"] * hf.WAVES * 16 * hf.STRIP
    assert P > (l["tiles"] - 1) * hf.WAVES * 16 * hf.STRIP
    # "level0": not capped, ragged last tile;  "two_levels": level 2 starts where level 1 ends
    P, (l,) = exp["level0"]
    assert l["grid"] == l["tiles"] and (l["tiles"] - 1) * 64 * hf.STRIP < P < l["tiles"] * 64 * hf.STRIP
    P, (a, b) = exp["two_levels"]
    assert b["col0"] == a["tiles"] * hf.WAVES * 8 * hf.STRIP < P
    # the narrow widths all take level 2 alone
    for P in hf.SMALL_P + (hf.P_LEVEL2,):
        (l,) = kh.reduce16_plan(cus, 5, P)
        assert (l["V"], l["U"]) == (2, 8)


def test_headline_shapes():
    """1000 x 25 M on 256 CUs: one level-0 launch, 763 tiles in 4 rounds on 191 workgroups; config 2's 100 x 1 M:
    level 2 alone, 245 workgroups."""
    (l,) = kh.reduce16_plan(256, 1000, 25_000_000)
    assert (l["V"], l["U"], l["tiles"], l["grid"]) == (16, 2, 763, 191)
    (l,) = kh.reduce16_plan(256, 100, 1_000_000)
    assert (l["V"], l["U"], l["tiles"], l["grid"]) == (2, 8, 245, 245)


@pytest.mark.parametrize("args", [(0, 1, 8), (-1, 1, 8), (256, -1, 8), (256, 1, -1)])
def test_plan_refuses_bad_arguments(args):
    buf = np.zeros(8 * nh.PLAN_FIELDS, dtype=np.int64)
    lib = nh.load()
    assert lib.fh_reduce_plan(args[0], args[1], args[2], 0, buf.ctypes.data, 8) == -1
    assert "fh_reduce_plan" in lib.fa_last_error_string().decode()


def test_plan_with_no_room_returns_the_count_alone():
    lib = nh.load()
    P = hf.p_two_levels(256)
    assert lib.fh_reduce_plan(256, 3, P, 0, None, 0) == 2
    buf = np.full(2 * nh.PLAN_FIELDS, -7, dtype=np.int64)
    assert lib.fh_reduce_plan(256, 3, P, 0, buf.ctypes.data, 1) == 2
    assert (buf[nh.PLAN_FIELDS:] == -7).all() and buf[0] == 8
