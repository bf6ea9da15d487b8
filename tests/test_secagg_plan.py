"""CPU checks of the secure-aggregation path's native surface that need no GPU: the binding table against
include/fedsecagg.h, the build's source lists, and fsa_reduce's host-only launch plan against its restatement
(tests/secagg_fixtures.py) over widths on either side of every boundary of strip_plan — the launches tile [0, P)
exactly once."""
import os
import re

import numpy as np
import pytest

from fedscale_amd import _native_secagg as ns
from fedscale_amd import buildinfo
from fedscale_amd import kernels_secagg as ks
from tests import secagg_fixtures as sf

CUS = (1, 2, 8, 104, 256, 304)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _widths(cus):
    """Widths on either side of every level boundary of the plan at this CU count, and of the tile seams."""
    cap = max(1, cus * sf.CAP_PCT // 100)
    span0, span1 = (sf.WAVES * v for v, _ in sf.LEVELS[:2])
    S = {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33}
    t0 = (cap * 85 + 99) // 100  # first tile count that takes the single level-0 launch
    S |= {span0 * (t0 - 1), span0 * (t0 - 1) + 1, span0 * t0, span0 * t0 + 1}
    for rounds in (1, 2, 3):  # capped grid: tiles on either side of a whole number of rounds
        S |= {span0 * rounds * cap - 1, span0 * rounds * cap, span0 * rounds * cap + 1, span0 * (rounds * cap + 1)}
    n1 = (cus + 1) // 2  # first level-1 tile count that covers half the CUs
    S |= {span1 * n1 - 1, span1 * n1, span1 * n1 + 1, span1 * (n1 - 1), span1 * n1 + 4, span1 * n1 + 5}
    P = {0, 1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025}
    for s in S:
        if s > 0:
            P |= {s * sf.STRIP - 4, s * sf.STRIP - 3, s * sf.STRIP - 1, s * sf.STRIP, s * sf.STRIP + 1}
    return sorted(p for p in P if p >= 0)


def test_binding_table_lists_exactly_the_headers_symbols_and_version():
    with open(os.path.join(ROOT, "include", "fedsecagg.h")) as f:
        hdr = f.read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fsa_\w+)\s*\(", body))
    assert declared == set(ns.SIGNATURES) == {"fsa_abi_version", "fsa_encode_row", "fsa_mask_sum", "fsa_reduce",
                                              "fsa_reduce_plan", "fsa_finish"}
    assert int(re.search(r"#define FSA_ABI_VERSION (\d+)", hdr).group(1)) == ns.ABI_VERSION
    assert int(re.search(r"#define FSA_PLAN_FIELDS (\d+)", hdr).group(1)) == ns.PLAN_FIELDS
    assert int(re.search(r"#define FSA_MAX_KEYS \(1 << (\d+)\)", hdr).group(1)) == 20 and ns.MAX_KEYS == 1 << 20
    assert ns.MAX_KEYS >= 65536
    assert int(re.search(r"#define FSA_MAX_FRAC_BITS (\d+)", hdr).group(1)) == ns.MAX_FRAC_BITS == 30
    assert int(re.search(r"#define FSA_MAX_MAG_BITS (\d+)", hdr).group(1)) == ns.MAX_MAG_BITS == 30
    assert int(re.search(r"#define FSA_MASK_TILE (\d+)", hdr).group(1)) == ns.MASK_TILE
    assert int(re.search(r"#define FSA_MASK_GRID_PER_CU (\d+)", hdr).group(1)) == ns.MASK_GRID_PER_CU
    # the argument counts of the table are the header's
    for name, (_, argtypes) in ns.SIGNATURES.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, body).group(1).strip()
        n = 0 if decl == "void" else decl.count(",") + 1
        assert n == len(argtypes), name
    lib = ns.load()
    assert lib.fsa_abi_version() == ns.ABI_VERSION
    for name in ns.SIGNATURES:
        assert hasattr(lib, name)


def test_the_unit_and_header_are_in_the_build():
    assert "fedscale_amd/csrc/secagg.hip" in buildinfo.SRCS and "include/fedsecagg.h" in buildinfo.HDRS


@pytest.mark.parametrize("cus", CUS)
def test_library_plan_equals_the_restated_plan(cus):
    for P in _widths(cus):
        for K in (1, 33, 1000):
            got, want = ks.reduce32_plan(cus, K, P), sf.plan(cus, K, P)
            assert got == want, (cus, K, P, got, want)


@pytest.mark.parametrize("cus", CUS)
def test_every_plan_tiles_the_columns_exactly_once(cus):
    widths = set(_widths(cus))
    for P in list(widths):  # and one width just past every level and tile seam of each of those plans
        widths |= set(sf.seam_widths(ks.reduce32_plan(cus, 5, P)))
    for P in sorted(widths):
        launches = ks.reduce32_plan(cus, 5, P)
        col = 0
        for l in launches:
            assert l["col0"] == col and l["col0"] % sf.STRIP == 0
            assert 1 <= l["grid"] <= l["tiles"] and l["sw"] == l["V"]
            assert (l["V"], l["U"]) in sf.LEVELS
            col += l["tiles"] * sf.WAVES * l["sw"] * sf.STRIP
        if P > 0:
            last = launches[-1]
            span = sf.WAVES * last["sw"] * sf.STRIP
            assert col - span < P <= col, (cus, P, launches)  # all of [0, P), and no empty last tile
            for l in launches[:-1]:  # only the last launch has a ragged tile
                assert l["col0"] + l["tiles"] * sf.WAVES * l["sw"] * sf.STRIP <= P
        else:
            assert launches == []
        for l in launches:  # a capped grid gives every workgroup the same number of tiles, give or take one
            if l["grid"] < l["tiles"]:
                assert l["V"] == sf.LEVELS[0][0] and l["grid"] <= max(1, cus * sf.CAP_PCT // 100)
                rounds = -(-l["tiles"] // l["grid"])
                assert l["grid"] * (rounds - 1) < l["tiles"] <= l["grid"] * rounds


def test_headline_shapes():
    """1000 x 25 M on 256 CUs: one level-0 launch of 16 KiB runs, 1526 tiles in 8 rounds on 191 workgroups;
    100 x 1 M: level 2 alone (122 whole level-1 tiles do not cover half the CUs)."""
    (l,) = ks.reduce32_plan(256, 1000, 25_000_000)
    assert (l["V"], l["U"], l["tiles"], l["grid"]) == (16, 2, 1526, 191)
    (l,) = ks.reduce32_plan(256, 100, 1_000_000)
    assert (l["V"], l["U"], l["tiles"], l["grid"]) == (2, 8, 489, 489)


@pytest.mark.parametrize("args", [(0, 1, 8), (-1, 1, 8), (256, -1, 8), (256, 1, -1)])
def test_plan_refuses_bad_arguments(args):
    buf = np.zeros(8 * ns.PLAN_FIELDS, dtype=np.int64)
    lib = ns.load()
    assert lib.fsa_reduce_plan(args[0], args[1], args[2], buf.ctypes.data, 8) == -1
    msg = lib.fa_last_error_string().decode()
    assert "fsa_reduce_plan" in msg and "nothing was launched" in msg
