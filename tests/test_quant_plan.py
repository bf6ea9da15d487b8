"""CPU checks of the MXFP8 path's native surface that need no GPU: the binding table against include/fedquant.h, the
build's source lists, and fq_reduce's host-only launch plan against its restatement (tests/quant_fixtures.py) over
widths on either side of every boundary of strip_plan — the launches tile [0, P) exactly once."""
import os
import re

import numpy as np
import pytest

from fedscale_amd import _native_quant as nq
from fedscale_amd import buildinfo
from fedscale_amd import kernels_quant as kq
from tests import quant_fixtures as qf

CUS = (1, 2, 8, 104, 256, 304)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _widths(cus):
    """Widths on either side of every level boundary of the plan at this CU count."""
    cap = max(1, cus * qf.CAP_PCT // 100)
    span0, span1 = (qf.WAVES * v for v, _ in qf.LEVELS[:2])
    S = {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33}
    t0 = (cap * 85 + 99) // 100  # first tile count that takes the single level-0 launch
    S |= {span0 * (t0 - 1), span0 * (t0 - 1) + 1, span0 * t0, span0 * t0 + 1}
    for rounds in (1, 2, 3):  # capped grid: tiles on either side of a whole number of rounds
        S |= {span0 * rounds * cap - 1, span0 * rounds * cap, span0 * rounds * cap + 1, span0 * (rounds * cap + 1)}
    n1 = (cus + 1) // 2  # first level-1 tile count that covers half the CUs
    S |= {span1 * n1 - 1, span1 * n1, span1 * n1 + 1, span1 * (n1 - 1), span1 * n1 + 4, span1 * n1 + 5}
    P = {0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025}
    for s in S:
        if s > 0:
            P |= {s * qf.STRIP - 16, s * qf.STRIP - 15, s * qf.STRIP - 1, s * qf.STRIP, s * qf.STRIP + 1}
    return sorted(p for p in P if p >= 0)


def test_binding_table_lists_exactly_the_headers_symbols_and_version():
    with open(os.path.join(ROOT, "include", "fedquant.h")) as f:
        hdr = f.read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fq_\w+)\s*\(", body))
    assert declared == set(nq.SIGNATURES) == {"fq_abi_version", "fq_reduce", "fq_reduce_plan", "fq_quantize_row"}
    assert int(re.search(r"#define FQ_ABI_VERSION (\d+)", hdr).group(1)) == nq.ABI_VERSION
    assert int(re.search(r"#define FQ_PLAN_FIELDS (\d+)", hdr).group(1)) == nq.PLAN_FIELDS
    assert int(re.search(r"#define FQ_BLOCK (\d+)", hdr).group(1)) == nq.BLOCK == qf.BLOCK
    lib = nq.load()
    assert lib.fq_abi_version() == nq.ABI_VERSION
    for name in nq.SIGNATURES:
        assert hasattr(lib, name)


def test_the_unit_and_header_are_in_the_build():
    assert "fedscale_amd/csrc/quant_reduce.hip" in buildinfo.SRCS and "include/fedquant.h" in buildinfo.HDRS


@pytest.mark.parametrize("cus", CUS)
def test_library_plan_equals_the_restated_plan(cus):
    for P in _widths(cus):
        for K in (1, 33, 1000):
            got, want = kq.reduce8_plan(cus, K, P), qf.plan(cus, K, P)
            assert got == want, (cus, K, P, got, want)


@pytest.mark.parametrize("cus", CUS)
def test_every_plan_tiles_the_columns_exactly_once(cus):
    for P in _widths(cus):
        launches = kq.reduce8_plan(cus, 5, P)
        col = 0
        for l in launches:
            assert l["col0"] == col and l["col0"] % qf.STRIP == 0
            assert 1 <= l["grid"] <= l["tiles"] and l["sw"] == l["V"]
            assert (l["V"], l["U"]) in qf.LEVELS
            col += l["tiles"] * qf.WAVES * l["sw"] * qf.STRIP
        if P > 0:
            last = launches[-1]
            span = qf.WAVES * last["sw"] * qf.STRIP
            assert col - span < P <= col, (cus, P, launches)  # all of [0, P), and no empty last tile
            for l in launches[:-1]:  # only the last launch has a ragged tile
                assert l["col0"] + l["tiles"] * qf.WAVES * l["sw"] * qf.STRIP <= P
        else:
            assert launches == []
        for l in launches:  # a capped grid gives every workgroup the same number of tiles, give or take one
            if l["grid"] < l["tiles"]:
                assert l["V"] == qf.LEVELS[0][0] and l["grid"] <= max(1, cus * qf.CAP_PCT // 100)
                rounds = -(-l["tiles"] // l["grid"])
                assert l["grid"] * (rounds - 1) < l["tiles"] <= l["grid"] * rounds


def test_headline_shapes():
    """1000 x 25 M on 256 CUs: one level-0 launch, 763 tiles in 4 rounds on 191 workgroups; 100 x 1 M: level 2
    alone."""
    (l,) = kq.reduce8_plan(256, 1000, 25_000_000)
    assert (l["V"], l["U"], l["tiles"], l["grid"]) == (8, 4, 763, 191)
    (l,) = kq.reduce8_plan(256, 100, 1_000_000)
    assert (l["V"], l["U"], l["tiles"], l["grid"]) == (1, 8, 245, 245)


@pytest.mark.parametrize("args", [(0, 1, 8), (-1, 1, 8), (256, -1, 8), (256, 1, -1)])
def test_plan_refuses_bad_arguments(args):
    buf = np.zeros(8 * nq.PLAN_FIELDS, dtype=np.int64)
    lib = nq.load()
    assert lib.fq_reduce_plan(args[0], args[1], args[2], buf.ctypes.data, 8) == -1
    msg = lib.fa_last_error_string().decode()
    assert "fq_reduce_plan" in msg and "nothing was launched" in msg
