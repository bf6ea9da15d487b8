"""CPU checks of the 1-bit sign path's native surface that need no GPU: the binding table against include/fedsign.h,
the build's source lists, and fsg_reduce's host-only launch plan against its restatement (tests/sign_fixtures.py) over
widths on either side of every boundary of strip_plan — the launches tile [0, P) exactly once."""
import os
import re

import numpy as np
import pytest

from fedscale_amd import _native_sign as ns
from fedscale_amd import buildinfo
from fedscale_amd import kernels_sign as kg
from tests import sign_fixtures as sg

CUS = (1, 2, 8, 104, 256, 304)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _widths(cus):
    """Widths on either side of every level boundary of the plan at this CU count."""
    cap = max(1, cus * sg.CAP_PCT // 100)
    span0, span1 = (sg.WAVES * v for v, _ in sg.LEVELS[:2])
    S = {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33}
    t0 = (cap * 85 + 99) // 100  # first tile count that takes the single level-0 launch
    S |= {span0 * (t0 - 1), span0 * (t0 - 1) + 1, span0 * t0, span0 * t0 + 1}
    for rounds in (1, 2, 3):  # capped grid: tiles on either side of a whole number of rounds
        S |= {span0 * rounds * cap - 1, span0 * rounds * cap, span0 * rounds * cap + 1, span0 * (rounds * cap + 1)}
    n1 = (cus + 1) // 2  # first level-1 tile count that covers half the CUs
    S |= {span1 * n1 - 1, span1 * n1, span1 * n1 + 1, span1 * (n1 - 1), span1 * n1 + 4, span1 * n1 + 5}
    P = {0, 1, 31, 32, 33, 255, 256, 257, 2047, 2048, 2049}
    for s in S:
        if s > 0:
            P |= {s * sg.STRIP - 32, s * sg.STRIP - 31, s * sg.STRIP - 1, s * sg.STRIP, s * sg.STRIP + 1}
    return sorted(p for p in P if p >= 0)


def test_binding_table_lists_exactly_the_headers_symbols_and_version():
    with open(os.path.join(ROOT, "include", "fedsign.h")) as f:
        hdr = f.read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fsg_\w+)\s*\(", body))
    assert declared == set(ns.SIGNATURES) == {"fsg_abi_version", "fsg_reduce", "fsg_reduce_plan", "fsg_sign_row"}
    assert int(re.search(r"#define FSG_ABI_VERSION (\d+)", hdr).group(1)) == ns.ABI_VERSION == 1
    assert int(re.search(r"#define FSG_PLAN_FIELDS (\d+)", hdr).group(1)) == ns.PLAN_FIELDS
    assert int(re.search(r"#define FSG_BLOCK (\d+)", hdr).group(1)) == ns.BLOCK == sg.BLOCK == 256
    lib = ns.load()
    assert lib.fsg_abi_version() == ns.ABI_VERSION
    for name in ns.SIGNATURES:
        assert hasattr(lib, name)


def test_the_unit_and_header_are_in_the_build():
    assert "fedscale_amd/csrc/sign_reduce.hip" in buildinfo.SRCS and "include/fedsign.h" in buildinfo.HDRS


def test_staging_strides_are_the_contracts():
    for P in (0, 1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 25_000_000):
        assert kg.bit_bytes(P) == sg.bit_bytes(P) == -(-P // 8)
        assert kg.blocks(P) == sg.blocks(P) == -(-P // 256)
        assert kg.bit_stride(P) == sg.bit_stride(P) and kg.bit_stride(P) % 16 == 0
        assert 0 <= kg.bit_stride(P) - kg.bit_bytes(P) < 16
        assert kg.scale_stride(P) == sg.scale_stride(P) and kg.scale_stride(P) % 4 == 0
        assert 0 <= kg.scale_stride(P) - kg.blocks(P) < 4


@pytest.mark.parametrize("cus", CUS)
def test_library_plan_equals_the_restated_plan(cus):
    for P in _widths(cus):
        for K in (1, 33, 1000):
            got, want = kg.reduce_sign_plan(cus, K, P), sg.plan(cus, K, P)
            assert got == want, (cus, K, P, got, want)


@pytest.mark.parametrize("cus", CUS)
def test_every_plan_tiles_the_columns_exactly_once(cus):
    for P in _widths(cus):
        launches = kg.reduce_sign_plan(cus, 5, P)
        col = 0
        for l in launches:
            assert l["col0"] == col and l["col0"] % sg.STRIP == 0
            assert 1 <= l["grid"] <= l["tiles"] and l["sw"] == l["V"]
            assert (l["V"], l["U"]) in sg.LEVELS
            col += l["tiles"] * sg.WAVES * l["sw"] * sg.STRIP
        if P > 0:
            last = launches[-1]
            span = sg.WAVES * last["sw"] * sg.STRIP
            assert col - span < P <= col, (cus, P, launches)  # all of [0, P), and no empty last tile
            for l in launches[:-1]:  # only the last launch has a ragged tile
                assert l["col0"] + l["tiles"] * sg.WAVES * l["sw"] * sg.STRIP <= P
        else:
            assert launches == []
        for l in launches:  # a capped grid gives every workgroup the same number of tiles, give or take one
            if l["grid"] < l["tiles"]:
                assert l["grid"] <= max(1, cus * sg.CAP_PCT // 100)
                rounds = -(-l["tiles"] // l["grid"])
                assert l["grid"] * (rounds - 1) < l["tiles"] <= l["grid"] * rounds


def test_headline_shapes():
    """1000 x 25 M and 100 x 25 M on 256 CUs: one level-0 launch, 3052 tiles in 2 rounds on 1526 workgroups (six per
    CU at most); 100 x 1 M: 122 whole tiles would not cover half the CUs, so all 123 tiles are one level-2 launch."""
    for K in (100, 1000):
        (l,) = kg.reduce_sign_plan(256, K, 25_000_000)
        assert (l["V"], l["U"], l["tiles"], l["grid"]) == (1, 8, 3052, 1526)
        assert l["grid"] <= 6 * 256
    (l,) = kg.reduce_sign_plan(256, 100, 1_000_000)
    assert (l["V"], l["U"], l["col0"], l["tiles"], l["grid"]) == (1, 8, 0, 123, 123)


@pytest.mark.parametrize("args", [(0, 1, 8), (-1, 1, 8), (256, -1, 8), (256, 1, -1)])
def test_plan_refuses_bad_arguments(args):
    buf = np.zeros(8 * ns.PLAN_FIELDS, dtype=np.int64)
    lib = ns.load()
    assert lib.fsg_reduce_plan(args[0], args[1], args[2], buf.ctypes.data, 8) == -1
    msg = lib.fa_last_error_string().decode()
    assert "fsg_reduce_plan" in msg and "nothing was launched" in msg
    assert lib.fsg_reduce_plan(256, 1, 4096, None, 8) == -1  # a capacity without a buffer


def test_the_measured_file_carries_the_fields_the_documents_quote():
    """profiles/sign_reduce_measure.json (tools/sign_reduce_measure.py, a run on the card): the three shapes, each
    with the four reduces' times and byte rates, fsg_reduce's pair rate against the lane rate, the ratios to the two
    predictions at the headline, fsg_sign_row, and updates/s from pickled payloads beside float32.  No time is
    asserted."""
    import json

    with open(os.path.join(ROOT, "profiles", "sign_reduce_measure.json")) as f:
        m = json.load(f)
    assert m["read_ceiling_Bps"] == 7.23e12 and m["lane_ops_per_s"] == 78.6e12 and m["build_defs"] == ""
    shapes = {s["config"]: s for s in m["shapes"]}
    assert {(s["K"], s["P"]) for s in shapes.values()} == {(100, 1_000_000), (100, 25_000_000), (1000, 25_000_000)}
    for s in shapes.values():
        for k in ("fsg_reduce", "fq_reduce", "fh_reduce_bf16", "fa_reduce"):
            assert s[k]["ms_median"] > 0 and s[k]["TBps"] > 0 and 0 < s[k]["share_of_read_ceiling"] <= 1.0, k
        g = s["fsg_reduce"]
        assert g["row_column_pairs"] == s["K"] * s["P"] and 0 < g["pairs_per_s_over_lane_ops_per_s"] < 1
        assert g["bytes"] == s["K"] * (sg.bit_bytes(s["P"]) + 4 * sg.blocks(s["P"])) + 4 * s["P"]
        assert s["fsg_reduce_plan"] == sg.plan(256, s["K"], s["P"])
    head = shapes["head"]
    assert head["fsg_reduce"]["predicted_ms"] == {"bytes": 0.49, "three_vector_ops_per_pair": 0.95}
    assert set(head["fsg_reduce"]["ratio_to_predictions"]) == {"bytes", "three_vector_ops_per_pair"}
    assert isinstance(head["fsg_reduce"]["beats_fq_reduce"], bool) and head["fsg_sign_row"]["ms_median"] > 0
    pc = m["pcie_inclusive"]
    assert pc["P"] == 25_000_000 and pc["float32"]["updates_per_s"] > 0 and pc["sign1"]["updates_per_s"] > 0
    assert pc["sign1"]["payload_bytes"] < pc["float32"]["payload_bytes"] * 9 / 64 / 4 + 4096
