"""The restatement of fa_qfed_accumulate (tests/qfed_fixtures.py) checked on the CPU: every listed shape reaches the
form it is listed for, the restated summation order stays within its derived distance of the exact sum, and every
planted mistake changes a bit at a shape that tests/test_gpu_qfed_kernels.py runs."""
import math

import numpy as np
import pytest

from tests import qfed_fixtures as qf

F32, F64 = np.float32, np.float64


def test_constants_match_the_source():
    """The mirrored macros still carry the values of fedscale_amd/csrc/fedagg.hip."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fedscale_amd", "csrc",
                            "fedagg.hip")).read()
    for name, want in (("QF_V", "16"), ("QF_G", "4"), ("QF_GRID", "256"), ("QF_CHAIN_GRID", "QF_GRID"),
                       ("QF_PART", "4"), ("QF_CHAIN_PART", "8"), ("QF_GATHER_SEG", "16"), ("QF_MAXK", "2048"),
                       ("QF_CHAIN_V", "8"), ("QF_GWIN_MAX", "1024"), ("QF_WIN_ROUNDS", "1"),
                       ("QF_CHAIN_WIN_ROUNDS", "QF_WIN_ROUNDS"), ("QF_WIDE_BYTES", "(1LL << 31)")):
        m = re.search(r"^#define %s (\S+( << \d+\))?)" % name, src, flags=re.M)
        assert m and m.group(1) == want, (name, m and m.group(1))
    assert (qf.QF_V, qf.QF_CHAIN_V, qf.QF_G, qf.QF_GRID, qf.QF_PART, qf.QF_CHAIN_PART, qf.QF_GATHER_SEG, qf.QF_MAXK,
            qf.QF_GWIN_MAX, qf.QF_WIDE_BYTES) == (16, 8, 4, 256, 4, 8, 16, 2048, 1024, 1 << 31)
    assert qf.window_cols(False) == 4_194_304 and qf.window_cols(True) == 2_097_152


def test_listed_conditions():
    """Every entry of SHAPES has the sw, tile count, window count and gather form it is listed for, and the tile
    shapes are the least P reaching their sw with a ragged last strip and a ragged float4.

    Out of reach of these shapes, and left to test_gpu_edges.py::test_qfed_accumulate_wide_rows_and_column_windows
    (no shapes are built for them here):
      * the per-row-descriptor path (WIDE false) needs ld > 2^27;
      * k_qfed_gather_win needs more than 1024 windows in one call."""
    for c in qf.SHAPES:
        wins = qf.plan(qf.ld_of(c), c["P"], c["chain"])
        cond = c["cond"]
        assert tuple(w["sw"] for w in wins) == cond["sw"], c["name"]
        assert tuple(w["ntiles"] for w in wins) == cond["ntiles"], c["name"]
        assert len(wins) == cond["nwin"], c["name"]
        assert qf.gather_form(c["K"], c["P"], c["chain"], qf.ws_bytes_of(c)) == cond["gather"], c["name"]
        assert all(w["ntiles"] <= qf.QF_GRID for w in wins)
        assert qf.ld_of(c) > qf.round_up4(c["P"]) and 1 <= c["K"] <= qf.QF_MAXK
    for chain, sws in ((False, (2, 3, 8, 15, 16)), (True, (2, 3, 7, 8))):
        for sw in sws:
            P = qf._tile_P(sw)
            (w,) = qf.plan(P + 63, P, chain)
            assert w["sw"] == sw and P % 4 == 1 and w["P4"] % 64 == 1
            (below,) = qf.plan(P + 63, P - 1, chain)  # one column fewer: the float4 and its strip are gone
            assert below["sw"] == sw - 1
    # every wave of every workgroup owns exactly one whole strip at S = 1024; at 1025 the last tile is partly empty
    (w,) = qf.plan(262144 + 64, 262144, False)
    assert all(len(qf.strips_of(w, g, v)) == 1 for g in range(256) for v in range(4))
    (w,) = qf.plan(262148 + 60, 262145, False)
    assert [len(qf.strips_of(w, 128, v)) for v in range(4)] == [1, 0, 0, 0] and not len(qf.strips_of(w, 129, 0))
    assert sorted(s for g in range(256) for v in range(4) for s in qf.strips_of(w, g, v)) == list(range(1025))
    # the K edges and P of the issue, plain and chain, each as two chunks
    for P in (3, 257, 1025):
        for K in (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 2047, 2048):
            for kind in ("plain", "chain"):
                assert qf.BY_NAME[f"k{K}_p{P}_{kind}"]["calls"] == 2


def test_plan_matches_the_library():
    """The window count and the workspace sizes of the restatement against the library's own host-side exports."""
    from fedscale_amd._native import load

    lib = load()
    for c in qf.SHAPES:
        ld = qf.ld_of(c)
        assert lib.fa_qfed_launches(ld, c["P"], 1 if c["chain"] else 0) == c["cond"]["nwin"], c["name"]
        assert lib.fa_qfed_workspace_bytes(c["K"], ld, c["P"]) == qf.workspace_bytes(c["K"], ld, c["P"]), c["name"]
        assert lib.fa_qfed_workspace_bytes(c["K"], 0, 0) == qf.workspace_bytes(c["K"]), c["name"]
    assert lib.fa_qfed_max_chunk() == qf.QF_MAXK


@pytest.mark.parametrize("name", ["sw2_s1025_plain", "sw2_s1025_chain", "k5_p1025_plain", "k2047_p257_chain"])
def test_restated_order_against_fsum(name):
    """The restated norm differs from math.fsum of the fp32 squares by at most ((PART - 1) 2^-24 + n 2^-53) * sum:
    a partial chains PART squares with PART - 1 fp32 adds, each within 2^-24 relative of its (positive) exact sum, and
    the partials then meet in fewer than n fp64 adds, n the squares of the row."""
    c = qf.BY_NAME[name]
    d = qf.make(c)
    part = qf.QF_CHAIN_PART if c["chain"] else qf.QF_PART
    C = qf.round_up4(c["P"])
    _, _, sq = qf.accumulate(d["x"][0], d["last"], d["alpha"][0], d["lr"], c["chain"], P=c["P"])
    g = (d["last"][None, :C] - d["x"][0][:, :C]) / F32(d["lr"])
    g2 = g * g
    for k in range(min(c["K"], 5)):
        exact = math.fsum(g2[k].astype(F64).tolist())
        assert abs(sq[k] - exact) <= ((part - 1) * 2.0 ** -24 + C * 2.0 ** -53) * exact, (name, k, sq[k], exact)


@pytest.mark.parametrize("name", [c["name"] for c in qf.SHAPES if c["kind"] == "integer" and c["P"] < 1 << 20])
def test_integer_data_equals_the_integer_sum(name):
    c = qf.BY_NAME[name]
    d = qf.make(c)
    sq = qf.reference(c, d)[-1][2]
    assert np.array_equal(sq, qf.integer_norms(c, d)) and (sq != d["sqnorm0"]).all()


def _differs(case, data, mistake):
    return any(not (qf.same_bits(a[0], b[0]) and qf.same_bits(a[2], b[2]) and
                    (a[1] is None or qf.same_bits(a[1], b[1])))
               for a, b in zip(qf.reference(case, data), qf.reference(case, data, mistake)))


# What the comparison this file replaces (rtol 5e-7 against a plain fp64 sum, K <= 33, P <= 262,147, norms from zero)
# would have let through, as far as reasoning goes (nothing asserts this record):
#   partials_of_8        passes: a reordering of fp32 adds, ~1e-8 relative
#   sqnorm_overwritten   passes: every norm there started from zero
#   pad_columns_left_out passes: the padding was zero
#   redo_keeps_acc       passes: no input left the fast division's range, and lr never did
#   sw_off_by_one        seen only at P > 262,144 (sw 2), which one drawn edge reached
#   segments_of_8        passes but for that edge: one float4 of 65,537 is lost, ~1e-5 relative
#   lane_left_out, tail_client_shifted, wave_missing: seen (whole terms go missing)
@pytest.mark.parametrize("mistake", qf.MISTAKES)
def test_each_mistake_is_seen(mistake):
    """Every planted mistake changes at least one bit the GPU file asserts, at the listed shape SEEN_BY names."""
    assert set(qf.SEEN_BY) == set(qf.MISTAKES)
    c = qf.BY_NAME[qf.SEEN_BY[mistake]]
    assert _differs(c, qf.make(c), mistake), mistake


def test_specials_leave_the_other_clients_alone():
    """In the restatement a client's denormal, huge, infinite or NaN entries move no other client's norm and no other
    column of delta and chain; non-finite norms are those of the clients that hold the entries."""
    for c in (qf.BY_NAME["specials_lr0.05_chain"], qf.BY_NAME["specials_lr3e+25_plain"]):
        d = qf.make(c)
        (dl, ch, sq), = qf.reference(c, d)
        (dl0, ch0, sq0), = qf.reference(c, d, x=d["clean"])
        for k in (0, 1, 4):  # each client's norm is what it is with no other client in the call
            solo = qf.accumulate(d["x"][0][k:k + 1], d["last"], d["alpha"][0][k:k + 1], d["lr"], c["chain"],
                                 sqnorm0=d["sqnorm0"][k:k + 1], P=c["P"])[2]
            assert qf.same_bits(solo, sq[k:k + 1]), k
        assert np.isfinite(sq[0]) and np.isinf(sq[2]) and np.isnan(sq[3])
        assert np.isfinite(sq[[1, 4]]).all() == (c["lr"] > 1)  # 2^81 / 0.05 squares to inf, 2^90 / 3e25 does not
        cols = np.ones(dl.size, dtype=bool)
        cols[[col for pokes in qf.SPECIAL_AT.values() for col, _ in pokes]] = False
        assert qf.same_bits(dl[cols], dl0[cols]) and (ch is None or qf.same_bits(ch[cols], ch0[cols]))
