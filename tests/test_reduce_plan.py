"""tests/reduce_fixtures.py on the CPU: its restatement of k_reduce's launch plan covers every column once at every
CU count, the shapes it lists reach the tile forms they are listed for, the two window branches are as (un)reachable
as its docstring says, its model of reduce_tile is the plain in-order chain, and each planted mistake changes a bit of
a case tests/test_gpu_reduce_kernels.py runs."""
import numpy as np
import pytest

from tests import reduce_fixtures as rf
from tests.side_kernel_models import same_bits

CUS = (1, 2, 8, 104, 256, 304)
KS = (1, 199, 200, 1000)
SEEN_CUS = 4  # the smallest CU count at which every form, two-window ones included, is reached


def _widths(cus):
    """P on either side of every boundary of the plan: strip counts 4 * g * q and one more, for the three grids the
    plan divides by and every tile width it compares with, and the ends of one, two and three windows."""
    cap, gb = cus * rf.FA_GRID_CAP_PCT // 100, cus * rf.FA_BAL_GRID // 256
    strips = {1, 2}
    for g in (cus, cap, gb):
        for q in (4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33):
            strips.add(rf.FA_RED_WAVES * g * q)
    for R in (1, 2, 3):
        strips.add(rf.FA_RED_WAVES * rf.FA_CAP_SW_MAX * cap * R)
        strips.add(rf.FA_RED_WAVES * rf.FA_CAP_SW_MAX * cus * R)
    out = set()
    for s in strips:
        for P in (s * 256 - 1, s * 256, s * 256 + 1, s * 256 + 256, s * 256 + 257):
            if P >= 1:
                out.add(P)
    return sorted(out)


def _plans(cus):
    for K in KS:
        for P in _widths(cus):
            try:
                yield K, P, rf.plan(cus, K, P)
            except rf.NoPlan:
                assert cus == 1, (cus, K, P)
                yield K, P, None


@pytest.mark.parametrize("cus", CUS)
def test_every_plan_covers_every_column_once(cus):
    planned = 0
    for K, P, launches in _plans(cus):
        if launches is None:
            continue
        rf.check_cover(launches, P)
        assert len(launches) == 1 or all(L["window"] and not L["pipe"] for L in launches)
        planned += 1
    assert planned > (0 if cus == 1 else 100)


def test_one_compute_unit_has_no_plan():
    """cap = 1 * 75 / 100 = 0 and the FA_BAL_GRID grid 1 * 224 / 256 = 0: launch_plan divides by one of them unless K
    < FA_BAL_SHORT_K and 8 <= ceil(S / 4) <= 32."""
    for K in KS:
        for S in (1, 28, 29, 128, 129, 1000):
            ok = K < rf.FA_BAL_SHORT_K and 29 <= S <= 128
            if ok:
                rf.check_cover(rf.plan(1, K, S * 256), S * 256)
            else:
                with pytest.raises(rf.NoPlan):
                    rf.plan(1, K, S * 256)


def test_owners_partition_the_columns():
    """Column by column, at a CU count small enough to list them: each float4 column has one owner."""
    for s in rf.shapes(SEEN_CUS):
        P4 = (s["P"] + 3) // 4
        launches = rf.plan(SEEN_CUS, s["K"], s["P"])
        c = np.concatenate([o["c"] for o in rf.owners(launches, P4)])
        assert np.array_equal(np.sort(c), np.arange(P4)), s["name"]
        for L, o in zip(launches, rf.owners(launches, P4)):
            assert o["j"].max() < L["sw"] and o["tile"].max() == L["tiles"] - 1 and o["wave"].max() <= 3


def test_shapes_reach_the_forms_they_are_listed_for():
    names = [s["name"] for s in rf.shapes(256)]
    fulls = [n for n, (_, _, form) in rf.FORMS.items() if form[2] and n != "short"]
    assert sorted(names) == sorted(list(rf.FORMS) + [n + "_fill" for n in fulls])
    forms = {rf.FORMS[n][2] for n in rf.FORMS if not n.startswith("win_")}
    assert forms == {(32, 1, True), (32, 1, False), (16, 2, True), (16, 2, False), (8, 4, True), (8, 4, False),
                     (4, 4, True)}  # the seven tile forms; the three window forms are the win_ names
    for cus in (SEEN_CUS, 8, 104, 256, 304):
        for s in rf.shapes(cus):
            base = s["name"].replace("_fill", "")
            n, i, form = rf.FORMS[base]
            launches = rf.plan(cus, s["K"], s["P"])
            assert rf.plan_is(cus, s["K"], s["P"], s["name"]) and len(launches) == n
            L = launches[i]
            assert rf.form_of(L) == form and L["sw"] == s["sw"] and L["window"] == (n > 1)
            assert L["pipe"] == (base == "short")
            width = L["end4"] - L["col0"]
            span = rf.LANES * rf.FA_RED_WAVES * L["sw"]
            if s["fill"]:
                assert s["P"] % 4 == 0 and width == L["tiles"] * span
            else:
                assert s["P"] % 256 == 1 and width % span != 0  # one float in the last float4, a ragged last tile
                if s["S"] > 1:  # the lowest strip count: one strip fewer runs another form
                    assert not rf.plan_is(cus, s["K"], s["P"] - 256, s["name"])


def test_the_forms_test_gpu_fullsize_names():
    """The shapes of test_gpu_fullsize.py's balanced-plan tests at 256 CUs, as their comments state them."""
    want = {(200, 1_000_003): [(8, 4, 5)], (200, 2_300_001): [(16, 2, 12)], (1000, 3_125_056): [(16, 2, 16)],
            (100, 5_000_001): [(32, 1, 20)], (150, 5_000_001): [(32, 1, 20)], (60, 9_000_001): [(32, 1, 23)] * 2}
    for (K, P), forms in want.items():
        assert [(L["V"], L["U"], L["sw"]) for L in rf.plan(256, K, P)] == forms


def test_narrow_window_branches():
    """launch_window's sw < 16 branch is not reached over the grid, and its sw == 16 branch only by a last window of
    exactly 4 * 16 * cap strips."""
    for cus in CUS:
        cap = cus * rf.FA_GRID_CAP_PCT // 100
        hit16 = 0
        for K, P, launches in _plans(cus):  # (the widths hold S = 4 * 32 * cap + 1)
            if launches is None or len(launches) == 1:
                continue
            for i, L in enumerate(launches):
                assert L["sw"] >= 16, (cus, K, P, L)
                if L["sw"] == 16:
                    hit16 += 1
                    strips = -(-(L["end4"] - L["col0"]) // rf.LANES)
                    assert i == len(launches) - 1 and strips == 4 * 16 * cap and L["full"]
                    assert K >= rf.FA_BAL_SHORT_K
        assert hit16 > 0 or cap == 0


def test_the_narrow_window_branch_needs_thousands_of_windows():
    """... but it is reachable: the last of R windows holds S - (R - 1) * ceil(S / R) strips.  At 2 CUs 69 windows
    do it; at 256 CUs (cap 192) the bound (S - (R - 1)^2) / R with S > (R - 1) * 4 * 32 * cap stays above 15 tiles'
    worth until R = 13,057, rows of more than 300 GB."""
    last = rf.plan(2, 3, 8764 * 256)[-1]
    assert len(rf.plan(2, 3, 8764 * 256)) == 69 and last["sw"] == 15 and not last["full"] and last["V"] == 16
    cap = 256 * rf.FA_GRID_CAP_PCT // 100
    per_round = rf.FA_RED_WAVES * rf.FA_CAP_SW_MAX * cap
    for R in range(2, 13_057):
        S = (R - 1) * per_round + 1
        assert (S - (R - 1) ** 2) / R > 15 * rf.FA_RED_WAVES * cap, R
    S = 320_875_776
    launches = rf.plan(256, 200, S * 256)
    assert len(launches) == 13_057 and launches[-1]["sw"] == 15 and 4 * S * 256 > 300e9


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
_BASE = {}


def _inputs(case):
    if case["id"] not in _BASE:
        inp = rf.case_inputs(case)
        x = rf.expand_rows(inp["rows"], case["P"])
        bufs = rf.expand_buffers(rf.block_buffers(inp), case["P"])
        denom = rf.case_denom(case, inp)
        want = _run(case, x, bufs, inp, denom, None)
        _BASE[case["id"]] = (inp, x, bufs, denom, want)
    return _BASE[case["id"]]


def _run(case, x, bufs, inp, denom, mistake):
    return rf.run_model(case, x, bufs, inp["a"], denom,
                        lambda K: rf.plan(SEEN_CUS, K, case["P"], case["weighted"]), mistake)


def _differs(case, mistake):
    inp, x, bufs, denom, want = _inputs(case)
    got = _run(case, x, bufs, inp, denom, mistake)
    P = case["P"]
    return any(not same_bits(got[k][:P], want[k][:P]) for k in want)


def _cases():
    return rf.cases(SEEN_CUS)


def test_cases_have_the_plans_they_are_listed_for():
    ids = [c["id"] for c in _cases()]
    assert len(set(ids)) == len(ids) and ids == [c["id"] for c in rf.cases(256)]
    for cus in (SEEN_CUS, 256):
        for c in rf.cases(cus):
            K = max(call["k1"] - call["k0"] for call in c["calls"])
            assert rf.plan_is(cus, K, c["P"], c["form"]), (cus, c["id"])
            assert K <= c["Krows"]
    inst = {(rf.FORMS[c["form"].replace("_fill", "")][2], c["calls"][-1]["epi"], c["weighted"]) for c in _cases()
            if len(c["calls"]) == 1}
    assert len(inst) == 42  # 7 tile forms x 3 epilogues x weighted or not


def test_the_model_is_the_plain_chain():
    """Without a mistake the tiles, the groups of U rows and the calls of a fold leave no trace: the model's result is
    one loop over the rows (chain and mean), and the same as its own column-wise form (FedYoGi too); the padding and
    the four floats past cols(P) come back as they were."""
    for case in _cases():
        inp, x, bufs, denom, want = _inputs(case)
        P = case["P"]
        blk = {k: v[:P] for k, v in bufs.items()}
        flat = rf.run_model(case, x[:, :P], blk, inp["a"], denom, lambda K: None)
        for k in want:
            assert same_bits(want[k][:P], flat[k]), (case["id"], k)
            assert same_bits(want[k][rf.cols(P):], bufs[k][rf.cols(P):]), (case["id"], k)
        last = case["calls"][-1]
        if last["epi"] != "yogi":
            ref = rf.plain_reference(case, x[:, :P], dict(inp, acc=bufs["acc"][:P]), denom)
            assert same_bits(want[last["dst"]][:P], ref), case["id"]


@pytest.mark.parametrize("mistake", rf.MISTAKES)
def test_each_mistake_is_seen(mistake):
    """Every planted mistake changes a bit of the case SEEN_BY names for it.  The two that make a thread touch columns
    of another thread are seen by in-place cases only: out of place a column written twice is written the same."""
    by_id = {c["id"]: c for c in _cases()}
    assert _differs(by_id[rf.SEEN_BY[mistake]], mistake), mistake
    if mistake in rf.IN_PLACE_ONLY:
        seen = [c for c in _cases() if _differs(c, mistake)]
        assert seen and all(c["in_place"] for c in seen), [c["id"] for c in seen if not c["in_place"]]
        assert by_id[rf.SEEN_BY[mistake]]["calls"][-1]["src"] == by_id[rf.SEEN_BY[mistake]]["calls"][-1]["dst"]


def test_a_full_kernel_on_narrower_tiles_changes_nothing():
    """The FULL instantiation of a launch's own V, launched whatever sw is: more tiles than columns, the surplus
    masked by the window end.  Not a bit of any case moves (it costs empty workgroups only)."""
    assert set(rf.SEEN_BY) == set(rf.MISTAKES)
    for mistake in rf.HARMLESS:
        assert not [c["id"] for c in _cases() if _differs(c, mistake)]
