"""The host-only half of include/fedlowrank.h, no GPU: the binding table against the header, the sources in the
build, flr_reduce_plan / flr_reduce_table covering every output of every entry exactly once, and flr_row_layout
against the fixture's packer."""
import os
import re

import numpy as np
import pytest

from fedscale_amd import _native_lowrank as NL
from fedscale_amd import buildinfo
from fedscale_amd import kernels_lowrank as kl
from tests import lowrank_fixtures as lf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3,), (33, 95), (130, 260), (8, 40), (4, 5), (7,)]
RANKS = (1, 3, 8, 64)


def test_binding_table_lists_exactly_the_headers_symbols_and_constants():
    with open(os.path.join(ROOT, "include", "fedlowrank.h")) as f:
        hdr = f.read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(flr_\w+)\s*\(", body)) == set(NL.SIGNATURES)
    for name, val in (("ABI_VERSION", NL.ABI_VERSION), ("MAX_RANK", NL.MAX_RANK), ("PLAN_FIELDS", NL.PLAN_FIELDS),
                      ("DEPTH", NL.DEPTH), ("DENSE_COLS", NL.DENSE_COLS), ("KIND_LARGE", NL.KIND_LARGE)):
        assert int(re.search(rf"#define FLR_{name} (\d+)", hdr).group(1)) == val
    lib = NL.load()
    assert lib.flr_abi_version() == 1 and all(hasattr(lib, n) for n in NL.SIGNATURES)
    assert (kl.HEAD_T.itemsize, kl.ENTRY_T.itemsize, kl.TILE_T.itemsize) == (64, 64, 16)


def test_the_unit_and_header_are_in_the_build():
    assert "fedscale_amd/csrc/lowrank_reduce.hip" in buildinfo.SRCS and "include/fedlowrank.h" in buildinfo.HDRS


@pytest.mark.parametrize("force", (0, 64, 128))
@pytest.mark.parametrize("cus", (1, 4, 256))
@pytest.mark.parametrize("rank", RANKS)
def test_the_table_covers_every_output_exactly_once(rank, cus, force):
    dims = kl.entry_dims(SHAPES, rank)
    n, plan = kl.reduce_plan(cus, rank, dims, force)
    head, ents, tiles = kl.parse_table(kl.reduce_table(cus, rank, dims, force))
    assert n == len(tiles) == int(head["n_tiles"]) and int(head["P"]) == sum(int(np.prod(s)) for s in SHAPES)
    seen = np.zeros(int(head["P"]), dtype=np.int32)
    for row, t in enumerate(tiles):
        e, p = ents[t["entry"]], plan[t["entry"]]
        assert t["kind"] == e["kind"] == p["kind"] and p["first"] <= row < p["first"] + p["tiles"]
        if t["kind"] == NL.KIND_DENSE:
            c0 = t["tc"] * NL.DENSE_COLS
            seen[e["chain_off"] + c0:e["chain_off"] + min(c0 + NL.DENSE_COLS, e["O"])] += 1
        else:
            T = {NL.KIND_SMALL: 64, NL.KIND_LARGE: 128}[int(t["kind"])]
            assert T == p["tile"] and (force in (0, T))
            m = seen[e["chain_off"]:e["chain_off"] + e["O"] * e["I"]].reshape(e["O"], e["I"])
            m[t["tr"] * T:(t["tr"] + 1) * T, t["tc"] * T:(t["tc"] + 1) * T] += 1
    assert np.all(seen == 1)
    # the large tile only when the factored entries' large tiles together give every CU one
    large = sum(p["tiles"] for p in kl.reduce_plan(cus, rank, dims, 128)[1] if p["kind"] == NL.KIND_LARGE)
    assert {p["tile"] for p in plan if p["kind"] != NL.KIND_DENSE} == {force or (128 if large >= cus else 64)}
    assert 6 <= large <= 9  # (130, 260) alone is 6


@pytest.mark.parametrize("rank", RANKS)
def test_row_layout_is_the_fixtures_packer(rank):
    dims = kl.entry_dims(SHAPES, rank)
    ldf, off = kl.row_layout(rank, dims)
    ups = [[np.zeros((rank, sum(lf.matrix_dims(s))) if lf.factored(s, rank) else s, np.float32) for s in SHAPES]]
    rows, offs = lf.pack_rows(ups, SHAPES, rank)
    assert rows.shape[1] == ldf and ldf % 64 == 0 and [tuple(o) for o in off.tolist()] == offs
    assert all(o[0] % 4 == 0 and o[1] % 4 == 0 for o in offs)


@pytest.mark.parametrize("rank,force", [(0, 0), (65, 0), (3, 32)])
def test_the_plan_refuses_bad_arguments(rank, force):
    dims = np.asarray([[130, 260]], dtype=np.int64)
    assert NL.load().flr_reduce_plan(4, rank, 1, dims.ctypes.data, force, None) == -1
