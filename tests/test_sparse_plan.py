"""CPU checks of the sparse path's native surface that need no GPU: the binding table against include/fedsparse.h,
the build's source lists, fs_reduce's host-only launch plan — every column owned exactly once, tiles a function of P
alone — and fs_topk_workspace."""
import os
import re

import numpy as np
import pytest

from fedscale_amd import _native_sparse as ns
from fedscale_amd import buildinfo
from fedscale_amd import kernels_sparse as ks
from tests import sparse_fixtures as sf

CUS = (1, 2, 8, 104, 256, 304)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _widths(cus):
    """Widths on either side of a tile, and of a whole number of rounds of the capped grid."""
    P = {0, 1, 63, 64, 65, sf.TILE - 1, sf.TILE, sf.TILE + 1, 2 * sf.TILE + 5}
    cap = cus * sf.WG_PER_CU
    for rounds in (1, 2, 3):
        for t in (rounds * cap - 1, rounds * cap, rounds * cap + 1):
            if t > 0:
                P |= {t * sf.TILE - 1, t * sf.TILE, t * sf.TILE + 1}
    return sorted(p for p in P if p < (1 << 31))


def test_binding_table_lists_exactly_the_headers_symbols_and_version():
    with open(os.path.join(ROOT, "include", "fedsparse.h")) as f:
        hdr = f.read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fs_\w+)\s*\(", body))
    assert declared == set(ns.SIGNATURES) == {"fs_abi_version", "fs_row_offsets", "fs_check_rows", "fs_reduce",
                                              "fs_reduce_plan", "fs_topk_workspace", "fs_topk_row"}
    assert int(re.search(r"#define FS_ABI_VERSION (\d+)", hdr).group(1)) == ns.ABI_VERSION
    assert int(re.search(r"#define FS_PLAN_FIELDS (\d+)", hdr).group(1)) == ns.PLAN_FIELDS
    assert int(re.search(r"#define FS_TILE (\d+)", hdr).group(1)) == ns.TILE == ks.TILE == sf.TILE
    lib = ns.load()
    assert lib.fs_abi_version() == ns.ABI_VERSION
    for name in ns.SIGNATURES:
        assert hasattr(lib, name)


def test_the_unit_and_header_are_in_the_build():
    assert "fedscale_amd/csrc/sparse_reduce.hip" in buildinfo.SRCS and "include/fedsparse.h" in buildinfo.HDRS
    # nothing else in the tree uses the prefix
    for rel in buildinfo.SRCS + buildinfo.HDRS:
        if "sparse" in rel:
            continue
        with open(os.path.join(ROOT, rel)) as f:
            assert not re.search(r"\bfs_[a-z]", f.read()), rel


@pytest.mark.parametrize("cus", CUS)
def test_every_column_is_owned_exactly_once_and_tiles_depend_on_P_only(cus):
    for P in _widths(cus):
        for K in (1, 33, 1000):
            got = ks.reduce_sparse_plan(cus, K, P)
            assert got == sf.plan(cus, K, P), (cus, K, P, got)
        if P == 0:
            assert got == []
            continue
        (l,) = got
        assert l["tile"] == sf.TILE and l["col0"] == 0
        # tiles t = 0 .. tiles - 1 cover [t * TILE, (t + 1) * TILE): all of [0, P), no empty last tile, whatever cus
        assert (l["tiles"] - 1) * l["tile"] < P <= l["tiles"] * l["tile"]
        assert l["tiles"] == ks.reduce_sparse_plan(7, 5, P)[0]["tiles"] == ks.boundaries(P) - 1
        # workgroup b walks tiles b, b + grid, ...: every tile by exactly one workgroup, `per` of them at most
        assert 1 <= l["grid"] <= min(l["tiles"], cus * sf.WG_PER_CU)
        owners = np.zeros(l["tiles"], dtype=np.int64)
        walked = np.zeros(l["grid"], dtype=np.int64)
        for b in range(l["grid"]):
            t = np.arange(b, l["tiles"], l["grid"])
            owners[t] += 1
            walked[b] = t.size
        assert (owners == 1).all() and walked.max() == l["per"] and walked.min() >= l["per"] - 1


def test_headline_shapes():
    """1000 x 25 M on 256 CUs: 6104 tiles in 3 rounds on 2035 workgroups; 100 x 1 M: 245 tiles, one each."""
    (l,) = ks.reduce_sparse_plan(256, 1000, 25_000_000)
    assert (l["tiles"], l["per"], l["grid"]) == (6104, 3, 2035)
    (l,) = ks.reduce_sparse_plan(256, 100, 1_000_000)
    assert (l["tiles"], l["per"], l["grid"]) == (245, 1, 245)


@pytest.mark.parametrize("args", [(0, 1, 8), (-1, 1, 8), (256, -1, 8), (256, 1, -1)])
def test_plan_refuses_bad_arguments(args):
    buf = np.zeros(8 * ns.PLAN_FIELDS, dtype=np.int64)
    lib = ns.load()
    assert lib.fs_reduce_plan(args[0], args[1], args[2], buf.ctypes.data, 8) == -1
    msg = lib.fa_last_error_string().decode()
    assert "fs_reduce_plan" in msg and "nothing was launched" in msg


def test_topk_workspace():
    """A multiple of 16 bytes, at least the fixed header, monotone in P, two words per 1024 columns beyond it, and
    refused for a negative P."""
    sizes = [ks.topk_workspace(P) for P in (0, 1, 1024, 1025, 4097, 70001, 25_000_000, (1 << 31) - 1)]
    assert all(s % 16 == 0 and s >= 2048 for s in sizes)
    assert sizes == sorted(sizes)
    assert ks.topk_workspace(1024) == ks.topk_workspace(1)  # one tile
    assert ks.topk_workspace(25_000_000) - ks.topk_workspace(1024) == 8 * (-(-25_000_000 // 1024) - 1)
    assert ks.topk_workspace(25_000_000) < 25_000_000 * 4 // 100  # far below the row itself
    lib = ns.load()
    assert lib.fs_topk_workspace(-1) == -1 and "fs_topk_workspace" in lib.fa_last_error_string().decode()
