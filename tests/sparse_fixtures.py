"""A numpy restatement of the top-k sparse delta-upload contract (include/fedsparse.h), independent of the product
code: the selection as a stable sort by (-key, index), the in-order fp32 chain as a plain loop over pairs, the
densified upload and the finish.  Test infrastructure, shared by the CPU and GPU tests of the path."""
import numpy as np

F32 = np.float32
TILE = 4096  # FS_TILE of include/fedsparse.h (tests/test_sparse_plan.py reads it from the header)
WG_PER_CU = 8  # tiles the plan keeps resident per compute unit

#: the values the heavy-tie cases draw from
TIE_VALUES = np.asarray([0.0, -0.0, 1.0, -1.0, 2.0, 3.5, 1e-40, np.inf, np.nan], dtype=F32)


def keys(e: np.ndarray) -> np.ndarray:
    """|e| as its bits, uint32: NaN > inf > finite, +-0 lowest."""
    return np.ascontiguousarray(e, dtype=F32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def delta(x, base=None, r_in=None) -> np.ndarray:
    """e = x - base (+ r_in), each an fp32 operation of its own."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.asarray(x, dtype=F32) if base is None else (np.asarray(x, dtype=F32) - np.asarray(base, dtype=F32))
        if r_in is not None:
            e = (e + np.asarray(r_in, dtype=F32)).astype(F32)
    return e.astype(F32)


def select(e: np.ndarray, k: int):
    """(idx uint32, val float32, r_out float32) of the float32 vector ``e``: the first min(k, P) columns of a stable
    sort by (-key, index), re-sorted by index; r_out holds e where a column was dropped and +0 where it was kept."""
    e = np.ascontiguousarray(e, dtype=F32)
    P = e.size
    k = min(int(k), P)
    order = np.argsort(-keys(e).astype(np.int64), kind="stable")  # ties keep their index order
    idx = np.sort(order[:k]).astype(np.uint32)
    val = e[idx.astype(np.int64)].copy()
    r_out = e.copy()
    r_out[idx.astype(np.int64)] = F32(0.0)
    return idx, val, r_out


def densify(idx, val, P: int) -> np.ndarray:
    d = np.zeros(int(P), dtype=F32)
    d[np.asarray(idx).astype(np.int64)] = np.asarray(val, dtype=F32)
    return d


def chain(rows, P: int, acc_in=None) -> np.ndarray:
    """acc_in (or +0), then for rows in order and each pair of the row chain[idx] = chain[idx] + val, in fp32; a
    column a row does not name is not touched.  ``rows``: (idx, val) pairs."""
    c = np.zeros(int(P), dtype=F32) if acc_in is None else np.asarray(acc_in, dtype=F32)[:P].copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for idx, val in rows:
            i = np.asarray(idx).astype(np.int64)
            assert i.size < 2 or (i[1:] > i[:-1]).all()  # unique within a row: the pairs of one row do not interact
            c[i] = (c[i] + np.asarray(val, dtype=F32)).astype(F32)
    return c


def finish(L: np.ndarray, c: np.ndarray, K: int) -> np.ndarray:
    """L + chain / float(K), fp32."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (L.astype(F32) + (c / F32(K)).astype(F32)).astype(F32)


def tiles(P: int) -> int:
    return (int(P) + TILE - 1) // TILE


def plan(cus: int, K: int, P: int) -> list:
    """fs_reduce's launch at (K, P) on ``cus`` compute units, restated: dicts tile, U, col0, tiles, per, grid."""
    if P <= 0:
        return []
    t = tiles(P)
    per = max(1, -(-t // (cus * WG_PER_CU)))
    return [dict(tile=TILE, U=16, col0=0, tiles=t, per=per, grid=-(-t // per))]


def random_row(rng, P: int, nnz: int, binades: int = 30):
    """One valid row: (up to) ``nnz`` distinct sorted columns and values mixed over ``binades`` binades, so that the
    fp32 sum of a column depends on the order."""
    if 4 * nnz >= P:
        idx = np.sort(rng.choice(P, size=nnz, replace=False)).astype(np.uint32)
    else:  # a draw with replacement, made unique: a few pairs fewer than asked for
        idx = np.unique(rng.integers(0, P, nnz)).astype(np.uint32)
    nnz = idx.size
    val = (rng.standard_normal(nnz) * np.exp2(rng.integers(-binades // 2, binades // 2, nnz))).astype(F32)
    return idx, val
