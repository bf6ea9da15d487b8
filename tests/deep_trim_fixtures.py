"""Shared by the deep trimmed-mean tests: rows whose reference (tests/trim_fixtures.py, general in t) stays finite at
small t and large K, and the shapes the kernel test runs as a function of ``kernels_deeptrim.plan``."""
import numpy as np

from tests import trim_fixtures as tf

HIGH = np.concatenate([tf.NANS, np.asarray([np.inf, 1e15], dtype=np.float32)])
LOW = np.asarray([-np.inf, -1e15], dtype=np.float32)
NAN_COLS = 2  # the first columns of every case hold t + 1 NaNs and must come out NaN


def tied_rows(rng, K: int, ld: int, P: int, t: int, poison: float = 3.0e4) -> np.ndarray:
    """[K, ld] fp32 rows of integers in -3..3 with free +-0 (heavy ties).  Per column at most t rows are replaced from
    HIGH (the four NaN patterns, +inf, 1e15) and at most t from LOW, so the reference is finite; the first NAN_COLS
    columns get t + 1 NaNs instead.  Columns [P, ld) hold a poison that no output or count may see."""
    v = rng.integers(-3, 4, size=(K, ld)).astype(np.float32)
    v[(v == 0) & (rng.random((K, ld)) < 0.5)] = np.float32(-0.0)
    rank = rng.random((K, ld)).argsort(axis=0).argsort(axis=0)  # a random order of the rows, per column
    n_hi = rng.integers(0, t + 1, size=ld)
    n_lo = rng.integers(0, t + 1, size=ld)
    n_hi[:NAN_COLS] = t + 1
    hi, lo = rank < n_hi, rank >= K - n_lo
    v[hi] = HIGH[rng.integers(0, HIGH.size, size=int(hi.sum()))]
    v[lo] = LOW[rng.integers(0, LOW.size, size=int(lo.sum()))]
    nan = rank[:, :NAN_COLS] <= t
    v[:, :NAN_COLS][nan] = tf.NANS[rng.integers(0, tf.NANS.size, size=int(nan.sum()))]
    v[:, P:] = poison
    return v


def rows_of(kind: str, rng, K: int, ld: int, P: int, t: int) -> np.ndarray:
    return tied_rows(rng, K, ld, P, t) if kind == "tied" else tf.normal_rows(rng, K, ld, P)


def trims(K: int) -> list:
    """t = 1, 16, 17, a mid value and the median's, where K takes them."""
    return sorted({t for t in (1, 16, 17, (K - 1) // 4, (K - 1) // 2) if 1 <= t and 2 * t < K})


def widths(C: int) -> list:
    """P = 1, C - 1, C, C + 1 and a ragged width of four tiles (two per workgroup on a grid of two)."""
    return sorted({P for P in (1, C - 1, C, C + 1, 3 * C + 5) if P >= 1})


def assert_same(got: np.ndarray, want: np.ndarray, what):
    """Bit patterns, except that a column whose reference is NaN must be NaN."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN columns differ")
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad[:5], g[bad[:5]], w[bad[:5]])
