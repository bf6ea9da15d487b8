"""Shared by the Bulyan tests: include/fedbulyan.h restated in numpy, and the rows the kernel tests run."""
import numpy as np

from tests import trim_fixtures as tf


def dist2_of(G: np.ndarray) -> np.ndarray:
    """[K, K] float64 by the lines ``v`` and ``dist2`` of include/fedkrum.h (the diagonal is not used)."""
    g = np.diag(G)
    with np.errstate(all="ignore"):
        v = (g[:, None] + g[None, :]) - 2.0 * G
    return np.where(np.isnan(v), np.inf, np.where(v > 0, v, 0.0))


def select_of(G: np.ndarray, f: int):
    """(picks, sel, n_sel, score_0).  A removed neighbour adds +0.0, which changes no bit of a non-negative sum."""
    K = G.shape[0]
    theta = K - 2 * f - 2
    assert f >= 0 and 4 * f + 3 <= K
    d = dist2_of(G)
    order = np.argsort(d, axis=1, kind="stable")  # (the row itself is masked out below)
    ds = np.take_along_axis(d, order, axis=1)
    gone = np.zeros(K, dtype=bool)
    picks, score0 = [], None
    for s in range(theta):
        rows = np.flatnonzero(~gone)
        m = K - s - f - 2
        alive = ~gone[order[rows]]
        alive &= order[rows] != rows[:, None]
        take = alive & (np.cumsum(alive, axis=1) <= m)
        with np.errstate(all="ignore"):
            score = np.cumsum(np.where(take, ds[rows], 0.0), axis=1)[:, -1]  # sequential fp64 adds, ascending
        if s == 0:
            score0 = score.copy()
        best = rows[np.lexsort((rows, score))[0]]
        if not np.isfinite(score[rows == best][0]):
            break
        picks.append(best)
        gone[best] = True
    pad = [-1] * (theta - len(picks))
    return (np.asarray(picks + pad, dtype=np.int32), np.asarray(sorted(picks) + pad, dtype=np.int32), len(picks),
            score0)


def reduce_of(x: np.ndarray, sel: np.ndarray, beta: int):
    """(out, kept): fp32 [P] and int64 [K] of the mean around the median over the rows x[sel]."""
    assert x.dtype == np.float32
    v = x[sel]
    theta, P = v.shape
    key = tf.keys_of(v)
    cols = np.arange(P)
    med = v[np.argsort(key, axis=0, kind="stable")[(theta - 1) // 2], cols]
    with np.errstate(all="ignore"):
        e = np.abs(v - med)
    ekey = np.where(np.isnan(e), np.uint32(0xFFFFFFFF), e.view(np.uint32))
    cut = np.partition(ekey, beta - 1, axis=0)[beta - 1]
    n_cut = beta - (ekey < cut).sum(axis=0)
    eq = ekey == cut
    keep = (ekey < cut) | (eq & (np.cumsum(eq, axis=0) - eq < n_cut))
    assert (keep.sum(axis=0) == beta).all()
    chain = np.zeros(P, dtype=np.float32)
    started = np.zeros(P, dtype=bool)
    with np.errstate(all="ignore"):
        for r in range(theta):
            chain = np.where(keep[r], np.where(started, chain + v[r], v[r]), chain)
            started |= keep[r]
        out = np.divide(chain, np.float32(beta))
    kept = np.zeros(x.shape[0], dtype=np.int64)
    np.add.at(kept, sel, keep.sum(axis=1))
    return out, kept


def rows_of(rng, K: int, ld: int, P: int, sel: np.ndarray) -> np.ndarray:
    """Rows of ``sel`` by column p % 8: normal; all equal; integers with +-0 (ties straddling the cut); denormals;
    mostly +inf; a few +-inf; a few NaNs; mostly NaN.  Every other row is NaN; columns [P, ld) hold a poison."""
    n = sel.size
    v = rng.standard_normal((n, ld)).astype(np.float32)
    r = rng.random((n, ld))
    ints = rng.integers(-2, 3, size=(n, ld)).astype(np.float32)
    ints[(ints == 0) & (r < 0.5)] = np.float32(-0.0)
    den = rng.integers(-40, 41, size=(n, ld)).astype(np.int64)
    den = np.where(den < 0, (-den).astype(np.uint32) | np.uint32(0x80000000), den.astype(np.uint32)).view(np.float32)
    nans = tf.NANS[rng.integers(0, tf.NANS.size, size=(n, ld))]
    p = np.arange(ld) % 8
    v = np.where(p == 1, np.float32(0.375), v)
    v = np.where(p == 2, ints, v)
    v = np.where(p == 3, den, v)
    v = np.where((p == 4) & (r < 0.7), np.float32(np.inf), v)
    v = np.where((p == 5) & (r < 0.2), np.where(r < 0.1, np.float32(np.inf), np.float32(-np.inf)), v)
    v = np.where((p == 6) & (r < 0.2), nans, v)
    v = np.where((p == 7) & (r < 0.7), nans, v).astype(np.float32)
    x = np.full((K, ld), np.nan, dtype=np.float32)
    x[sel] = v
    x[:, P:] = np.float32(3.0e4)
    return x
