"""The numpy restatement of include/fedgeomed.h (geometric-median / RFA aggregation by the smoothed Weiszfeld
iteration), shared by test_geomed_plan.py and the GPU tests: the fixed-order sum S, the start weights, the weights of
an iteration, the distances in Gram space, both whole rounds (continued from the device's Gram or streamed distances
when given), and a plain fp64 Weiszfeld with unordered numpy sums as the independent reference.

What shaped the contract, found with this restatement on ``krum_fixtures.Case(11)`` (one upload scaled by 2^50, one all
NaN, one sign-flipped x 8) and ``krum_fixtures.nonint_case()`` before any kernel was written:

* Starting from the plain mean (RFA's own start) is not usable: with the 2^50 attacker the mean sits at 10^14 and
  three iterations only bring it to 3 * 10^12.
* Starting from L (the round's model) is not usable either: a lazy client that uploads L unchanged is a data point at
  the start, gets weight 1 / nu and pins the iterate — the error is still 0.19 of 0.30 after 8 iterations.
* The start that works is the mean of the updates clipped to the median update norm, cheap because the norms are on
  the device already (the Gram diagonal, or the first fcl_row_sqnorms).  On Case(11) at R = 3 the distance to the
  honest mean is 0.88 against a bound of 33.7; on the non-integer case the objective is 23.3 at the plain mean, 21.105
  at this start and 21.066 after three steps, and the lazy-client variant converges at the same rate.
* The two methods agree within 1 fp32 ulp of the model (often 0) at R = 1, 3, 4, 8 on both cases.
* K = 1 returns the upload, K = 2 the midpoint, all-NaN returns L, all-equal uploads return the upload.
"""
import math

import numpy as np

from tests import krum_fixtures as kf

F32, F64 = np.float32, np.float64
MAX_K, MAX_ITERS, CHUNK = 4096, 64, 256
AUTO_GRAM_PASSES = 12

# ---- shapes of the GPU kernel tests ----------------------------------------------------------------------------------
# fgm_start / fgm_weights: below / at / above one and two rows of the 64-lane sum, and at the LDS capacity
WEIGHTS_K = (1, 2, 3, 63, 64, 65, 127, 128, 129, 4095, 4096)
# fgm_gram_dist2: the boundaries of the 64-lane sum, of the 256 chunk (= the j block) and of the 1024-thread workgroup
DIST2_K = (1, 2, 3, 64, 65, 255, 256, 257, 513, 4096)
FINISH_P = (1, 3, 4, 5, 1023, 4097)

# Both restated rounds (and the device's) against ``weiszfeld_fp64`` of the same R, in fp32 ulps of the model's largest
# magnitude: the largest difference seen on Case(11), nonint_case() and lazy_case() at R = 1, 3, 4, 8, both methods,
# was 0.52 ulp (4.93e-7 at scale 8; 5.4e-8 at scale 1 is 0.45) — the final rounding of the model to fp32 plus the
# fp32 chain.  Times 8:
WEISZFELD_TOL_ULPS = 8 * 0.52
METHODS_TOL_ULPS = 4  # the two methods against each other (the issue's bound); observed here: 0 to 0.25


# ---- the contract ----------------------------------------------------------------------------------------------------
def S(v) -> float:
    """The fixed-order sum of the header: pad with +0.0 to a multiple of 64, lane-strided adds from +0.0, butterfly."""
    v = np.asarray(v, dtype=F64)
    K = v.shape[0]
    pad = np.zeros(-(-max(K, 1) // 64) * 64, dtype=F64)
    pad[:K] = v
    with np.errstate(all="ignore"):
        t = np.zeros(64, dtype=F64)
        for row in pad.reshape(-1, 64):
            t = t + row
        lanes = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            t = t + t[lanes ^ m]
    return F64(t[0])


def start_of(q0):
    """(w float64[K], c float32[K], n_valid) of fgm_start."""
    q0 = np.asarray(q0, dtype=F64)
    valid = np.isfinite(q0)
    n = int(valid.sum())
    w = np.zeros(q0.shape[0], dtype=F64)
    if n > 0:
        med = np.sort(q0[valid])[n // 2]
        with np.errstate(all="ignore"):
            ratio = np.where(q0 <= med, 1.0, np.sqrt(med) / np.sqrt(q0))
            w = np.where(valid, ratio / F64(n), 0.0)
    return w, w.astype(F32), n


def weights_of(q, nu):
    """(w float64[K], c float32[K], obj, n_valid) of fgm_weights."""
    q = np.asarray(q, dtype=F64)
    nu = F64(nu)
    valid = np.isfinite(q)
    with np.errstate(all="ignore"):
        dist = np.where(valid, np.sqrt(np.where(q > 0, q, 0.0)), 0.0)
        r = np.where(valid, 1.0 / np.where(dist > nu, dist, nu), 0.0)
        B, obj, n = S(r), S(dist), int(valid.sum())
        w = r / B if n > 0 else np.zeros(q.shape[0], dtype=F64)
    return w, w.astype(F32), obj, n


def gram_dist2_of(G, w):
    """float64[K] of fgm_gram_dist2: chunk partials in k order, chunks in order, b = S(u), q = (G_jj - 2 a_j) + b."""
    G, w = np.asarray(G, dtype=F64), np.asarray(w, dtype=F64)
    K = w.shape[0]
    a = np.zeros(K, dtype=F64)
    with np.errstate(all="ignore"):
        for k0 in range(0, K, CHUNK):
            part = np.zeros(K, dtype=F64)
            for k in range(k0, min(k0 + CHUNK, K)):
                if w[k] != 0:
                    part = part + G[k] * w[k]  # (G[k][j]: the matrix is symmetric and the kernel reads it this way)
            a = a + part
        u = np.where(w != 0, w * a, 0.0)
        b = S(u)
        return (np.diag(G) - 2.0 * a) + b


def finish_of(chain, L, n_valid):
    if n_valid <= 0:
        return L.astype(F32).copy()
    with np.errstate(all="ignore"):
        return (L + chain).astype(F32)


def sqnorms_ref(x, z, P):
    """float64[K]: the fsum squared norms of the fp32 differences x_k - z (fcl_row_sqnorms' reference)."""
    out = np.zeros(x.shape[0], dtype=F64)
    with np.errstate(all="ignore"):
        for k in range(x.shape[0]):
            d = (x[k, :P].astype(F32) - z[:P].astype(F32)).astype(F64)
            sq = d * d
            out[k] = math.fsum(sq.tolist()) if np.isfinite(sq).all() else sq.sum()
    return out


def sqnorm_bound(q, P):
    """The any-order summation bound P u / (1 - P u) * q of a sum of P exact non-negative products."""
    return P * kf.U / (1.0 - P * kf.U) * q


def resolve(K, R, method="auto"):
    if method != "auto":
        return method
    return "gram" if K <= AUTO_GRAM_PASSES * (1 + 2 * R) else "stream"


def geomed_round(x, L, P, R, nu, method, G=None, q_hist=None):
    """dict(out, w, c, obj, q, q0, n_valid, G, z) of a whole round.  ``G`` ("gram"): the Gram to continue from (the
    device's), else the reference Gram.  ``q_hist`` ("stream"): float64[R + 1, K], the start norms and every
    iteration's squared distances to continue from (the device's), else fsum references.  ``z`` ("stream"): the R
    fp32 iterates the iterations started from."""
    assert method in ("gram", "stream")
    d = kf.diffs(x, L, P)
    Lp = L[:P].astype(F32)
    K = x.shape[0]
    q, obj, zs = np.zeros((R, K), dtype=F64), np.zeros(R, dtype=F64), []
    if method == "gram":
        if G is None:
            G = kf.gram_ref(d)
        q0 = np.diag(G).copy()
        w, c, n = start_of(q0)
        for t in range(R):
            q[t] = gram_dist2_of(G, w)
            w, c, obj[t], n = weights_of(q[t], nu)
        out = finish_of(kf.chain_of(d, c), Lp, n)
    else:
        q0 = sqnorms_ref(x, Lp, P) if q_hist is None else np.asarray(q_hist[0], dtype=F64)
        w, c, n = start_of(q0)
        z = finish_of(kf.chain_of(d, c), Lp, n)
        for t in range(R):
            zs.append(z)
            q[t] = sqnorms_ref(x, z, P) if q_hist is None else np.asarray(q_hist[t + 1], dtype=F64)
            w, c, obj[t], n = weights_of(q[t], nu)
            z = finish_of(kf.chain_of(d, c), Lp, n)
        out = z
    return dict(out=out, w=w, c=c, obj=obj, q=q, q0=q0, n_valid=n, G=G, z=zs)


# ---- the independent reference ---------------------------------------------------------------------------------------
def weiszfeld_fp64(x, L, P, R, nu):
    """A plain smoothed Weiszfeld in fp64 with unordered numpy sums, from the same start (the mean of the updates
    clipped to the median norm); rows with an inf or NaN are left out.  (out float64[P], objective float64[R])."""
    with np.errstate(all="ignore"):
        d = x[:, :P].astype(F64) - L[:P].astype(F64)
    d = d[np.isfinite(d).all(axis=1)]
    if d.shape[0] == 0:
        return L[:P].astype(F64), np.zeros(R)
    norm = np.sqrt((d * d).sum(axis=1))
    med = np.sort(norm)[d.shape[0] // 2]
    scale = np.where(norm <= med, 1.0, med / np.where(norm > 0, norm, 1.0))
    z = (d * scale[:, None]).mean(axis=0)
    obj = np.zeros(R)
    for t in range(R):
        dist = np.sqrt(((d - z) ** 2).sum(axis=1))
        obj[t] = dist.sum()
        r = 1.0 / np.maximum(dist, nu)
        z = (d * (r / r.sum())[:, None]).sum(axis=0)
    return L[:P].astype(F64) + z, obj


# ---- data ------------------------------------------------------------------------------------------------------------
def crafted_q(rng, K, nu):
    """Squared distances with the crafted entries of the contract's edge cases (as many as K allows): NaN, +inf, a tiny
    negative (clamped to +0), 0, a value below nu^2 (its distance counts as nu), -inf."""
    q = (rng.random(K) * 4.0 + 0.01) ** 2
    special = (np.nan, np.inf, -1e-30, 0.0, 0.25 * nu * nu, -np.inf)
    if K >= 3:
        where = rng.permutation(K)[:min(len(special), K - 2)]  # at least two ordinary entries stay
        q[where] = special[:len(where)]
    return q


def symmetric(rng, K, integer):
    """A symmetric K x K fp64 matrix with a dominant diagonal (integer-valued: every step of the kernel is exact when
    the weights are dyadic)."""
    if integer:
        g = rng.integers(-4, 5, size=(K, K)).astype(F64)
        g = np.triu(g) + np.triu(g, 1).T
        g[np.arange(K), np.arange(K)] = rng.integers(20, 40, size=K)
    else:
        g = rng.standard_normal((K, K))
        g = np.triu(g) + np.triu(g, 1).T
        g[np.arange(K), np.arange(K)] = 3.0 + rng.random(K) * 5.0
    assert np.array_equal(g, g.T)
    return g


def lazy_case():
    """``krum_fixtures.nonint_case()`` with a lazy client: upload 0 is the round's model, unchanged."""
    case = kf.nonint_case()
    case.x[0] = case.L
    for e in case.layout.f_entries:
        case.uploads[0][e.index] = case.x[0, e.offset:e.offset + e.numel].reshape(e.shape).copy()
    return case


def ulps32(a, b, scale):
    """The largest |a - b| in units of the fp32 ulp of ``scale`` (the model's largest magnitude)."""
    return float(np.abs(a.astype(F64) - b.astype(F64)).max() / np.spacing(F32(scale)))

