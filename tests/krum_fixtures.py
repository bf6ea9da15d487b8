"""The numpy restatement of include/fedkrum.h (Krum / Multi-Krum selection), shared by test_krum_plan.py and the GPU
tests: the plan of fk_gram, exact and fsum Gram references with the derived any-order error bound, and everything after
the Gram (dist2, scores, rank, c, n_sel, chain, out) bit for bit."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -53
MAX_K = 4096
ROW_TILE, STEP, TARGET_WGS, MIN_STEPS, MAX_WS = 64, 32, 2048, 4, 512 << 20

# ---- shapes of the GPU kernel tests ----------------------------------------------------------------------------------
GRAM_K = (3, 16, 17, 64, 65, 130)       # 130: three row tiles, so the tile (2, 1) has both indices above 0
P_SPLIT = 301                           # nsplit >= 2, a short last split, >= 2 steps in every split
GRAM_P = (1, 3, 4, 5, STEP - 1, STEP, STEP + 1, P_SPLIT)
NONINT_SHAPE = (40, 3001)               # non-integer data at a shape whose splits iterate
# fk_scores: K = 3, and below / at / above where the sorted width (a power of two >= K - 1) doubles at the wave (64),
# at the workgroup (256 lanes; 512 entries are one compare-exchange per lane) and at the LDS capacity (4096 entries)
SCORE_K = (3, 4, 5, 6, 64, 65, 66, 256, 257, 258, 512, 513, 514, 2049, 4095, 4096)


def plan(K: int, P: int) -> dict:
    """fk_gram_plan, restated."""
    T = -(-K // ROW_TILE)
    tiles = T * (T + 1) // 2
    steps = -(-P // STEP) if P > 0 else 1
    ns = min(-(-TARGET_WGS // tiles), -(-steps // MIN_STEPS))
    while ns > 1 and ns * K * K * 8 > MAX_WS:
        ns -= 1
    per = -(-steps // ns)
    nsplit = -(-steps // per)
    return dict(row_tile=ROW_TILE, tiles=tiles, nsplit=nsplit, split_cols=per * STEP, step_cols=STEP,
                last_steps=steps - (nsplit - 1) * per)


def workspace_bytes(K: int, P: int) -> int:
    return plan(K, P)["nsplit"] * K * K * 8


# ---- data ------------------------------------------------------------------------------------------------------------
def int_rows(rng, K, P, ld):
    """(x, L): L in small integers and asymmetric, d in {-3 .. 3}, x = L + d exact; NaN in the columns [P, ld)."""
    L = np.full(ld, np.nan, dtype=F32)
    L[:P] = rng.integers(-5, 9, size=P).astype(F32) + (np.arange(P) % 3).astype(F32)
    x = np.full((K, ld), np.nan, dtype=F32)
    x[:, :P] = L[:P] + rng.integers(-3, 4, size=(K, P)).astype(F32)
    return x, L


def normal_rows(rng, K, P, ld, scale=0.05):
    L = np.zeros(ld, dtype=F32)
    L[:P] = rng.standard_normal(P).astype(F32)
    x = np.zeros((K, ld), dtype=F32)
    x[:, :P] = L[:P] + rng.standard_normal((K, P)).astype(F32) * F32(scale)
    return x, L


def diffs(x, L, P):
    """d_k = x_k - L in fp32, columns [0, P)."""
    with np.errstate(all="ignore"):
        return (x[:, :P].astype(F32) - L[:P].astype(F32)).astype(F32)


# ---- the Gram --------------------------------------------------------------------------------------------------------
def gram_exact(d):
    """G of integer-valued finite d, exact: int64 numpy for small values, Python integers beyond.  float64[K, K];
    asserts that every entry is representable."""
    assert np.isfinite(d).all() and (d == np.rint(d)).all()
    if d.size == 0 or np.abs(d).max() < 2 ** 20:
        g = d.astype(np.int64) @ d.astype(np.int64).T
        assert np.abs(g).max(initial=0) < 2 ** 53
        return g.astype(F64)
    rows = [[int(v) for v in r] for r in d]
    K = len(rows)
    g = np.zeros((K, K), dtype=F64)
    for i in range(K):
        for j in range(i + 1):
            s = sum(a * b for a, b in zip(rows[i], rows[j]))
            assert int(float(s)) == s
            g[i, j] = g[j, i] = float(s)
    return g


def gram_fsum(d):
    """G by math.fsum over the products widened exactly to fp64 (correctly rounded sums)."""
    dd = d.astype(F64)
    K = dd.shape[0]
    g = np.zeros((K, K), dtype=F64)
    with np.errstate(all="ignore"):
        for i in range(K):
            for j in range(i + 1):
                prod = dd[i] * dd[j]
                g[i, j] = g[j, i] = math.fsum(prod) if np.isfinite(prod).all() else prod.sum()
    return g


def gram_ref(d):
    """The reference Gram: exact integers for integer-valued data, fsum for everything else."""
    if np.isfinite(d).all() and (d == np.rint(d)).all():
        return gram_exact(d)
    return gram_fsum(d)


def gram_bound(d):
    """float64[K, K]: the any-order summation bound P u / (1 - P u) * sum_p |d_i[p] d_j[p]| of include/fedkrum.h."""
    a = np.abs(d.astype(F64))
    P = d.shape[1]
    return P * U / (1.0 - P * U) * (a @ a.T) * (1.0 + 4 * P * U)  # (the last factor: this matmul's own rounding)


# ---- everything after the Gram: bit for bit --------------------------------------------------------------------------
def dist2_of(G):
    """float64[K, K] (the diagonal is unused and set to +inf)."""
    g = np.diag(G)
    with np.errstate(all="ignore"):
        v = (g[:, None] + g[None, :]) - 2.0 * G
        d2 = np.where(np.isnan(v), np.inf, np.where(v > 0, v, 0.0))
    np.fill_diagonal(d2, np.inf)
    return d2


def scores_of(G, f):
    K = G.shape[0]
    assert f >= 0 and 2 * f + 3 <= K
    d2 = dist2_of(G)
    srt = np.sort(d2, axis=1)  # (the diagonal's +inf sorts last; at most K - 2 entries are taken)
    sc = np.zeros(K, dtype=F64)
    for s in range(K - f - 2):  # one by one in ascending order
        sc = sc + srt[:, s]
    return sc


def scores_brute(G, f):
    """The same by a per-row Python loop (an independent route for test_krum_plan)."""
    K = G.shape[0]
    out = []
    for i in range(K):
        vals = []
        for j in range(K):
            if j == i:
                continue
            v = (float(G[i, i]) + float(G[j, j])) - 2.0 * float(G[i, j])
            vals.append(math.inf if v != v else (v if v > 0 else 0.0))
        s = 0.0
        for v in sorted(vals)[:K - f - 2]:
            s = s + v
        out.append(s)
    return np.asarray(out, dtype=F64)


def select_of(score, m):
    """(c float32[K], n_sel)."""
    K = len(score)
    order = np.lexsort((np.arange(K), score))
    rank = np.empty(K, dtype=np.int64)
    rank[order] = np.arange(K)
    c = (np.isfinite(score) & (rank < m)).astype(F32)
    return c, int((c != 0).sum())


def chain_of(d, c):
    chain = np.zeros(d.shape[1], dtype=F32)
    with np.errstate(all="ignore"):
        for k in range(d.shape[0]):
            if c[k] != 0:
                chain = (chain + (c[k] * d[k]).astype(F32)).astype(F32)
    return chain


def finish_of(chain, L, n_sel):
    if n_sel <= 0:
        return L.astype(F32).copy()
    with np.errstate(all="ignore"):
        return (L + (chain / F32(n_sel)).astype(F32)).astype(F32)


def krum_round(x, L, P, f, m, G=None):
    """dict(out, score, c, n_sel, G) of a whole round; ``G``: the Gram to continue from (the device's), else the
    reference Gram."""
    d = diffs(x, L, P)
    if G is None:
        G = gram_ref(d)
    score = scores_of(G, f)
    c, n_sel = select_of(score, m)
    out = finish_of(chain_of(d, c), L[:P].astype(F32), n_sel)
    return dict(out=out, score=score, c=c, n_sel=n_sel, G=G)


def score_bound(d, f):
    """float64[K]: a bound on |score_device - score_reference| that follows from gram_bound alone.  dist2's error is at
    most e_ij = B_ii + B_jj + 2 B_ij + 4 u (G_ii + G_jj + 2 |G_ij|) (the three fp64 ops of v on either side); the sum of
    the n smallest is 1-Lipschitz in every entry, so the exact sums differ by at most sum_j e_ij; each sequential sum
    of n non-negative terms is within n u of its exact value, relatively."""
    G = gram_fsum(d)
    B = gram_bound(d)
    g, b = np.diag(G), np.diag(B)
    e = b[:, None] + b[None, :] + 2 * B + 4 * U * (g[:, None] + g[None, :] + 2 * np.abs(G))
    np.fill_diagonal(e, 0.0)
    n = d.shape[0] - f - 2
    tot = e.sum(axis=1)
    return tot + 2 * (n + 1) * U * (scores_of(G, f) + tot)


def poisoned_int_round(rng, K, P, L):
    """K = 11 style rows: honest integer updates in {-3 .. 3} around a common direction, and three attackers — row 2
    scaled by 2^50, row 5 all NaN, row 8 sign-flipped and scaled by 8.  Returns (x, attackers)."""
    base = rng.integers(-2, 3, size=P)
    d = (base + rng.integers(-1, 2, size=(K, P))).astype(F32)
    x = (L[:P] + d).astype(F32)
    x[2] = (L[:P] + d[2] * F32(2.0 ** 50)).astype(F32)
    x[5] = np.nan
    x[8] = (L[:P] - F32(8) * d[8]).astype(F32)
    return x, (2, 5, 8)


# ---- whole rounds on a small model -----------------------------------------------------------------------------------
NONINT = (12, 3, 6)  # (K, f, m) of the non-integer round


class Case:
    """A small model (fp32 parameters, BatchNorm buffers, an int64 ``num_batches_tracked``), its layout, and K uploads
    as per-entry arrays and as flat fp32 rows in the bucket's order.  ``integer``: the model's fp32 entries are small
    integers and the uploads are ``poisoned_int_round``'s; otherwise normal updates of scale 0.05 around a drift, the
    last ``far`` of them displaced."""

    def __init__(self, K, seed=0, integer=True, far=0):
        import torch
        from collections import OrderedDict

        from fedscale_amd.bucket import BucketLayout

        self.torch = torch
        self.integer = integer
        self.model = self.net()
        sd = self.model.state_dict()
        self.names, self.init = list(sd.keys()), [v.clone() for v in sd.values()]
        self.layout = BucketLayout.from_state_dict(OrderedDict(zip(self.names, self.init)))
        self.P, self.K = self.layout.P, K
        assert self.P == 182 and len(self.layout.i_entries) == 1
        self.L = self.flat([v.numpy() for v in self.init])
        rng = np.random.default_rng(70 + seed)
        if integer:
            assert (self.L == np.rint(self.L)).all() and np.abs(self.L).max() <= 8
            self.x, self.bad = poisoned_int_round(rng, K, self.P, self.L)
        else:
            drift = rng.standard_normal(self.P).astype(F32) * F32(0.02)
            d = drift + rng.standard_normal((K, self.P)).astype(F32) * F32(0.05)
            for k in range(K - far, K):
                d[k] += F32(0.4) * rng.standard_normal(self.P).astype(F32)
            self.x, self.bad = (self.L + d).astype(F32), tuple(range(K - far, K))
        self.uploads = []
        for k in range(K):
            vals = []
            for i, v in enumerate(self.init):
                a = v.numpy()
                if a.dtype == np.int64:
                    vals.append(np.asarray(10 + 2 * k, dtype=np.int64).reshape(a.shape))
                    continue
                e = next(e for e in self.layout.f_entries if e.index == i)
                vals.append(self.x[k, e.offset:e.offset + e.numel].reshape(a.shape).copy())
            self.uploads.append(vals)
        tot = sum(10 + 2 * k for k in range(K))
        self.side = int(np.float64(tot) / np.float64(K))  # the int64 entry: plain FedAvg's, denominator K

    def net(self):
        torch = self.torch

        class _Net(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.conv = torch.nn.Conv2d(1, 3, 3)
                self.bn = torch.nn.BatchNorm2d(3)
                self.fc = torch.nn.Linear(27, 5)

        torch.manual_seed(5)
        m = _Net()
        if self.integer:
            with torch.no_grad():
                for p in m.parameters():
                    p.copy_(torch.clamp(torch.round(p * 16), -8, 8))
        return m

    def flat(self, values):
        buf = np.zeros(self.P, dtype=F32)
        for e in self.layout.f_entries:
            buf[e.offset:e.offset + e.numel] = np.asarray(values[e.index], dtype=F32).reshape(-1)
        return buf

    def flat_of_weights(self, got):
        return self.flat([t.numpy() for t in got])

    def upload(self, k, form="dict"):
        return dict(zip(self.names, self.uploads[k])) if form == "dict" else list(self.uploads[k])

    def adapter(self, capacity=None, policy=None, args=None):
        from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
        from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

        opt = TorchServerOptimizer(policy, args, "cuda:0") if policy else None
        return TorchModelAdapter(self.net(), optimizer=opt, device="cuda:0", staging_capacity=capacity)


def nonint_case():
    K, f, m = NONINT
    return Case(K, seed=1, integer=False, far=f)
