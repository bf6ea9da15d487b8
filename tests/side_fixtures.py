"""Inputs of the exact tests of the int64 side-table kernels and the elementwise finishers, shared by the CPU half
(tests/test_side_oracle.py) and the device half (tests/test_gpu_side_kernels.py, tests/test_gpu_finish_kernels.py).
Numpy only; everything is a pure function of its arguments, so both halves see the same bytes.

int64 values come in classes spread over the element index q (class = q mod NCLS), so that every 64-thread
workgroup sees every class; within a class the value cycles over the client index k."""
import numpy as np

from oracle.cpu_reference import fedbuff_weight
from tests.side_kernel_models import F32, F64, I64, I64_MAX, I64_MIN, STRIDE_BLOCK, STRIDE_MAX_BLOCKS

POISON = 0x7EDCBA9876543210  # columns [Q:ldq] of the client rows: huge, so a stray read shows in any sum
SENT_I64 = -0x0123456789ABCDEF  # prefill of int64 outputs
SENT_F64 = -7.0e77  # ... of float64 outputs
SENT_F32 = F32(-7.0e33)  # ... of float32 outputs

NCLS = 12
_EXTREME = (7, 8, 9, 10)  # classes beyond 2^41 in magnitude: their q-FedAvg squares overflow float32


def _class_value(c, k, q, rng_small, rng_wide, last_q):
    if c == 0:
        return int(rng_small[k, q])  # counters below 100
    if c == 1:
        return (2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 24 + 3, -(2 ** 24 + 3))[(k + q // NCLS) % 4]  # fp32 ties / non-ties
    if c == 2:
        return (2 ** 25 + 2, 2 ** 25 + 6, -(2 ** 25 + 2), -(2 ** 25 + 6))[(k + q // NCLS) % 4]
    if c == 3:
        return (2 ** 40 + 2 ** 16, 2 ** 40 + 2 ** 16 + 1)[(k + q // NCLS) % 2]  # a tie, and the tie with a sticky bit
    if c == 4:
        return (2 ** 40 + 2 ** 16 + 1, -(2 ** 40 + 2 ** 16 + 1), 2 ** 40 + 2 ** 16)[(k + q // NCLS) % 3]
    if c == 6:
        return int(last_q)  # L == W: g = 0
    if c == 7:
        return (2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53 + 1))[(k + q // NCLS) % 3]  # fp64 ties
    if c == 8:
        return I64_MAX if k == 0 else (1, 0, 2)[k % 3]  # INT64_MAX + 1 wraps
    if c == 9:
        return I64_MIN if k == 0 else (-1, 0, -2)[k % 3]  # INT64_MIN - 1 wraps
    if c == 10:
        return (I64_MIN + 3, I64_MAX - 2)[(k + q // NCLS) % 2]  # L - W wraps for a small L of either sign
    return int(rng_wide[k, q])  # classes 5, 11: |x| < 2^40


def last_i64(Q, ldq=None, seed=0):
    """A model's int64 entries: every class that stays below 2^41 in magnitude (the q-FedAvg squares of a round
    whose differences stay there are finite)."""
    rng = np.random.default_rng(1000 + seed)
    small = rng.integers(-99, 100, size=(1, Q))
    wide = rng.integers(-2 ** 40 + 1, 2 ** 40, size=(1, Q))
    out = np.full(ldq or Q, SENT_I64, I64)
    for q in range(Q):
        c = q % NCLS
        out[q] = _class_value(5 if c in _EXTREME or c == 6 else c, 0, q, small, wide, 0)
    return out


def client_rows(K, Q, ldq, seed=0, extreme="all", last=None):
    """xi[K, ldq] int64: columns [0:Q] by class, columns [Q:ldq] POISON.  ``extreme``: 'all' rows carry the classes
    beyond 2^41, or only the 'odd' ones, or 'none' (the other rows draw |x| < 2^40 there)."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 100, size=(K, Q))
    wide = rng.integers(-2 ** 40 + 1, 2 ** 40, size=(K, Q))
    last = last_i64(Q, seed=seed) if last is None else last
    xi = np.full((K, ldq), POISON, I64)
    for k in range(K):
        for q in range(Q):
            c = q % NCLS
            if c in _EXTREME and (extreme == "none" or (extreme == "odd" and k % 2 == 0)):
                c = 5
            xi[k, q] = _class_value(c, k, q, small, wide, last[q])
    return xi


def fedbuff_weights(K):
    """async_aggregator.py:125 at staleness 0..8."""
    return np.array([fedbuff_weight(9, 9 - k % 9) for k in range(K)], F64)


# (K, Q, ldq): the seams of the element axis (one thread per element, 64 per workgroup), a K of 1, ldq != Q
ACCUM_CASES = [(1, 1, 1), (3, 63, 63), (2, 64, 71), (5, 65, 65), (3, 129, 136), (1, 65, 72)]
# ... and of the client axis as well (k_side_qfed_sq: one thread per client)
QFED_CASES = [(1, 65, 72), (2, 1, 1), (3, 63, 63), (65, 64, 64), (129, 129, 136), (3, 65, 65)]
QFED_LRS = (0.05, 1.0 / 3.0, 7e-5)


def splits(K):
    return sorted({1, K - 1}) if K >= 2 else []


def qfed_inputs(K, Q, ldq, i):
    """One q-FedAvg side case: client rows (extreme classes in odd rows only), the model, alpha, lr, and the
    non-zero prefill of sqnorm.  Case 2 has alpha = 0 throughout, so that first terms are +-0."""
    last = last_i64(Q, ldq, seed=i)
    xi = client_rows(K, Q, ldq, seed=50 + i, extreme="odd", last=last)
    rng = np.random.default_rng(70 + i)
    alpha = rng.uniform(0.3, 2.5, size=K).astype(F32)
    if i == 2:
        alpha[:] = 0
    sq0 = rng.uniform(0.5, 1.5, size=K).astype(F64)
    return dict(xi=xi, last=last, alpha=alpha, lr=QFED_LRS[i % 3], sqnorm0=sq0)


# ------------------------------------------------------------------------------------------------------------------
# close
# ------------------------------------------------------------------------------------------------------------------
_CLOSE_DOUBLES = (0.99999999, -0.99999999, 1.5, -1.5, 2.5, 16777216.9, 2.0 ** 53 + 1, 0.0, -0.0, 2.0 ** 63, -2.0 ** 63,
                  1e300, -1e300, np.nan, np.inf, -np.inf, 9.2e18, -9.2e18, 2.0 ** 24 + 1, 33554435.0, -3.999999999,
                  7.0)


def close_acc(Q, seed=0):
    """The accumulators a close call is handed: (acc_i, acc_d), each Q + 7 long.  In mode 1 acc_d is the input and
    carries the doubles on either side of float32 and int64 values; acc_i then holds other numbers."""
    acc_i = np.full(Q + 7, POISON, I64)
    acc_i[:Q] = client_rows(1, Q, Q, seed=200 + seed)[0]
    acc_d = np.full(Q + 7, 3.0e200, F64)
    rng = np.random.default_rng(300 + seed)
    acc_d[:Q] = rng.normal(size=Q) * 2.0 ** rng.integers(0, 45, size=Q)
    for q in range(Q):
        if q % 3 != 2:
            acc_d[q] = _CLOSE_DOUBLES[(q - q // 3) % len(_CLOSE_DOUBLES)]
    return acc_i, acc_d


# (Q, mode, denom): an integer count, a FedBuff denominator, and 0 (0/0 and +-x/0); every Q seam
CLOSE_CASES = [(1, 0, 3.0), (63, 0, 3.0), (64, 1, float(sum(fedbuff_weights(3)))), (65, 0, float(sum(fedbuff_weights(5)))),
               (129, 1, 1.0), (129, 0, 0.0), (65, 1, 0.0), (129, 1, 3.0)]
CLOSE_OUTPUTS = ("both", "cur", "model")


# ------------------------------------------------------------------------------------------------------------------
# FedYoGi on the side table
# ------------------------------------------------------------------------------------------------------------------
def yogi_hparams(tau):
    return dict(eta=3e-3, tau=tau, beta=0.9, omb=1.0 - 0.9, omb2=1.0 - 0.99)


# (Q, last given, first round is the init round, tau, outputs)
YOGI_CASES = [(1, True, True, 1e-3, "both"), (63, False, True, 1e-8, "step"), (64, True, False, 1e-3, "model"),
              (65, True, True, 1e-8, "both"), (129, True, False, 1e-8, "both"), (129, False, False, 1e-3, "none")]
YOGI_ROUNDS = 3


def yogi_inputs(Q, with_last, init, seed=0):
    """last (int64, Q + 7 long, or None), the three rounds' cur (float64, last + a gradient of magnitude 1e-6..30,
    both signs, some exactly 0), and the state a first round without init starts from (else NaN, as the device test
    prefills it).  Without init every 8th element has g*g == v exactly in the first round (v - g*g == 0)."""
    rng = np.random.default_rng(400 + seed)
    last = last_i64(Q, Q + 7, seed=seed) if with_last else None
    L = last[:Q].astype(F64) if with_last else np.zeros(Q, F64)
    curs = []
    for r in range(YOGI_ROUNDS):
        g = np.exp(rng.uniform(np.log(1e-6), np.log(30.0), size=Q)) * rng.choice([-1.0, 1.0], size=Q)
        g[5::16] = 0.0
        curs.append(L + g)
    if init:
        m0, v0 = np.full(Q + 7, np.nan, F64), np.full(Q + 7, np.nan, F64)
    else:
        m0, v0 = np.full(Q + 7, SENT_F64, F64), np.full(Q + 7, SENT_F64, F64)
        m0[:Q] = rng.normal(size=Q) * 0.1
        v0[:Q] = np.exp(rng.uniform(np.log(1e-6), np.log(10.0), size=Q))
        g_exact = np.array([1.5, -0.75, 2.25, 0.0078125])[np.arange(Q) // 8 % 4]
        sel = np.arange(Q) % 8 == 3
        curs[0][sel] = (L + g_exact)[sel]
        v0[:Q][sel] = (g_exact * g_exact)[sel]
        assert np.all((curs[0] - L)[sel] == g_exact[sel])  # |last| < 2^41: the sum is exact
    return dict(last=last, curs=curs, m0=m0, v0=v0)


# ------------------------------------------------------------------------------------------------------------------
# q-FedAvg finalize on the side table
# ------------------------------------------------------------------------------------------------------------------
FINALIZE_CASES = [(1, "near"), (65, "near"), (129, "near"), (64, "zero_hs"), (129, "huge"), (63, "nan_hs")]


def finalize_inputs(Q, kind, seed=0):
    """last, delta_s (Q + 7 long) and hs.  'near': quotients on both sides of integers and halves (hs[1] = 3);
    'zero_hs': hs[1] = 0, so quotients are NaN and +-inf; 'huge': quotients of +-1e19 (finite, beyond int64),
    +-9e18 (inside) and +-inf by overflow; 'nan_hs': hs[1] NaN."""
    last = last_i64(Q, Q + 7, seed=seed + 9)
    d = np.full(Q + 7, SENT_F32, F32)
    q = np.arange(Q)
    if kind == "near":
        hs = np.array([7.0, 3.0], F32)
        n = (q % 23 - 11).astype(F64)
        e = np.array([0.0, 2.0 ** -20, -2.0 ** -20, 0.5, -0.5, 0.5 + 2.0 ** -18, 1.0 / 3.0])[q % 7]
        d[:Q] = (3.0 * (n + e)).astype(F32)
    elif kind == "zero_hs":
        hs = np.array([2.0, 0.0], F32)
        d[:Q] = np.array([0.0, 1.5, -2.0, -0.0, 1e-40], F32)[q % 5]
    elif kind == "huge":
        hs = np.array([1.0, 1e-30], F32)
        d[:Q] = np.array([1e10, -1e10, 1e-11, -1e-11, 9e-12, -9e-12, 3e-30], F32)[q % 7]
    else:
        hs = np.array([1.0, np.nan], F32)
        d[:Q] = np.array([0.0, 1.0, -1.0], F32)[q % 3]
    return dict(last=last, delta_s=d, hs=hs)


# ------------------------------------------------------------------------------------------------------------------
# the fp32 finishers
# ------------------------------------------------------------------------------------------------------------------
STRIDE_SEAM = 4 * STRIDE_BLOCK * STRIDE_MAX_BLOCKS  # columns of one full trip of a stride_grid() launch
FA_YOGI_NT_MIN_BYTES = 256 << 20
# fa_yogi_step takes its non-temporal variant when P4 * 16 * 7 > FA_YOGI_NT_MIN_BYTES, P4 = ceil(P / 4)
NT_P4 = FA_YOGI_NT_MIN_BYTES // (16 * 7)  # the largest P4 of the plain variant
NT_SEAM = (4 * NT_P4, 4 * NT_P4 + 1)  # the last P of the plain variant and the first of the non-temporal one
assert NT_P4 * 16 * 7 <= FA_YOGI_NT_MIN_BYTES < (NT_P4 + 1) * 16 * 7 and (NT_SEAM[1] + 3) // 4 == NT_P4 + 1
FINISH_SMALL_P = (1, 3, 4, 5, 1023, 1024, 1025)
FINISH_SEAM_P = (STRIDE_SEAM, STRIDE_SEAM + 5)  # the largest P of one trip, and a ragged P whose loop makes a second
FINISH_HP = {k: float(F32(v)) for k, v in dict(eta=3e-3, tau=1e-8, beta=0.9, omb=1.0 - 0.9, omb2=1.0 - 0.99).items()}
FINISH_HS = np.array([5.0, 0.7], F32)  # hs[1] = 0.7f: quotients are inexact

# (cur, last, m, v) of the specials band: NaN, +-inf, +-0, denormals, g*g == v, v of 0 / negative / denormal
_Y_SPECIALS = [(np.nan, 0.0, 0.1, 1e-4), (np.inf, 0.0, 0.1, 1e-4), (-np.inf, 1.0, 0.1, 1e-4), (np.inf, np.inf, 0.0, 1.0),
               (0.0, -0.0, 0.0, 0.0), (-0.0, 0.0, -0.0, 1e-4), (1e-42, 0.0, 1e-41, 1e-43), (0.5, 0.0, 0.3, 0.25),
               (1.0, 1.5, -0.2, 0.25), (0.25, 0.0, 0.0, 0.0), (0.1, 0.0, np.inf, 1e-4), (0.1, 0.0, 0.1, -1.0),
               (0.1, 0.0, 0.1, np.nan), (3e-23, 0.0, 1e-30, 1e-45), (1e20, -1e20, 1.0, 1e38), (0.1, 0.0, 0.1, np.inf)]
_Q_SPECIALS = [(np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, np.inf), (np.inf, np.inf), (0.0, 0.0), (-0.0, 0.0),
               (0.0, -0.0), (1e-42, 1e-44), (1.0, 1e-45), (-1.0, -np.inf), (3e38, -3e38)]  # (last, delta)
_BAND = 1021  # the specials recur every _BAND columns, the first band ending at column _BAND - 7


def cols(P):
    return (P + 3) // 4 * 4


def _band(P, n):
    i = np.arange(P)
    j = (i + 7) % _BAND
    return i[j < n], j[j < n]


def yogi_step_inputs(P, seed=0):
    """cur, last, m0, v0: cols(P) + 4 floats each, columns [P:] NaN in cur / last (read, never used) and SENT_F32 in
    m0 / v0."""
    rng = np.random.default_rng(seed)
    n = cols(P) + 4
    last = np.full(n, np.nan, F32)
    cur = np.full(n, np.nan, F32)
    m0, v0 = np.full(n, SENT_F32, F32), np.full(n, SENT_F32, F32)
    last[:P] = rng.standard_normal(P, dtype=F32) * F32(0.05)
    cur[:P] = last[:P] + rng.standard_normal(P, dtype=F32) * F32(0.01)
    m0[:P] = rng.standard_normal(P, dtype=F32) * F32(0.01)
    v0[:P] = rng.uniform(1e-8, 1e-3, size=P).astype(F32)
    at, which = _band(P, len(_Y_SPECIALS))
    sp = np.array(_Y_SPECIALS, F32)
    cur[at], last[at], m0[at], v0[at] = sp[which, 0], sp[which, 1], sp[which, 2], sp[which, 3]
    return cur, last, m0, v0


def qfed_finalize_inputs(P, seed=0):
    rng = np.random.default_rng(seed + 1)
    n = cols(P) + 4
    last, delta = np.full(n, np.nan, F32), np.full(n, np.nan, F32)
    last[:P] = rng.standard_normal(P, dtype=F32) * F32(0.05)
    delta[:P] = rng.standard_normal(P, dtype=F32) * F32(3.0)
    at, which = _band(P, len(_Q_SPECIALS))
    sp = np.array(_Q_SPECIALS, F32)
    last[at], delta[at] = sp[which, 0], sp[which, 1]
    return last, delta


# ------------------------------------------------------------------------------------------------------------------
# the round-level model: 70 int64 elements (two workgroups), negative and > 2^24 values
# ------------------------------------------------------------------------------------------------------------------
ROUND_NAMES = ["conv.weight", "bn.counts", "bn.num_batches_tracked"]


def round_init():
    rng = np.random.default_rng(11)
    counts = client_rows(1, 69, 69, seed=12, extreme="none")[0]  # |x| < 2^41: ties, sticky bits, both signs
    assert np.any(counts < 0) and np.any(np.abs(counts) > 2 ** 24)
    return [rng.standard_normal((3, 11)).astype(F32), counts.reshape(3, 23), np.array(5, I64)]


def round_uploads(K, r):
    """K uploads of round r, each a list in state_dict order."""
    rows = client_rows(K, 69, 69, seed=20 + r, extreme="none")
    rng = np.random.default_rng(30 + r)
    return [[rng.standard_normal((3, 11)).astype(F32), rows[k].reshape(3, 23), np.array(5 + r + k, I64)]
            for k in range(K)]
