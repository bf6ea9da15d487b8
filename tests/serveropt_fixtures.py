"""The numpy float32 restatement of the adaptive server optimizers (include/fedserveropt.h): FedAdam, FedAdagrad and
FedAvgM, one IEEE operation per line, every array float32 throughout — ``np.sqrt`` and ``/`` on float32 are the
correctly rounded operations, as the kernel's are.  Plus the bit-pattern comparison the exact tests use (NaNs equal
by class), the plan's restatement, and the edge-case inputs."""
import numpy as np

F32 = np.float32
RULES = ("adam", "adagrad", "avgm")
STREAMS = {"adam": 7, "adagrad": 7, "avgm": 5}  # float4 streams a step reads plus writes
NT_MIN_BYTES = 256 << 20
BLOCK, MAX_GRID = 256, 8192


def hparams(eta=1e-2, tau=1e-3, beta=0.9, beta2=0.99, v0=None) -> dict:
    """The scalars as fp32: 1 - beta, 1 - beta2 and the default v0 = tau*tau formed in double first."""
    v0 = tau * tau if v0 is None else v0
    return dict(eta=F32(eta), tau=F32(tau), beta=F32(beta), omb=F32(1.0 - beta), beta2=F32(beta2),
                omb2=F32(1.0 - beta2), v0=F32(v0))


def step(rule, cur, last, m, v, hp, init):
    """One step: (m', v', out), float32 arrays; ``v'`` is None for "avgm".  ``init``: m = 0 and v = v0, the arrays
    passed are not read."""
    cur, last = np.asarray(cur, F32), np.asarray(last, F32)
    m = np.zeros_like(cur) if init else np.asarray(m, F32)
    with np.errstate(all="ignore"):
        g = cur - last
        if rule == "avgm":
            bm = hp["beta"] * m
            m1 = bm + g
            em = hp["eta"] * m1
            out = last + em
            return m1, None, out
        v = np.full_like(cur, hp["v0"]) if init else np.asarray(v, F32)
        g2 = g * g
        bm = hp["beta"] * m
        og = hp["omb"] * g
        m1 = bm + og
        if rule == "adam":
            bv = hp["beta2"] * v
            o2 = hp["omb2"] * g2
            v1 = bv + o2
        elif rule == "adagrad":
            v1 = v + g2
        else:
            raise ValueError(rule)
        s = np.sqrt(v1)
        den = s + hp["tau"]
        q = m1 / den
        eq = hp["eta"] * q
        out = last + eq
    for a in (m1, v1, out):
        assert a.dtype == F32
    return m1, v1, out


def step64(rule, cur, last, m, v, hp, init):
    """The same formulas in float64 (the fp32 scalars widened, no intermediate rounding): (m', v', out)."""
    h = {k: np.float64(x) for k, x in hp.items()}
    cur, last = np.asarray(cur, np.float64), np.asarray(last, np.float64)
    m = np.zeros_like(cur) if init else np.asarray(m, np.float64)
    g = cur - last
    if rule == "avgm":
        m1 = h["beta"] * m + g
        return m1, None, last + h["eta"] * m1
    v = np.full_like(cur, h["v0"]) if init else np.asarray(v, np.float64)
    m1 = h["beta"] * m + h["omb"] * g
    v1 = h["beta2"] * v + h["omb2"] * (g * g) if rule == "adam" else v + g * g
    return m1, v1, last + h["eta"] * (m1 / (np.sqrt(v1) + h["tau"]))


def bits_equal(a, b) -> bool:
    """Whether two float32 arrays hold the same bit patterns, a NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def first_difference(a, b) -> str:
    """Where and how two arrays differ, for an assertion's message."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))
    idx = np.flatnonzero(bad)
    if idx.size == 0:
        return "equal"
    i = int(idx[0])
    return f"{idx.size} of {a.size} differ; first at {i}: {a[i]!r} ({a.view(np.uint32)[i]:#010x}) != " \
           f"{b[i]!r} ({b.view(np.uint32)[i]:#010x})"


def plan(rule, P, init=False, nt=None) -> dict:
    """What fso_step_plan reports, restated."""
    P4 = (P + 3) // 4
    blocks = min((P4 + BLOCK - 1) // BLOCK, MAX_GRID)
    trips = -(-P4 // (blocks * BLOCK)) if blocks else 0
    s = STREAMS[rule]
    policy = P4 * 16 * s > NT_MIN_BYTES
    unread = (1 if rule == "avgm" else 2) if init else 0
    return dict(blocks=blocks, trips=trips, nt=bool(P > 0 and (policy if nt is None else nt)),
                bytes=P4 * 16 * (s - unread))


LAST_ONE_TRIP_P = MAX_GRID * BLOCK * 4       # the last P with one grid-stride trip; + 1 is the first with two


def last_cached_P(rule) -> int:
    """The last P whose step is cached by policy (+ 1 is the first non-temporal one)."""
    return NT_MIN_BYTES // (16 * STREAMS[rule]) * 4


def inputs(P, seed):
    """(cur, last, m, v) of ld = round_up(P, 4) float32 each, with the contract's edge cases in fixed columns where P
    has them: g = 0, v = 0, denormal g and v, +inf, -inf and NaN (one column each)."""
    ld = (P + 3) // 4 * 4
    rng = np.random.default_rng(seed)
    last = rng.standard_normal(ld).astype(F32)
    cur = (last + (rng.standard_normal(ld) * np.ldexp(1.0, rng.integers(-12, 2, ld))).astype(F32)).astype(F32)
    m = (rng.standard_normal(ld) * 0.1).astype(F32)
    v = (rng.random(ld) * np.ldexp(1.0, rng.integers(-20, 2, ld))).astype(F32)

    def put(col, **kw):
        if col < ld:
            for k, x in kw.items():
                {"cur": cur, "last": last, "m": m, "v": v}[k][col] = x

    put(0, cur=last[0])                                        # g = 0
    put(1, v=0.0)                                              # v = 0 with tau > 0
    put(2, cur=F32(1e-41), last=F32(0.0), m=0.0, v=F32(3e-42))  # denormal g and v (and so m' and v')
    put(5, cur=F32(np.inf))
    put(6, cur=F32(-np.inf))
    put(7, cur=F32(np.nan))
    put(8, cur=last[8] if 8 < ld else 0, v=0.0, m=0.0)         # g = 0, m = 0, v = 0: 0 / tau
    put(9, v=F32(np.inf))
    put(10, m=F32(np.nan))
    return cur, last, m, v
