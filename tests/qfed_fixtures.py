"""fa_qfed_accumulate restated in numpy, in the kernel's own order of operations (k_qfed_accum<WIDE, CHAIN, GLDS, QV>
and the gather kernels of fedscale_amd/csrc/fedagg.hip), with the shapes that reach each of its forms.  Numpy only:
nothing here imports the library or the oracle.

The order the restatement pins, per client and column window:
  lane      fp32 squares of the quotients g = (last - x) / lr; each float4 column gives (x^2 + y^2) + (z^2 + w^2);
            PART / 4 consecutive float4 columns j of the lane chain into one fp32 partial; the partials are added to an
            fp64 accumulator in j order (lanes and j >= sw outside the row add +0.0);
  wave      the 64 lane sums fold pairwise over lane bit 5, then 4, 3, 2, 1, 0 (the multi-reduce butterfly: which side
            keeps and which sends is irrelevant, the adds commute);
  workgroup ((w0 + w1) + w2) + w3, one row of QF_GRID per workgroup (a workgroup without a tile writes 0.0);
  window    16 segment sums of 16 rows each, from 0.0 in row order, then the 16 segments from 0.0 in order;
  call      sqnorm[k] plus the window sums in window order (the deferred and the per-window gathers alike).
delta and chain are per column in arrival order in fp32.  The fast division is correctly rounded wherever the kernel
uses it, so the IEEE quotient stands for both; which waves redo a client is modelled only for the planted mistake
that needs it."""
import numpy as np

F32, F64 = np.float32, np.float64

QF_V = 16  # QF_V: float4 columns per lane and tile of the plain launches
QF_CHAIN_V = 8  # QF_CHAIN_V: the same of the chain launches
QF_G = 4  # QF_G: clients per multi-reduce group
QF_GRID = 256  # QF_GRID = QF_CHAIN_GRID: workgroups of a launch, 4 waves each
QF_PART = 4  # QF_PART: squares per fp32 partial, plain launches
QF_CHAIN_PART = 8  # QF_CHAIN_PART: the same, chain launches
QF_GATHER_SEG = 16  # QF_GATHER_SEG: segments the partial rows are summed in
QF_MAXK = 2048  # QF_MAXK: clients per call
QF_GWIN_MAX = 1024  # QF_GWIN_MAX: windows the wave-per-client window fold takes
QF_WIDE_BYTES = 1 << 31  # QF_WIDE_BYTES: QF_G rows within it share one buffer descriptor
QF_WS_ROWS_ONE = 2048 + 32  # qfed_ws_one: rows of K doubles in the one-window workspace (k_qfed_accum2's figure)
FAST_LR = (F32(9.5367432e-07), F32(1048576.0))  # fa_qfed_accumulate: the constant-divisor division's range of lr

MISTAKES = ("lane_left_out", "tail_client_shifted", "wave_missing", "partials_of_8", "segments_of_8",
            "sqnorm_overwritten", "sw_off_by_one", "redo_keeps_acc", "pad_columns_left_out")


def window_cols(chain):
    """qfed_window: one round of full-width tiles, 256 * 4 * qv * 256 columns."""
    return QF_GRID * 4 * (QF_CHAIN_V if chain else QF_V) * 256


def round_up4(P):
    return (P + 3) // 4 * 4


def plan(ld, P, chain):
    """The column windows of one call (launch_qfed1) and each one's tiles: a list of dicts w0, cols, P4, S, sw, ntiles,
    qv.  Tile t is workgroup t's; its wave w owns strips [(4 t + w) sw, (4 t + w + 1) sw) below S (strips_of)."""
    assert P >= 1 and ld >= P and ld % 4 == 0
    assert ld * 4 * QF_G <= QF_WIDE_BYTES, "the per-row-descriptor path is left to the big-row test"
    qv = QF_CHAIN_V if chain else QF_V
    win = min(P, window_cols(chain))
    out = []
    for w0 in range(0, P, win):
        cols = min(win, P - w0)
        P4 = (cols + 3) // 4
        S = (P4 + 63) // 64
        r = -(-S // (QF_GRID * 4 * qv))
        strips = -(-S // (QF_GRID * r))
        sw = min(max((strips + 3) // 4, 1), qv)
        ntiles = -(-S // (4 * sw))
        # the product build's window is one round, so the tile loop of a workgroup runs at most once
        assert r == 1 and ntiles <= QF_GRID, (P, chain, r, ntiles)
        out.append(dict(w0=w0, cols=cols, P4=P4, S=S, sw=sw, ntiles=ntiles, qv=qv))
    return out


def strips_of(win, wg, wave):
    """The strips (of 64 float4 columns) that wave ``wave`` of workgroup ``wg`` sums in window ``win``."""
    if wg >= win["ntiles"]:
        return range(0)
    lo = (wg * 4 + wave) * win["sw"]
    return range(min(lo, win["S"]), min(lo + win["sw"], win["S"]))


def workspace_bytes(K, ld=0, P=0):
    """fa_qfed_workspace_bytes."""
    b = QF_WS_ROWS_ONE * K * 8
    if ld >= P > 0:
        for chain in (False, True):
            b = max(b, deferred_bytes(K, P, chain))
    return b


def deferred_bytes(K, P, chain):
    return -(-P // window_cols(chain)) * (QF_GRID + QF_GATHER_SEG) * K * 8


def gather_form(K, P, chain, ws_bytes):
    """Which gather kernels a call runs: 'per_window' (k_qfed_gather_seg + k_qfed_gather after every launch), or one
    pair at the end, 'deferred_wave' (k_qfed_gather_win_wave) or 'deferred_thread' (k_qfed_gather_win)."""
    nwin = -(-P // window_cols(chain))
    if nwin == 1 or ws_bytes < deferred_bytes(K, P, chain):
        return "per_window"
    return "deferred_wave" if nwin <= QF_GWIN_MAX else "deferred_thread"


def _window_norms(g, t, win, chain, fast, mistake):
    """Per-client sums of squares of one window: g (K, 4 P4) quotients, t the differences they came from."""
    K = g.shape[0]
    P4, S, sw, nt, qv = win["P4"], win["S"], win["sw"], win["ntiles"], win["qv"]
    part = QF_CHAIN_PART if chain else QF_PART
    if mistake == "partials_of_8" and not chain:
        part = 8
    m = part // 4
    lim = sw + (1 if mistake == "sw_off_by_one" and sw < qv else 0)
    jn = -(-lim // m) * m  # partials wholly past sw add +0.0 to a sum that is never -0.0: left out
    ti, wi, ji = np.arange(nt)[:, None, None], np.arange(4)[None, :, None], np.arange(jn)[None, None, :]
    strip = (ti * 4 + wi) * sw + ji
    idx = np.where((ji < lim) & (strip < S), strip, S)  # S: a strip of zeros (the out-of-range loads)

    def by_lane(v, dtype):  # (K, P4) per float4 column -> (K, nt, 4, jn, 64) per tile, wave, j and lane
        buf = np.zeros((K, (S + 1) * 64), dtype=dtype)
        buf[:, :P4] = v
        return buf.reshape(K, S + 1, 64)[:, idx]

    q = (g * g).reshape(K, P4, 4)
    s4 = by_lane((q[:, :, 0] + q[:, :, 1]) + (q[:, :, 2] + q[:, :, 3]), F32).reshape(K, nt, 4, jn // m, m, 64)
    p = s4[..., 0, :]
    for i in range(1, m):
        p = p + s4[..., i, :]
    acc = np.zeros((K, nt, 4, 64), dtype=F64)
    for jj in range(jn // m):
        acc = acc + p[..., jj, :].astype(F64)
    if mistake == "redo_keeps_acc":
        # the waves that redo a client with the IEEE division (all of them when lr is outside the fast range; else
        # those holding a denormal, huge or infinite difference) go through the partials again from the first sum
        a = np.abs(t)
        bad = ((a != 0) & ((a < F32(2.0 ** -80)) | (a >= F32(2.0 ** 80)))).reshape(K, P4, 4).any(axis=2)
        redo = by_lane(bad, bool).any(axis=(3, 4)) if fast else np.ones((K, nt, 4), dtype=bool)
        again = acc
        for jj in range(jn // m):
            again = again + p[..., jj, :].astype(F64)
        acc = np.where(redo[..., None], again, acc)
    v = acc
    for half in (32, 16, 8, 4, 2, 1):
        hi = v[..., half:]
        if mistake == "lane_left_out" and half == 8:
            hi = hi.copy()
            hi[..., 3] = 0.0
        v = v[..., :half] + hi
    y = v[..., 0]  # (K, nt, 4): sq[wave][k] of workgroup t, 0.0 + y
    if mistake == "tail_client_shifted" and K % QF_G:
        kg = K - K % QF_G
        y = y.copy()
        y[kg + 1:] = y[kg:K - 1]
        y[kg] = 0.0
    wg = (y[..., 0] + y[..., 1]) + y[..., 3] if mistake == "wave_missing" else \
        ((y[..., 0] + y[..., 1]) + y[..., 2]) + y[..., 3]
    rows = np.zeros((K, QF_GRID), dtype=F64)
    rows[:, :nt] = wg
    rps = 8 if mistake == "segments_of_8" else QF_GRID // QF_GATHER_SEG
    rows = rows[:, :QF_GATHER_SEG * rps].reshape(K, QF_GATHER_SEG, rps)
    seg = np.zeros((K, QF_GATHER_SEG), dtype=F64)
    for r in range(rps):
        seg = seg + rows[:, :, r]
    tot = np.zeros(K, dtype=F64)
    for b in range(QF_GATHER_SEG):
        tot = tot + seg[:, b]
    return tot


def accumulate(x, last, alpha, lr, chain, delta0=None, chain0=None, sqnorm0=None, P=None, mistake=None):
    """One fa_qfed_accumulate call over x[:, :P] (rows of x.shape[1] floats): (delta, chain, sqnorm), delta and chain
    over the 4 ceil(P / 4) columns the kernel reads and writes.  ``delta0`` given: the call carries FA_ACCUMULATE."""
    K, ld = x.shape
    P = ld if P is None else P
    C = round_up4(P)
    assert 1 <= K <= QF_MAXK and x.dtype == F32 and last.dtype == F32 and alpha.dtype == F32
    assert (chain0 is not None) == (chain and delta0 is not None)
    lr = F32(lr)
    fast = bool(FAST_LR[0] <= lr <= FAST_LR[1])
    with np.errstate(all="ignore"):
        t = last[None, :C] - x[:, :C]
        g = t / lr
        d = None if delta0 is None else delta0[:C].copy()
        c = None if chain0 is None else chain0[:C].copy()
        for k in range(K):
            term = alpha[k] * g[k]
            d = term if d is None else d + term
            if chain:
                c = x[k, :C].copy() if c is None else c + x[k, :C]
        if mistake == "pad_columns_left_out":
            g = g.copy()
            g[:, P:] = 0
        sq = np.zeros(K, dtype=F64) if sqnorm0 is None or mistake == "sqnorm_overwritten" else \
            np.asarray(sqnorm0, dtype=F64).copy()
        for win in plan(ld, P, chain):
            a, b = win["w0"], win["w0"] + 4 * win["P4"]
            sq = sq + _window_norms(g[:, a:b], t[:, a:b], win, chain, fast, mistake)
    return d, c, sq


# ---- shapes ---------------------------------------------------------------------------------------------------------
PAD = 60  # floats of a row past the 4 ceil(P / 4) columns the kernel may touch (NaN in x and last)
SPECIAL_P = 70001  # 274 strips: sw 1, 69 tiles
SPECIAL_AT = {  # the poked columns of the "specials" rows: client -> ((column, value), ...)
    0: ((200 * 256 + 9, F32(3e-41)),),  # tile 50, wave 0: a lone denormal, so one redone wave keeps a finite norm
    1: ((14 * 256 + 6, F32(1e-40)), (14 * 256 + 116, F32(-2.0 ** 81))),  # tile 3, wave 2: a denormal and a huge one
    4: ((161 * 256 + 4, F32(2.0 ** -130)), (161 * 256 + 84, F32(2.0 ** 90))),  # tile 40, wave 1
    2: ((100, F32(np.inf)), (60000, F32(-np.inf))),
    3: ((5000, F32(np.nan)),),
}


def _case(name, K, P, chain, why, kind="normal", lr=0.05, calls=1, ws="call", **cond):
    return dict(name=name, K=K, P=P, chain=chain, kind=kind, lr=lr, calls=calls, ws=ws, why=why, cond=cond)


def _tile_P(sw):
    """The least P whose single window runs tiles of ``sw`` strips per wave: S = 1024 (sw - 1) + 1 strips, the last
    strip one float4 wide and that float4 one column wide (a ragged strip and a ragged float4)."""
    return 262144 * (sw - 1) + 1


def _shapes():
    s = []
    for chain in (False, True):
        kind, qv, win = ("chain" if chain else "plain"), (QF_CHAIN_V if chain else QF_V), window_cols(chain)
        s.append(_case(f"sw1_every_wave_{kind}", 5, 262144, chain, "S = 1024: every wave of every workgroup owns one "
                       "whole strip", sw=(1,), ntiles=(256,), nwin=1, gather="per_window"))
        s.append(_case(f"sw2_s1025_{kind}", 5, _tile_P(2), chain, "S = 1025: sw 2, 129 tiles, the last tile's waves "
                       "partly empty", sw=(2,), ntiles=(129,), nwin=1, gather="per_window"))
        for sw in ((3, 7, 8) if chain else (3, 8, 15, 16)):
            s.append(_case(f"sw{sw}_{kind}", 5, _tile_P(sw), chain, f"the least P with tiles of {sw} strips per wave",
                           sw=(sw,), ntiles=(-(-(1024 * (sw - 1) + 1) // (4 * sw)),), nwin=1, gather="per_window"))
        s.append(_case(f"full_window_{kind}", 5, win, chain, "exactly one full window", sw=(qv,), ntiles=(256,),
                       nwin=1, gather="per_window"))
        for ws in ("call", "one"):
            # two windows' partials fit the one-window workspace too (2 x 272 rows < 2080): both sizes defer
            s.append(_case(f"window_plus5_{kind}_ws_{ws}", 5, win + 5, chain, "a full window and a second of two "
                           "float4", ws=ws, sw=(qv, 1), ntiles=(256, 1), nwin=2, gather="deferred_wave"))
    # per-window gathers over several windows need more windows than the one-window workspace holds: 8 at the least
    s.append(_case("eight_windows_chain_ws_one", 1, 7 * window_cols(True) + 5, True, "the fewest windows the "
                   "one-window workspace cannot hold: a gather pair after every launch", ws="one",
                   sw=(8,) * 7 + (1,), ntiles=(256,) * 7 + (1,), nwin=8, gather="per_window"))
    for P, S, nt in ((3, 1, 1), (257, 2, 1), (1025, 5, 2)):
        for K in (1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 2047, 2048):
            for chain in (False, True):
                s.append(_case(f"k{K}_p{P}_{'chain' if chain else 'plain'}", K, P, chain, "K edge: the multi-reduce "
                               "tail, the gather grids, the partial-row loop, the LDS table", calls=2, sw=(1,),
                               ntiles=(nt,), nwin=1, gather="per_window"))
    for chain in (False, True):
        kind, win = ("chain" if chain else "plain"), window_cols(chain)
        s.append(_case(f"int_sw1_every_wave_{kind}", 5, 262144, chain, "integer data: exact in any order",
                       kind="integer", lr=0.25, calls=2, sw=(1,), ntiles=(256,), nwin=1, gather="per_window"))
        s.append(_case(f"int_sw2_s1025_{kind}", 5, _tile_P(2), chain, "integer data: exact in any order",
                       kind="integer", lr=0.25, calls=2, sw=(2,), ntiles=(129,), nwin=1, gather="per_window"))
        s.append(_case(f"int_window_plus5_{kind}", 5, win + 5, chain, "integer data over two windows", kind="integer",
                       lr=0.25, sw=(QF_CHAIN_V if chain else QF_V, 1), ntiles=(256, 1), nwin=2,
                       gather="deferred_wave"))
        s.append(_case(f"int_k2047_p257_{kind}", 2047, 257, chain, "integer data at a K edge", kind="integer",
                       lr=0.25, calls=2, sw=(1,), ntiles=(1,), nwin=1, gather="per_window"))
        for lr in (0.05, 2.0 ** -21, 3e25):
            s.append(_case(f"specials_lr{lr:.3g}_{kind}", 5, SPECIAL_P, chain, "denormal, huge, infinite and NaN "
                           "differences; lr inside and outside the fast division's range", kind="specials", lr=lr,
                           sw=(1,), ntiles=(69,), nwin=1, gather="per_window"))
        s.append(_case(f"pad_columns_counted_{kind}", 5, 1025, chain, "non-zero columns in [P, 4 ceil(P / 4)): the "
                       "kernel reads, squares and chains them", kind="padded", sw=(1,), ntiles=(2,), nwin=1,
                       gather="per_window"))
    return s


SHAPES = _shapes()
BY_NAME = {c["name"]: c for c in SHAPES}
assert len(BY_NAME) == len(SHAPES)

# the listed shape at which each planted mistake changes an asserted bit
SEEN_BY = {
    "lane_left_out": "sw2_s1025_plain",
    "tail_client_shifted": "k5_p1025_plain",
    "wave_missing": "sw2_s1025_chain",
    "partials_of_8": "sw2_s1025_plain",
    "segments_of_8": "sw2_s1025_chain",
    "sqnorm_overwritten": "k5_p1025_chain",
    "sw_off_by_one": "sw2_s1025_plain",
    "redo_keeps_acc": "specials_lr0.05_plain",  # by client 0: its redone wave's norm stays finite
    "pad_columns_left_out": "pad_columns_counted_plain",
}


def ld_of(case):
    return round_up4(case["P"]) + PAD


def ws_bytes_of(case):
    ld = ld_of(case)
    return workspace_bytes(case["K"], ld, case["P"]) if case["ws"] == "call" else workspace_bytes(case["K"])


def make(case):
    """The inputs of a case: x (calls, K, ld), last (ld,), alpha (calls, K), lr, sqnorm0 (K,).  Columns [P, 4 ceil(P/4))
    of x and last are zero (the bucket contract) except for kind "padded"; [4 ceil(P/4), ld) hold NaN."""
    K, P, n, kind = case["K"], case["P"], case["calls"], case["kind"]
    C, ld = round_up4(P), ld_of(case)
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(case["name"]))
    rng = np.random.default_rng(seed)
    x = np.full((n * K, ld), np.nan, dtype=F32)
    last = np.full(ld, np.nan, dtype=F32)
    x[:, P:C] = 0
    last[P:C] = 0
    if kind == "integer":
        x[:, :P] = rng.integers(-8, 9, size=(n * K, P)).astype(F32)
        last[:P] = rng.integers(-8, 9, size=P).astype(F32)
        alpha = rng.integers(1, 5, size=n * K).astype(F32)
        sq0 = 0.5 + 0.25 * np.arange(K, dtype=F64)
    else:
        # the base-plus-noise rows of test_gpu_properties
        base = rng.standard_normal(P, dtype=F32) * F32(0.05)
        for k in range(n * K):
            x[k, :P] = base + rng.standard_normal(P, dtype=F32) * F32(0.01)
        last[:P] = x[:min(n * K, 8), :P].mean(axis=0, dtype=F32) + F32(0.001)
        alpha = np.float_power(rng.uniform(0.5, 2.0, size=n * K) + 1e-10, 1.0).astype(F32)
        sq0 = 1.0 / 3.0 + np.arange(K, dtype=F64) / 7.0
    if kind == "padded":
        x[:, P:C] = rng.standard_normal((n * K, C - P), dtype=F32)
        last[P:C] = rng.standard_normal(C - P, dtype=F32)
    clean = None
    if kind == "specials":
        for k, pokes in SPECIAL_AT.items():
            for col, v in pokes:
                if np.isfinite(v) and abs(v) < 1:
                    last[col] = 0  # the difference is the poked denormal itself
        clean = x.copy()
        for k, pokes in SPECIAL_AT.items():
            for col, v in pokes:
                x[k, col] = v
    return dict(x=x.reshape(n, K, ld), last=last, alpha=alpha.reshape(n, K), lr=case["lr"], sqnorm0=sq0,
                clean=None if clean is None else clean.reshape(n, K, ld))


def reference(case, data, mistake=None, x=None):
    """The restated outputs after each call of the case: a list of (delta, chain, sqnorm)."""
    x = data["x"] if x is None else x
    d = c = None
    sq = data["sqnorm0"]
    outs = []
    for i in range(case["calls"]):
        d, c, sq = accumulate(x[i], data["last"], data["alpha"][i], data["lr"], case["chain"], delta0=d, chain0=c,
                              sqnorm0=sq, P=case["P"], mistake=mistake)
        outs.append((d, c, sq))
    return outs


def integer_norms(case, data):
    """Kind "integer": the norms as plain integer sums, in no particular order."""
    sq = data["sqnorm0"].copy()
    P, inv = case["P"], int(round(1 / case["lr"]))
    for i in range(case["calls"]):
        gi = (data["last"][None, :P].astype(np.int64) - data["x"][i][:, :P].astype(np.int64)) * inv
        sq = sq + (gi * gi).sum(axis=1).astype(F64)
    return sq


def same_bits(got, want):
    """Equal bits, NaN meeting NaN (of any payload)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    u = np.uint32 if got.dtype == F32 else np.uint64
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u)[~nan], want.view(u)[~nan]))
