"""The launch plan and the tile arithmetic of k_reduce (fedscale_amd/csrc/fedagg.hip) restated on the host, the shapes
that reach each of its compiled tile forms, and the cases the device test runs.  Numpy and integers only.

``plan(cus, K, P)`` restates launch_plan, launch_balanced, launch_window and launch_short of the default build (no
FA_TUNING: no LOOP kernels, no level cascade): one dict per kernel launch.  ``model_reduce`` follows reduce_tile over
that plan: for every float4 column it knows the launch, tile, wave, strip j and lane that own it (``owners``), and
gives the column's result: row 0 taken as it is (times a[0] when weighted) or acc_in when accumulating, the other
rows added in arrival order, each add one rounded fp32 operation, the weighted form a rounded multiply and then a
rounded add (``#pragma clang fp contract(off)``, fedagg.hip:14), then the epilogue: nothing (EPI_CHAIN), an IEEE divide
(EPI_MEAN), or the divide and tests/side_kernel_models.model_yogi_step on the mean (EPI_YOGI).  Without a mistake
every column is owned once and its result does not depend on the owner, so ``model_reduce(None, ...)`` is the plain
column-wise chain; with one of ``MISTAKES`` planted the result differs on the inputs of a case the device test runs
(``SEEN_BY``; tests/test_reduce_plan.py holds the model to that).

What restating the plan shows (tests/test_reduce_plan.py asserts each):

* launch_window's ``sw < 16`` branch.  With R = 2 windows the first holds ceil(S / 2) and the last floor(S / 2) >=
  4 * 16 * cap strips (S > 4 * 32 * cap), so sw >= 16: the branch is not reached.  In general the last window holds
  S - (R - 1) * ceil(S / R) >= (S - (R - 1)^2) / R strips, which falls below 4 * 15 * cap only when R is of the order
  of 4 * 32 * cap itself.  At 2 CUs (cap = 1) S = 8,764 strips (P = 2.2 M, R = 69) already has a last window of 60
  strips, sw = 15; at 256 CUs no R below 13,057 can (S > 3.2 * 10^8 strips: rows of more than 300 GB).  So:
  unreachable on an MI355X at any row that fits its memory, reachable in principle and on small devices.
* the ``sw == 16`` window branch is reached, with two windows, only by a last window of exactly 4 * 16 * cap strips:
  S = 4 * 32 * cap + 1 (24,577 at 256 CUs) and K >= FA_BAL_SHORT_K (with fewer clients sw1 divides by the CU count
  and two windows start at S > 4 * 32 * cus).
* a FULL instantiation launched with sw < V changes no bit: the FULL kernel strides its tiles by V whatever r.sw
  says, the launch then holds more tiles than columns, and the surplus is masked by the window end (``HARMLESS``).
  The planted form is the other direction, a FULL launch given the FULL kernel of half its width.
* at 1 CU the plan divides by zero (cap = 1 * 75 / 100 = 0, and FA_BAL_GRID's grid 1 * 224 / 256 = 0) for every K and
  P except K < FA_BAL_SHORT_K with 29..128 strips.  No device has one CU; ``plan`` raises ``NoPlan`` there."""
from functools import lru_cache

import numpy as np

from tests.side_kernel_models import F32, model_yogi_step

FA_RED_WAVES = 4  # fedagg.hip:199
FA_GRID_CAP_PCT = 75  # fedagg.hip:381
FA_BAL_GRID = 224  # fedagg.hip:458
FA_BAL_MIN_SW = 5  # fedagg.hip:461
FA_BAL_MIN_WORK = 1000  # fedagg.hip:464
FA_BAL_SHORT_K = 200  # fedagg.hip:467
FA_CAP_SW_MAX = 32  # fedagg.hip:470
LANES = 64  # float4 columns of one strip (one per lane)

SENT = F32(-7.0e33)  # prefill of every output
HP = {k: float(F32(v)) for k, v in dict(eta=3e-3, tau=1e-8, beta=0.9, omb=1.0 - 0.9, omb2=1.0 - 0.99).items()}
PERIOD = 65_537  # columns of the host block the large shapes tile along each row (prime)
TILED_BYTES = 256 << 20  # rows larger than this are tiled on the device from a [K, PERIOD] block


class NoPlan(ValueError):
    """launch_plan would divide by zero here (a CU count whose capped grid is empty)."""


def cols(P):
    return (P + 3) // 4 * 4


def _cdiv(a, b):
    if b <= 0:
        raise NoPlan(f"ceil({a} / {b})")
    return -(-a // b)


# ----------------------------------------------------------------------------------------------------------------------
# the plan
# ----------------------------------------------------------------------------------------------------------------------
def _route(cus, K, S):
    """The launches of launch_plan over S strips as (V, U, pipe, sw, s0, ns) with ns strips from strip s0; ``ns``
    None: the launch is not a column window (it ends at P4)."""
    W = FA_RED_WAVES
    cap = cus * FA_GRID_CAP_PCT // 100
    g1 = cus if K < FA_BAL_SHORT_K else cap
    sw1 = _cdiv(S, W * g1)
    if sw1 > 32:
        R = _cdiv(S, W * FA_CAP_SW_MAX * cap)
        Sw = _cdiv(S, R)
        out = []
        for s0 in range(0, S, Sw):  # launch_window
            ns = min(S - s0, Sw)
            sw = _cdiv(ns, W * cap)
            out.append((32, 1, False, sw, s0, ns) if sw > 16 else (16, 2, False, sw, s0, ns))
        return out
    if sw1 >= 8:
        return [(32, 1, False, sw1, 0, None) if sw1 > 16 else (16, 2, False, sw1, 0, None)]
    gb = cus * FA_BAL_GRID // 256
    swb = _cdiv(S, W * gb)
    if swb >= FA_BAL_MIN_SW and K * swb >= FA_BAL_MIN_WORK:
        return [(16, 2, False, swb, 0, None) if swb > 8 else (8, 4, False, swb, 0, None)]
    return [(4, 4, True, 4, 0, None)]  # launch_short


def plan(cus, K, P, weighted=False):
    """The k_reduce launches of one fa_reduce / fa_reduce_mirror / fa_reduce_yogi call at (K, P) on a device of
    ``cus`` compute units, in launch order.  ``weighted`` picks the W instantiation and nothing else.  K = 0 (a
    finalize of acc_in alone) is planned like any K below FA_BAL_SHORT_K; fa_reduce_launches answers 0 for it."""
    if P <= 0 or K < 0:
        return []
    P4 = (P + 3) // 4
    S = (P4 + LANES - 1) // LANES
    out = []
    for V, U, pipe, sw, s0, ns in _route(cus, K, S):
        if pipe:  # launch_short: tiles counted in float4 columns
            tiles = _cdiv(P4, LANES * FA_RED_WAVES * 4)
        else:
            tiles = _cdiv(S if ns is None else ns, FA_RED_WAVES * sw)
        end4 = P4 if ns is None else min((s0 + ns) * LANES, P4)
        out.append(dict(V=V, U=U, full=(sw == V), pipe=pipe, sw=sw, col0=s0 * LANES, end4=end4, tiles=tiles,
                        grid=tiles, window=ns is not None))
    return out


def form_of(launch):
    return (launch["V"], launch["U"], launch["full"])


def check_cover(launches, P):
    """Every float4 column of [0, ceil(P/4)) lies in exactly one launch and, there, in exactly one tile; only the last
    tile of a launch is ragged; windows abut at whole strips; sw <= V and full == (sw == V).  By intervals."""
    P4 = (P + 3) // 4
    at = 0
    for i, L in enumerate(launches):
        assert 1 <= L["sw"] <= L["V"] and L["full"] == (L["sw"] == L["V"]), L
        assert L["V"] * L["U"] in (32, 16) and L["grid"] == L["tiles"] >= 1, L
        assert L["col0"] == at and L["col0"] % LANES == 0, (i, L, at)
        span = LANES * FA_RED_WAVES * L["sw"]
        width = L["end4"] - L["col0"]
        assert width > 0 and (L["tiles"] - 1) * span < width <= L["tiles"] * span, (i, L)
        assert L["end4"] % LANES == 0 or L["end4"] == P4, L
        at = L["end4"]
    assert at == P4, (at, P4)


def owners(launches, P4, mistake=None):
    """Per launch, the float4 columns its threads touch, in (tile, wave, j, lane) order, as a dict of equally long
    arrays c, tile, wave, j, lane.  Without a mistake the c of all launches partition [0, P4)."""
    out = []
    for L in launches:
        V, sw = L["V"], L["sw"]
        full = L["full"]
        if mistake == "full_sw_wide" and full and V > 4:
            V = V // 2  # the FULL kernel of the next narrower variant: strides and covers V / 2 strips
        if mistake == "full_sw_narrow":
            full = True  # the FULL kernel of the launch's own V, whatever sw is
        stride = V if full else sw
        cover = V if (full or mistake == "mask_missing") else sw
        bound = P4 if mistake == "window_end_unclipped" else L["end4"]
        t, w, j, lane = np.meshgrid(np.arange(L["tiles"], dtype=np.int64), np.arange(FA_RED_WAVES), np.arange(cover),
                                    np.arange(LANES), indexing="ij")
        c = L["col0"] + (t * FA_RED_WAVES + w) * (LANES * stride) + lane + LANES * j
        keep = c < bound
        out.append({k: a[keep] for k, a in dict(c=c, tile=t, wave=w, j=j, lane=lane).items()})
    return out


# ----------------------------------------------------------------------------------------------------------------------
# reduce_tile
# ----------------------------------------------------------------------------------------------------------------------
MISTAKES = ("tail_dropped", "group_weight_k0", "pipe_buffers_swapped", "mask_missing", "window_end_unclipped",
            "col0_dropped", "accumulate_ignored", "full_sw_wide", "mean_out_chain", "yogi_init_ignored")
HARMLESS = ("full_sw_narrow",)  # changes no bit of any case (module docstring)
IN_PLACE_ONLY = ("mask_missing", "window_end_unclipped")  # a column written twice: the same value, unless acc_in is out


def _schedule(K, U, pipe, start, mistake):
    """(row, index of its weight) in the order reduce_tile adds rows start..K-1: whole groups of U (pairs of them
    through the two pipeline buffers when ``pipe``), then the K % U tail one row at a time."""
    n = (K - start) // U
    groups = [list(range(start + g * U, start + (g + 1) * U)) for g in range(n)]
    if pipe and mistake == "pipe_buffers_swapped":
        for g in range(0, n - 1, 2):  # both buffers loaded: tb's group added before ta's
            groups[g], groups[g + 1] = groups[g + 1], groups[g]
    order = [(k, g[0] if mistake == "group_weight_k0" else k) for g in groups for k in g]
    if mistake != "tail_dropped":
        order += [(k, k) for k in range(start + n * U, K)]
    return order


def _chain(x, sel, K, a, acc, U, pipe, mistake):
    """The fp32 chain of float columns ``sel`` (a slice or an index array)."""
    with np.errstate(all="ignore"):
        if acc is not None:
            s, start = np.array(acc, dtype=F32, copy=True), 0
        else:
            s, start = (x[0][sel] * a[0] if a is not None else x[0][sel].copy()), 1
        for k, wk in _schedule(K, U, pipe, start, mistake):
            s = s + a[wk] * x[k][sel] if a is not None else s + x[k][sel]
    return s


def model_reduce(launches, x, K, P, *, epi, out, a=None, acc_in=None, in_place=False, denom=1.0, mean_out=None,
                 last=None, m=None, v=None, init=False, mistake=None):
    """fa_reduce (epi 'chain' / 'mean', ``mean_out`` the mirror) or fa_reduce_yogi (epi 'yogi') of rows x[0:K] over
    ``launches``.  The per-column arrays come as the device test allocates them (cols(P) + 4 floats, prefilled) and
    are returned as new arrays in a dict out, mean_out, m, v.  ``in_place``: acc_in is out.  ``launches`` None: the
    column-wise chain on every element of the arrays, no tiles (P is ignored; any array length)."""
    res = dict(out=np.array(out, dtype=F32, copy=True))
    for name, arr in (("mean_out", mean_out), ("m", m), ("v", v)):
        res[name] = None if arr is None else np.array(arr, dtype=F32, copy=True)
    if in_place:
        acc_in = res["out"]  # live: a column written earlier in the call is read back as written
    accumulate = acc_in is not None and not (mistake == "accumulate_ignored" and K > 0)
    a = None if a is None else np.asarray(a, F32)
    denom = F32(denom)

    def columns(sel, osel, U, pipe):
        s = _chain(x, sel, K, a, acc_in[sel] if accumulate else None, U, pipe, mistake)
        with np.errstate(all="ignore"):
            if epi == "chain":
                res["out"][osel] = s
                return
            mean = s / denom
            if res["mean_out"] is not None:
                res["mean_out"][osel] = s if mistake == "mean_out_chain" else mean
            if epi == "mean":
                res["out"][osel] = mean
                return
            n = len(mean)
            first = init and mistake != "yogi_init_ignored"
            res["m"][osel], res["v"][osel], res["out"][osel] = model_yogi_step(
                mean, last[sel], res["m"][sel], res["v"][sel], res["out"][sel], n, HP, first)

    if launches is None:
        columns(slice(None), slice(None), 1, False)
        return res
    P4 = (P + 3) // 4
    lane4 = np.arange(4)
    for L, own in zip(launches, owners(launches, P4, mistake)):
        rest = own["c"]
        shift = L["col0"] if mistake == "col0_dropped" else 0
        while rest.size:  # one pass per time a column is touched (once, without a mistake)
            u, first = np.unique(rest, return_index=True)
            if u[-1] - u[0] + 1 == u.size:
                sel = slice(4 * u[0], 4 * u[-1] + 4)
                osel = slice(sel.start - 4 * shift, sel.stop - 4 * shift)
            else:
                sel = (4 * u[:, None] + lane4).ravel()
                osel = sel - 4 * shift
            columns(sel, osel, L["U"], L["pipe"])
            rest = np.delete(rest, first)
    return res


# ----------------------------------------------------------------------------------------------------------------------
# shapes
# ----------------------------------------------------------------------------------------------------------------------
K_SMALL = 3  # rows of the shapes any K reaches
# name -> what identifies the plan: (launches, index of the launch of the form, (V, U, full))
FORMS = {
    "short": (1, 0, (4, 4, True)),
    "v16_sw": (1, 0, (16, 2, False)),
    "v16_full": (1, 0, (16, 2, True)),
    "v32_sw": (1, 0, (32, 1, False)),
    "v32_full": (1, 0, (32, 1, True)),
    "win_v32_sw": (2, 0, (32, 1, False)),
    "win_v32_full": (2, 0, (32, 1, True)),
    "v8_sw": (1, 0, (8, 4, False)),
    "v8_full": (1, 0, (8, 4, True)),
    "win_v16_full": (2, 1, (16, 2, True)),
}


def _name_of(route):
    """The FORMS names a route answers to."""
    names = []
    for name, (n, i, (V, U, full)) in FORMS.items():
        if len(route) != n:
            continue
        rV, rU, _, sw, _, ns = route[i]
        if (rV, rU, sw == rV) != (V, U, full) or (ns is not None) != (n > 1):
            continue
        if name == "win_v32_sw" and any(r[3] == r[0] for r in route):
            continue  # both windows of run-time width
        names.append(name)
    return names


@lru_cache(maxsize=None)
def shapes(cus):
    """For every reachable tile form, as a single launch or as a column window, the smallest (K, P) the plan routes
    there: K the fewest rows the form admits (K_SMALL where any K does; FA_BAL_MIN_WORK / sw rounded up for the (8,4)
    forms; FA_BAL_SHORT_K for the (16,2) FULL window) and the first P of the lowest strip count S that selects it, P =
    (S - 1) * 256 + 1: the last strip one float4, the last float4 one float, the last tile ragged.  For a FULL form
    also (``fill``) the first P at or above it that fills the form's last tile exactly.  A list of dicts name, K, P,
    S, fill, sw (of the launch of the form)."""
    k_of = {name: K_SMALL for name in FORMS}
    k_of["v8_sw"] = -(-FA_BAL_MIN_WORK // FA_BAL_MIN_SW)  # the narrowest (8,4) tile: K x 5 >= FA_BAL_MIN_WORK
    k_of["v8_full"] = -(-FA_BAL_MIN_WORK // 8)
    k_of["win_v16_full"] = FA_BAL_SHORT_K
    found = {}
    for K in sorted(set(k_of.values())):
        seen = None
        for S in range(1, 2 * FA_RED_WAVES * FA_CAP_SW_MAX * cus + 1):  # past two windows of full tiles
            try:
                route = _route(cus, K, S)
            except NoPlan:
                continue
            key = tuple((r[0], r[3], r[5] is None) for r in route)
            if key == seen:
                continue
            seen = key
            for name in _name_of(route):
                if k_of[name] == K and name not in found:
                    found[name] = (K, S)
    out = []
    for name, (n, i, (V, U, full)) in FORMS.items():
        if name not in found:
            continue
        K, S = found[name]
        sw = _route(cus, K, S)[i][3]
        out.append(dict(name=name, K=K, P=(S - 1) * 4 * LANES + 1, S=S, fill=False, sw=sw))
        if full and name != "short":
            S2 = S
            while True:
                route = _route(cus, K, S2)
                assert name in _name_of(route), (name, S2)
                ns = S2 if route[i][5] is None else route[i][5]
                if ns % (FA_RED_WAVES * V) == 0:
                    break
                S2 += 1
            out.append(dict(name=name + "_fill", K=K, P=S2 * 4 * LANES, S=S2, fill=True, sw=sw))
    return out


def shape(cus, name):
    return next(s for s in shapes(cus) if s["name"] == name)


def plan_is(cus, K, P, name):
    """Does the plan at (K, P) have the form ``name`` (of FORMS, '_fill' ignored) stands for?"""
    S = ((P + 3) // 4 + LANES - 1) // LANES
    return name.replace("_fill", "") in _name_of(_route(cus, K, S))


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
BAND, NSPECIAL = 1021, 6  # the specials recur every BAND columns, the first band at columns BAND - 7 ..


def block_width(K, P):
    """Columns of the host block of a shape's rows: all P, or PERIOD when the rows are tiled from it."""
    return PERIOD if 4 * K * P > TILED_BYTES else P


def block_rows(K, B, seed):
    """[K, B] standard normals with a band of special columns: +inf in row 0; a NaN in row 1 (row 0 when K = 1);
    3e38, 3e38, -3e38 down the rows (overflows, and stays there); denormals; all -0.0; -0.0 in row 0 and +0.0 below."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((K, B), dtype=F32)
    i = np.arange(B)
    which = (i + 7) % BAND
    k = np.arange(K)
    fills = [None, None, np.array([3e38, 3e38, -3e38], F32)[k % 3],
             (np.array([1, -2, 3, 5, -7], F32) * F32(1e-42))[k % 5], np.full(K, -0.0, F32),
             np.where(k == 0, F32(-0.0), F32(0.0)).astype(F32)]
    for c, fill in enumerate(fills):
        at = i[which == c]
        if c == 0:
            x[0, at] = np.inf
        elif c == 1:
            x[min(1, K - 1), at] = np.nan
        else:
            x[:, at] = fill[:, None]
    return x


def block_vec(B, seed, scale=1.0):
    """A per-column input (acc_in, last) of B columns; the specials band holds +inf, NaN, 3e38, a denormal, -0.0, +0.0."""
    v = np.random.default_rng(seed).standard_normal(B, dtype=F32) * F32(scale)
    which = (np.arange(B) + 7) % BAND
    for c, val in enumerate((np.inf, np.nan, 3e38, 3e-42, -0.0, 0.0)):
        v[which == c] = val
    return v


def expand_rows(block, P):
    """[K, ld] rows of P columns tiled from the block along each row, ld = cols(P) + 8, NaN in [P, ld)."""
    K, B = block.shape
    x = np.full((K, cols(P) + 8), np.nan, F32)
    x[:, :P] = block if B == P else block[:, np.arange(P) % B]
    return x


def expand_vec(blk, P, pad):
    """cols(P) + 4 floats: the block tiled over [0, P), ``pad`` in [P, cols(P)), SENT in the last four."""
    v = np.full(cols(P) + 4, SENT, F32)
    v[:P] = blk if len(blk) == P else blk[np.arange(P) % len(blk)]
    v[P:cols(P)] = pad
    return v


def weights(K, seed):
    return np.random.default_rng(9000 + seed).uniform(0.2, 1.0, size=K).astype(F32)


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
def _call(k0, k1, epi, src=None, dst="out", mean=False, init=False):
    """One library call: rows [k0, k1), continuing buffer ``src`` (None: starting from row k0) into buffer ``dst``."""
    return dict(k0=k0, k1=k1, epi=epi, src=src, dst=dst, mean=mean, init=init)


def _one(epi, K):
    return [_call(0, K, epi, mean=(epi != "chain"), init=True)]


def _fold(epi, K, h, in_place):
    dst = "acc" if in_place else "out"
    return [_call(0, h, "chain", dst="acc"), _call(h, K, epi, src="acc", dst=dst, mean=(epi == "yogi"), init=True)]


def cases(cus):
    """Every case of tests/test_gpu_reduce_kernels.py at ``cus`` compute units: dicts id, rows (the key of the rows it
    reads: cases of one key share them), form (the FORMS name the plan of its widest call must have, '_fill'
    included), Krows, P, weighted, calls, in_place."""
    out = []

    def add(cid, rows, form, Krows, P, weighted, calls):
        # in place: acc_in is out, or a continuing FedYoGi round (m and v are read and written where they lie)
        in_place = any((c["src"] is not None and c["src"] == c["dst"]) or (c["epi"] == "yogi" and not c["init"])
                       for c in calls)
        out.append(dict(id=cid, rows=rows, form=form, Krows=Krows, P=P, weighted=weighted, calls=calls,
                        in_place=in_place))

    sh = {s["name"]: s for s in shapes(cus)}
    extra = {"v8_sw": 3, "v8_full": 3}  # rows for the four smallest K of the (8,4) forms
    krows = {n: s["K"] + extra.get(n, 0) for n, s in sh.items()}
    # every instantiation: each tile form x epilogue x weighted or not (the 5 GB window shape once per epilogue)
    for name, s in sh.items():
        if name == "short":
            continue  # the short form has its own rows below
        K, P = s["K"], s["P"]
        if s["fill"]:
            add(f"{name}-mean", name, name, krows[name], P, False, _one("mean", K))
            continue
        for epi in ("chain", "mean", "yogi"):
            for weighted in (False, True):
                if name == "win_v16_full" and weighted != (epi == "mean"):
                    continue
                add(f"{name}-{epi}-{'w' if weighted else 'u'}", name, name, krows[name], P, weighted, _one(epi, K))
    # K residues, U = 1 and 2: K = 1, 2, 3 from row 0 and continuing an accumulator
    for name in ("v32_sw", "v16_sw"):
        P = sh[name]["P"]
        for K in (1, 2, 3):
            add(f"{name}-K{K}", name, name, krows[name], P, K == 2, _one("mean", K))
            add(f"{name}-K{K}-acc", name, name, krows[name], P, K != 2, [_call(0, K, "chain", src="acc")])
    # ... U = 4: the four smallest K of each (8,4) form
    for name in ("v8_sw", "v8_full"):
        P, K0 = sh[name]["P"], sh[name]["K"]
        for K in range(K0 + 1, K0 + 4):
            add(f"{name}-K{K}", name, name, krows[name], P, K % 2 == 0, _one("mean", K))
        for K in range(K0, K0 + 4):
            add(f"{name}-K{K}-acc", name, name, krows[name], P, K % 2 == 1, [_call(0, K, "mean", src="acc")])
    # the short form: every exit of the two-buffer pipeline, every instantiation, the small widths
    for K in tuple(range(1, 15)) + (17,):
        add(f"short-K{K}", "short_P8195", "short", 17, 8195, K % 2 == 0, _one("mean", K))
        add(f"short-K{K}-acc", "short_P8195", "short", 17, 8195, K % 2 == 1, [_call(0, K, "chain", src="acc")])
    for epi in ("chain", "mean", "yogi"):
        for weighted in (False, True):
            add(f"short-{epi}-{'w' if weighted else 'u'}", "short_P8195", "short", 17, 8195, weighted, _one(epi, 17))
    for P in (1, 3, 4, 5, 4095, 4096, 4097):
        add(f"short-P{P}", f"short_P{P}", "short", 17, P, P % 2 == 0, _one("mean", 17))
    # chunk folding as DeviceRound does it: [0, h) into acc, then [h, K) continuing acc, in place and out of place
    for name in ("v16_sw", "v16_full", "win_v32_sw", "win_v32_full"):
        K, P = sh[name]["K"], sh[name]["P"]
        for epi in ("mean", "yogi"):
            for in_place in (True, False):
                add(f"{name}-fold-{epi}-{'inplace' if in_place else 'outofplace'}", name, name, krows[name], P,
                    epi == "yogi", _fold(epi, K, 1, in_place))
    for name in ("v16_sw", "win_v32_sw"):  # finalize only: K = 0, x = None
        add(f"{name}-finalize-only", name, name, krows[name], sh[name]["P"], False, [_call(0, 0, "mean", src="acc")])
    # FedYoGi over two rounds: init (m and v prefilled NaN), then the continuing state; with and without mean_out
    for name, K, P, rows in (("v32_sw", sh["v32_sw"]["K"], sh["v32_sw"]["P"], "v32_sw"), ("short", 17, 8195, "short_P8195")):
        for mean in (True, False):
            calls = [_call(0, K, "yogi", mean=mean, init=True), _call(0, K, "yogi", mean=mean, init=False)]
            add(f"{name}-yogi-rounds-{'mean' if mean else 'nomean'}", rows, name, K, P, False, calls)
    return out


def case_inputs(case):
    """The host blocks of a case: rows [Krows, B], weights, and the per-column inputs acc and last (B columns)."""
    B = block_width(case["Krows"], case["P"])
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(case["rows"])) % 100_000
    return dict(B=B, rows=block_rows(case["Krows"], B, seed), a=weights(case["Krows"], seed),
                acc=block_vec(B, seed + 1), last=block_vec(B, seed + 2, 0.05))


PAD = dict(acc=np.nan, last=np.nan, m=np.nan, v=np.nan, out=SENT, mean=SENT)  # columns [P, cols(P)) of each buffer


def block_buffers(inp):
    """The per-column buffers of a case before its first call, B columns each: acc and last as drawn, out and the mean
    (or mirror) the sentinel, m and v NaN (an init round must not read them)."""
    B = inp["B"]
    return dict(acc=inp["acc"], last=inp["last"], out=np.full(B, SENT, F32), mean=np.full(B, SENT, F32),
                m=np.full(B, np.nan, F32), v=np.full(B, np.nan, F32))


def expand_buffers(bufs, P):
    return {k: expand_vec(v, P, PAD[k]) for k, v in bufs.items()}


def case_denom(case, inp):
    K = max(c["k1"] for c in case["calls"])
    if K == 0:
        return F32(3)  # a finalize of acc_in alone
    return F32(np.sum(inp["a"][:K].astype(np.float64))) if case["weighted"] else F32(K)


def run_model(case, x, bufs, a, denom, launches_of, mistake=None):
    """The case's calls on the model.  ``bufs``: dict acc, out, mean, m, v, last of per-column arrays; ``launches_of(K)``
    gives the plan of a call over K rows (None: column-wise, no tiles).  Returns the buffers after the last call."""
    b = {k: np.array(v, dtype=F32, copy=True) for k, v in bufs.items()}
    for c in case["calls"]:
        K = c["k1"] - c["k0"]
        src, dst = c["src"], c["dst"]
        r = model_reduce(launches_of(K), x[c["k0"]:c["k1"]] if K else None, K, case["P"], epi=c["epi"], out=b[dst],
                         a=a[c["k0"]:c["k1"]] if case["weighted"] else None,
                         acc_in=None if src is None else b[src], in_place=(src is not None and src == dst),
                         denom=denom, mean_out=b["mean"] if c["mean"] else None, last=b["last"], m=b["m"], v=b["v"],
                         init=c["init"], mistake=mistake)
        b[dst] = r["out"]
        if c["mean"]:
            b["mean"] = r["mean_out"]
        if c["epi"] == "yogi":
            b["m"], b["v"] = r["m"], r["v"]
    return b


def plain_reference(case, xb, inp, denom):
    """The case's final ``out`` (or ``acc``) by the plainest statement of the operation: one loop over the rows of the
    whole case, whatever its calls and tiles (a fold equals one call).  Only for cases of mean / chain epilogues."""
    calls = case["calls"]
    K = max(c["k1"] for c in calls)
    a = inp["a"] if case["weighted"] else None
    with np.errstate(all="ignore"):
        if calls[0]["src"] is not None:
            s = np.array(inp["acc"], copy=True)
        else:
            s = None
        for k in range(K):
            t = a[k] * xb[k] if a is not None else xb[k]
            s = np.array(t, copy=True) if s is None else s + t
        return s / denom if calls[-1]["epi"] == "mean" else s


# mistake -> what it is, and the case of cases() that sees it (the ids do not depend on the CU count)
SEEN_BY = {
    # the K % U rows after the last whole group of U are never added.  Seen by v16_sw-K2: U = 2, row 1 is the tail.
    "tail_dropped": "v16_sw-K2",
    # a group's U rows all take the group's first weight, a[k0].  Seen by v8_sw-K202: weighted, groups of 4.
    "group_weight_k0": "v8_sw-K202",
    # the pipeline adds buffer tb's group before ta's.  Seen by short-K9: rows 1-4 and 5-8 are the two buffers.
    "pipe_buffers_swapped": "short-K9",
    # a run-time-width tile without `j < sw`: a wave runs on into the strips of the next wave, which are reduced
    # twice.  Seen by v16_sw-fold-mean-inplace (sw 8 of 16): the second time starts from the first's result.
    "mask_missing": "v16_sw-fold-mean-inplace",
    # a window launch bounded by P4, not by its window: its ragged last tile runs on into the next window.  Seen by
    # win_v32_sw-fold-mean-inplace: the next launch continues from what that tile wrote.
    "window_end_unclipped": "win_v32_sw-fold-mean-inplace",
    # outputs indexed from the launch's first column.  Seen by win_v32_sw-mean-u: the second window lands on the first.
    "col0_dropped": "win_v32_sw-mean-u",
    # FA_ACCUMULATE ignored: the chain starts from row 0.  Seen by v32_sw-K1-acc.
    "accumulate_ignored": "v32_sw-K1-acc",
    # a FULL launch given the FULL kernel of half its width (tiles counted for sw = V, strided by V / 2): the far
    # half of the launch is never written.  Seen by v32_full-chain-u.
    "full_sw_wide": "v32_full-chain-u",
    # mean_out (the mirror) given the chain, not the mean.  Seen by v16_full-mean-u.
    "mean_out_chain": "v16_full-mean-u",
    # FA_YOGI_INIT ignored: m and v are read (NaN before an init round).  Seen by v8_full-yogi-u.
    "yogi_init_ignored": "v8_full-yogi-u",
}
