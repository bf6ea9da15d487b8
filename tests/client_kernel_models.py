"""Inputs, expected results and host restatements for the exact tests of the client kernels
(fedscale_amd/csrc/client_update.hip).  Numpy only: tests/test_client_oracle.py runs all of it without a GPU, and
tests/test_gpu_client_exact.py runs the device on the same inputs and compares with the same expected results.

Three kinds of thing live here.

* Cases: tensor lists as views into a few flat fp32 arrays (``Table``), so that the device test can rebuild the same
  views, with the same offsets from a 16-byte boundary, on device memory, and can compare whole allocations, gaps
  between the views included.
* Expected results, built on oracle/cpu_reference.py (``sgd_prox_step_ref``; the tests add ``dp_clip_exact`` and
  ``dp_normals_ref``).
* ``model_*``: restatements of what the library's host code and kernels do with a list: the cut into launch groups,
  the tables of a launch, the workspace indices, the strided loops, the choice of the float4 path.  Each takes a
  ``mistake`` that plants one indexing error.  Without a mistake a model must equal the expected result; with one
  it must not, on the very inputs the device test uses: that is how tests/test_client_oracle.py shows that each
  device test can see the mistake it is there for.

A misaligned float4 access has no defined result.  The models give it the one a strict-alignment memory path
gives: the low address bits are dropped, so the access lands on the 16-byte granule below.  Hardware that serves
unaligned vector accesses would hide a wrong ``vec`` bit from any test of results."""
import numpy as np

from oracle.cpu_reference import dp_noise_hashes, sgd_prox_step_ref

F32, F64 = np.float32, np.float64
MT_MAX, MT_CHUNK, SGD_MAX = 64, 4096, 48  # constants of client_update.hip
NESTEROV, FIRST = 1, 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == F32 else np.uint64)


def same_bits(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Table:
    """Tensor lists as views into flat arrays.  ``base[name]`` is a flat array; tensor t of list ``name`` is
    ``base[name][off[name][t] : off[name][t] + n[t]]``, or None where ``off[name][t]`` is None.  Slots start on
    a multiple of 4 elements (16 bytes once the base is 16-byte aligned), so ``off % 4`` is the view's distance
    from the 16-byte grid in elements."""

    def __init__(self, n):
        self.n = [int(x) for x in n]
        self.T = len(self.n)
        self.base, self.off = {}, {}

    def add(self, name, base, off):
        self.base[name], self.off[name] = base, list(off)

    def view(self, name, t, base=None, n=None, off=None):
        o = self.off[name][t] if off is None else off
        if o is None:
            return None
        b = self.base[name] if base is None else base
        return b[o:o + (self.n[t] if n is None else n)]

    def views(self, name, base=None):
        return [self.view(name, t, base) for t in range(self.T)]

    def copy(self):
        c = Table(self.n)
        c.__dict__.update(self.__dict__)
        c.base = {k: v.copy() for k, v in self.base.items()}
        return c

    def device_views(self, name, dev_base):
        return [None if o is None else dev_base[o:o + n] for o, n in zip(self.off[name], self.n)]


def _slots(n):
    """Slot starts (multiples of 4) with room for the largest shift, and the total length."""
    starts, o = [], 4  # a guard granule in front of the first slot
    for x in n:
        starts.append(o)
        o += (x + 3 + 3) // 4 * 4 + 4
    return starts, o


# ------------------------------------------------------------------------------------------------------------------
# noise stream
# ------------------------------------------------------------------------------------------------------------------
NOISE_N = 4099
NOISE_SEEDS = [0, 77, 77 + 2 ** 32, 2 ** 63 + 5, 2 ** 64 - 1]
NOISE_OFFSETS = [0, 1, 4095, 2 ** 33 - 3, 2 ** 40 + 1]
# |z - z_ref| <= NOISE_BOUND * |z_ref|: see tests/test_gpu_client_exact.py::test_noise_stream_matches_the_twin
NOISE_BOUND = 4.5 * 2.0 ** -23
# counters at seed 77 whose pair has h1 >> 8 == 0 (u1 = 2^-24, the largest radius) and h1 >> 8 == 0xFFFFFF (u1 = 1,
# radius 0); found by scan_edge_draws() over the first 2^28 counters
EDGE_SEED = 77
EDGE_U1_MIN = [111583388, 176293646]
EDGE_U1_ONE = [38276152, 44598952]


def scan_edge_draws(seed=EDGE_SEED, n=1 << 28, block=1 << 24):
    """The even counters below n whose pair has h1 >> 8 == 0, and those with h1 >> 8 == 0xFFFFFF."""
    lo, hi = [], []
    for s in range(0, n, block):
        e = np.arange(s, s + block, 2, dtype=np.uint64)
        k = dp_noise_hashes(seed, e)[0] >> np.uint32(8)
        lo += e[k == 0].tolist()
        hi += e[k == 0xFFFFFF].tolist()
    return lo, hi


def model_normals(seed, off, n, mistake=None):
    """``k_dp_normals`` / ``noise_at`` restated (float64 transcendentals, as the twin has them), element i of a
    read of n at offset ``off``.  Mistakes: 'seed_hi' (high word of the seed dropped), 'j_hi' (high word of the
    pair counter dropped), 'parity_i' (parity from the index in the read, not from off + i), 'u1_plus1' (u1
    without the + 1)."""
    M = np.uint64(0xFFFFFFFF)

    def mix(x):
        x = ((x ^ (x >> np.uint64(16))) * np.uint64(0x7FEB352D)) & M
        x = ((x ^ (x >> np.uint64(15))) * np.uint64(0x846CA68B)) & M
        return x ^ (x >> np.uint64(16))

    seed = int(seed) & (2 ** 64 - 1)
    i = np.arange(n, dtype=np.uint64)
    e = np.uint64(off) + i
    j = e >> np.uint64(1)
    s_hi = np.array([0 if mistake == "seed_hi" else seed >> 32], dtype=np.uint64)
    s = mix(np.array([seed & 0xFFFFFFFF], dtype=np.uint64) ^ mix((s_hi + np.uint64(0x9E3779B9)) & M))
    j_hi = np.zeros_like(j) if mistake == "j_hi" else j >> np.uint64(32)
    h1 = mix(s ^ mix((j & M) ^ mix((j_hi + np.uint64(0x85EBCA6B)) & M)))
    h2 = mix((h1 + np.uint64(0x27D4EB2F)) & M)
    k1 = (h1 >> np.uint64(8)).astype(F32)
    u1 = (k1 if mistake == "u1_plus1" else k1 + F32(1)) * F32(2.0 ** -24)
    u2 = (h2 >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)
    ang = (F32(6.283185307179586) * u2).astype(F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(-2.0 * np.log(u1.astype(F64)))
        odd = ((i if mistake == "parity_i" else e) & np.uint64(1)).astype(bool)
        return np.where(odd, r * np.sin(ang), r * np.cos(ang))


def within_noise_bound(z, z_ref) -> np.ndarray:
    z, z_ref = np.asarray(z, F64), np.asarray(z_ref, F64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (np.abs(z - z_ref) <= NOISE_BOUND * np.abs(z_ref))


# ------------------------------------------------------------------------------------------------------------------
# DP list: T = 130 (+ 3 for fa_dp_apply)
# ------------------------------------------------------------------------------------------------------------------
DP_SIZES = [0, 1, 3, 4, 5, 4095, 4096, 4097]
DP_LONG = {70: 64 * MT_CHUNK + 1, 129: 128 * MT_CHUNK + 5}  # 262145 (65 workgroups), 524293 (129)
DP_DATA_SEED = 20
_P_SHIFT, _L_SHIFT, _U_SHIFT = [0, 1, 0, 3, 0], [0, 1, 0, 0, 2], [0, 0, 2, 0, 0]  # by t % 5, in elements


def dp_case(extra: bool = False, empties: bool = True) -> Table:
    """130 tensors: sizes from DP_SIZES, empties at 0, 63 and 64, 65 workgroups at index 70 (16-byte aligned: the
    float4 path; the second launch group, so its partials do not start at 0), 129 workgroups at index 129 (its
    ``last`` 8 bytes off: the element path); views off the 16-byte grid by t % 5; ``last`` None where t % 7 == 3.
    ``extra``: three more tensors of 4097 elements with exactly one of param / last / upload off the grid.
    ``empties=False``: the same list without its empty tensors (the inf norm has no value for them); with
    ``extra`` that leaves 130 tensors, so still three launch groups."""
    rng = np.random.default_rng(DP_DATA_SEED)
    n = [int(x) for x in rng.choice(DP_SIZES[1:], size=130)]
    n[:8] = DP_SIZES
    n[63] = n[64] = 0
    for t, x in DP_LONG.items():
        n[t] = x
    ps = [_P_SHIFT[t % 5] for t in range(130)]
    ls = [None if (t % 7 == 3 and t not in DP_LONG) else _L_SHIFT[t % 5] for t in range(130)]
    us = [_U_SHIFT[t % 5] for t in range(130)]
    if extra:
        n += [4097] * 3
        ps += [1, 0, 0]
        ls += [0, 1, 0]
        us += [0, 0, 1]
    if not empties:
        keep = [t for t in range(len(n)) if n[t] > 0]
        n, ps, ls, us = ([v[t] for t in keep] for v in (n, ps, ls, us))
    starts, total = _slots(n)
    tab = Table(n)
    p = rng.normal(0, 0.1, size=total).astype(F32)
    tab.add("p", p, [s + k for s, k in zip(starts, ps)])
    tab.add("l", rng.normal(0, 0.1, size=total).astype(F32), [None if k is None else s + k for s, k in zip(starts, ls)])
    tab.add("u", np.full(total, F32(-7.5)), [s + k for s, k in zip(starts, us)])
    return tab


INF_PLANTS = ["last", "long_last", "t64", "t5", "nan"]


def plant_inf(tab: Table, where: str) -> Table:
    """A copy of dp_case(extra=True, empties=False) (130 tensors, three launch groups) with |delta| = 1000 planted:
    'last' in the last element of the last tensor (third group), 'long_last' in the last element of the tensor of
    129 workgroups (the third trip of lane 0 in k_dp_tensor_norm), 't64' in the first element of tensor 64 (the
    first of the second group), 't5' in tensor 5 (the first group); 'nan': a NaN in the third group."""
    tab = tab.copy()
    long_t = max(range(tab.T), key=lambda t: tab.n[t])
    t, i = {"last": (tab.T - 1, -1), "long_last": (long_t, -1), "t64": (64, 0), "t5": (5, 0),
            "nan": (tab.T - 2, 3)}[where]
    assert tab.T > 2 * MT_MAX + 1 and tab.n[t] > 3
    tab.view("p", t)[i] = np.nan if where == "nan" else 1000.0
    if where != "nan" and tab.off["l"][t] is not None:
        tab.view("l", t)[i] = 0.0
    return tab


def dp_noise_offsets(tab: Table):
    """Explicit counter offsets for fa_dp_apply: odd ones, and from tensor 40 on beyond 2^33."""
    offs, o = [], 1
    for t in range(tab.T):
        if t == 40:
            o = 2 ** 33 + 7
        if t == 100:
            o = 2 ** 40 + 2 ** 33 - 1
        offs.append(o)
        o += tab.n[t] + (t % 2)
    return offs


def tiny_dp_case(T: int) -> Table:
    """T tensors of 1..5 elements for the group-count seams (T = 64, 65, 128, 129)."""
    rng = np.random.default_rng(1000 + T)
    n = [1 + t % 5 for t in range(T)]
    starts, total = _slots(n)
    tab = Table(n)
    tab.add("p", rng.normal(0, 1, size=total).astype(F32), [s + t % 3 for t, s in enumerate(starts)])
    tab.add("l", rng.normal(0, 1, size=total).astype(F32), [None if t % 4 == 2 else s for t, s in enumerate(starts)])
    return tab


def dp_precondition(ex: dict) -> bool:
    """The device owes the bits of ``dp_clip_exact``: no fp32 rounding, of a tensor's norm or of the total, moves
    when the sum under the root moves by a relative 2^-46.  (The device adds exact fp64 squares with fewer than 64
    roundings of non-negative partial sums at these sizes, each within 2^-53 of the running sum: its sum is within
    64 * 2^-53 = 2^-47 of S, the root of that within 2^-48 of sqrt(S) plus its own 2^-53.)"""
    import math

    eps = 2.0 ** -46
    for s in list(ex["S"]) + [ex["S_total"]]:
        if not (F32(math.sqrt(s * (1 - eps))) == F32(math.sqrt(s)) == F32(math.sqrt(s * (1 + eps)))):
            return False
    return True


def _chunk_partials(d, inf):
    """Per-workgroup partials of one tensor: k_dp_partial."""
    nb = (len(d) + MT_CHUNK - 1) // MT_CHUNK
    x = np.zeros(nb * MT_CHUNK, F64)
    if inf:
        x[:len(d)] = np.abs(d)
        x = x.reshape(nb, MT_CHUNK)
        return np.where(np.isnan(x).any(axis=1), np.nan, x.max(axis=1, initial=0.0))
    x[:len(d)] = d.astype(F64) ** 2
    return x.reshape(nb, MT_CHUNK).sum(axis=1)


def _nanmax(a, b):
    return b if (b > a or b != b) else a


def model_dp_clip(params, last, max_norm, norm_inf=False, mistake=None):
    """fa_dp_clip_coef restated: launch groups of MT_MAX tensors, partials at part[part0 + block], one wave per
    tensor over its partials with stride 64 into tsum[t0 + t], one wave over the tensors with stride 64.  The
    workspace starts zeroed here (on the device it is uninitialised).  Mistakes: 'part0_write' (k_dp_partial
    ignores part0), 'part0_read' (k_dp_tensor_norm ignores it), 'part0_both' (left at 0 for every group: harmless,
    both kernels of a group agree and run in stream order), 'tsum_t0', 'norm_one_trip', 'coef_one_trip'.
    Returns (total, coef, apply) as fp32, fp32, bool."""
    import math

    T = len(params)
    d = [np.asarray(p, F32) if l is None else np.asarray(p, F32) - np.asarray(l, F32) for p, l in zip(params, last)]
    nb = [(len(x) + MT_CHUNK - 1) // MT_CHUNK for x in d]
    part, tsum = np.zeros(sum(nb) + 1, F64), np.zeros(T + 1, F64)
    t, part0 = 0, 0
    while t < T:
        t0, Tg = t, min(MT_MAX, T - t)
        blk0 = np.concatenate([[0], np.cumsum(nb[t0:t0 + Tg])]).astype(int)
        pw = 0 if mistake in ("part0_write", "part0_both") else part0
        pr = 0 if mistake in ("part0_read", "part0_both") else part0
        for j in range(Tg):
            part[pw + blk0[j]:pw + blk0[j + 1]] = _chunk_partials(d[t0 + j], norm_inf)
        for j in range(Tg):
            lanes = [0.0] * 64
            for lane in range(64):
                b = blk0[j] + lane
                while b < blk0[j + 1]:
                    lanes[lane] = _nanmax(lanes[lane], part[pr + b]) if norm_inf else lanes[lane] + part[pr + b]
                    b += 64
                    if mistake == "norm_one_trip":
                        break
            s = 0.0
            for v in lanes:
                s = _nanmax(s, v) if norm_inf else s + v
            tsum[(0 if mistake == "tsum_t0" else t0) + j] = s
        part0 += int(blk0[-1])
        t += Tg
    s = 0.0
    for lane in range(64):
        tt = lane
        while tt < T:
            if norm_inf:
                s = _nanmax(s, tsum[tt])
            else:
                s += float(F32(math.sqrt(tsum[tt]))) ** 2
            tt += 64
            if mistake == "coef_one_trip":
                break
    total = F32(0) if T == 0 else (F32(s) if norm_inf else F32(math.sqrt(s)))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        coef = F32(max_norm) / (total + F32(1e-6))
    return total, coef, bool(T > 0 and coef < 1)


# ------------------------------------------------------------------------------------------------------------------
# fa_dp_apply / fa_dp_noise_i64
# ------------------------------------------------------------------------------------------------------------------
def dp_apply_expected(tab: Table, coef3, sigma, z, write_param=True):
    """What fa_dp_apply owes on ``tab`` (lists p, l, u): (p base after, u base after).  ``coef3`` = (total, coef,
    apply); ``z[t]``: the fp32 N(0,1) draws of tensor t.  Parameters: recovered = last + fp32(fp32(p - last) * coef)
    when clipping, last + fp32(p - last) otherwise; buffers (last None) untouched; upload = recovered +
    fp32(fp32(z * sigma) + 0).  Everything outside the views keeps its value."""
    coef, apply, sigma = F32(coef3[1]), bool(coef3[2]), F32(sigma)
    pb, ub = tab.base["p"].copy(), tab.base["u"].copy()
    for t in range(tab.T):
        p, l = tab.view("p", t), tab.view("l", t)
        rec = p
        if l is not None:
            d = p - l
            rec = l + (d * coef if apply else d)
            if write_param:
                tab.view("p", t, pb)[:] = rec
        tab.view("u", t, ub)[:] = rec + (np.asarray(z[t], F32) * sigma + F32(0))
    return pb, ub


def model_dp_apply(tab: Table, coef3, sigma, z, write_param=True, mistake=None):
    """k_dp_apply<0> with build_group's ``vec`` bit restated.  Mistakes: 'write_param' (flag ignored: parameters
    always written), 'coef_on_buffers' (d * coef applied where last is None), 'vec_upload' (the vec bit ignores
    the upload pointer)."""
    coef, apply, sigma = F32(coef3[1]), bool(coef3[2]), F32(sigma)
    pb, ub = tab.base["p"].copy(), tab.base["u"].copy()
    for t in range(tab.T):
        n, po, lo, uo = tab.n[t], tab.off["p"][t], tab.off["l"][t], tab.off["u"][t]
        vec = po % 4 == 0 and (lo is None or lo % 4 == 0) and (uo % 4 == 0 or mistake == "vec_upload")
        x, y = tab.view("p", t), tab.view("l", t)
        if y is not None:
            d = x - y
            pn = y + (d * coef if apply else d)
        else:
            pn = x * coef if (mistake == "coef_on_buffers" and apply) else x
        if (write_param or mistake == "write_param") and (y is not None or mistake == "coef_on_buffers"):
            pb[po:po + n] = pn
        c = pn + (np.asarray(z[t], F32) * sigma + F32(0))
        nv = n // 4 * 4 if vec else 0  # whole float4 groups; the tail and the scalar path go element by element
        ua = uo - uo % 4               # where a misaligned 16-byte store lands (see the module docstring)
        ub[ua:ua + nv] = c[:nv]
        ub[uo + nv:uo + n] = c[nv:]
    return pb, ub


def interleaved_module(layers: int, seed: int = 0):
    """A module whose state_dict interleaves fp32 parameters (integer-valued, 2 x 3), fp32 buffers (3) and 0-d
    int64 buffers, ``layers`` of each."""
    import torch

    g = torch.Generator().manual_seed(seed)
    m = torch.nn.Module()
    for i in range(layers):
        sub = torch.nn.Module()
        sub.register_parameter("weight", torch.nn.Parameter(torch.randint(-4, 5, (2, 3), generator=g).float(),
                                                            requires_grad=False))
        sub.register_buffer("running", torch.randn(3, generator=g))
        sub.register_buffer("count", torch.tensor(int(torch.randint(0, 1000, (1,), generator=g)) - 500))
        m.add_module(f"l{i}", sub)
    return m


I64_VALUES = [0, -1, 2 ** 53 + 1, -(2 ** 63), 2 ** 63 - 1, 12345]


def i64_case():
    """66 int64 tensors: 65 of one element and one of 4097."""
    rng = np.random.default_rng(66)
    xs = [np.array([I64_VALUES[t % len(I64_VALUES)]], dtype=np.int64) for t in range(65)]
    big = rng.integers(-2 ** 62, 2 ** 62, size=4097, dtype=np.int64)
    big[:len(I64_VALUES)] = I64_VALUES
    xs.insert(33, big)
    offs, o = [], 2 ** 33 - 1
    for x in xs:
        offs.append(o)
        o += len(x) + 1
    return xs, offs


# ------------------------------------------------------------------------------------------------------------------
# fused SGD + FedProx
# ------------------------------------------------------------------------------------------------------------------
SGD_SIZES = [0, 1, 3, 4, 5, 4095, 4096, 4097, 12289]
SGD_C = float(0.05 * 0.1)
SGD_OFFGRID = {44: "p", 45: "g", 46: "m", 47: "w"}  # exactly one operand 4 bytes off the 16-byte grid
# per-tensor scalars (lr, momentum, dampening, weight decay, nesterov) by position in the list
_CFG_A = (0.05, 0.9, 0.0, 5e-4, 0)
_CFG_A2 = (0.05, 0.5, 0.3, 5e-4, 0)
_CFG_B = (0.01, 0.0, 0.0, 0.0, 0)
_CFG_C = (0.2, 0.9, 0.0, 1e-3, 1)
SGD_UNIFORM = (0.05, 0.9, 0.3, 5e-4, 0)  # fa_sgd_prox_step: one group


def sgd_cfg(t: int):
    """The scalars change between 47 and 48 and between 95 and 96: the launch seams."""
    if t >= 96:
        return _CFG_C
    if t >= 48:
        return _CFG_B
    return _CFG_A2 if t % 5 == 2 else _CFG_A


def sgd_case(T: int, uniform: bool) -> Table:
    """T tensors with the lists p, g0..g2 (three steps' gradients), m, w.  Tensors 44-47 have exactly one operand
    off the grid; where t % 7 == 3 all four are off it by t % 3 + 1 elements.  ``cfg[t]``: the tensor's scalars
    (``uniform``: SGD_UNIFORM for all, as the single-group entry takes them); m is None where momentum is 0."""
    rng = np.random.default_rng(300 + T)
    n = [SGD_SIZES[t % 9] if t % 9 != 8 or t in (8, 53) else 4097 - t for t in range(T)]
    for t in SGD_OFFGRID:
        n[t] = 4097
    starts, total = _slots(n)
    tab = Table(n)
    tab.uniform = uniform
    tab.cfg = [SGD_UNIFORM if uniform else sgd_cfg(t) for t in range(T)]

    def shift(t, name):
        if t in SGD_OFFGRID:
            return 1 if SGD_OFFGRID[t] == name else 0
        return t % 3 + 1 if t % 7 == 3 else 0

    for name in ("p", "g0", "g1", "g2", "m", "w"):
        op = name[0]
        off = [s + shift(t, op) for t, s in enumerate(starts)]
        if op == "m":
            off = [None if tab.cfg[t][1] == 0 else o for t, o in enumerate(off)]
        tab.add(name, rng.normal(0, 1.0 if op == "g" else 0.5, size=total).astype(F32), off)
    return tab


def sgd_first(tab: Table, step: int, t: int) -> bool:
    """First-step tensors: most at step 0 (not t % 4 == 1: their buffers come initialised, so one launch mixes
    both kinds), and those with t % 6 == 0 again at step 1.  The single-group entry has one flag for the whole
    list: step 0."""
    if tab.cfg[t][1] == 0:
        return False
    if tab.uniform:
        return step == 0
    return (step == 0 and t % 4 != 1) or (step == 1 and t % 6 == 0)


def sgd_flags(tab: Table, step: int):
    return [(NESTEROV if tab.cfg[t][4] else 0) | (FIRST if sgd_first(tab, step, t) else 0) for t in range(tab.T)]


def sgd_poison(tab: Table, step: int, mb):
    """NaN into the buffer of every first-step tensor: a first step must not read it."""
    for t in range(tab.T):
        if sgd_first(tab, step, t):
            tab.view("m", t, mb)[:] = np.nan


def sgd_expected(tab: Table, fma: bool, prox: bool, steps: int = 3):
    """[(p base, m base) after step s]: sgd_prox_step_ref on the views, everything else untouched."""
    pb, mb = tab.base["p"].copy(), tab.base["m"].copy()
    lr, mom, damp, wd, _ = zip(*tab.cfg)
    out = []
    for s in range(steps):
        sgd_poison(tab, s, mb)
        newp, newm = sgd_prox_step_ref(tab.views("p", pb), tab.views(f"g{s}"), tab.views("m", mb),
                                       tab.views("w") if prox else None, lr, mom, damp, wd, sgd_flags(tab, s),
                                       SGD_C, fma)
        for t in range(tab.T):
            tab.view("p", t, pb)[:] = newp[t]
            if newm[t] is not None:
                tab.view("m", t, mb)[:] = newm[t]
        out.append((pb.copy(), mb.copy()))
    return out


def model_sgd(tab: Table, fma: bool, prox: bool, single: bool, steps: int = 3, mistake=None):
    """sgd_groups / fa_sgd_prox_step restated: launches of SGD_MAX tensors, each with its table of pointers and
    scalars by launch slot j = t - (first tensor of the launch); ``single``: the single-group entry, which cuts
    the list itself and passes each piece on with every table advanced.  A table outlives a launch here (the next
    launch finds the previous one's entries where it writes none).  Mistakes: 'scalars_from_slot' (slot j filled
    from scalar[j], the launch slot where the list position belongs), 'scalars_to_list_pos' (scalar[t] stored at
    table index t, the list position where the launch slot belongs: past the table's end from the second launch
    on, so the slot keeps its old entry), 'bufs_not_advanced' (single: momentum_buf not advanced with the other
    tables), 'first_reads' (a first step reads the buffer), 'vec_momentum' (the vec bit ignores the momentum
    pointer).  Returns [(p base, m base) after step s]."""
    pb, mb = tab.base["p"].copy(), tab.base["m"].copy()
    out = []
    for s in range(steps):
        sgd_poison(tab, s, mb)
        flags = sgd_flags(tab, s)
        table = [None] * SGD_MAX
        for t0 in range(0, tab.T, SGD_MAX):
            Tg = min(SGD_MAX, tab.T - t0)
            for j in range(Tg):
                t = t0 + j
                if mistake == "scalars_from_slot":
                    table[j] = (tab.cfg[j], flags[j])
                elif mistake == "scalars_to_list_pos":
                    if t < SGD_MAX:
                        table[t] = (tab.cfg[t], flags[t])
                else:
                    table[j] = (tab.cfg[t], flags[t])
            for j in range(Tg):  # the workgroups of tensor j
                t = t0 + j
                (lr, mom, damp, wd, _), fl = table[j]
                n = tab.n[t]
                mt = j if (single and mistake == "bufs_not_advanced") else t
                mo = tab.off["m"][mt] if mom != 0 else None
                offs = [tab.off["p"][t], tab.off[f"g{s}"][t], mo, tab.off["w"][t] if prox else None]
                vec = all(o is None or o % 4 == 0 or (mistake == "vec_momentum" and k == 2)
                          for k, o in enumerate(offs))
                nv = n // 4 * 4 if vec else 0
                m_in = None
                if mo is not None:
                    ma = mo - mo % 4  # misaligned float4 accesses land on the granule below
                    m_in = np.concatenate([mb[ma:ma + nv], mb[mo + nv:mo + n]])
                elif mom != 0:  # wrong scalars ask for a buffer the tensor does not have: no defined result
                    m_in = np.full(n, np.nan, F32)
                f = fl & ~FIRST if mistake == "first_reads" else fl
                newp, newm = sgd_prox_step_ref([tab.view("p", t, pb)], [tab.view(f"g{s}", t)], [m_in],
                                               [tab.view("w", t)] if prox else None, [lr], [mom], [damp], [wd],
                                               [f], SGD_C, fma)
                tab.view("p", t, pb)[:] = newp[0]
                if mo is not None:
                    mb[ma:ma + nv] = newm[0][:nv]
                    mb[mo + nv:mo + n] = newm[0][nv:]
        out.append((pb.copy(), mb.copy()))
    return out
