"""The secure-aggregation path restated in numpy (include/fedsecagg.h): encode, the ChaCha20 word stream with col0,
mask sum, reduce, finish with the range count, fsa_reduce's launch plan, and a whole round over a mask graph with
dropouts.  Everything the device computes is held to bit equality with this file.

The stream is written here from RFC 8439 section 2.3 alone (scalar-looking code vectorised over the block counter),
independently of fedscale_amd/cloud/execution/secagg_upload.py.  Known answers 1 and 2 are the published ones
(RFC 8439 section 2.3.2, and the all-zero key / nonce blocks 0 and 1 of the RFC's appendix A.1).  Known answer 3
comes only from this restatement, which reproduces 1 and 2; no crypto library was at hand to cross-check it.
"""
import numpy as np

U32 = np.uint32
INT32_MAX = (1 << 31) - 1

RFC_KEY = tuple(0x03020100 + 0x04040404 * i for i in range(8))  # bytes 00 01 .. 1f, as little-endian words
KAT1 = dict(key=RFC_KEY, nonce=(0x09000000, 0x4A000000, 0), col0=16, P=16, lo=0,
            words="e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
                  "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2")
KAT2 = dict(key=(0,) * 8, nonce=(0, 0, 0), col0=0, P=20, lo=0,
            words="ade0b876 903df1a0 e56a5d40 28bd8653 b819d2bd 1aed8da0 ccef36a8 c70d778b "
                  "7c5941da 8d485751 3fe02477 374ad8b8 f4b8436a 1ca11815 69b687c3 8665eeb2 "
                  "bee7079f 7a385155 7c97ba98 0d082d73")
#: the counter crosses 0x7FFFFFFF -> 0x80000000 inside the call; from this restatement only (see the module docstring)
KAT3 = dict(key=RFC_KEY, nonce=(1, 2, 3), col0=16 * ((1 << 31) - 1), P=21, lo=13,
            words="9a094b37 21450ad8 e92c01bf 90c0d0fa aaaee375 f4ed1c01 939e54d6 4d3594fc")
KATS = (KAT1, KAT2, KAT3)


def kat_words(kat) -> np.ndarray:
    return np.asarray([int(w, 16) for w in kat["words"].split()], dtype=U32)


def _rotl(v, n):
    return (v << U32(n)) | (v >> U32(32 - n))


def _qr(s, a, b, c, d):
    s[a] = s[a] + s[b]; s[d] = _rotl(s[d] ^ s[a], 16)
    s[c] = s[c] + s[d]; s[b] = _rotl(s[b] ^ s[c], 12)
    s[a] = s[a] + s[b]; s[d] = _rotl(s[d] ^ s[a], 8)
    s[c] = s[c] + s[d]; s[b] = _rotl(s[b] ^ s[c], 7)


def streams(keys, nonce, col0: int, P: int) -> np.ndarray:
    """uint32 [M, P]: for each of the M keys, word (c mod 16) of the ChaCha20 block with counter (c div 16), for
    c = col0 .. col0 + P - 1 (the block function vectorised over keys and counters)."""
    assert col0 >= 0 and col0 % 16 == 0 and col0 + P <= 1 << 36
    keys = np.asarray(keys, dtype=U32).reshape(-1, 8)
    M, nb = len(keys), (P + 15) // 16
    ctr = (np.arange(nb, dtype=np.uint64) + np.uint64(col0 // 16))
    assert nb == 0 or int(ctr[-1]) < 1 << 32
    const = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
    init = [np.full((M, nb), w, dtype=U32) for w in const]
    init += [np.broadcast_to(keys[:, i:i + 1], (M, nb)).copy() for i in range(8)]
    init += [np.broadcast_to(ctr.astype(U32), (M, nb)).copy()]
    init += [np.full((M, nb), int(n), dtype=U32) for n in nonce]
    s = [v.copy() for v in init]
    for _ in range(10):
        _qr(s, 0, 4, 8, 12); _qr(s, 1, 5, 9, 13); _qr(s, 2, 6, 10, 14); _qr(s, 3, 7, 11, 15)
        _qr(s, 0, 5, 10, 15); _qr(s, 1, 6, 11, 12); _qr(s, 2, 7, 8, 13); _qr(s, 3, 4, 9, 14)
    out = np.stack([s[i] + init[i] for i in range(16)], axis=2).reshape(M, 16 * nb)
    return out[:, :P]


def stream(key, nonce, col0: int, P: int) -> np.ndarray:
    """uint32 [P]: PRG(key, nonce, c) for c = col0 .. col0 + P - 1."""
    return streams([key], nonce, col0, P)[0]


def mask_sum(acc, add_keys, sub_keys, nonce, col0: int = 0) -> np.ndarray:
    out = np.array(acc, dtype=U32, copy=True)
    for k in add_keys:
        out = out + stream(k, nonce, col0, out.size)
    for k in sub_keys:
        out = out - stream(k, nonce, col0, out.size)
    return out


def encode(x, base, frac_bits: int, mag_bits: int):
    """(uint32 [P] words, n_clamped, n_nan) of the fp32 rows x - base."""
    B = float((1 << mag_bits) - 1)
    with np.errstate(all="ignore"):
        d = np.asarray(x, dtype=np.float32) - np.asarray(base, dtype=np.float32)
        t = d * np.float32(2.0 ** frac_bits)
        assert t.dtype == np.float32
        r = np.rint(t).astype(np.float64)
    nan = np.isnan(r)
    clamped = ~nan & (np.abs(r) > B)
    q = np.where(nan, 0.0, np.clip(r, -B, B)).astype(np.int64)
    return q.astype(np.int32).view(U32), int(clamped.sum()), int(nan.sum())


def reduce(rows, acc=None) -> np.ndarray:
    """The sum mod 2^32 of the uint32 rows [n, P], continuing ``acc``."""
    rows = np.asarray(rows, dtype=U32)
    tot = rows.astype(np.uint64).sum(axis=0) + (0 if acc is None else np.asarray(acc, dtype=U32).astype(np.uint64))
    return (tot & np.uint64(0xFFFFFFFF)).astype(U32)


def finish(total, last, frac_bits: int, mag_bits: int, n: int):
    """(float32 [P] new model, columns with |s| > n B)."""
    s = np.asarray(total, dtype=U32).view(np.int32).astype(np.int64)
    bound = n * ((1 << mag_bits) - 1)
    assert bound <= INT32_MAX
    m = ((s.astype(np.float64) * 2.0 ** -frac_bits) / np.float64(n)).astype(np.float32)
    out = np.asarray(last, dtype=np.float32) + m
    assert out.dtype == np.float32
    return out, int((np.abs(s) > bound).sum())


def crafted_encode_case(frac_bits: int = 16, mag_bits: int = 20):
    """(x, base, expected int32 words, n_clamped, n_nan): every rule of the encoder on one row, written down by hand
    — ties to even, +-B and one past it, +-inf, NaN, -0, a tiny value, a product that overflows fp32, a non-zero
    base."""
    u = 2.0 ** -frac_bits
    B = (1 << mag_bits) - 1
    cases = [  # (x, base, q, clamped, nan)
        (0.5 * u, 0.0, 0, 0, 0), (1.5 * u, 0.0, 2, 0, 0), (2.5 * u, 0.0, 2, 0, 0), (3.5 * u, 0.0, 4, 0, 0),
        (-0.5 * u, 0.0, 0, 0, 0), (-1.5 * u, 0.0, -2, 0, 0), (-2.5 * u, 0.0, -2, 0, 0),
        (B * u, 0.0, B, 0, 0), ((B + 1) * u, 0.0, B, 1, 0), (-B * u, 0.0, -B, 0, 0), (-(B + 1) * u, 0.0, -B, 1, 0),
        (np.inf, 0.0, B, 1, 0), (-np.inf, 0.0, -B, 1, 0), (np.nan, 0.0, 0, 0, 1), (1.0, np.nan, 0, 0, 1),
        (np.inf, np.inf, 0, 0, 1),  # inf - inf
        (-0.0, 0.0, 0, 0, 0), (1e-30, 0.0, 0, 0, 0), (-1e-30, 0.0, 0, 0, 0),
        (1e38, 0.0, B, 1, 0), (-1e38, 0.0, -B, 1, 0),  # d * 2^f overflows fp32 to +-inf
        (1.0, 0.75, int(0.25 / u), 0, 0), (0.75, 1.0, -int(0.25 / u), 0, 0), (3.0 * u, 1.0 * u, 2, 0, 0),
    ]
    assert float(np.float32(B * u)) == B * u  # B / 2^f is an fp32: the +-B cases are what they say
    x = np.asarray([c[0] for c in cases], dtype=np.float32)
    base = np.asarray([c[1] for c in cases], dtype=np.float32)
    q = np.asarray([c[2] for c in cases], dtype=np.int32)
    return x, base, q, sum(c[3] for c in cases), sum(c[4] for c in cases)


def crafted_finish_case(n: int, mag_bits: int = 20):
    """(uint32 sums, expected out-of-range count): INT32_MIN, -1, 0, +-nB, +-(nB + 1), INT32_MAX and small odd sums
    whose division by n rounds."""
    nB = n * ((1 << mag_bits) - 1)
    s = [-(1 << 31), -1, 0, nB, nB + 1, -nB, -nB - 1, INT32_MAX, 1, 2, 5, 7, -7, 100003, -100003, nB - 1]
    bad = sum(1 for v in s if abs(v) > nB)
    return np.asarray(s, dtype=np.int64).astype(np.int32).view(U32), bad


# ---- fsa_reduce's launch plan (strip_plan of fa_common.h over strips of 256 columns) -------------------------------
WAVES = 4
LEVELS = ((16, 2), (8, 4), (2, 8))  # (V, U) of levels 0, 1, 2
CAP_PCT = 75
STRIP = 256  # columns of one strip: 64 lanes x 4 columns


def strips(P: int) -> int:
    return ((P + 3) // 4 + 63) // 64


def plan(cus: int, K: int, P: int) -> list:
    """The launches of fsa_reduce at (K, P) on ``cus`` compute units: dicts V, U, col0, tiles, sw, grid."""
    if P <= 0 or cus <= 0:
        return []
    S = strips(P)
    cap = max(1, cus * CAP_PCT // 100)
    span = [WAVES * v for v, _ in LEVELS]

    def launch(level, strip0, tiles, grid):
        v, u = LEVELS[level]
        return dict(V=v, U=u, col0=strip0 * STRIP, tiles=tiles, sw=v, grid=grid)

    t0 = (S + span[0] - 1) // span[0]
    if t0 * 100 >= cap * 85:
        rounds = (t0 + cap - 1) // cap
        return [launch(0, 0, t0, (t0 + rounds - 1) // rounds)]
    out, s = [], 0
    n1 = S // span[1]
    if n1 > 0 and 2 * n1 >= cus:
        out.append(launch(1, 0, n1, n1))
        s = n1 * span[1]
    if s < S:
        t2 = (S - s + span[2] - 1) // span[2]
        out.append(launch(2, s, t2, t2))
    return out


def seam_widths(launches) -> list:
    """One width just past each tile or level seam of a plan: the first column of every launch after the first, of the
    second tile of every launch, and of the second strip — plus one, so that a lone column sits past the seam."""
    out = set()
    for l in launches:
        tile = WAVES * l["sw"] * STRIP
        for seam in (l["col0"], l["col0"] + tile, l["col0"] + STRIP):
            if seam > 0:
                out.add(seam + 1)
    return sorted(out)


# ---- a whole round over a mask graph --------------------------------------------------------------------------------
def make_keys(rng, n: int) -> list:
    return [tuple(int(v) for v in rng.integers(0, 1 << 32, 8, dtype=np.uint64)) for _ in range(n)]


class RingGraph:
    """K clients on a ring, every client paired with its neighbours at distance 1 .. reach (reach = 2: 4-regular).
    Client u ADDS the pairwise mask towards a neighbour with a larger id and SUBTRACTS it towards a smaller one."""

    def __init__(self, rng, K: int, reach: int = 2):
        self.K = K
        self.self_keys = make_keys(rng, K)
        self.pairs = {}
        for u in range(K):
            for dist in range(1, reach + 1):
                v = (u + dist) % K
                if u != v:
                    self.pairs.setdefault((min(u, v), max(u, v)), None)
        for p, k in zip(sorted(self.pairs), make_keys(rng, len(self.pairs))):
            self.pairs[p] = k

    def client_keys(self, u: int):
        """(self key, keys to add, keys to subtract) of client u."""
        add = [k for (a, b), k in sorted(self.pairs.items()) if a == u]
        sub = [k for (a, b), k in sorted(self.pairs.items()) if b == u]
        return self.self_keys[u], add, sub

    def unmask_keys(self, arrived, skip_pair=None):
        """(sub_keys, add_keys) for ``SecAggRound.unmask`` when only ``arrived`` uploaded: their self keys, and every
        pairwise key between an arrived client and a dropped neighbour, with the sign that cancels what the arrived
        one applied.  ``skip_pair``: leave that pair's key out (a faulty reconstruction)."""
        arrived = set(arrived)
        sub = [self.self_keys[u] for u in sorted(arrived)]
        add = []
        for (a, b), k in sorted(self.pairs.items()):
            if (a, b) == skip_pair:
                continue
            if a in arrived and b not in arrived:
                sub.append(k)  # a added it
            elif b in arrived and a not in arrived:
                add.append(k)  # b subtracted it
        return sub, add


def masked_upload(q, graph: RingGraph, u: int, nonce) -> np.ndarray:
    self_key, add, sub = graph.client_keys(u)
    return mask_sum(q, [self_key] + add, sub, nonce)


def round_model(xs, last, frac_bits: int, mag_bits: int, graph=None, arrived=None, nonce=(0, 0, 0), skip_pair=None):
    """A whole round restated: ``xs`` the arrived clients' fp32 rows (in ``arrived``'s order), ``last`` the starting
    model.  Returns (new model, out-of-range count, the unmasked sum, n_clamped)."""
    n = len(xs)
    enc = [encode(x, last, frac_bits, mag_bits) for x in xs]
    rows = [e[0] for e in enc]
    if graph is not None:
        rows = [masked_upload(q, graph, u, nonce) for q, u in zip(rows, arrived)]
    total = reduce(rows)
    if graph is not None:
        sub, add = graph.unmask_keys(arrived, skip_pair)
        total = mask_sum(total, add, sub, nonce)
    out, bad = finish(total, last, frac_bits, mag_bits, n)
    return out, bad, total, sum(e[1] for e in enc)
