"""A numpy restatement of the block Hadamard rotation contract (include/fedrotate.h), written from the header's text
and independent of the product code: the splitmix64 diagonal (python integers), the twelve staged butterflies over
index pairs, the forward and inverse transforms, and the whole rotated round — rotate, sign encode with the residual
in rotated space, chain, unrotate, L + chain / K.  The sign encoding, the chain and the finish are those of
tests/sign_fixtures.py.  Test infrastructure, shared by the CPU and GPU tests of the path.  All parity against it is
bit for bit."""
import numpy as np

from tests import sign_fixtures as sg

BLOCK = 4096
F32 = np.float32
M64 = (1 << 64) - 1
ROTATE_KEY = "__rot_seed__"
SPLITMIX_SEED0 = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC)


def padded(P: int) -> int:
    return -(-int(P) // BLOCK) * BLOCK


def diag_word(seed: int, w: int) -> int:
    """z(w): the 64 diagonal bits of columns [64w, 64w + 64)."""
    z = (seed + (w + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def diag(seed: int, n: int) -> np.ndarray:
    """uint32 [n]: d[p] = (z(p >> 6) >> (p & 63)) & 1."""
    words = np.array([diag_word(seed, w) for w in range((n + 63) // 64)], dtype=np.uint64)
    p = np.arange(n, dtype=np.uint64)
    return ((words[p >> np.uint64(6)] >> (p & np.uint64(63))) & np.uint64(1)).astype(np.uint32)


def flip(v: np.ndarray, seed: int) -> np.ndarray:
    """v with d[p] xored into every column's fp32 sign bit."""
    u = np.ascontiguousarray(v, dtype=F32).view(np.uint32) ^ (diag(seed, v.size) << np.uint32(31))
    return u.view(F32)


def butterflies(v: np.ndarray) -> np.ndarray:
    """The twelve stages h = 1, 2, ..., 2048 over every block of 4096 columns, then the multiply by 2^-6: for every
    index i of the block with (i & h) == 0, (v[i], v[i + h]) <- (v[i] + v[i + h], v[i] - v[i + h]) in fp32."""
    v = np.array(v, dtype=F32).reshape(-1, BLOCK)
    idx = np.arange(BLOCK)
    with np.errstate(invalid="ignore", over="ignore"):
        h = 1
        while h < BLOCK:
            lo = idx[(idx & h) == 0]
            a, b = v[:, lo].copy(), v[:, lo + h].copy()
            v[:, lo] = (a + b).astype(F32)
            v[:, lo + h] = (a - b).astype(F32)
            h *= 2
        v = (v * F32(2.0 ** -6)).astype(F32)
    return v.reshape(-1)


def rotate(x, base=None, seed: int = 0) -> np.ndarray:
    """frt_rotate: float32 [P']."""
    x = np.asarray(x, dtype=F32).reshape(-1)
    P = x.size
    e = np.zeros(padded(P), dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        e[:P] = x if base is None else (x - np.asarray(base, dtype=F32).reshape(-1)).astype(F32)
    return butterflies(flip(e, seed)) if P else e


def unrotate(y, P: int, seed: int = 0) -> np.ndarray:
    """frt_unrotate: float32 [P]."""
    y = np.asarray(y, dtype=F32).reshape(-1)
    assert y.size == padded(P)
    if P == 0:
        return np.zeros(0, dtype=F32)
    return flip(butterflies(y), seed)[:P].copy()


def dense(x, seed: int) -> np.ndarray:
    """float64 [4096]: H D x / 64 for one block by the dense Sylvester matrix."""
    H = np.array([[1.0]])
    while H.shape[0] < BLOCK:
        H = np.block([[H, H], [H, -H]])
    d = 1.0 - 2.0 * diag(seed, BLOCK).astype(np.float64)
    return H @ (d * np.asarray(x, dtype=np.float64)) / 64.0


def encode(x, base, seed: int, residual=None):
    """(bits [P' / 8], scales [P' / 256], residual_out [P']) of one executor's upload: rotate, add the rotated-space
    residual (one fp32 rounding), sign encode."""
    y = rotate(x, base, seed)
    if residual is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            y = (y + np.asarray(residual, dtype=F32)).astype(F32)
    return sg.encode_fast(y)


def round_model(L, rows, seed: int) -> np.ndarray:
    """The new model of a rotated round: chain the (bits, scales) rows over P' columns in order, unrotate, then
    L + chain / K."""
    L = np.asarray(L, dtype=F32).reshape(-1)
    P = L.size
    c = sg.chain(rows, P=padded(P))
    return sg.finish(L, unrotate(c, P, seed), len(rows))


def kept_energy(e, bits, scales) -> float:
    """The share of ||e||^2 an encoding keeps: 1 - ||e - deq||^2 / ||e||^2, in float64."""
    e = np.asarray(e, dtype=np.float64)
    deq = sg.dequantize(bits, scales, e.size).astype(np.float64)
    return 1.0 - float(((e - deq) ** 2).sum() / (e ** 2).sum())


def same(got, want, ctx=None):
    sg.same(got, want, ctx)
