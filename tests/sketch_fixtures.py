"""The contract of include/fedsketch.h restated in numpy and Python integers, independently of
fedscale_amd/cloud/execution/sketch_upload.py: the hash on Python ints, the chain as one sequential fp32 add per block
in ascending block order, the median by sorting keys, and the FetchSGD round."""
import numpy as np

M64 = (1 << 64) - 1
G = 0xD1B54A32D192ED03


def mix(s, w):
    z = (s + (w + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def signs(seed, j, P):
    """uint32 [P]: sigma_j(p) << 31."""
    s = (seed + (2 * j + 1) * G) & M64
    words = np.array([mix(s, w) for w in range((P + 63) // 64)], dtype=np.uint64)
    p = np.arange(P, dtype=np.uint64)
    bits = (words[(p >> np.uint64(6)).astype(np.int64)] >> (p & np.uint64(63))) & np.uint64(1)
    return bits.astype(np.uint32) << np.uint32(31)


def buckets(seed, j, P, C):
    """int64 [P]: the bucket of every column in row j."""
    s = (seed + (2 * j + 2) * G) & M64
    m = np.array([mix(s, b) & (C - 1) for b in range((P + C - 1) // C)], dtype=np.int64)
    p = np.arange(P, dtype=np.int64)
    return (p & (C - 1)) ^ m[p // C] if P else p


def sketch(e, R, C, seed):
    e = np.asarray(e, dtype=np.float32)
    P = e.size
    T = np.zeros((R, C), dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(R):
            t = (e.view(np.uint32) ^ signs(seed, j, P)).view(np.float32)
            q = buckets(seed, j, P, C)
            for lo in range(0, P, C):  # one column per bucket and block: a vector add is the chain's next term
                hi = min(P, lo + C)
                T[j, q[lo:hi]] = T[j, q[lo:hi]] + t[lo:hi]
    return T


def keys(v):
    b = np.asarray(v, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkeys(k):
    return (k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def estimate(T, P, seed):
    R, C = T.shape
    v = np.stack([(T[j, buckets(seed, j, P, C)].view(np.uint32) ^ signs(seed, j, P)).view(np.float32)
                  for j in range(R)])
    return unkeys(np.sort(keys(v), axis=0)[R // 2])


def topk(est, k):
    """The columns fs_topk_row keeps (include/fedsparse.h): the k largest |bits|, ties to the lowest index."""
    key = est.view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.sort(np.argsort(-key.astype(np.int64), kind="stable")[:min(k, est.size)])


def fetch_round(L, tables, Su, Se, rho, k, seed):
    """(new L, S_u, S_e, idx) of one round over the uploaded tables, in arrival order."""
    with np.errstate(all="ignore"):
        S = tables[0].copy()
        for t in tables[1:]:
            S = S + t
        S = S / np.float32(len(tables))
        Su = np.float32(rho) * Su + S
        Se = Se + Su
        est = estimate(Se, L.size, seed)
        idx = topk(est, k)
        delta = np.zeros(L.size, dtype=np.float32)
        delta[idx] = est[idx]
        new = L.copy()
        new[idx] = L[idx] + est[idx]
        return new, Su, Se - sketch(delta, Se.shape[0], Se.shape[1], seed), idx
