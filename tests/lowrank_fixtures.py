"""What the low-rank tests share: the staged-row packer, the float64 reference and the error bound.

An upload is a list, one array per float32 entry of ``shapes``: float32 [r, O + I] for a factored entry (row j is
Ut[j, :O] then V[j, :I]), the dense delta in the entry's shape otherwise.

The bound.  An output element is acc_in plus m = n * r2 products u * v (the padding rows' are +0), each rounded once
at most (fused: not at all) and added by m additions in some order.  Whatever the order and whether or not the
products are rounded first, every term passes through at most m + 1 roundings (its own, then at most m additions;
acc_in through at most m), each of relative size at most u = 2^-24, so by the standard induction (Higham, Accuracy
and Stability of Numerical Algorithms, §3.1 and §4.2: fl(sum) = sum x_i (1 + theta_i), |theta_i| <= gamma_k for k
roundings) with one more rounding allowed for a doubly rounded product inside the instruction,

    |out - exact| <= gamma_{m+2} * (sum |u| |v| + |acc_in|),      gamma_k = k 2^-24 / (1 - k 2^-24),

provided nothing is subnormal (the tests scale their data so).  ``exact`` is taken in float64, whose own error
(gamma in 2^-53) is nine orders below the bound.
"""
import numpy as np

from fedscale_amd.cloud.execution.lowrank_upload import factored, matrix_dims


def up(v, m):
    return (v + m - 1) // m * m


def pack_rows(uploads, shapes, rank):
    """(rows float32 [n, ldf], offsets [(ut, v)]) — the staged format of include/fedlowrank.h, restated."""
    r2, off, offs = up(rank, 2), 0, []
    for s in shapes:
        off = up(off, 4)
        O, I = matrix_dims(s)
        if factored(s, rank):
            offs.append((off, off + r2 * up(O, 4)))
            off = offs[-1][1] + r2 * up(I, 4)
        else:
            offs.append((off, 0))
            off += int(np.prod(s, dtype=np.int64))
    ldf = max(64, up(off, 64))
    rows = np.zeros((len(uploads), ldf), dtype=np.float32)
    for k, upl in enumerate(uploads):
        for s, (uo, vo), a in zip(shapes, offs, upl):
            O, I = matrix_dims(s)
            if factored(s, rank):
                rows[k, uo:uo + r2 * up(O, 4)].reshape(r2, -1)[:rank, :O] = a[:, :O]
                rows[k, vo:vo + r2 * up(I, 4)].reshape(r2, -1)[:rank, :I] = a[:, O:]
            else:
                rows[k, uo:uo + a.size] = a.reshape(-1)
    return rows, offs


def _terms(uploads, shapes, rank, acc, absolute):
    out = np.zeros(sum(int(np.prod(s, dtype=np.int64)) for s in shapes), dtype=np.float64)
    if acc is not None:
        out += np.abs(acc[:out.size]) if absolute else acc[:out.size]
    p = 0
    for e, s in enumerate(shapes):
        O, I = matrix_dims(s)
        n = O * I if len(s) else 1
        for upl in uploads:
            a = upl[e].astype(np.float64)
            a = np.abs(a) if absolute else a
            out[p:p + n] += (a[:, :O].T @ a[:, O:]).reshape(-1) if factored(s, rank) else a.reshape(-1)
        p += n
    return out


def ref64(uploads, shapes, rank, acc=None):
    """float64 sum over the uploads of Ut^T V (dense entries: of the deltas), plus ``acc``: the whole bucket."""
    return _terms(uploads, shapes, rank, acc, False)


def bound(uploads, shapes, rank, acc=None):
    """The any-order bound above per element of the bucket, m = n * r2."""
    m = len(uploads) * up(rank, 2) + 2
    g = m * 2.0 ** -24 / (1 - m * 2.0 ** -24)
    return g * _terms(uploads, shapes, rank, acc, True)
