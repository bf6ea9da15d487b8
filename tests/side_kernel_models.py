"""Host restatements of the int64 side-table kernels and of the two elementwise finishers of
fedscale_amd/csrc/fedagg.hip (k_side_accum, k_side_close, k_side_yogi, k_side_qfed_delta / _sq / _finalize,
k_yogi_step, k_qfed_finalize).  Numpy only.

Every arithmetic step of those kernels is one IEEE basic operation (the library is built with -ffp-contract=off),
and numpy performs the same operation: int64 addition wraps, int64 -> float32 / float64 ``astype`` rounds to nearest
even, ``np.sqrt`` and ``1.0 / x`` on float64 are correctly rounded.  So each ``model_*`` follows its kernel
operation by operation and the device is held to it bit for bit (tests/test_gpu_side_kernels.py,
tests/test_gpu_finish_kernels.py).

Each model takes a ``mistake`` that plants one error.  Without a mistake a model must equal the reference
semantics (oracle/cpu_reference.py's numpy and torch expressions); with one it must not, on the very inputs the
device tests use (tests/side_fixtures.py): that is how tests/test_side_oracle.py shows that each device test can see
the mistake it is there for.

Buffers are passed as the device test allocates them: ``ldq`` (or more) long, prefilled.  A model returns new
arrays of the same length with elements [0:Q] written and the rest as they came."""
from fractions import Fraction

import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
WG = 64  # threads of a side-kernel workgroup
STRIDE_BLOCK, STRIDE_MAX_BLOCKS = 256, 8192  # stride_grid(): threads per workgroup, most workgroups of a launch


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b) -> bool:
    """Equal bit for bit (so -0 is not +0), except that a NaN equals a NaN whatever its sign and payload: those are
    not arithmetic (x86 and gfx950 generate different default NaNs)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    eq = bits(a) == bits(b)
    if a.dtype.kind == "f":
        eq = eq | (np.isnan(a) & np.isnan(b))
    return bool(np.all(eq))


def _to_i64(f32) -> np.ndarray:
    """What a float32 becomes in an int64 state_dict entry (load_state_dict's float32 -> int64 ``copy_`` on the
    CPU): truncation toward zero, and INT64_MIN for NaN, +-inf and |v| >= 2^63."""
    f = np.asarray(f32)
    assert f.dtype == F32
    ok = np.isfinite(f) & (np.abs(f) < F32(2.0 ** 63))
    out = np.full(f.shape, I64_MIN, I64)
    out[ok] = np.trunc(f[ok]).astype(I64)
    return out


def _f64_to_i64(d) -> np.ndarray:
    """The mistake of truncating the double itself (no fp32 step)."""
    d = np.asarray(d, F64)
    ok = np.isfinite(d) & (np.abs(d) < 2.0 ** 63)
    out = np.full(d.shape, I64_MIN, I64)
    out[ok] = np.trunc(d[ok]).astype(I64)
    return out


def _sgn(x):
    """sgnf / sgnd: -1, 0, +1; a zero or a NaN passes through."""
    one = x.dtype.type(1)
    return np.where(x > 0, one, np.where(x < 0, -one, x))


def _rows(xi, ldq, K, Q, stride):
    flat = np.ascontiguousarray(xi).reshape(-1)
    assert flat.dtype == I64 and flat.size >= (K - 1) * ldq + Q
    return [flat[k * stride:k * stride + Q] for k in range(K)]


def _fma_f64(a, x, y):
    """y + a*x rounded once, elementwise, by exact rational arithmetic (float(Fraction) rounds correctly)."""
    out = np.empty(len(y), F64)
    for i in range(len(y)):
        vals = (float(a[i]), float(x[i]), float(y[i]))
        if not all(np.isfinite(v) for v in vals):
            out[i] = vals[2] + vals[0] * vals[1]
            continue
        r = Fraction(vals[2]) + Fraction(vals[0]) * Fraction(vals[1])
        out[i] = float(r) if r != 0 else vals[2] + vals[0] * vals[1]  # an exact zero keeps IEEE's sign
    return out


def _sat_add(a, b):
    s = [min(max(int(x) + int(y), I64_MIN), I64_MAX) for x, y in zip(a, b)]
    return np.array(s, dtype=I64)


# ------------------------------------------------------------------------------------------------------------------
# k_side_accum
# ------------------------------------------------------------------------------------------------------------------
ACCUM_MISTAKES = ("stride_q", "client0_twice", "accumulate_ignored", "first_workgroup_only")
ACCUM0_MISTAKES = ACCUM_MISTAKES + ("saturate",)
ACCUM1_MISTAKES = ACCUM_MISTAKES + ("fused", "w_prev", "via_f32")


def model_side_accum(xi, ldq, K, Q, mode, w, acc, accumulate, mistake=None):
    """mode 0: acc (int64) <- the wrapping sum of rows 0..K-1 (aggregator.py:497-503 on int64 arrays);
    mode 1: acc (float64) <- x0 * w0, then acc + w[k] * x[k] (async_aggregator.py:129-133).  ``accumulate``: the
    chain continues from acc.  Rows are ``ldq`` apart in ``xi``."""
    out = np.array(acc, copy=True)
    assert out.dtype == (I64 if mode == 0 else F64) and out.size >= Q
    if K == 0:
        return out
    rows = _rows(xi, ldq, K, Q, Q if mistake == "stride_q" else ldq)
    if mistake == "accumulate_ignored":
        accumulate = False
    k0 = 0 if accumulate or mistake == "client0_twice" else 1
    if mode == 0:
        s = out[:Q].copy() if accumulate else rows[0].copy()
        for k in range(k0, K):
            s = _sat_add(s, rows[k]) if mistake == "saturate" else s + rows[k]  # numpy int64 addition wraps
    else:
        w = np.asarray(w, F64)
        wide = (lambda x: x.astype(F32).astype(F64)) if mistake == "via_f32" else (lambda x: x.astype(F64))
        s = out[:Q].copy() if accumulate else wide(rows[0]) * w[0]
        for k in range(k0, K):
            wk = w[max(k - 1, 0)] if mistake == "w_prev" else w[k]
            if mistake == "fused":
                s = _fma_f64(np.full(Q, wk), wide(rows[k]), s)
            else:
                s = s + wk * wide(rows[k])
    n = min(Q, WG) if mistake == "first_workgroup_only" else Q
    out[:n] = s[:n]
    return out


# ------------------------------------------------------------------------------------------------------------------
# k_side_close
# ------------------------------------------------------------------------------------------------------------------
CLOSE_MISTAKES = ("trunc_double", "round_nearest", "div_f32", "first_workgroup_only")
CLOSE1_MISTAKES = CLOSE_MISTAKES + ("acc_i_in_mode1",)


def model_side_close(acc, Q, mode, denom, mistake=None, acc_i=None):
    """(cur, model) of Q elements: cur = acc / denom in float64 (np.divide of an int64 or float64 array,
    aggregator.py:505-507 / async_aggregator.py:134-135), model = np.asarray(cur, float32) copied into an int64
    entry (torch_model_adapter.py:28-33).  ``acc_i``: the int64 accumulator a mode 1 call is also handed (only the
    mistake reads it)."""
    src = acc_i if (mistake == "acc_i_in_mode1" and mode == 1) else acc
    a = np.asarray(src)[:Q]
    assert a.dtype == (I64 if (mode == 0 or src is acc_i) else F64)
    with np.errstate(all="ignore"):
        if mistake == "div_f32":
            cur = (a.astype(F32) / F32(denom)).astype(F64)
        else:
            cur = a.astype(F64) / F64(denom)
        if mistake == "trunc_double":
            model = _f64_to_i64(cur)
        elif mistake == "round_nearest":
            f = cur.astype(F32)
            model = _to_i64(np.where(np.isfinite(f), np.rint(f), f).astype(F32))
        else:
            model = _to_i64(cur.astype(F32))
    if mistake == "first_workgroup_only":
        cur, model = cur.copy(), model.copy()
        cur[WG:], model[WG:] = np.nan, -1
    return cur, model


# ------------------------------------------------------------------------------------------------------------------
# k_side_yogi
# ------------------------------------------------------------------------------------------------------------------
YOGI_MISTAKES = ("init_ignored", "eta_div_den", "sign_of_v", "last_ignored", "model_from_double",
                 "first_workgroup_only")


def model_side_yogi(cur, last, m, v, hparams, init, mistake=None):
    """(m, v, step, model) of len(cur) elements, float64: yogi.py:22-31 on the gradient cur - last
    (optimizers.py:53), the model np.array(last + step, float32) into an int64 entry (optimizers.py:58).
    ``hparams``: eta, tau, beta, omb (1 - beta), omb2 (1 - beta2) as Python floats.  ``last`` None: zeros."""
    eta, tau, beta, omb, omb2 = (F64(hparams[k]) for k in ("eta", "tau", "beta", "omb", "omb2"))
    cur = np.asarray(cur, F64)
    Q = len(cur)
    L = np.zeros(Q, F64) if last is None or mistake == "last_ignored" else np.asarray(last)[:Q].astype(F64)
    if init and mistake != "init_ignored":
        M, V = np.zeros(Q, F64), np.full(Q, tau, F64)
    else:
        M, V = np.asarray(m, F64)[:Q].copy(), np.asarray(v, F64)[:Q].copy()
    with np.errstate(all="ignore"):
        g = cur - L
        g2 = g * g
        M = beta * M + omb * g
        V = V - (omb2 * g2) * _sgn(V if mistake == "sign_of_v" else V - g2)
        den = np.sqrt(V) + tau
        lr = eta / den if mistake == "eta_div_den" else (F64(1.0) / den) * eta
        st = lr * M
        new = L + st
        model = _f64_to_i64(new) if mistake == "model_from_double" else _to_i64(new.astype(F32))
    if mistake == "first_workgroup_only":
        M[WG:], V[WG:], st[WG:], model[WG:] = np.nan, np.nan, np.nan, -1
    return M, V, st, model


# ------------------------------------------------------------------------------------------------------------------
# k_side_qfed_delta / k_side_qfed_sq / k_side_qfed_finalize
# ------------------------------------------------------------------------------------------------------------------
QFED_MISTAKES = ("stride_q", "float_diff", "mul_rcp", "sq_f64", "sqnorm_overwritten", "zero_plus",
                 "accumulate_ignored", "first_workgroup_only", "first_client_group_only")
QFED_FINALIZE_MISTAKES = ("hs0", "sub_f64", "first_workgroup_only")


def side_g(L, W, lr, mistake=None):
    """(L - W) * 1.0 / lr of optimizers.py:76 on int64 tensors: the wrapped int64 difference, converted to float32,
    times 1.0f, divided by lr rounded to float32."""
    lr = F32(lr)
    with np.errstate(all="ignore"):
        d = L.astype(F32) - W.astype(F32) if mistake == "float_diff" else (L - W).astype(F32)
        d = d * F32(1.0)
        return d * (F32(1.0) / lr) if mistake == "mul_rcp" else d / lr


def model_side_qfed(xi, ldq, K, Q, last, alpha, lr, delta_s, sqnorm, accumulate, mistake=None):
    """(delta_s, sqnorm): delta_s[q] (float32) is the chain of alpha[k] * g[k][q] over the clients, its first term
    taken as it is (optimizers.py:83-89); sqnorm[k] (float64) gains the sum over q, in order, of the float32
    squares g*g (optimizers.py:93-97)."""
    d_out, s_out = np.array(delta_s, copy=True), np.array(sqnorm, copy=True)
    assert d_out.dtype == F32 and s_out.dtype == F64
    if K == 0 or Q == 0:
        return d_out, s_out
    rows = _rows(xi, ldq, K, Q, Q if mistake == "stride_q" else ldq)
    L = np.asarray(last)[:Q]
    alpha = np.asarray(alpha, F32)
    if mistake == "accumulate_ignored":
        accumulate = False
    with np.errstate(all="ignore"):
        g = [side_g(L, rows[k], lr, mistake) for k in range(K)]
        d = d_out[:Q].copy() if accumulate else np.zeros(Q, F32)
        for k in range(K):
            t = alpha[k] * g[k]
            d = t if (k == 0 and not accumulate and mistake != "zero_plus") else d + t
        s = np.zeros(K, F64)
        G = np.stack(g)
        for q in range(Q):
            col = G[:, q]
            s = s + (col.astype(F64) * col.astype(F64) if mistake == "sq_f64" else (col * col).astype(F64))
    n = min(Q, WG) if mistake == "first_workgroup_only" else Q
    d_out[:n] = d[:n]
    kn = min(K, WG) if mistake == "first_client_group_only" else K
    with np.errstate(all="ignore"):
        s_out[:kn] = s[:kn] if mistake == "sqnorm_overwritten" else s_out[:kn] + s[:kn]
    return d_out, s_out


def model_side_qfed_finalize(last, delta_s, hs, mistake=None):
    """float32(last) - delta_s / hs[1] in float32 (optimizers.py:101-104), into an int64 entry."""
    L, d = np.asarray(last), np.asarray(delta_s, F32)[:len(last)]
    h = F32(hs[0 if mistake == "hs0" else 1])
    with np.errstate(all="ignore"):
        quo = d / h
        if mistake == "sub_f64":
            v = (L.astype(F64) - quo.astype(F64)).astype(F32)
        else:
            v = L.astype(F32) - quo
    out = _to_i64(v)
    if mistake == "first_workgroup_only":
        out[WG:] = -1
    return out


# ------------------------------------------------------------------------------------------------------------------
# k_yogi_step / k_qfed_finalize (float32, grid-stride float4)
# ------------------------------------------------------------------------------------------------------------------
FINISH_MISTAKES = ("tail_float4_skipped", "one_trip")
YOGI_STEP_MISTAKES = FINISH_MISTAKES + ("state_read_on_init",)


def stride_trip(P4: int) -> int:
    """float4 columns the first trip of a stride_grid() launch covers."""
    blocks = min(max((P4 + STRIDE_BLOCK - 1) // STRIDE_BLOCK, 1), STRIDE_MAX_BLOCKS)
    return blocks * STRIDE_BLOCK


def _written(P, mistake):
    """Elements [0:n) of the [0:P) a finisher writes under a planted mistake."""
    n = P
    if mistake == "tail_float4_skipped":
        n = P // 4 * 4
    if mistake == "one_trip":
        n = min(n, 4 * stride_trip((P + 3) // 4))
    return n


def yogi_elem_f32(cur, last, m, v, hp):
    """yogi_elem: yogi.py:22-31 + optimizers.py:52-58 in float32, every operation rounded; returns (m, v, new)."""
    f = F32
    with np.errstate(all="ignore"):
        g = cur - last
        g2 = g * g
        m = f(hp["beta"]) * m + f(hp["omb"]) * g
        v = v - (f(hp["omb2"]) * g2) * _sgn(v - g2)
        step = ((f(1) / (np.sqrt(v) + f(hp["tau"]))) * f(hp["eta"])) * m
        return m, v, last + step


def model_yogi_step(cur, last, m, v, out, P, hp, init, mistake=None):
    """(m, v, out) after fa_yogi_step over columns [0:P); the arrays come as allocated and prefilled."""
    m2, v2, o2 = (np.array(a, dtype=F32, copy=True) for a in (m, v, out))
    n = _written(P, mistake)
    if init and mistake != "state_read_on_init":
        M, V = np.zeros(n, F32), np.full(n, F32(hp["tau"]))
    else:
        M, V = m2[:n], v2[:n]
    m2[:n], v2[:n], o2[:n] = yogi_elem_f32(np.asarray(cur, F32)[:n], np.asarray(last, F32)[:n], M, V, hp)
    return m2, v2, o2


def model_qfed_finalize(last, delta, hs, out, P, mistake=None):
    """out[0:P) = last - delta / hs[1] in float32 (optimizers.py:101-104)."""
    o2 = np.array(out, dtype=F32, copy=True)
    n = _written(P, mistake)
    with np.errstate(all="ignore"):
        o2[:n] = np.asarray(last, F32)[:n] - np.asarray(delta, F32)[:n] / F32(hs[1])
    return o2
