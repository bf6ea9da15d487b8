"""CPU checks of the host restatements of the int64 side-table kernels and the elementwise finishers
(tests/side_kernel_models.py), and of what the device tests can see.

First half: with no mistake planted a restatement equals the reference semantics, i.e. the very numpy and torch
expressions oracle/cpu_reference.py runs.  Second half: one mistake at a time is planted in a restatement and, on
the inputs the device tests use (tests/side_fixtures.py), the restatement with the mistake must differ from the
expected result in at least one case of the device test named in the docstring; that test would go red."""
import numpy as np
import pytest
import torch

from oracle.cpu_reference import OracleYoGi, fedavg_close, fedavg_step, fedbuff_close, fedbuff_step
from tests import side_fixtures as sf
from tests import side_kernel_models as skm
from tests.side_kernel_models import F32, F64, I64, I64_MIN, same_bits


def _torch_to_i64(f32):
    """np.asarray(x, float32) followed by load_state_dict's copy_ into an int64 tensor (torch_model_adapter.py:28-33,
    OracleModel.load_state_dict)."""
    dst = torch.zeros(len(f32), dtype=torch.int64)
    dst.copy_(torch.from_numpy(np.asarray(f32, dtype=np.float32)))
    return dst.numpy()


# ------------------------------------------------------------------------------------------------------------------
# the restatements against the reference's own expressions
# ------------------------------------------------------------------------------------------------------------------
def test_to_i64_is_the_reference_cast_on_every_class():
    """Truncation toward zero; NaN, +-inf and every |v| >= 2^63 become INT64_MIN in numpy's astype, torch's
    .to(int64) and copy_ into an int64 tensor alike."""
    big = np.nextafter(F32(2.0 ** 63), F32(0))  # the largest float32 below 2^63
    f = np.array([0.0, -0.0, 0.99999994, -0.99999994, 1.5, -1.5, 2.5, -2.5, 16777216.0, 33554436.0, -1e10, big, -big,
                  2.0 ** 63, -2.0 ** 63, 2.0 ** 64, -2.0 ** 64, 3e38, -3e38, np.inf, -np.inf, np.nan, 1e-45, -1e-45],
                 dtype=F32)
    got = skm._to_i64(f)
    assert np.array_equal(got, _torch_to_i64(f))
    assert np.array_equal(got, torch.from_numpy(f).to(torch.int64).numpy())
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got, f.astype(I64))
    assert np.all(got[13:22] == I64_MIN) and got[11] == int(big) and got[12] == -int(big)
    assert list(got[:8]) == [0, 0, 0, 0, 1, -1, 2, -2]


def _reference_accum_close(xi, K, Q, mode, w, denom):
    ups = [[xi[k, :Q].copy()] for k in range(K)]
    acc = None
    for k, u in enumerate(ups):
        acc = fedavg_step(acc, u, k == 0) if mode == 0 else fedbuff_step(acc, u, float(w[k]), k == 0)
    with np.errstate(all="ignore"):
        closed = (fedavg_close(acc, denom) if mode == 0 else fedbuff_close(acc, denom))[0]
    return acc[0], closed, _torch_to_i64(np.asarray(closed, dtype=np.float32))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("K,Q,ldq", sf.ACCUM_CASES)
def test_sums_and_close_follow_the_reference(K, Q, ldq, mode):
    """fedavg_step / fedavg_close (mode 0) and fedbuff_step / fedbuff_close (mode 1) on int64 arrays, then
    set_weights' float32 array copied into the int64 entry."""
    xi, w = sf.client_rows(K, Q, ldq, seed=K + Q), sf.fedbuff_weights(K)
    denom = K if mode == 0 else float(sum(w))
    acc_ref, cur_ref, model_ref = _reference_accum_close(xi, K, Q, mode, w, denom)
    acc0 = np.full(ldq, sf.SENT_I64 if mode == 0 else sf.SENT_F64, I64 if mode == 0 else F64)
    acc = skm.model_side_accum(xi, ldq, K, Q, mode, w, acc0, False)
    assert same_bits(acc[:Q], acc_ref) and same_bits(acc[Q:], acc0[Q:])
    cur, model = skm.model_side_close(acc, Q, mode, denom)
    assert same_bits(cur, cur_ref) and np.array_equal(model, model_ref)


@pytest.mark.parametrize("Q,mode,denom", sf.CLOSE_CASES)
def test_close_follows_the_reference_on_the_device_tests_inputs(Q, mode, denom):
    acc_i, acc_d = sf.close_acc(Q)
    a = (acc_i if mode == 0 else acc_d)[:Q]
    with np.errstate(all="ignore"):
        cur_ref = np.divide(a, denom)
        model_ref = _torch_to_i64(np.asarray(cur_ref, dtype=np.float32))
    cur, model = skm.model_side_close(acc_i if mode == 0 else acc_d, Q, mode, denom)
    assert same_bits(cur, cur_ref) and np.array_equal(model, model_ref)
    if denom == 0.0 or mode == 1:
        assert np.any(model == I64_MIN)  # the non-representable classes are there


@pytest.mark.parametrize("i", range(len(sf.QFED_CASES)))
def test_side_g_follows_the_reference(i):
    """optimizers.py:76 on int64 tensors: ((L - W) * 1.0 / lr) is float32, the difference wraps, lr is rounded to
    float32."""
    K, Q, ldq = sf.QFED_CASES[i]
    d = sf.qfed_inputs(K, Q, ldq, i)
    L = torch.from_numpy(d["last"][:Q].copy())
    for k in range(K):
        W = torch.from_numpy(d["xi"][k, :Q].copy())
        ref = ((L - W) * 1.0 / d["lr"])
        assert ref.dtype == torch.float32
        assert same_bits(skm.side_g(d["last"][:Q], d["xi"][k, :Q], d["lr"]), ref.numpy())


@pytest.mark.parametrize("Q,with_last,init,tau,outputs", [c for c in sf.YOGI_CASES if c[2]])
def test_yogi_state_follows_the_reference_in_float64(Q, with_last, init, tau, outputs):
    """OracleYoGi on a float64 gradient: m_t and v_t bit for bit over three rounds.  The step is not compared:
    torch's float64 sqrt on the CPU is not correctly rounded (tests/test_numerics_notes.py); it agrees to 3 ulp."""
    hp, d = sf.yogi_hparams(tau), sf.yogi_inputs(Q, with_last, init, seed=Q)
    ref = OracleYoGi(eta=hp["eta"], tau=tau, beta=0.9, beta2=0.99)
    L = d["last"][:Q].astype(F64) if with_last else np.zeros(Q, F64)
    m, v = d["m0"], d["v0"]
    for r in range(sf.YOGI_ROUNDS):
        step_ref = ref.update([torch.from_numpy(d["curs"][r] - L)])[0].numpy()
        m, v, step, _ = skm.model_side_yogi(d["curs"][r], d["last"], m, v, hp, init and r == 0)
        assert same_bits(m, ref.m_t[0].numpy()) and same_bits(v, ref.v_t[0].numpy())
        ulp = np.abs(skm.bits(step).astype(np.int64) - skm.bits(step_ref).astype(np.int64))
        assert ulp.max() <= 3


@pytest.mark.parametrize("Q,kind", sf.FINALIZE_CASES)
def test_side_finalize_follows_the_reference(Q, kind):
    """optimizers.py:101-104 on an int64 entry: last - delta / (hs + 1e-10) promotes to float32; load_state_dict
    truncates."""
    d = sf.finalize_inputs(Q, kind)
    L = torch.from_numpy(d["last"][:Q].copy())
    ref = L - torch.from_numpy(d["delta_s"][:Q].copy()) / torch.tensor(d["hs"][1])
    assert ref.dtype == torch.float32
    dst = torch.zeros(Q, dtype=torch.int64)
    dst.copy_(ref)
    got = skm.model_side_qfed_finalize(d["last"][:Q], d["delta_s"], d["hs"])
    assert np.array_equal(got, dst.numpy())
    if kind != "near":
        assert np.any(got == I64_MIN)


# ------------------------------------------------------------------------------------------------------------------
# what the device tests run, restated once (tests/test_gpu_side_kernels.py follows the same steps on the device)
# ------------------------------------------------------------------------------------------------------------------
def accum_flow(K, Q, ldq, mode, split=None, mistake=None):
    xi, w = sf.client_rows(K, Q, ldq, seed=K + Q), sf.fedbuff_weights(K)
    acc = np.full(ldq, sf.SENT_I64 if mode == 0 else sf.SENT_F64, I64 if mode == 0 else F64)
    if split is None:
        return skm.model_side_accum(xi, ldq, K, Q, mode, w, acc, False, mistake)
    acc = skm.model_side_accum(xi[:split], ldq, split, Q, mode, w[:split], acc, False, mistake)
    return skm.model_side_accum(xi[split:], ldq, K - split, Q, mode, w[split:], acc, True, mistake)


def qfed_flow(i, split=None, mistake=None):
    K, Q, ldq = sf.QFED_CASES[i]
    d = sf.qfed_inputs(K, Q, ldq, i)
    ds, sq = np.full(ldq, sf.SENT_F32, F32), d["sqnorm0"].copy()
    args = (d["last"], d["alpha"], d["lr"])
    if split is None:
        return skm.model_side_qfed(d["xi"], ldq, K, Q, *args, ds, sq, False, mistake)
    ds, sq1 = skm.model_side_qfed(d["xi"][:split], ldq, split, Q, d["last"], d["alpha"][:split], d["lr"], ds,
                                  sq[:split], False, mistake)
    ds, sq2 = skm.model_side_qfed(d["xi"][split:], ldq, K - split, Q, d["last"], d["alpha"][split:], d["lr"], ds,
                                  sq[split:], True, mistake)
    return ds, np.concatenate([sq1, sq2])


def yogi_flow(case, mistake=None):
    Q, with_last, init, tau, outputs = case
    hp, d = sf.yogi_hparams(tau), sf.yogi_inputs(Q, with_last, init, seed=Q)
    m, v, out = d["m0"], d["v0"], []
    for r in range(sf.YOGI_ROUNDS):
        m, v, step, model = skm.model_side_yogi(d["curs"][r], d["last"], m, v, hp, init and r == 0, mistake)
        out.append((m, v, step if outputs in ("both", "step") else None,
                    model if outputs in ("both", "model") else None))
    return out


def _differs(a, b):
    if isinstance(a, (tuple, list)):
        return any(_differs(x, y) for x, y in zip(a, b))
    if a is None:
        return False
    return not same_bits(a, b)


def _seen(flows):
    """flows: [(expected, mistaken)] over the cases of one device test."""
    return [i for i, (want, got) in enumerate(flows) if _differs(want, got)]


# ------------------------------------------------------------------------------------------------------------------
# planted mistakes
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mistake", [(0, m) for m in skm.ACCUM0_MISTAKES] + [(1, m) for m in skm.ACCUM1_MISTAKES])
def test_accumulate_mistakes_are_seen(mode, mistake):
    """Seen by test_gpu_side_kernels.py::test_side_accumulate (single calls) or, for the accumulate flag,
    ::test_side_accumulate_split_and_pinned."""
    single = [(accum_flow(*c, mode), accum_flow(*c, mode, mistake=mistake)) for c in sf.ACCUM_CASES]
    split = [(accum_flow(*c, mode, split=h), accum_flow(*c, mode, split=h, mistake=mistake))
             for c in sf.ACCUM_CASES for h in sf.splits(c[0])]
    if mistake == "accumulate_ignored":
        assert not _seen(single) and _seen(split)
    else:
        assert _seen(single), mistake


def test_split_sums_equal_whole_sums():
    for mode in (0, 1):
        for c in sf.ACCUM_CASES:
            for h in sf.splits(c[0]):
                assert same_bits(accum_flow(*c, mode), accum_flow(*c, mode, split=h))
    for i, c in enumerate(sf.QFED_CASES):
        for h in sf.splits(c[0]):
            assert not _differs(qfed_flow(i), qfed_flow(i, split=h))


def test_fused_multiply_add_would_show_in_a_tenth_of_the_sums():
    """The FedBuff chain at K = 5: a contracted s + w*x differs from the two-operation form in more than a tenth of
    the elements (36 % was measured on |x| < 2^40), so no lucky draw hides it."""
    c = next(c for c in sf.ACCUM_CASES if c[0] == 5)
    want, got = accum_flow(*c, 1), accum_flow(*c, 1, mistake="fused")
    assert np.mean(skm.bits(want[:c[1]]) != skm.bits(got[:c[1]])) > 0.10


@pytest.mark.parametrize("mistake", skm.CLOSE1_MISTAKES)
def test_close_mistakes_are_seen(mistake):
    """Seen by test_gpu_side_kernels.py::test_side_close."""
    flows = []
    for Q, mode, denom in sf.CLOSE_CASES:
        acc_i, acc_d = sf.close_acc(Q)
        acc = acc_i if mode == 0 else acc_d
        flows.append((skm.model_side_close(acc, Q, mode, denom, acc_i=acc_i),
                      skm.model_side_close(acc, Q, mode, denom, mistake, acc_i=acc_i)))
    assert _seen(flows), mistake
    if mistake in ("trunc_double", "round_nearest"):  # a cast mistake leaves cur alone and shows in the model
        assert all(same_bits(w[0], g[0]) for w, g in flows)


@pytest.mark.parametrize("mistake", skm.YOGI_MISTAKES)
def test_yogi_mistakes_are_seen(mistake):
    """Seen by test_gpu_side_kernels.py::test_side_yogi_three_rounds."""
    flows = [(yogi_flow(c), yogi_flow(c, mistake)) for c in sf.YOGI_CASES]
    assert _seen(flows), mistake


def test_yogi_inputs_take_every_branch_of_the_sign():
    for c in sf.YOGI_CASES:
        Q, with_last, init, tau, _ = c
        if Q < 63:
            continue
        d = sf.yogi_inputs(Q, with_last, init, seed=Q)
        L = d["last"][:Q].astype(F64) if with_last else np.zeros(Q, F64)
        g = d["curs"][0] - L
        v = np.full(Q, tau) if init else d["v0"][:Q]
        s = np.sign(v - g * g)
        assert (s > 0).any() and (s < 0).any()
        if not init:
            assert (s == 0).sum() >= Q // 8


@pytest.mark.parametrize("mistake", skm.QFED_MISTAKES)
def test_qfed_side_mistakes_are_seen(mistake):
    """Seen by test_gpu_side_kernels.py::test_side_qfed_accumulate (the accumulate flag: by its split calls)."""
    n = range(len(sf.QFED_CASES))
    single = [(qfed_flow(i), qfed_flow(i, mistake=mistake)) for i in n]
    split = [(qfed_flow(i, split=h), qfed_flow(i, split=h, mistake=mistake))
             for i in n for h in sf.splits(sf.QFED_CASES[i][0])]
    if mistake == "accumulate_ignored":
        assert _seen(split)
    elif mistake == "zero_plus":  # visible only through -0: the case with alpha = 0 and negative differences
        assert _seen(single) == [2]
    else:
        assert _seen(single), mistake


@pytest.mark.parametrize("mistake", skm.QFED_FINALIZE_MISTAKES)
def test_side_finalize_mistakes_are_seen(mistake):
    """Seen by test_gpu_side_kernels.py::test_side_qfed_finalize."""
    flows = []
    for Q, kind in sf.FINALIZE_CASES:
        d = sf.finalize_inputs(Q, kind)
        flows.append((skm.model_side_qfed_finalize(d["last"][:Q], d["delta_s"], d["hs"]),
                      skm.model_side_qfed_finalize(d["last"][:Q], d["delta_s"], d["hs"], mistake)))
    assert _seen(flows), mistake


@pytest.mark.parametrize("mistake", skm.YOGI_STEP_MISTAKES)
def test_finisher_mistakes_are_seen(mistake):
    """Seen by test_gpu_finish_kernels.py::test_yogi_step_at_the_seams and ::test_qfed_finalize_at_the_seams: the
    tail float4 at a ragged P, the second trip at the P past the seam, the state read on init at any P (the
    device test prefills m and v with NaN on init, as here)."""
    Ps = (5, 1025) if mistake != "one_trip" else sf.FINISH_SEAM_P[1:]  # the first of the pair fills one trip exactly
    for P in Ps:
        cur, last, m0, v0 = sf.yogi_step_inputs(P, seed=P)
        m0, v0 = np.full_like(m0, np.nan), np.full_like(v0, np.nan)
        out0 = np.full(len(cur), sf.SENT_F32, F32)
        want = skm.model_yogi_step(cur, last, m0, v0, out0, P, sf.FINISH_HP, True)
        got = skm.model_yogi_step(cur, last, m0, v0, out0, P, sf.FINISH_HP, True, mistake)
        assert _differs(want, got), (mistake, P)
        if mistake in skm.FINISH_MISTAKES:
            lq, dq = sf.qfed_finalize_inputs(P, seed=P)
            assert _differs(skm.model_qfed_finalize(lq, dq, sf.FINISH_HS, out0, P),
                            skm.model_qfed_finalize(lq, dq, sf.FINISH_HS, out0, P, mistake)), (mistake, P)


def test_finisher_seams_are_where_the_library_has_them():
    """stride_grid(): 256 threads, at most 8192 workgroups, one float4 per thread and trip; fa_yogi_step's
    non-temporal variant above 256 MiB of traffic at 7 float4 streams of 16 bytes per column group."""
    assert sf.STRIDE_SEAM == 4 * 256 * 8192 == 8388608
    assert skm.stride_trip(sf.STRIDE_SEAM // 4) == sf.STRIDE_SEAM // 4
    assert skm.stride_trip((sf.STRIDE_SEAM + 5 + 3) // 4) < (sf.STRIDE_SEAM + 5 + 3) // 4
    lo, hi = sf.NT_SEAM
    assert (lo + 3) // 4 * 16 * 7 <= 256 * 2 ** 20 < (hi + 3) // 4 * 16 * 7 and hi == lo + 1 == 9586981
