"""The int64 side-table kernels of fedscale_amd/csrc/fedagg.hip (k_side_accum, k_side_close, k_side_yogi,
k_side_qfed_delta / _sq / _finalize) against their numpy restatements (tests/side_kernel_models.py), bit for bit, on
the inputs of tests/side_fixtures.py: the seams of each kernel's thread axis, rows with ldq != Q and poisoned
padding, fp32 and fp64 ties, wrapping sums and differences, and the values an int64 entry cannot hold.  Every output
buffer is longer than Q and prefilled; the whole buffer is compared, so a write past Q shows.

tests/test_side_oracle.py shows on the CPU, mistake by mistake, what each test here can see.  The last test runs a
round through DeviceAggregator with a model of 70 int64 elements and compares them exactly."""
import numpy as np
import pytest
import torch

from tests import side_fixtures as sf
from tests import side_kernel_models as skm
from tests.side_kernel_models import F32, F64, I64, I64_MIN, same_bits

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, copy=True)).cuda()


def _host(t):
    return t.cpu().numpy()


def _accum_args(K, Q, ldq, mode):
    xi, w = sf.client_rows(K, Q, ldq, seed=K + Q), sf.fedbuff_weights(K)
    acc0 = np.full(ldq, sf.SENT_I64 if mode == 0 else sf.SENT_F64, I64 if mode == 0 else F64)
    return xi, w, acc0


def _accumulate(kx, xi, K, Q, mode, w, acc, accumulate=False):
    kx.side_accumulate(xi, K, Q, mode, w=w, acc_i=acc if mode == 0 else None, acc_d=acc if mode == 1 else None,
                       accumulate=accumulate)


@pytest.mark.parametrize("mode", [0, 1], ids=["int64_sum", "fedbuff_chain"])
@pytest.mark.parametrize("K,Q,ldq", sf.ACCUM_CASES)
def test_side_accumulate(gpu_device, K, Q, ldq, mode):
    """The wrapping int64 sum and the weighted fp64 chain (two operations per client, never fused)."""
    from fedscale_amd import kernels as kx

    xi, w, acc0 = _accum_args(K, Q, ldq, mode)
    want = skm.model_side_accum(xi, ldq, K, Q, mode, w, acc0, False)
    acc = _dev(acc0)
    _accumulate(kx, _dev(xi), K, Q, mode, _dev(w), acc)
    assert same_bits(_host(acc), want)


@pytest.mark.parametrize("mode", [0, 1], ids=["int64_sum", "fedbuff_chain"])
@pytest.mark.parametrize("K,Q,ldq", [c for c in sf.ACCUM_CASES if c[0] >= 2])
def test_side_accumulate_split_and_pinned(gpu_device, K, Q, ldq, mode):
    """One call over K rows equals two calls, [0:h] then [h:K] continuing the chain, at h = 1 and h = K - 1; and
    the same bits come out of rows read from pinned host memory."""
    from fedscale_amd import kernels as kx

    xi, w, acc0 = _accum_args(K, Q, ldq, mode)
    want = skm.model_side_accum(xi, ldq, K, Q, mode, w, acc0, False)
    x, wd = _dev(xi), _dev(w)
    for h in sf.splits(K):
        acc = _dev(acc0)
        _accumulate(kx, x[:h], h, Q, mode, wd[:h], acc)
        _accumulate(kx, x[h:], K - h, Q, mode, wd[h:], acc, accumulate=True)
        assert same_bits(_host(acc), want), h
    acc = _dev(acc0)
    _accumulate(kx, torch.from_numpy(xi.copy()).pin_memory(), K, Q, mode, wd, acc)
    torch.cuda.synchronize()
    assert same_bits(_host(acc), want)


@pytest.mark.parametrize("outputs", sf.CLOSE_OUTPUTS)
@pytest.mark.parametrize("Q,mode,denom", sf.CLOSE_CASES)
def test_side_close(gpu_device, Q, mode, denom, outputs):
    """acc / denom in fp64, and its float32 value into the int64 entry: truncated from the float32, INT64_MIN for
    NaN, +-inf and |v| >= 2^63 (0/0, +-x/0, +-2^63, 1e300)."""
    from fedscale_amd import kernels as kx

    acc_i, acc_d = sf.close_acc(Q)
    cur_w, model_w = skm.model_side_close(acc_i if mode == 0 else acc_d, Q, mode, denom)
    cur = _dev(np.full(Q + 7, sf.SENT_F64, F64)) if outputs != "model" else None
    model = _dev(np.full(Q + 7, sf.SENT_I64, I64)) if outputs != "cur" else None
    kx.side_close(Q, mode, denom, acc_i=_dev(acc_i), acc_d=_dev(acc_d), cur=cur, model=model)
    if cur is not None:
        assert same_bits(_host(cur)[:Q], cur_w) and np.all(_host(cur)[Q:] == sf.SENT_F64)
    if model is not None:
        assert np.array_equal(_host(model)[:Q], model_w) and np.all(_host(model)[Q:] == sf.SENT_I64)


@pytest.mark.parametrize("case", sf.YOGI_CASES, ids=lambda c: f"Q{c[0]}-last{int(c[1])}-init{int(c[2])}-tau{c[3]}-{c[4]}")
def test_side_yogi_three_rounds(gpu_device, case):
    """Three rounds of fp64 FedYoGi state: m, v, step and model bit for bit against numpy in every round, which
    holds the device's fp64 sqrt and reciprocal to correct rounding."""
    from fedscale_amd import kernels as kx

    Q, with_last, init, tau, outputs = case
    hp, d = sf.yogi_hparams(tau), sf.yogi_inputs(Q, with_last, init, seed=Q)
    m_w, v_w = d["m0"], d["v0"]
    m, v, last = _dev(d["m0"]), _dev(d["v0"]), _dev(d["last"])
    tail_m, tail_v = d["m0"][Q:], d["v0"][Q:]
    for r in range(sf.YOGI_ROUNDS):
        first = init and r == 0
        step = _dev(np.full(Q + 7, sf.SENT_F64, F64)) if outputs in ("both", "step") else None
        model = _dev(np.full(Q + 7, sf.SENT_I64, I64)) if outputs in ("both", "model") else None
        kx.side_yogi(_dev(d["curs"][r]), last, m, v, Q, step=step, model=model, init=first, **hp)
        m_w, v_w, step_w, model_w = skm.model_side_yogi(d["curs"][r], d["last"], m_w, v_w, hp, first)
        assert same_bits(_host(m)[:Q], m_w) and same_bits(_host(v)[:Q], v_w), r
        assert same_bits(_host(m)[Q:], tail_m) and same_bits(_host(v)[Q:], tail_v), r
        if step is not None:
            assert same_bits(_host(step)[:Q], step_w) and np.all(_host(step)[Q:] == sf.SENT_F64), r
        if model is not None:
            assert np.array_equal(_host(model)[:Q], model_w) and np.all(_host(model)[Q:] == sf.SENT_I64), r


@pytest.mark.parametrize("i", range(len(sf.QFED_CASES)), ids=lambda i: "K%d-Q%d-ldq%d" % sf.QFED_CASES[i])
def test_side_qfed_accumulate(gpu_device, i):
    """delta_s and sqnorm against the model: the wrapped int64 difference, IEEE division by lr, float32 squares
    summed in fp64 in element order and added to a non-zero sqnorm; then the same from two calls."""
    from fedscale_amd import kernels as kx

    K, Q, ldq = sf.QFED_CASES[i]
    d = sf.qfed_inputs(K, Q, ldq, i)
    ds0 = np.full(ldq, sf.SENT_F32, F32)
    sq0 = np.concatenate([d["sqnorm0"], np.full(3, sf.SENT_F64)])
    ds_w, sq_w = skm.model_side_qfed(d["xi"], ldq, K, Q, d["last"], d["alpha"], d["lr"], ds0, sq0, False)
    xi, last, alpha = _dev(d["xi"]), _dev(d["last"]), _dev(d["alpha"])
    for h in [None] + sf.splits(K):
        ds, sq = _dev(ds0), _dev(sq0)
        if h is None:
            kx.side_qfed_accumulate(xi, K, Q, last=last, alpha=alpha, lr=d["lr"], delta_s=ds, sqnorm=sq,
                                    accumulate=False)
        else:
            kx.side_qfed_accumulate(xi[:h], h, Q, last=last, alpha=alpha[:h], lr=d["lr"], delta_s=ds, sqnorm=sq[:h],
                                    accumulate=False)
            kx.side_qfed_accumulate(xi[h:], K - h, Q, last=last, alpha=alpha[h:], lr=d["lr"], delta_s=ds,
                                    sqnorm=sq[h:], accumulate=True)
        assert same_bits(_host(ds), ds_w), h
        assert same_bits(_host(sq), sq_w), h


@pytest.mark.parametrize("Q,kind", sf.FINALIZE_CASES)
def test_side_qfed_finalize(gpu_device, Q, kind):
    """float32(last) - delta_s / hs[1] into the int64 entry: quotients on both sides of integers, and NaN, +-inf
    and beyond-int64 quotients, which come out as INT64_MIN."""
    from fedscale_amd import kernels as kx

    d = sf.finalize_inputs(Q, kind)
    want = skm.model_side_qfed_finalize(d["last"][:Q], d["delta_s"], d["hs"])
    model = _dev(np.full(Q + 7, sf.SENT_I64, I64))
    kx.side_qfed_finalize(_dev(d["last"]), _dev(d["delta_s"]), _dev(d["hs"]), model, Q)
    assert np.array_equal(_host(model)[:Q], want) and np.all(_host(model)[Q:] == sf.SENT_I64)
    if kind != "near":
        assert np.any(want == I64_MIN)


@pytest.mark.parametrize("asynchronous", [False, True], ids=["fedavg", "fedbuff"])
def test_round_int64_entries_exact(gpu_device, asynchronous):
    """A round through DeviceAggregator / TorchModelAdapter against OracleAggregator with 70 int64 elements (two
    workgroups of the side kernels), negative and beyond 2^24: FedAvg (K = 3) and FedBuff, two rounds, every entry
    equal (no integer slack)."""
    import argparse

    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator, DeviceAsyncAggregator
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from oracle.cpu_reference import OracleAggregator, OracleModel, OracleModelAdapter
    from tests.golden_io import StateDictModule, assert_state_equal

    K = 3
    args = argparse.Namespace(gradient_policy=None, yogi_eta=3e-3, yogi_tau=1e-8, yogi_beta=0.9, yogi_beta2=0.99,
                              learning_rate=0.05, qfed_q=1.0)
    init = [torch.from_numpy(a.copy()) for a in sf.round_init()]
    assert sum(t.numel() for t in init if t.dtype == torch.int64) == 70
    dev = TorchModelAdapter(StateDictModule(sf.ROUND_NAMES, init), device="cuda:0")
    ref = OracleModelAdapter(OracleModel(sf.ROUND_NAMES, init))
    if asynchronous:
        agg, oagg = DeviceAsyncAggregator(dev, args), OracleAggregator(ref, args, asynchronous=True)
        for a in (agg, oagg):
            a.round = 7
            a.client_task_model_version = {k: 7 - 2 * k for k in range(K)}
    else:
        agg, oagg = DeviceAggregator(dev, args), OracleAggregator(ref, args)
    for r in range(2):
        agg.start_round(K)
        oagg.start_round(K)
        for k, upd in enumerate(sf.round_uploads(K, r)):
            res = {"client_id": k, "update_weight": upd, "moving_loss": 1.0}
            oagg.on_result({**res, "update_weight": [u.copy() for u in upd]})
            agg.on_result(res)
        want = [w.numpy() for w in ref.get_weights()]
        assert_state_equal(dev.get_weights(), want, f"async={asynchronous} round {r}")
        assert np.abs(want[1]).max() > 2 ** 24 and want[1].min() < 0
