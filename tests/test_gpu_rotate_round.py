"""End to end on the MI355X: rounds over an adapter with ``upload_sign="sign1", upload_rotate="rht4096"`` against the
numpy restatement of the rotated round (tests/rotate_fixtures.py: rotate, sign encode with the residual in rotated
space, chain over P' columns in arrival order, unrotate, L + chain / K), bit for bit — K = 5 on a model with an int64
counter and P = 2 * 4096 + 777 float32 columns, two rounds with error feedback, host and device uploads, a staging
capacity of 2 (the chain crosses chunks), fed-yogi, the mixin attribute, and the refused uploads."""
import argparse
import copy

import numpy as np
import pytest
import torch

from tests import rotate_fixtures as rf
from tests.golden_io import DEFAULT_ARGS, StateDictModule, assert_state_close, assert_state_equal

pytestmark = pytest.mark.gpu

K = 5
SEED = 0x5EED0F7E57C0DE
SHAPES = [("emb.weight", (2, 4096)), ("bn.num_batches_tracked", None), ("fc.weight", (37, 20)), ("fc.bias", (37,))]
P = 2 * 4096 + 777
F32 = np.float32


def _model():
    rng = np.random.default_rng(7)
    names, tensors = [], []
    for name, shape in SHAPES:
        names.append(name)
        if shape is None:
            tensors.append(torch.tensor(11, dtype=torch.int64))
        else:
            tensors.append(torch.from_numpy(np.asarray(rng.standard_normal(shape) * 0.05, dtype=F32)))
    return names, tensors


def _args(policy):
    a = dict(DEFAULT_ARGS)
    a["gradient_policy"] = policy
    return argparse.Namespace(**a)


def _flat(values):
    return np.concatenate([np.asarray(v, dtype=F32).reshape(-1) for v in values if np.asarray(v).dtype == F32])


def _client_states(rng, names, L, n=K):
    """n trained states around the round's model: one embedding row touched, the other not — the update the rotation
    is for — and dense deltas of mixed magnitude elsewhere."""
    out = []
    for k in range(n):
        st = {}
        for name, a in zip(names, L):
            if a.dtype == np.int64:
                st[name] = np.asarray(a + 5 + k, dtype=np.int64)
            elif name == "emb.weight":
                d = np.zeros(a.shape, dtype=F32)
                d[k % 2, rng.integers(0, 4096, 40)] = rng.standard_normal(40).astype(F32)
                st[name] = np.asarray(a + d, dtype=F32)
            else:
                st[name] = np.asarray(a + rng.standard_normal(a.shape) * 10.0 ** rng.uniform(-4, 0), dtype=F32)
        out.append(st)
    return out


def _want_round(L, states, residuals, seed=SEED):
    Lf = _flat(L)
    enc = [rf.encode(_flat(st.values()), Lf, seed, r) for st, r in zip(states, residuals)]
    rows = [(b, s) for b, s, _ in enc]
    return rf.round_model(Lf, rows, seed), rows, [r for _, _, r in enc]


def _mean_with(L, states, new_f):
    from oracle.cpu_reference import fedavg_close, fedavg_step

    acc = []
    for i, st in enumerate(states):
        acc = fedavg_step(acc, dict(st), i == 0)
    mean = fedavg_close(acc, len(states))
    o = 0
    for i, a in enumerate(L):
        if a.dtype == F32:
            mean[i] = new_f[o:o + a.size].reshape(a.shape)
            o += a.size
    return mean


def _run(policy, capacity, via_mixin_attr, dev="cuda:0", rounds=2):
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator
    from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
    from fedscale_amd.cloud.execution.rotate_upload import ROTATE_KEY, compress_sign_rotated
    from fedscale_amd.cloud.execution.sign_upload import BITS_KEY, SCALES_KEY
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.rotate_round import RotatedSignRound, RotatedSignStaging
    from oracle.cpu_reference import OracleModel, OracleModelAdapter, OracleServerOptimizer

    names, init = _model()
    args = _args(policy)
    if via_mixin_attr:
        class Base:
            def init_model(self):
                self.model_wrapper = StateDictModule(names, init)
                self.model_wrapper.get_model = lambda m=self.model_wrapper: m

        class Agg(DeviceAggregator, Base):
            device_upload_sign = "sign1"
            device_upload_rotate = "rht4096"
            device_round_capacity = capacity
            device = dev

            def __init__(self):
                DeviceAggregator.__init__(self, None, args)
                self.init_model()

        agg = Agg()
        adapter = agg.model_wrapper
        assert type(adapter) is TorchModelAdapter
    else:
        adapter = TorchModelAdapter(StateDictModule(names, init), device=dev,
                                    optimizer=TorchServerOptimizer(policy, args, dev), staging_capacity=capacity,
                                    upload_sign="sign1", upload_rotate="rht4096")
        agg = DeviceAggregator(adapter, args)
    assert adapter.upload_sign == "sign1" and adapter.upload_rotate == "rht4096" and adapter.layout.P == P
    ref = OracleModelAdapter(OracleModel(names, init), OracleServerOptimizer(policy, args))
    rng = np.random.default_rng(3)
    history = []
    residuals = [None] * K  # every executor's rotated-space error-feedback state, kept between rounds
    tdev = torch.device(dev)
    for rnd in range(rounds):
        L = [t.numpy() for t in adapter.get_weights()]
        states = _client_states(rng, names, L)
        new_f, rows, want_res = _want_round(L, states, residuals)
        agg.start_round(K)
        for k, st in enumerate(states):
            if k % 2:  # a state on the GPU: frt_rotate + fsg_sign_row, the residual a device tensor
                r_in = None if residuals[k] is None else torch.from_numpy(residuals[k]).to(tdev)
                up, r = compress_sign_rotated({n: torch.from_numpy(v).to(tdev) for n, v in st.items()},
                                              [torch.from_numpy(a).to(tdev) for a in L], SEED, residual=r_in,
                                              residual_out=True)
                residuals[k] = r.cpu().numpy()
            else:
                up, residuals[k] = compress_sign_rotated(st, L, SEED, residual=residuals[k], residual_out=True)
            assert np.array_equal(up[BITS_KEY], rows[k][0]), (rnd, k)
            assert np.array_equal(up[SCALES_KEY].view(np.uint32), rows[k][1].view(np.uint32)), (rnd, k)
            assert np.array_equal(residuals[k].view(np.uint32), want_res[k].view(np.uint32)), (rnd, k)
            if k == 2:
                up = list(up.values())
            elif k == 3:
                up = {n: torch.from_numpy(np.array(a)).to(tdev) for n, a in up.items()}
            else:
                assert list(up)[-3:] == [BITS_KEY, SCALES_KEY, ROTATE_KEY]
            agg.on_result({"client_id": k, "update_weight": up, "moving_loss": 0.5})
            if k == 0:
                r = agg._device_round
                assert type(r) is RotatedSignRound and type(adapter.staging) is RotatedSignStaging
                assert r.cap == min(capacity, K) and r.seed == SEED and r.upload_sign == "sign1"
                assert r.chain.numel() == rf.padded(P)
            if k == 3:
                assert agg._device_round.chunks_done == (1 if capacity < K else 0)
        ref.set_weights(copy.deepcopy(_mean_with(L, states, new_f)), client_training_results=[])
        got, want = adapter.get_weights(), [t.numpy() for t in ref.get_weights()]
        ctx = f"{policy} capacity {capacity} round {rnd}"
        if policy is None:
            assert_state_equal(got, want, ctx)
        else:
            assert_state_close(got, want, 1e-6, ctx)
            y, oy = adapter.optimizer.gradient_controller, ref.optimizer.gradient_controller
            for i, a in enumerate(L):
                if a.dtype == F32:
                    assert torch.equal(y.m_t[i].cpu(), oy.m_t[i]) and torch.equal(y.v_t[i].cpu(), oy.v_t[i]), (ctx, i)
        history.append([t.clone() for t in got])
        ref.model.load_state_dict({n: t for n, t in zip(names, got)})  # same trajectory
    Pp = rf.padded(P)
    assert adapter.staging.bits.shape == (min(capacity, K), Pp // 8)
    assert adapter.staging.scales.shape == (min(capacity, K), Pp // 256)
    return history


def test_fedavg_rounds_are_the_restatement_and_a_fold_changes_no_bit(gpu_device):
    folded, whole = _run(None, 2, False), _run(None, K, False)
    for a, b in zip(folded, whole):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_fed_yogi_rounds(gpu_device):
    _run("fed-yogi", 2, False)


def test_rounds_through_the_mixins_device_upload_rotate(gpu_device):
    a, b = _run(None, 2, True), _run(None, 2, False)
    for x, y in zip(a, b):
        assert all(torch.equal(p, q) for p, q in zip(x, y))


def test_refused_uploads_leave_the_round_usable(gpu_device):
    from fedscale_amd.cloud.execution.rotate_upload import ROTATE_KEY, compress_sign_rotated
    from fedscale_amd.cloud.execution.sign_upload import compress_sign
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    names, init = _model()
    adapter = TorchModelAdapter(StateDictModule(names, init), device="cuda:0", upload_sign="sign1",
                                upload_rotate="rht4096")
    L = [t.numpy() for t in adapter.get_weights()]
    states = _client_states(np.random.default_rng(5), names, L, 3)
    rnd = adapter.begin_round(3, "fedavg")
    plain, _ = compress_sign(states[0], L)
    with pytest.raises(ValueError, match=ROTATE_KEY + ".*not set yet"):  # a plain sign upload, first
        rnd.add(plain)
    assert rnd.n == 0 and rnd.seed is None
    ups = [compress_sign_rotated(st, L, SEED)[0] for st in states]
    rnd.add(ups[0])
    other, _ = compress_sign_rotated(states[1], L, SEED + 1)
    with pytest.raises(ValueError, match=f"seed {SEED + 1:#x}.*seed {SEED:#x}"):
        rnd.add(other)
    with pytest.raises(ValueError, match=f"{ROTATE_KEY}.*{SEED:#x}"):
        rnd.add({k: v for k, v in ups[1].items() if k != ROTATE_KEY})
    with pytest.raises(ValueError, match=ROTATE_KEY):
        rnd.add(plain)
    with pytest.raises(ValueError, match=ROTATE_KEY):
        rnd.add(list(plain.values()))
    assert rnd.n == 1 and rnd.slot == 1 and rnd.seed == SEED
    rnd.add(ups[1])
    rnd.add(ups[2])
    adapter.apply_round(rnd, float(np.float32(3)), 3.0)
    want, _, _ = _want_round(L, states, [None] * 3)
    got = _flat([t.numpy() for t in adapter.get_weights()])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a rotated upload on a plain sign1 adapter
    plain_adapter = TorchModelAdapter(StateDictModule(names, init), device="cuda:0", upload_sign="sign1")
    prnd = plain_adapter.begin_round(2, "fedavg")
    with pytest.raises((TypeError, ValueError)):
        prnd.add(ups[0])
    assert prnd.n == 0
    prnd.add(plain)
    assert prnd.n == 1


def test_a_nan_poisons_exactly_its_4096_column_block(gpu_device):
    from fedscale_amd.cloud.execution.rotate_upload import compress_sign_rotated
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    names, init = _model()
    adapter = TorchModelAdapter(StateDictModule(names, init), device="cuda:0", upload_sign="sign1",
                                upload_rotate="rht4096")
    L = [t.numpy() for t in adapter.get_weights()]
    states = _client_states(np.random.default_rng(6), names, L, 3)
    states[1]["emb.weight"][1, 300] = np.nan  # column 4096 + 300: block 1
    rnd = adapter.begin_round(3, "fedavg")
    for st in states:
        rnd.add(compress_sign_rotated(st, L, SEED)[0])
    adapter.apply_round(rnd, float(np.float32(3)), 3.0)
    got = _flat([t.numpy() for t in adapter.get_weights()])
    want, _, _ = _want_round(L, states, [None] * 3)
    nan = np.zeros(P, dtype=bool)
    nan[4096:8192] = True
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def test_upload_rotate_unset_is_the_adapter_built_without_the_keyword(gpu_device):
    from fedscale_amd.cloud.execution.sign_upload import compress_sign
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.sign_round import SignRound, SignStaging

    names, init = _model()
    outs = []
    for kw in ({}, {"upload_rotate": None}):
        adapter = TorchModelAdapter(StateDictModule(names, init), device="cuda:0", upload_sign="sign1", **kw)
        assert adapter.upload_rotate is None and "upload_rotate" not in adapter.__dict__
        L = [t.numpy() for t in adapter.get_weights()]
        states = _client_states(np.random.default_rng(8), names, L, 3)
        rnd = adapter.begin_round(3, "fedavg")
        assert type(rnd) is SignRound and type(adapter.staging) is SignStaging
        for st in states:
            rnd.add(compress_sign(st, L)[0])
        adapter.apply_round(rnd, float(np.float32(3)), 3.0)
        outs.append([t.clone() for t in adapter.get_weights()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
