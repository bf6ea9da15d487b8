"""FedAdam, FedAdagrad and FedAvgM rounds end to end on the MI355X: ``TorchModelAdapter`` with
``TorchServerOptimizer("fed-adam" | "fed-adagrad" | "fed-avgm")`` against the numpy float32 restatement
(tests/serveropt_fixtures.py) applied to the oracle's mean (oracle/cpu_reference.py), bit for bit in the model, m_t and
v_t; the int64 entry as a round without an optimizer writes it; ``set_weights`` and the reference-typed list path; the
opt-in rounds the step composes with; a model sharded over two parts; pickling; and the caller-stream ordering."""
import argparse
import pickle

import numpy as np
import pytest
import torch

from tests import serveropt_fixtures as sf
from tests.golden_io import StateDictModule

pytestmark = pytest.mark.gpu

F32 = np.float32
K = 5
MODES = {"fed-adam": "adam", "fed-adagrad": "adagrad", "fed-avgm": "avgm"}
NAMES = ["a", "bn.num_batches_tracked", "b", "c"]
SHAPES = [(5,), (), (8, 8), (1000,)]
ARGS = dict(server_eta=0.02, server_tau=1e-3, server_beta=0.9, server_beta2=0.99)


def _init():
    rng = np.random.default_rng(1)
    return [torch.tensor(7, dtype=torch.int64) if s == () else
            torch.from_numpy((rng.standard_normal(s) * 0.1).astype(F32)) for s in SHAPES]


def _hp(mode):
    return sf.hparams(eta=ARGS["server_eta"], tau=ARGS["server_tau"], beta=ARGS["server_beta"],
                      beta2=ARGS["server_beta2"])


def _optimizer(mode, dev="cuda:0"):
    from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer

    return TorchServerOptimizer(mode, argparse.Namespace(gradient_policy=mode, **ARGS), dev)


def _adapter(mode, **kw):
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

    return TorchModelAdapter(StateDictModule(NAMES, _init()), device="cuda:0",
                             optimizer=None if mode is None else _optimizer(mode), **kw)


def _flat(values):
    return np.concatenate([np.asarray(v, dtype=F32).reshape(-1) for v in values
                           if np.asarray(v).dtype == F32])


def _uploads(rng, L, n=K):
    """n client states around the model ``L`` (list of arrays), deltas over several binades."""
    return [{name: (np.asarray(a + 3 + k, dtype=np.int64) if a.dtype == np.int64 else
                    (a + rng.standard_normal(a.shape) * 10.0 ** rng.uniform(-4, -1)).astype(F32))
             for name, a in zip(NAMES, L)} for k in range(n)]


def _oracle_mean(ups, weights=None):
    """(fp32 flat mean, the mean in the reference's list form) by oracle/cpu_reference.py."""
    from oracle.cpu_reference import fedavg_close, fedavg_flat, fedavg_step, fedbuff_flat

    x = np.stack([_flat(u.values()) for u in ups])
    if weights is not None:
        return fedbuff_flat(x, weights).astype(F32), None
    acc = []
    for i, u in enumerate(ups):
        acc = fedavg_step(acc, dict(u), i == 0)
    return fedavg_flat(x), fedavg_close(acc, len(ups))


def _same(got, want, what):
    assert sf.bits_equal(got, want), f"{what}: {sf.first_difference(got, want)}"


def _check_state(ctl, rule, m, v, ctx):
    P = m.size
    _same(ctl.m[:P].cpu().numpy(), m, ctx + ("m",))
    _same(_flat([t.cpu().numpy() for t in ctl.m_t if t is not None]), m, ctx + ("m_t",))
    assert [t is None for t in ctl.m_t] == [s == () for s in SHAPES]
    if rule == "avgm":
        assert ctl.v is None and ctl.v_t == []
    else:
        _same(ctl.v[:P].cpu().numpy(), v, ctx + ("v",))
        _same(_flat([t.cpu().numpy() for t in ctl.v_t if t is not None]), v, ctx + ("v_t",))


def _run_rounds(mode, adapter, plain=None, rounds=3, seed=5, hook=None, begin_kw=None):
    """``rounds`` plain FedAvg rounds under ``mode``, every one checked against the restatement; returns the history
    of (model bits, m, v).  ``plain``: an adapter without an optimizer that follows the same trajectory, for the int64
    entry.  ``hook(r, adapter)`` may swap the optimizer between rounds."""
    rule, hp = MODES[mode], _hp(mode)
    rng = np.random.default_rng(seed)
    m = v = None
    hist = []
    for r in range(rounds):
        L = [t.numpy() for t in adapter.get_weights()]
        ups = _uploads(rng, L)
        rnd = adapter.begin_round(K, "fedavg", **(begin_kw or {}))
        for u in ups:
            rnd.add(dict(u))
        adapter.apply_round(rnd, float(F32(K)), float(K))
        mean_f, mean_list = _oracle_mean(ups)
        m, v, out = sf.step(rule, mean_f, _flat(L), m, v, hp, r == 0)
        got = adapter.get_weights()
        ctx = (mode, "round", r)
        _same(_flat([t.numpy() for t in got]), out, ctx + ("model",))
        assert not sf.bits_equal(out, mean_f), ctx  # a server step, not the FedAvg mean
        ctl = adapter.optimizer.gradient_controller
        assert ctl.initialized
        _check_state(ctl, rule, m, v, ctx)
        # the mean survives the step
        rm = list(adapter.round_mean_weights())
        _same(_flat(rm), mean_f, ctx + ("round_mean_weights",))
        assert rm[1].dtype == np.float64 and rm[1] == mean_list[1]
        if plain is not None:  # the same uploads through a round without a server step: the int64 entry's value
            plain.set_weights([torch.from_numpy(np.array(a)) for a in L])
            prnd = plain.begin_round(K, "fedavg")
            for u in ups:
                prnd.add(dict(u))
            plain.apply_round(prnd, float(F32(K)), float(K))
            pw = plain.get_weights()
            assert got[1].dtype == torch.int64 and torch.equal(got[1], pw[1]), ctx
            _same(_flat([t.numpy() for t in pw]), mean_f, ctx + ("the plain round is the mean",))
        hist.append((out.copy(), m.copy(), None if v is None else v.copy(), int(got[1])))
        if hook is not None:
            hook(r, adapter)
    return hist


# ---- three rounds, every mode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_three_rounds_equal_the_restatement_on_the_oracles_mean(gpu_device, mode):
    _run_rounds(mode, _adapter(mode), plain=_adapter(None))


def test_fed_adam_differs_from_the_fedavg_mean_through_init_model(gpu_device):
    """``gradient_policy = "fed-adam"`` through DeviceAggregatorMixin.init_model: not the FedAvg mean (what an unknown
    mode silently gave), but the restatement."""
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator
    from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter
    from fedscale_amd.utils.optimizer.adaptive import FedAdam

    args = argparse.Namespace(gradient_policy="fed-adam", **ARGS)

    class Base:
        def init_model(self):
            self.model_wrapper = StateDictModule(NAMES, _init())
            self.model_wrapper.get_model = lambda m=self.model_wrapper: m

    class Agg(DeviceAggregator, Base):
        device = "cuda:0"

        def __init__(self):
            DeviceAggregator.__init__(self, None, args)
            self.init_model()

    agg = Agg()
    adapter = agg.model_wrapper
    assert type(adapter) is TorchModelAdapter and type(adapter.optimizer.gradient_controller) is FedAdam
    L = [t.numpy() for t in adapter.get_weights()]
    ups = _uploads(np.random.default_rng(9), L)
    agg.start_round(K)
    for k, u in enumerate(ups):
        agg.on_result({"client_id": k, "update_weight": dict(u), "moving_loss": 0.5})
    mean_f, _ = _oracle_mean(ups)
    _, _, out = sf.step("adam", mean_f, _flat(L), None, None, _hp("fed-adam"), True)
    got = _flat([t.numpy() for t in adapter.get_weights()])
    _same(got, out, "init_model fed-adam")
    assert not sf.bits_equal(got, mean_f)
    _same(_flat(list(agg.model_weights)), mean_f, "model_weights is the mean")


# ---- the other ways in ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_set_weights_and_the_list_path_give_the_rounds_bits(gpu_device, mode):
    rule, hp = MODES[mode], _hp(mode)
    by_round, by_set = _adapter(mode), _adapter(mode)
    module = StateDictModule(NAMES, _init())
    list_opt = _optimizer(mode)
    rng = np.random.default_rng(13)
    for r in range(3):
        L = [t.numpy() for t in by_round.get_weights()]
        ups = _uploads(rng, L)
        rnd = by_round.begin_round(K, "fedavg")
        for u in ups:
            rnd.add(dict(u))
        by_round.apply_round(rnd, float(F32(K)), float(K))
        want = by_round.get_weights()
        mean = list(by_round.round_mean_weights())  # fp32 entries float32, the int64 entry float64
        # set_weights(weights): the reference's aggregator hands the mean to the adapter
        by_set.set_weights([torch.from_numpy(np.array(a)) for a in mean])
        got = by_set.get_weights()
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.dtype == b.dtype and a.shape == b.shape
            if a.dtype == torch.int64:
                assert torch.equal(a, b), (mode, r, i)
            else:
                _same(a.numpy(), b.numpy(), (mode, "set_weights", r, i))
        # the reference-typed path: lists in, nn.Module loaded
        last = [torch.from_numpy(np.array(a)) for a in L]
        cur = [torch.from_numpy(np.array(a)) for a in mean]
        list_opt.update_round_gradient(last, cur, module)
        sd = module.state_dict()
        for i, (n, b) in enumerate(zip(NAMES, want)):
            if b.dtype == torch.int64:
                assert torch.equal(sd[n].cpu(), b), (mode, r, i)
            else:
                _same(sd[n].cpu().numpy(), b.numpy(), (mode, "list path", r, i))
        for ctl in (by_set.optimizer.gradient_controller, list_opt.gradient_controller):
            ref = by_round.optimizer.gradient_controller
            _same(ctl.m.cpu().numpy()[:ref.layout.P], ref.m.cpu().numpy()[:ref.layout.P], (mode, r, "m"))
            if rule != "avgm":
                _same(ctl.v.cpu().numpy()[:ref.layout.P], ref.v.cpu().numpy()[:ref.layout.P], (mode, r, "v"))
    del hp


@pytest.mark.parametrize("mode", list(MODES))
def test_update_returns_the_step_in_the_references_list_form(gpu_device, mode):
    from fedscale_amd.utils.optimizer.adaptive import MODES as CLASSES

    rule, hp = MODES[mode], _hp(mode)
    opt = CLASSES[mode](eta=ARGS["server_eta"], tau=ARGS["server_tau"], beta=ARGS["server_beta"],
                        beta2=ARGS["server_beta2"])
    assert opt.m_t == [] and not opt.initialized
    rng = np.random.default_rng(2)
    m = v = None
    for r in range(2):
        grads = [torch.from_numpy(rng.standard_normal(s).astype(F32)) if s != () else
                 torch.tensor(2.5, dtype=torch.float64) for s in SHAPES]
        steps = opt.update(grads)
        g = _flat([t.numpy() for t in grads])
        m, v, out = sf.step(rule, g, np.zeros_like(g), m, v, hp, r == 0)
        _same(_flat([t.numpy() for t in steps if t.dtype == torch.float32]), out, (mode, "update", r))
        assert steps[1].dtype == torch.float64 and float(steps[1]) == 2.5
        assert [tuple(t.shape) for t in steps] == SHAPES


# ---- composition ----------------------------------------------------------------------------------------------------------
def test_a_trim_zero_round_under_fed_adam_is_the_plain_fed_adam_round(gpu_device):
    from tests import trim_fixtures as tf

    trimmed, plain = _adapter("fed-adam"), _adapter("fed-adam")
    rng = np.random.default_rng(21)
    L = [t.numpy() for t in trimmed.get_weights()]
    ups = _uploads(rng, L)
    for ad, kw in ((trimmed, dict(trim=0)), (plain, {})):
        rnd = ad.begin_round(K, "fedavg", **kw)
        for u in ups:
            rnd.add(dict(u))
        ad.apply_round(rnd, float(F32(K)), float(K))
    x = np.stack([_flat(u.values()) for u in ups])
    mean = tf.trimmed_mean(x, 0)[0]
    _, _, out = sf.step("adam", mean, _flat(L), None, None, _hp("fed-adam"), True)
    got = trimmed.get_weights()
    _same(_flat([t.numpy() for t in got]), out, "trim=0 under fed-adam")
    for a, b in zip(got, plain.get_weights()):
        assert torch.equal(a, b)
    _same(_flat(list(trimmed.round_mean_weights())), mean, "the trimmed round's mean")


def test_an_mxfp8_round_under_fed_adagrad(gpu_device):
    from fedscale_amd.cloud.execution.quant_upload import compress_delta
    from tests import quant_fixtures as qf

    adapter = _adapter("fed-adagrad", upload_quant="mxfp8")
    L = [t.numpy() for t in adapter.get_weights()]
    ups = _uploads(np.random.default_rng(22), L)
    rnd = adapter.begin_round(K, "fedavg")
    for u in ups:
        rnd.add(compress_delta(u, L))
    adapter.apply_round(rnd, float(F32(K)), float(K))
    Lf = _flat(L)
    rows = [qf.quantize((_flat(u.values()) - Lf).astype(F32)) for u in ups]
    mean = qf.finish(Lf, qf.chain(rows, P=Lf.size), K)
    _, _, out = sf.step("adagrad", mean, Lf, None, None, _hp("fed-adagrad"), True)
    _same(_flat([t.numpy() for t in adapter.get_weights()]), out, "mxfp8 under fed-adagrad")


def test_a_fedbuff_round_under_fed_avgm(gpu_device):
    adapter = _adapter("fed-avgm")
    L = [t.numpy() for t in adapter.get_weights()]
    ups = _uploads(np.random.default_rng(23), L)
    s = [1 / (1 + k) ** 0.5 for k in (0, 2, 1, 0, 3)]
    rnd = adapter.begin_round(K, "fedbuff")
    for u, w in zip(ups, s):
        rnd.add(dict(u), weight=w)
    den = 0.0
    for w in s:
        den += w
    adapter.apply_round(rnd, float(F32(den)), float(den))
    mean, _ = _oracle_mean(ups, weights=s)  # async_aggregator.py:129-135 on the fp32 rows
    _, _, out = sf.step("avgm", mean, _flat(L), None, None, _hp("fed-avgm"), True)
    _same(_flat([t.numpy() for t in adapter.get_weights()]), out, "fedbuff under fed-avgm")


# ---- sharded --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at_once", (True, False), ids=("at-once", "per-part"))
def test_two_parts_on_one_card_equal_one_gpu(gpu_device, at_once):
    from fedscale_amd.cloud.internal.sharded_model_adapter import ShardedModelAdapter

    mode = "fed-adam"
    single = _adapter(mode)
    sharded = ShardedModelAdapter(StateDictModule(NAMES, _init()), optimizer=_optimizer(mode), devices=[0, 0],
                                  transport="copy")
    sharded.FINISH_PARTS_AT_ONCE = at_once
    rng = np.random.default_rng(31)
    for r in range(3):
        L = [t.numpy() for t in single.get_weights()]
        ups = _uploads(rng, L)
        for ad in (single, sharded):
            rnd = ad.begin_round(K, "fedavg")
            for u in ups:
                rnd.add(dict(u))
            ad.apply_round(rnd, float(F32(K)), float(K))
        for i, (a, b) in enumerate(zip(sharded.get_weights(), single.get_weights())):
            assert a.dtype == b.dtype and torch.equal(a, b), (at_once, r, i)
        ref = single.optimizer.gradient_controller
        ctls = [o.gradient_controller for o in sharded.shard_optimizers()]
        assert len(ctls) == 2 and all(c.initialized for c in ctls)
        for name in ("m", "v"):
            cat = np.concatenate([getattr(c, name)[:c.layout.P].cpu().numpy() for c in ctls])
            _same(cat, getattr(ref, name)[:ref.layout.P].cpu().numpy(), (at_once, r, name))


# ---- pickle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_a_pickled_optimizer_continues_with_the_same_bits(gpu_device, mode):
    def swap(r, adapter):
        if r == 1:
            ctl = adapter.optimizer.gradient_controller
            back = pickle.loads(pickle.dumps(ctl))
            assert type(back) is type(ctl) and back is not ctl and back.initialized
            assert back.m.data_ptr() != ctl.m.data_ptr()
            assert back.fp32_hparams() == ctl.fp32_hparams()
            ctl.m.fill_(float("nan"))  # the old state is not what round 3 reads
            adapter.optimizer.gradient_controller = back

    whole = _run_rounds(mode, _adapter(mode), seed=41)
    resumed = _run_rounds(mode, _adapter(mode), seed=41, hook=swap)
    for a, b in zip(whole, resumed):
        _same(a[0], b[0], (mode, "model"))
        _same(a[1], b[1], (mode, "m"))


# ---- caller-stream ordering -----------------------------------------------------------------------------------------------
def test_round_exposes_device_state_follows_the_controllers_attribute(gpu_device):
    for mode in list(MODES) + ["fed-yogi"]:
        args = argparse.Namespace(gradient_policy=mode, yogi_eta=3e-3, yogi_tau=1e-8, yogi_beta=0.9, yogi_beta2=0.99)
        from fedscale_amd.cloud.aggregation.optimizers import TorchServerOptimizer
        from fedscale_amd.cloud.internal.torch_model_adapter import TorchModelAdapter

        ad = TorchModelAdapter(StateDictModule(NAMES, _init()), device="cuda:0",
                               optimizer=TorchServerOptimizer(mode, args, "cuda:0"))
        assert ad.optimizer.gradient_controller.exposes_device_state is True
        assert ad._round_exposes_device_state() is True, mode
    assert _adapter(None)._round_exposes_device_state() is False
    for mode in (None, "fed-avg", "fed-prox", "q-fedavg"):
        args = argparse.Namespace(gradient_policy=mode, learning_rate=0.05, qfed_q=1.0)
        ad = TorchModelAdapter(StateDictModule(NAMES, _init()), device="cuda:0",
                               optimizer=TorchServerOptimizer(mode, args, "cuda:0"))
        assert ad._round_exposes_device_state() is False, mode

    class Controller:
        exposes_device_state = True

    class Stub:
        mode = "fed-something-new"
        gradient_controller = Controller()

        def update_round_gradient(self, *a, **k):
            pass

    ad = TorchModelAdapter(StateDictModule(NAMES, _init()), device="cuda:0", optimizer=Stub())
    assert ad._round_exposes_device_state() is True
    Controller.exposes_device_state = False
    assert ad._round_exposes_device_state() is False
