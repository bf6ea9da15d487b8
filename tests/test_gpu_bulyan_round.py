"""Bulyan rounds end to end on the MI355X against tests/bulyan_fixtures.py, bit for bit, on a small model."""
import argparse

import numpy as np
import pytest
import torch

from tests import bulyan_fixtures as bf
from tests import serveropt_fixtures as sf
from tests.golden_io import DEFAULT_ARGS
from tests.test_gpu_trim_round import _assert_model, _Case, _Net, _run

pytestmark = pytest.mark.gpu

K, F = 15, 2  # theta = 9, beta = 5


class _IntNet(_Net):
    """The same model with every fp32 entry a small integer, so that integer uploads give an exact Gram matrix."""

    def __init__(self):
        super().__init__()
        with torch.no_grad():
            for v in self.state_dict().values():
                if v.dtype == torch.float32:
                    v.copy_(torch.round(v * 8))


def _case(kind):
    if kind == "random":  # one upload scaled by 1e15, one carrying NaNs
        return _Case(K)
    case = _Case(K, poisoned=False, net=_IntNet)
    case.uploads = [[u if u.dtype == np.int64 else np.round(u * 8).astype(np.float32) for u in up]
                    for up in case.uploads]
    case.x = np.stack([case.flat(u) for u in case.uploads])
    return case


def _want(case, rnd, G):
    picks, sel, n_sel, _ = bf.select_of(G, F)
    assert n_sel == rnd.theta == 9 and rnd.beta == 5
    return picks, bf.reduce_of(case.x, sel, rnd.beta)


@pytest.mark.parametrize("kind", ["integer", "random"])
def test_round_through_begin_round(gpu_device, kind):
    from fedscale_amd.bulyan_round import BulyanRound, BulyanSpec

    case = _case(kind)
    adapter = case.adapter()
    L = case.flat([v.numpy() for v in case.init])
    rnd = _run(case, adapter, bulyan=F)
    assert type(rnd) is BulyanRound and rnd.bulyan == BulyanSpec(F)
    G = rnd.gram()  # the device's own matrix: everything after it is defined bit for bit
    if kind == "integer":
        d = (case.x - L).astype(np.float64)
        assert np.array_equal(G, d @ d.T)
    picks, (want, want_kept) = _want(case, rnd, G)
    assert np.array_equal(rnd.selected(), picks) and rnd.n_selected == rnd.theta and np.isfinite(want).all()
    _assert_model(case, adapter.get_weights(), want, kind)
    assert np.array_equal(rnd.kept(), want_kept) and rnd.kept().sum() == rnd.beta * case.P


def test_colluders_and_a_hidden_coordinate_stay_inside_the_honest_range(gpu_device):
    """f identical uploads shifted by +3 and an otherwise honest one carrying 1e30 in one coordinate: in range."""
    case = _Case(K, poisoned=False)
    for a in case.uploads[9]:
        if a.dtype == np.float32:
            a += np.float32(3.0)
    case.uploads[10] = [a.copy() for a in case.uploads[9]]  # the colluders: zero mutual distance
    case.uploads[4][0].reshape(-1)[7] = np.float32(1e30)
    case.x = np.stack([case.flat(u) for u in case.uploads])
    honest = np.delete(case.x, [4, 9, 10], axis=0)
    adapter = case.adapter()
    rnd = _run(case, adapter, bulyan=F)
    got = case.flat_of_weights(adapter.get_weights())
    assert (got >= honest.min(axis=0)).all() and (got <= honest.max(axis=0)).all()
    assert not {9, 10} & set(rnd.selected().tolist()) and rnd.n_selected == rnd.theta


def test_fed_adam_on_the_bulyan_mean(gpu_device):
    """The mean feeds the existing server step: the new model is the restated step on the restated mean."""
    adam = dict(server_eta=0.02, server_tau=1e-3, server_beta=0.9, server_beta2=0.99)
    case = _case("integer")
    adapter = case.adapter(policy="fed-adam", args=argparse.Namespace(**{**DEFAULT_ARGS, "gradient_policy": "fed-adam",
                                                                         **adam}))
    rnd = _run(case, adapter, bulyan=F)
    _, (mean, _) = _want(case, rnd, rnd.gram())
    hp = sf.hparams(eta=adam["server_eta"], tau=adam["server_tau"], beta=adam["server_beta"],
                    beta2=adam["server_beta2"])
    L = case.flat([v.numpy() for v in case.init])
    _, _, want = sf.step("adam", mean, L, None, None, hp, True)
    got = case.flat_of_weights(adapter.get_weights())
    assert sf.bits_equal(got, want), sf.first_difference(got, want)
    assert not sf.bits_equal(got, mean)


def test_round_through_the_mixin_and_the_capacity_refusal(gpu_device):
    from fedscale_amd.bulyan_round import BulyanRound
    from fedscale_amd.cloud.aggregation.aggregator import DeviceAggregator

    case = _case("integer")
    adapter = case.adapter()
    with pytest.raises(ValueError, match="all K=15 uploads resident.*capacity is 4"):
        adapter.begin_round(K, "fedavg", capacity=4, bulyan=F)
    assert adapter.staging is None  # refused before anything was allocated or launched

    class BulyanAggregator(DeviceAggregator):
        device_bulyan = F

    agg = BulyanAggregator(adapter)  # the same adapter still runs a round that fits
    agg.start_round(case.K)
    rnd = None
    for k in range(case.K):
        agg.on_result({"client_id": k + 1, "update_weight": case.upload(k, "dict" if k % 2 else "list"),
                       "moving_loss": 1.0})
        rnd = rnd or agg._device_round
    assert type(rnd) is BulyanRound and agg._device_round is None
    picks, (want, want_kept) = _want(case, rnd, rnd.gram())
    _assert_model(case, adapter.get_weights(), want, "mixin")
    assert np.array_equal(rnd.selected(), picks) and np.array_equal(rnd.kept(), want_kept)
