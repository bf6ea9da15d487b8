"""fbl_select and fbl_reduce on the MI355X against the numpy restatement of tests/bulyan_fixtures.py, exactly."""
import numpy as np
import pytest
import torch

from tests import bulyan_fixtures as bf
from tests.deep_trim_fixtures import assert_same

pytestmark = pytest.mark.gpu


def _gram(K, kind, f):
    rng = np.random.default_rng(K)
    d = rng.integers(-4, 5, size=(K, 24)).astype(np.float64)
    if kind == "dup":  # zero distances and tied scores: ties go to the earlier arrival
        d[K // 2:] = d[:K - K // 2]
    nans = {"plain": 0, "dup": 0, "nan": 1, "nan_f1": f + 1, "nan_f2": f + 2}[kind]
    d[2:2 + nans, 5] = np.nan
    return d @ d.T


#: (1025, 255): the sort's padding crosses 1024; f + 2 NaN rows: the picks run out (f + 1 do not: include/fedbulyan.h)
@pytest.mark.parametrize("K, f, kind", [(3, 0, "plain"), (7, 1, "plain"), (11, 2, "plain"), (67, 16, "plain"),
                                        (1025, 255, "plain"), (11, 2, "dup"), (67, 16, "dup"), (7, 1, "nan"),
                                        (11, 2, "nan_f1"), (11, 2, "nan_f2"), (67, 16, "nan_f2")])
def test_select_equals_the_restatement(gpu_device, K, f, kind):
    from fedscale_amd import kernels_bulyan as kb
    from fedscale_amd import kernels_krum as kk

    G = _gram(K, kind, f)
    want_picks, want_sel, want_n, want_score0 = bf.select_of(G, f)
    theta = K - 2 * f - 2
    assert want_n == (0 if kind == "nan_f2" else theta) and (want_picks[want_n:] == -1).all()
    g = torch.from_numpy(G.reshape(-1)).to(gpu_device)
    picks = torch.full((theta + 2,), 77, dtype=torch.int32, device=gpu_device)
    sel = torch.full((theta + 2,), 77, dtype=torch.int32, device=gpu_device)
    n_sel = torch.full((1,), 77, dtype=torch.int32, device=gpu_device)
    kb.select(g, K, f, picks, sel, n_sel, kb.select_workspace(K, gpu_device))
    score = torch.zeros(K, dtype=torch.float64, device=gpu_device)
    c, n1 = torch.zeros(K, device=gpu_device), torch.zeros(1, dtype=torch.int32, device=gpu_device)
    kk.scores(g, K, f, score)
    kk.select(score, K, 1, c, n1)
    torch.cuda.synchronize()
    picks, sel = picks.cpu().numpy(), sel.cpu().numpy()
    assert (picks[theta:] == 77).all() and (sel[theta:] == 77).all()
    assert np.array_equal(picks[:theta], want_picks) and np.array_equal(sel[:theta], want_sel)
    assert int(n_sel.cpu()[0]) == want_n
    # iteration 0 is fk_scores and fk_select(m = 1)
    assert np.array_equal(score.cpu().numpy(), want_score0)
    assert np.flatnonzero(c.cpu().numpy()).tolist() == ([] if want_n == 0 else [int(want_picks[0])])
    if kind == "nan":
        assert 2 not in picks


def _reduce(x, K, P, sel, n_sel, theta, beta, last, *, counted, cus):
    from fedscale_amd import kernels_bulyan as kb

    out = torch.full((P + 3,), 7.0, dtype=torch.float32, device=x.device)
    mirror = torch.full((P + 3,), 7.0, dtype=torch.float32).pin_memory() if counted else None
    kept = torch.zeros(K, dtype=torch.int64, device=x.device) if counted else None
    kb.reduce_bulyan(x, K, P, sel, n_sel, theta, beta, last, out, mirror=mirror, kept=kept, cus=cus)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[P:] == 7.0).all() and (mirror is None or np.array_equal(mirror.numpy().view(np.uint32),
                                                                        got.view(np.uint32)))
    return got[:P], None if kept is None else kept.cpu().numpy()


#: both sides of every switch of lanes and rows per lane (80, 272, 1056) and of the tile width (315, 620, 1204, 2275)
@pytest.mark.parametrize("theta", [1, 2, 3, 80, 81, 272, 273, 315, 316, 620, 621, 1056, 1057, 1204, 1205, 2275, 2276,
                                   4094])
def test_reduce_equals_the_restatement(gpu_device, theta):
    from fedscale_amd import kernels_bulyan as kb

    W = kb.plan(1, theta, 1)["W"]
    K, Pmax = min(theta + 5, 4096), 4 * W + 3
    ld = (Pmax + 3) // 4 * 4 + 4
    rng = np.random.default_rng(theta)
    sel = np.sort(rng.permutation(K)[:theta]).astype(np.int32)
    x = bf.rows_of(rng, K, ld, Pmax, sel)
    xd, seld = torch.from_numpy(x).to(gpu_device), torch.from_numpy(sel).to(gpu_device)
    n_sel = torch.tensor([theta], dtype=torch.int32, device=gpu_device)
    last = torch.arange(ld, dtype=torch.float32, device=gpu_device)
    for P in sorted({1, W - 1, W, W + 1, Pmax}):  # Pmax: five tiles, no multiple of 4
        for beta in sorted({1, max(1, theta - 2), theta}):
            want, want_kept = bf.reduce_of(x[:, :P], sel, beta)
            got, kept = _reduce(xd, K, P, seld, n_sel, theta, beta, last, counted=True, cus=0)
            assert_same(got, want, (theta, beta, P))
            assert np.array_equal(kept, want_kept) and kept.sum() == beta * P
            # without counts and mirror, planned for one CU (at most 4 workgroups: one walks two tiles at Pmax)
            bare, _ = _reduce(xd, K, P, seld, n_sel, theta, beta, last, counted=False, cus=1)
            assert np.array_equal(bare.view(np.uint32), got.view(np.uint32)), (theta, beta, P)
    # a refused round leaves the model as it was
    n_sel.fill_(theta - 1)
    got, kept = _reduce(xd, K, Pmax, seld, n_sel, theta, theta, last, counted=True, cus=0)
    assert np.array_equal(got, np.arange(Pmax, dtype=np.float32)) and kept.sum() == 0
