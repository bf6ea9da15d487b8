"""fdt_reduce on the MI355X against the numpy restatement of tests/trim_fixtures.py, bit for bit: every tile class of
``kernels_deeptrim.plan``, K at and past each boundary where the tile width changes, t from 1 to the median's, widths
around one tile and over several, with and without the drop counts and the mirror, on two grids."""
import numpy as np
import pytest
import torch

from tests import deep_trim_fixtures as df
from tests import trim_fixtures as tf

pytestmark = pytest.mark.gpu

#: 3; 34..36 (36: the first K the register selection cannot take the median of); K at and one past every boundary where
#: C halves (174, 466, 1002, 1913) and where the 104 KiB instantiation starts (3280); 35 and 175 are no multiple of
#: the lanes per column; fdt_max_rows()
ROWS = (3, 34, 35, 36, 174, 175, 466, 467, 1002, 1003, 1913, 1914, 3280, 3281, 4096)
CASES = [(K, t) for K in ROWS for t in df.trims(K)]


def _launch(x, K, P, t, *, counted, cus):
    from fedscale_amd import kernels_deeptrim as kd

    out = torch.full((P + 3,), 7.0, dtype=torch.float32, device=x.device)
    mirror = torch.full((P + 3,), 7.0, dtype=torch.float32).pin_memory() if counted else None
    dropped = torch.zeros((K, 2), dtype=torch.int64, device=x.device) if counted else None
    kd.reduce_deep(x, K, P, t, out, mirror=mirror, dropped=dropped, cus=cus)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[P:] == 7.0).all() and (mirror is None or np.array_equal(mirror.numpy().view(np.uint32),
                                                                        got.view(np.uint32)))
    return got[:P], None if dropped is None else dropped.cpu().numpy()


@pytest.mark.parametrize("kind", ["tied", "normal"])
@pytest.mark.parametrize("K, t", CASES)
def test_reduce_equals_the_restatement(gpu_device, K, t, kind):
    from fedscale_amd import kernels_deeptrim as kd

    C = kd.plan(1, K, 1, t)["C"]
    Pmax = 3 * C + 5
    ld = (Pmax + 3) // 4 * 4 + 4
    x = df.rows_of(kind, np.random.default_rng(1000 * K + t), K, ld, Pmax, t)
    xd = torch.from_numpy(x).to(gpu_device)
    for P in df.widths(C):
        want, want_dropped = tf.trimmed_mean(x[:, :P], t)
        first = df.NAN_COLS if kind == "tied" else 0
        assert np.isfinite(want[first:]).all() and (kind != "tied" or np.isnan(want[:first]).all())
        got, dropped = _launch(xd, K, P, t, counted=True, cus=0)
        df.assert_same(got, want, (K, t, P))
        assert np.array_equal(dropped, want_dropped) and dropped.sum() == 2 * t * P
        # without the counts and the mirror, on a grid of one CU (two tiles per workgroup at the widest P): same bits
        assert kd.plan(1, K, P, t)["grid"] <= 2
        bare, _ = _launch(xd, K, P, t, counted=False, cus=1)
        assert np.array_equal(bare.view(np.uint32), got.view(np.uint32)), (K, t, P)


@pytest.mark.parametrize("kind", ["tied", "normal"])
@pytest.mark.parametrize("t", [1, 4, 16])
def test_same_function_as_the_register_selection(gpu_device, t, kind):
    """Where both run, fdt_reduce has the bits and the counts of ft_select + ft_reduce — on two grids."""
    from fedscale_amd import kernels_deeptrim as kd
    from fedscale_amd import kernels_trim as kt

    K, P, ld = 100, 3001, 3008
    x = torch.from_numpy(df.rows_of(kind, np.random.default_rng(t), K, ld, P, t)).to(gpu_device)
    thr = kt.thresholds(P, gpu_device)
    old, old_dropped = torch.zeros(P, device=gpu_device), torch.zeros((K, 2), dtype=torch.int64, device=gpu_device)
    kt.select(x, K, P, t, *thr)
    kt.reduce_trim(x, K, P, t, old, lo=thr[0], hi=thr[1], ties=thr[2], dropped=old_dropped)
    assert kd.plan(256, K, P, t)["grid"] != kd.plan(3, K, P, t)["grid"]
    for cus in (0, 3):
        new, new_dropped = _launch(x, K, P, t, counted=True, cus=cus)
        df.assert_same(new, old.cpu().numpy(), (t, kind, cus))
        assert np.array_equal(new_dropped, old_dropped.cpu().numpy())
