"""fs_topk_row on the MI355X against the numpy restatement of the selection rule (tests/sparse_fixtures.py) and
against the host path of ``compress_topk``: the same bytes, under ties of every kind, with and without a base, with
and without a residual in and out, from a poisoned workspace."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import sparse_fixtures as sf

pytestmark = pytest.mark.gpu

WIDTHS = (1, 31, 4097, 70001)
_CASES = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ks(P):
    return sorted({k for k in (1, 2, -(-P // 100), P - 1, P) if 1 <= k <= P})


def _inputs(P):
    """name -> (x, base, r_in): all magnitudes equal, four distinct magnitudes, NaN / inf / zeros, and random values,
    made once per width."""
    if P in _CASES:
        return _CASES[P]
    rng = np.random.default_rng(P)
    sign = rng.choice(np.asarray([1.0, -1.0], dtype=np.float32), P)
    c = OrderedDict()
    c["all_equal"] = ((sign * np.float32(0.5)).astype(np.float32), None, None)
    c["four_magnitudes"] = ((sign * rng.choice(np.asarray([0.25, 1.0, 3.0, 1e-41], np.float32), P)).astype(np.float32),
                            None, None)
    c["nan_inf_zero"] = (rng.choice(sf.TIE_VALUES, P).astype(np.float32), np.zeros(P, dtype=np.float32), None)
    x = rng.standard_normal(P).astype(np.float32)
    base = (x + rng.standard_normal(P).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
    r_in = (rng.standard_normal(P) * 1e-3 * (rng.random(P) < 0.5)).astype(np.float32)
    c["random_with_base"] = (x, base, None)
    c["random_with_base_and_residual"] = (x, base, r_in)
    c["ties_with_residual"] = (c["four_magnitudes"][0], None, np.where(rng.random(P) < 0.3, np.float32(0.75),
                                                                       np.float32(0.0)).astype(np.float32))
    _CASES[P] = c
    return c


@pytest.mark.parametrize("P", WIDTHS)
def test_device_selection_equals_the_restatement(gpu_device, P):
    from fedscale_amd import kernels_sparse as ks

    dev = gpu_device
    nws = ks.topk_workspace(P)
    for name, (x, base, r_in) in _inputs(P).items():
        e = sf.delta(x, base, r_in)
        dx = torch.from_numpy(x).to(dev)
        db = None if base is None else torch.from_numpy(base).to(dev)
        dr = None if r_in is None else torch.from_numpy(r_in).to(dev)
        for k in _ks(P):
            idx, val, r_out = sf.select(e, k)
            for want_r in (False, True):
                ws = torch.full((nws + 16,), 0xA5, dtype=torch.uint8, device=dev)  # poisoned beforehand
                io = torch.full((k + 8,), -7, dtype=torch.int32, device=dev)
                vo = torch.full((k + 8,), 7.0, dtype=torch.float32, device=dev)
                ro = torch.full((P + 8,), 7.0, dtype=torch.float32, device=dev) if want_r else None
                assert ks.topk_row(dx, db, dr, P, k, ws, io, vo, ro) == k
                gi, gv = io.cpu().numpy(), vo.cpu().numpy()
                ctx = (P, name, k, want_r)
                assert np.array_equal(gi[:k].view(np.uint32), idx), ctx
                assert np.array_equal(_bits(gv[:k]), _bits(val)), ctx
                assert (gi[k:] == -7).all() and (gv[k:] == 7.0).all(), ctx  # nothing past the k pairs
                assert (ws[nws:] == 0xA5).all().item(), ctx
                if want_r:
                    gr = ro.cpu().numpy()
                    assert np.array_equal(_bits(gr[:P]), _bits(r_out)) and (gr[P:] == 7.0).all(), ctx
    # k > P keeps every column; the residual out may be the residual in
    x, base, r_in = _inputs(P)["random_with_base_and_residual"]
    e = sf.delta(x, base, r_in)
    io = torch.zeros(P + 3, dtype=torch.int32, device=dev)
    vo = torch.zeros(P + 3, dtype=torch.float32, device=dev)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    args = (torch.from_numpy(x).to(dev), torch.from_numpy(base).to(dev))
    assert ks.topk_row(*args, torch.from_numpy(r_in).to(dev), P, P + 5, ws, io, vo) == P
    assert np.array_equal(io.cpu().numpy()[:P], np.arange(P)) and np.array_equal(_bits(vo.cpu().numpy()[:P]), _bits(e))
    k = _ks(P)[len(_ks(P)) // 2]
    r = torch.from_numpy(r_in).to(dev)
    ks.topk_row(*args, r, P, k, ws, io, vo, r)
    idx, val, r_out = sf.select(e, k)
    assert np.array_equal(io.cpu().numpy()[:k].view(np.uint32), idx)
    assert np.array_equal(_bits(r.cpu().numpy()), _bits(r_out))


def test_device_and_host_paths_of_compress_topk_agree(gpu_device):
    from fedscale_amd.cloud.execution.sparse_upload import IDX_KEY, VAL_KEY, compress_topk

    dev = gpu_device
    torch.manual_seed(4)
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(),
                              torch.nn.Linear(4 * 26 * 26, 10))
    base = OrderedDict((k, v.clone()) for k, v in net.state_dict().items())
    sd = OrderedDict((k, v + 0.01 * torch.randn_like(v) if v.dtype == torch.float32 else v + 5)
                     for k, v in base.items())
    sd["3.bias"][2] = float("nan")  # the NaN is kept first
    P = sum(v.numel() for v in sd.values() if v.dtype == torch.float32)
    res = (torch.randn(P) * 0.01).numpy()
    on = OrderedDict((k, v.to(dev)) for k, v in sd.items())
    for kw_h, kw_d in ((dict(), dict()), (dict(residual=res), dict(residual=torch.from_numpy(res).to(dev))),
                       (dict(residual_out=True), dict(residual_out=True))):
        host, rh = compress_topk(sd, list(base.values()), density=0.01, **kw_h)
        got, rd = compress_topk(on, list(base.values()), density=0.01, **kw_d)
        assert list(host) == list(got) and list(host)[-2:] == [IDX_KEY, VAL_KEY]
        for k in host:
            assert host[k].dtype == got[k].dtype and host[k].shape == got[k].shape, k
            assert host[k].tobytes() == got[k].tobytes(), k
        assert (rh is None) == (rd is None)
        if rh is not None:
            assert isinstance(rd, torch.Tensor) and rd.device == dev
            assert np.array_equal(_bits(rh), _bits(rd.cpu().numpy()))
        assert np.isnan(host[VAL_KEY]).sum() == 1
