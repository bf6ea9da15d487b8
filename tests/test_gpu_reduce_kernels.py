"""k_reduce on the MI355X against the numpy model of tests/reduce_fixtures.py: every compiled instantiation (7 tile forms
x chain / mean / FedYoGi x weighted or not), every column, bit for bit — no sampling, no tolerance.  The shapes are the
smallest the launch plan routes to each form at the device's CU count (reduce_fixtures.shapes; tests/
test_reduce_plan.py asserts the plan each is listed for, and that each mistake the model can plant is seen by a case
run here).

Rows have ld = cols(P) + 8 with NaN in columns [P, ld).  Every per-column buffer (out, the mean or mirror, m, v, the
accumulator) is cols(P) + 4 floats long and prefilled.  Columns [0, P) are compared with the model; [P, cols(P))
belong to the last float4, which the ABI lets a kernel write, and are not; the 4 floats past cols(P) must come back
as they were.  A NaN must meet a NaN, its payload is left open.  Each case first holds the restated plan to the
library's own launch count and to the form the case is listed for.

Rows of more than 256 MB (the (8,4) forms, which need K x sw >= 1000, and the (16,2) FULL window, which needs K >= 200:
0.7 to 5 GB) are tiled on the device from a host block of [K, 65,537] columns, and so is their reference; 65,537 is
prime, so no tile, strip or lane stride is a multiple of the period.  Cases that read the same rows run next to each
other and the rows are freed after them."""
import pytest
import torch

from tests import reduce_fixtures as rf

pytestmark = pytest.mark.gpu

_ROWS = {}  # the rows of one key at a time: key -> (host inputs, rows on the device, weights on the device)
_IDS = [c["id"] for c in sorted(rf.cases(256), key=lambda c: c["rows"])]  # (the ids do not depend on the CU count)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rows(case, dev):
    key = case["rows"]
    if key not in _ROWS:
        _ROWS.clear()
        torch.cuda.empty_cache()
        inp = rf.case_inputs(case)
        K, P, B = case["Krows"], case["P"], inp["B"]
        if B == P:
            xd = torch.from_numpy(rf.expand_rows(inp["rows"], P)).to(dev)
        else:  # tile the block along each row, a few rows at a time
            blk = torch.from_numpy(inp["rows"]).to(dev)
            idx = torch.arange(P, device=dev) % B
            xd = torch.full((K, rf.cols(P) + 8), float("nan"), device=dev)
            for k in range(0, K, 16):
                xd[k:k + 16, :P] = blk[k:k + 16][:, idx]
            del blk, idx
        _ROWS[key] = (inp, xd, torch.from_numpy(inp["a"]).to(dev))
    return _ROWS[key]


def _same(got, want, P, what):
    """got (device) against want (host) as the module docstring says."""
    w = torch.from_numpy(want).to(got.device)
    assert got.shape == w.shape, what
    g, e = got[:P], w[:P]
    ok = (g.view(torch.int32) == e.view(torch.int32)) | (torch.isnan(g) & torch.isnan(e))
    if not bool(ok.all()):
        bad = torch.nonzero(~ok).flatten()
        at = bad[:5].cpu().numpy()
        raise AssertionError((what, int(bad.numel()), at, g[bad[:5]].cpu().numpy(), want[at]))
    n = rf.cols(P)
    assert torch.equal(got[n:].view(torch.int32), w[n:].view(torch.int32)), (what, "written past the last float4")


def _launch(kx, call, case, xd, ad, dev_bufs, denom):
    K, P = call["k1"] - call["k0"], case["P"]
    xs = xd[call["k0"]:call["k1"]] if K else None
    a = ad[call["k0"]:call["k1"]] if case["weighted"] and K else None
    src = None if call["src"] is None else dev_bufs[call["src"]]
    dst = dev_bufs[call["dst"]]
    if call["epi"] == "chain":
        kx.reduce(xs, K, P, dst, a=a, acc_in=src)
    elif call["epi"] == "mean" and call["mean"]:
        kx.reduce_mirror(xs, K, P, dst, dev_bufs["mean"], a=a, acc_in=src, denom=float(denom))
    elif call["epi"] == "mean":
        kx.reduce(xs, K, P, dst, a=a, acc_in=src, denom=float(denom), finalize=True)
    else:
        kx.reduce_yogi(xs, K, P, last=dev_bufs["last"], m=dev_bufs["m"], v=dev_bufs["v"], out=dst, denom=float(denom),
                       init=call["init"], a=a, acc_in=src, mean_out=dev_bufs["mean"] if call["mean"] else None,
                       **rf.HP)


def _check_plan(kx, case, cus):
    P, w = case["P"], case["weighted"]
    widest = 0
    for call in case["calls"]:
        K = call["k1"] - call["k0"]
        widest = max(widest, K)
        launches = rf.plan(cus, K, P, w)
        rf.check_cover(launches, P)
        if K:  # (fa_reduce_launches answers 0 for K = 0, which is planned like K = 1)
            assert len(launches) == kx.reduce_launches(K, P, w), (case["id"], K)
        else:
            assert len(launches) == kx.reduce_launches(1, P, w), (case["id"], K)
    assert rf.plan_is(cus, widest, P, case["form"]), (case["id"], rf.plan(cus, widest, P, w))


def _run_case(kx, case, dev, xd=None):
    """The case's calls on the device and on the model, and the comparison of every buffer."""
    inp, rows_d, ad = _rows(case, dev)
    xd = rows_d if xd is None else xd
    P = case["P"]
    denom = rf.case_denom(case, inp)
    blk = rf.block_buffers(inp)
    want = rf.run_model(case, inp["rows"], blk, inp["a"], denom, lambda K: None)  # column-wise: on the block
    bufs = {k: torch.from_numpy(v).to(dev) for k, v in rf.expand_buffers(blk, P).items()}
    for call in case["calls"]:
        _launch(kx, call, case, xd, ad, bufs, denom)
    torch.cuda.synchronize()
    for k, v in want.items():
        _same(bufs[k], rf.expand_vec(v, P, rf.PAD[k]), P, (case["id"], k))


@pytest.mark.parametrize("cid", _IDS)
def test_reduce_case(gpu_device, cid):
    """One case of reduce_fixtures.cases(): every tile form x epilogue x weighting; every residue of K against U from
    row 0 and from an accumulator; every exit of the short form's two-buffer pipeline and its small widths; chunk
    folds in place and out of place over a run-time-width tile, a FULL tile and both window seams; a finalize of the
    accumulator alone; two FedYoGi rounds with and without mean_out."""
    from fedscale_amd import kernels as kx

    cus = _cus()
    case = next(c for c in rf.cases(cus) if c["id"] == cid)
    _check_plan(kx, case, cus)
    _run_case(kx, case, gpu_device)


def test_reduce_reads_pinned_host_rows(gpu_device):
    """fa_reduce(host_ok=True) on a run-time-width shape: the same kernel reads the rows over PCIe."""
    from fedscale_amd import kernels as kx

    cus = _cus()
    case = next(c for c in rf.cases(cus) if c["id"] == "v16_sw-mean-u")
    case = dict(case, calls=[dict(case["calls"][0], mean=False)])  # fa_reduce, no mirror
    _check_plan(kx, case, cus)
    inp, _, _ = _rows(case, gpu_device)
    xh = torch.from_numpy(rf.expand_rows(inp["rows"], case["P"])).pin_memory()
    real = kx.reduce

    class HostOk:  # kernels with reduce() defaulting to host_ok=True
        reduce = staticmethod(lambda *a, **kw: real(*a, host_ok=True, **kw))

    _run_case(HostOk, case, gpu_device, xd=xh)
    _ROWS.clear()
