"""The two elementwise finishers, fa_yogi_step and fa_qfed_finalize (k_yogi_step, k_qfed_finalize: grid-stride
float4 loops), against their numpy restatements on every column, at the sizes where such a loop goes wrong: ragged
P, the P that fills one trip of the grid (stride_grid(): 8192 workgroups x 256 threads x one float4) and a ragged
P past it, and for fa_yogi_step the two P on either side of its switch to non-temporal loads and stores.

Buffers are cols(P) + 4 floats long.  Columns [P:cols(P)) belong to the last float4: the ABI lets a kernel read and
write them (cols_bytes() in fedagg.hip is the extent of every per-column operand), so the inputs there are NaN, to
show that no column below P depends on them, and the outputs there are not compared.  The 4 floats past cols(P)
must come back as they were."""
import numpy as np
import pytest
import torch

from tests import side_fixtures as sf
from tests import side_kernel_models as skm
from tests.side_kernel_models import F32, same_bits

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def _check(got, want, P, what):
    g = got.cpu().numpy()
    assert same_bits(g[:P], want[:P]), what
    assert same_bits(g[sf.cols(P):], want[sf.cols(P):]), f"{what}: written past the last float4"


def _yogi_rounds(kx, cur, last, m0, v0, P):
    """Round 1 with init (m and v prefilled NaN), round 2 continuing its state on another mean; then one step from
    the given state (m0, v0: the band of special values)."""
    n = len(cur)
    nan, sent = np.full(n, np.nan, F32), np.full(n, sf.SENT_F32, F32)
    nan[sf.cols(P):] = sf.SENT_F32
    cur2 = cur.copy()
    cur2[:P] = cur[:P] + F32(0.004)
    m, v, out = _dev(nan), _dev(nan), _dev(sent)
    m_w, v_w, o_w = nan, nan, sent
    dl = _dev(last)
    for r, c in enumerate((cur, cur2)):
        kx.yogi_step(_dev(c), dl, m, v, out, P, init=(r == 0), **sf.FINISH_HP)
        m_w, v_w, o_w = skm.model_yogi_step(c, last, m_w, v_w, o_w, P, sf.FINISH_HP, r == 0)
        for got, want, name in ((m, m_w, "m"), (v, v_w, "v"), (out, o_w, "out")):
            _check(got, want, P, f"P={P} round {r} {name}")
    m, v, out = _dev(m0), _dev(v0), _dev(sent)
    kx.yogi_step(_dev(cur), dl, m, v, out, P, init=False, **sf.FINISH_HP)
    want = skm.model_yogi_step(cur, last, m0, v0, sent, P, sf.FINISH_HP, False)
    for got, w, name in zip((m, v, out), want, ("m", "v", "out")):
        _check(got, w, P, f"P={P} from a given state, {name}")
    return m, v, out


@pytest.mark.parametrize("P", sf.FINISH_SMALL_P + sf.FINISH_SEAM_P)
def test_yogi_step_at_the_seams(gpu_device, P):
    from fedscale_amd import kernels as kx

    _yogi_rounds(kx, *sf.yogi_step_inputs(P, seed=P), P)


def test_yogi_step_on_either_side_of_the_non_temporal_switch(gpu_device):
    """P4 * 16 * 7 > FA_YOGI_NT_MIN_BYTES (256 MiB) selects the non-temporal kernel: the largest P of the plain one
    and the next P (9,586,980 and 9,586,981 columns, 38 MB a buffer), each against the model, and the two against
    each other on their common columns."""
    from fedscale_amd import kernels as kx

    lo, hi = sf.NT_SEAM
    assert (lo + 3) // 4 * 16 * 7 <= sf.FA_YOGI_NT_MIN_BYTES < (hi + 3) // 4 * 16 * 7
    full = sf.yogi_step_inputs(hi, seed=3)
    got_hi = _yogi_rounds(kx, *full, hi)
    n = sf.cols(lo) + 4
    part = [a[:n].copy() for a in full]
    for a, fill in zip(part, (np.nan, np.nan, sf.SENT_F32, sf.SENT_F32)):
        a[lo:] = fill
    got_lo = _yogi_rounds(kx, *part, lo)
    for a, b in zip(got_lo, got_hi):
        assert torch.equal(a[:lo].view(torch.int32), b[:lo].view(torch.int32))


@pytest.mark.parametrize("P", sf.FINISH_SMALL_P + sf.FINISH_SEAM_P)
def test_qfed_finalize_at_the_seams(gpu_device, P):
    """last - delta / hs[1] with IEEE division, hs[1] = 0.7f (inexact quotients), on every column."""
    from fedscale_amd import kernels as kx

    last, delta = sf.qfed_finalize_inputs(P, seed=P)
    sent = np.full(len(last), sf.SENT_F32, F32)
    out = _dev(sent)
    kx.qfed_finalize(_dev(last), _dev(delta), _dev(sf.FINISH_HS), out, P)
    _check(out, skm.model_qfed_finalize(last, delta, sf.FINISH_HS, sent, P), P, f"P={P}")
