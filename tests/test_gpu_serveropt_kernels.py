"""fso_step and fso_step_parts on the GPU against the numpy float32 restatement of include/fedserveropt.h
(tests/serveropt_fixtures.py), bit for bit in m, v and the new model: every rule, first and carried steps, cached and
non-temporal loads, sizes on either side of a float4, a wave and a workgroup, the shapes the plan says take a second
grid-stride trip or go non-temporal by policy, guard regions, NaN-filled state under FSO_INIT, out aliasing cur, parts
against the concatenation, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

from tests import serveropt_fixtures as sf

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = (1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049)
GUARD = 64
GUARD_BITS = 0x7FC12345  # a NaN payload no step produces
HP = sf.hparams(eta=0.03, tau=1e-3, beta=0.9, beta2=0.99)


def _ld(P):
    return (P + 3) // 4 * 4


def _buf(a, dev):
    """A device buffer of a's ld floats followed by GUARD floats of GUARD_BITS."""
    a = np.ascontiguousarray(a, F32)
    g = np.full(GUARD, GUARD_BITS, dtype=np.uint32).view(F32)
    return torch.from_numpy(np.concatenate([a, g])).to(dev)


def _guard_ok(t, ld):
    return bool((t[ld:].cpu().numpy().view(np.uint32) == GUARD_BITS).all()) and t.numel() == ld + GUARD


def _same(got, want, what):
    assert sf.bits_equal(got, want), f"{what}: {sf.first_difference(got, want)}"


def _run_steps(dev, rule, P, init, nt, steps=3, seed=0, alias=False, state_fill=None, v_none=False):
    """``steps`` consecutive steps on the device and in the restatement; every step's m, v and out compared bit for
    bit, the guards after.  ``state_fill``: what m and v hold before an FSO_INIT step."""
    from fedscale_amd import kernels_serveropt as kso

    ld = _ld(P)
    cur0, last, m, v = sf.inputs(P, seed + P)
    rng = np.random.default_rng(seed + 7 * P + 1)
    if init and state_fill is not None:
        dm, dv = _buf(np.full(ld, state_fill, F32), dev), _buf(np.full(ld, state_fill, F32), dev)
    else:
        dm, dv = _buf(m, dev), _buf(v, dev)
    if rule == "avgm" and v_none:
        dv = None
    v_before = None if dv is None else dv[:ld].cpu().numpy()
    dlast = _buf(last, dev)
    results = []
    for s in range(steps):
        cur = cur0 if s == 0 else (cur0 + (rng.standard_normal(ld) * 0.01).astype(F32)).astype(F32)
        first = init and s == 0
        m, v1, out = sf.step(rule, cur, last, m, v, HP, first)
        v = v if v1 is None else v1
        dcur = _buf(cur, dev)
        dout = dcur if alias else _buf(np.full(ld, 7.0, F32), dev)
        kso.step(rule, dcur, dlast, dm, dv, dout, P, init=first, nt=nt, **HP)
        what = (rule, P, "init" if init else "carried", nt, s)
        _same(dm[:ld].cpu().numpy(), m, what + ("m",))
        if rule != "avgm":
            _same(dv[:ld].cpu().numpy(), v, what + ("v",))
        _same(dout[:ld].cpu().numpy(), out, what + ("out",))
        for name, t in (("cur", dcur), ("last", dlast), ("m", dm), ("v", dv), ("out", dout)):
            if t is not None:
                assert _guard_ok(t, ld), what + (name, "guard")
        if not alias:
            _same(dcur[:ld].cpu().numpy(), cur, what + ("cur untouched",))
        _same(dlast[:ld].cpu().numpy(), last, what + ("last untouched",))
        if rule == "avgm" and dv is not None:
            _same(dv[:ld].cpu().numpy(), v_before, what + ("v untouched by avgm",))
        results.append((m.copy(), None if rule == "avgm" else v.copy(), out.copy()))
    return results


# ---- exactness ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", (False, True), ids=("cached", "nt"))
@pytest.mark.parametrize("init", (True, False), ids=("init", "carried"))
@pytest.mark.parametrize("rule", sf.RULES)
def test_three_steps_equal_the_restatement_bit_for_bit(gpu_device, rule, init, nt):
    for P in SIZES:
        _run_steps(gpu_device, rule, P, init, nt)


def test_the_inputs_hold_the_contracts_edge_cases():
    cur, last, m, v = sf.inputs(2049, 0)
    assert cur[0] == last[0] and v[1] == 0 and np.isposinf(cur[5]) and np.isneginf(cur[6]) and np.isnan(cur[7])
    tiny = np.finfo(F32).tiny
    assert 0 < cur[2] - last[2] < tiny and 0 < v[2] < tiny  # denormal g and v
    m1, v1, out = sf.step("adam", cur, last, m, v, HP, False)
    assert out[0] != last[0] or m[0] == 0  # g = 0 still moves the model by the carried momentum
    assert m[2] == 0 and 0 < m1[2] < tiny and 0 < v1[2] < tiny  # denormal results a flush to zero would lose
    assert np.isnan(out[7]) and np.isnan(out[5]) and np.isnan(out[6])  # inf / inf and NaN propagate
    assert np.isfinite(out[:5]).all()


# ---- grid-stride and non-temporal shapes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", sf.RULES)
def test_the_first_shape_with_two_grid_stride_trips(gpu_device, rule):
    from fedscale_amd import kernels_serveropt as kso

    P = sf.LAST_ONE_TRIP_P + 1
    assert kso.plan(rule, P - 1)["trips"] == 1
    pl = kso.plan(rule, P)
    assert pl["trips"] == 2 and pl["blocks"] == sf.MAX_GRID and not pl["nt"]
    _run_steps(gpu_device, rule, P, init=False, nt=None)


@pytest.mark.parametrize("rule", sf.RULES)
def test_the_first_shape_that_is_non_temporal_by_policy(gpu_device, rule):
    from fedscale_amd import kernels_serveropt as kso

    P = sf.last_cached_P(rule) + 1
    assert not kso.plan(rule, P - 1)["nt"]
    pl = kso.plan(rule, P)
    assert pl["nt"] and pl["trips"] == 2
    _run_steps(gpu_device, rule, P, init=False, nt=None)


# ---- stray writes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", sf.RULES)
def test_init_ignores_what_the_state_buffers_hold(gpu_device, rule):
    for nt in (False, True):
        a = _run_steps(gpu_device, rule, 1025, True, nt, state_fill=0.0)
        b = _run_steps(gpu_device, rule, 1025, True, nt, state_fill=np.nan)
        for (ma, va, oa), (mb, vb, ob) in zip(a, b):
            _same(ma, mb, (rule, "m"))
            _same(oa, ob, (rule, "out"))
            if va is not None:
                _same(va, vb, (rule, "v"))


def test_avgm_runs_without_a_v_buffer(gpu_device):
    for P in (5, 1025):
        for init in (True, False):
            a = _run_steps(gpu_device, "avgm", P, init, None, v_none=True)
            b = _run_steps(gpu_device, "avgm", P, init, None)
            for x, y in zip(a, b):
                _same(x[0], y[0], "m")
                _same(x[2], y[2], "out")


# ---- in place and parts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", sf.RULES)
def test_out_aliasing_cur_gives_the_same_bits(gpu_device, rule):
    for P in (5, 1025, 2049):
        for nt in (False, True):
            _run_steps(gpu_device, rule, P, False, nt, alias=True)


@pytest.mark.parametrize("sizes", ((1025, 63), (5, 2049, 64)), ids=("two", "three"))
@pytest.mark.parametrize("rule", sf.RULES)
def test_parts_equal_one_step_over_the_concatenation(gpu_device, rule, sizes):
    from fedscale_amd import kernels_serveropt as kso

    dev = gpu_device
    ins = [sf.inputs(P, 100 + i) for i, P in enumerate(sizes)]
    # the concatenation, each part padded to its float4 (the step is elementwise, so the padding columns are harmless)
    cat = [np.concatenate([x[j] for x in ins]) for j in range(4)]
    Pcat = cat[0].size
    bufs = [[_buf(x[j], dev) for x in ins] for j in range(4)]
    outs = [_buf(np.full(_ld(P), 7.0, F32), dev) for P in sizes]
    streams = [torch.cuda.Stream(dev) for _ in sizes]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream(dev))
    for init in (True, False):
        kso.step_parts(rule, bufs[0], bufs[1], bufs[2], None if rule == "avgm" else bufs[3], outs, list(sizes),
                       [s.cuda_stream for s in streams], init=init, **HP)
        for s in streams:
            s.synchronize()
        one = [_buf(c, dev) for c in cat]
        one_out = _buf(np.full(Pcat, 7.0, F32), dev)
        kso.step(rule, one[0], one[1], one[2], one[3], one_out, Pcat, init=init, **HP)
        m, v, out = sf.step(rule, cat[0], cat[1], cat[2], cat[3], HP, init)
        _same(one_out[:Pcat].cpu().numpy(), out, (rule, init, "one step"))
        off = 0
        for i, P in enumerate(sizes):
            ld = _ld(P)
            _same(outs[i][:ld].cpu().numpy(), out[off:off + ld], (rule, init, i, "out"))
            _same(bufs[2][i][:ld].cpu().numpy(), m[off:off + ld], (rule, init, i, "m"))
            if rule != "avgm":
                _same(bufs[3][i][:ld].cpu().numpy(), v[off:off + ld], (rule, init, i, "v"))
            for j in range(4):
                assert _guard_ok(bufs[j][i], ld)
            assert _guard_ok(outs[i], ld)
            off += ld
        cat[2] = m
        if v is not None:
            cat[3] = v


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_call_and_leave_every_buffer_untouched(gpu_device):
    from fedscale_amd import _native_serveropt as ns

    dev = gpu_device
    lib = ns.load()
    P, ld = 65, 68
    cur, last, m, v = sf.inputs(P, 3)
    host = dict(cur=cur, last=last, m=m, v=v, out=np.full(ld, 7.0, F32))
    t = {k: _buf(a, dev) for k, a in host.items()}
    torch.cuda.synchronize()
    hp = [ctypes.c_float(float(HP[k])) for k in ("eta", "tau", "beta", "omb", "beta2", "omb2", "v0")]
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(rule=ns.ADAM, P=P, flags=0, **ptrs):
        p = {k: t[k].data_ptr() for k in t}
        p.update(ptrs)
        return lib.fso_step(rule, p["cur"], p["last"], p["m"], p["v"], p["out"], P, *hp, flags, st)

    cases = {
        "negative P": dict(P=-1),
        "unknown rule": dict(rule=3),
        "negative rule": dict(rule=-1),
        "both NT flags": dict(flags=ns.FSO_NT_ON | ns.FSO_NT_OFF),
        "unknown flag": dict(flags=8),
        "NULL cur": dict(cur=None), "NULL last": dict(last=None), "NULL m": dict(m=None),
        "NULL v (adam)": dict(v=None), "NULL v (adagrad)": dict(rule=ns.ADAGRAD, v=None), "NULL out": dict(out=None),
        "misaligned cur": dict(cur=t["cur"].data_ptr() + 4), "misaligned last": dict(last=t["last"].data_ptr() + 4),
        "misaligned m": dict(m=t["m"].data_ptr() + 8), "misaligned v": dict(v=t["v"].data_ptr() + 4),
        "misaligned out": dict(out=t["out"].data_ptr() + 12),
    }
    for what, kw in cases.items():
        assert call(**kw) == -1, what  # FA_E_ARG
        msg = lib.fa_last_error_string().decode()
        assert "fso_step" in msg and "nothing was launched" in msg, (what, msg)
    torch.cuda.synchronize()
    for k, a in host.items():
        _same(t[k][:ld].cpu().numpy(), a, (k, "untouched"))
        assert _guard_ok(t[k], ld)
    assert call(P=0) == 0 and call(P=0, cur=None, out=None) == 0  # P == 0 is FA_OK and queues nothing
    # fso_step_parts: every part is checked before anything launches — a bad second part leaves the first unstepped
    tab = lambda xs: np.asarray(xs, dtype=np.uint64)  # noqa: E731
    c, la, mm, vv = (tab([t[k].data_ptr(), t[k].data_ptr()]) for k in ("cur", "last", "m", "v"))
    oo = tab([t["out"].data_ptr(), t["out"].data_ptr() + 4])
    Ps = np.asarray([P, P], dtype=np.int64)
    side = torch.cuda.Stream(dev)  # fso_step_parts takes no NULL stream
    sts = (ctypes.c_void_p * 2)(side.cuda_stream, side.cuda_stream)
    rc = lib.fso_step_parts(2, ns.ADAM, c.ctypes.data, la.ctypes.data, mm.ctypes.data, vv.ctypes.data, oo.ctypes.data,
                            Ps.ctypes.data, *hp, 0, sts)
    assert rc == -1 and "fso_step_parts[1]" in lib.fa_last_error_string().decode()
    torch.cuda.synchronize()
    for k, a in host.items():
        _same(t[k][:ld].cpu().numpy(), a, (k, "untouched by the refused parts call"))


def test_wrapper_checks_are_those_of_yogi_step(gpu_device):
    from fedscale_amd import kernels_serveropt as kso

    dev = gpu_device
    ok = lambda: torch.zeros(8, dtype=torch.float32, device=dev)  # noqa: E731
    with pytest.raises(ValueError, match="rule"):
        kso.step("yogi", ok(), ok(), ok(), ok(), ok(), 8, init=True, **HP)
    with pytest.raises(ValueError, match="needs >= 12"):
        kso.step("adam", ok(), ok(), ok(), ok(), ok(), 9, init=True, **HP)
    with pytest.raises(TypeError, match="dtype"):
        kso.step("adam", ok().double(), ok(), ok(), ok(), ok(), 8, init=True, **HP)
    with pytest.raises(ValueError, match="device tensor"):
        kso.step("adam", ok().cpu(), ok(), ok(), ok(), ok(), 8, init=True, **HP)
    with pytest.raises(TypeError, match="torch.Tensor"):
        kso.step("adam", ok(), ok(), ok(), None, ok(), 8, init=True, **HP)
    with pytest.raises(ValueError, match="aligned"):
        kso.step("avgm", ok(), ok(), torch.zeros(12, dtype=torch.float32, device=dev)[1:], None, ok(), 8, init=True,
                 **HP)
