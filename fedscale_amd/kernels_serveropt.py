"""Typed torch-tensor wrappers over the adaptive server optimizers' C ABI (include/fedserveropt.h), with the same
host-side checks as ``kernels.yogi_step``: device / dtype / contiguity / size / alignment, launched on the current HIP
stream of the output's device.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _native_serveropt as NS
from ._native import ptr
from .kernels import _cols, _dev, _stream

RULES = {"adam": NS.ADAM, "adagrad": NS.ADAGRAD, "avgm": NS.AVGM}


def rule_id(rule) -> int:
    """``rule`` ("adam", "adagrad", "avgm") as the C ABI's number; ValueError otherwise."""
    try:
        return RULES[rule]
    except (KeyError, TypeError):
        raise ValueError(f"rule: expected one of {sorted(RULES)}, got {rule!r}") from None


def _flags(init: bool, nt: Optional[bool]) -> int:
    return (NS.FSO_INIT if init else 0) | (0 if nt is None else NS.FSO_NT_ON if nt else NS.FSO_NT_OFF)


def _hp(eta, tau, beta, omb, beta2, omb2, v0) -> tuple:
    return tuple(float(x) for x in (eta, tau, beta, omb, beta2, omb2, v0))


def step(rule, cur, last, m, v, out, P, *, eta, tau, beta, omb, beta2, omb2, v0, init, nt: Optional[bool] = None):
    """One step of ``rule`` over P parameters (fso_step): ``m`` and ``v`` in place, the new model into ``out`` (which
    may be ``cur``).  ``v`` may be None for "avgm".  ``nt``: None takes the size policy, True / False force the
    non-temporal / cached loads and stores."""
    r = rule_id(rule)
    ops = [("cur", cur), ("last", last), ("m", m), ("out", out)]
    if r != NS.AVGM or v is not None:
        ops.append(("v", v))
    for n, t in ops:
        _dev(t, torch.float32, n, _cols(P))
        if t.device != out.device:
            raise ValueError(f"{n}: on {t.device}, out on {out.device}")
    NS.call("fso_step", r, ptr(cur), ptr(last), ptr(m), ptr(v), ptr(out), int(P),
            *_hp(eta, tau, beta, omb, beta2, omb2, v0), _flags(init, nt), _stream(out))
    return out


def step_parts(rule, curs, lasts, ms, vs, outs, Ps, streams, *, eta, tau, beta, omb, beta2, omb2, v0, init,
               nt: Optional[bool] = None):
    """fso_step over every part of a sharded model in one native call (part i on streams[i]); ``vs`` may be None for
    "avgm"."""
    import ctypes

    import numpy as np

    r = rule_id(rule)
    n = len(curs)
    tabs = [("cur", curs), ("last", lasts), ("m", ms), ("out", outs)]
    if r != NS.AVGM or vs is not None:
        tabs.append(("v", vs))
    for i in range(n):
        for nm, ts in tabs:
            _dev(ts[i], torch.float32, f"{nm}[{i}]", _cols(Ps[i]))
            if ts[i].device != outs[i].device:
                raise ValueError(f"{nm}[{i}]: on {ts[i].device}, out[{i}] on {outs[i].device}")
    tab = lambda ts: np.asarray([t.data_ptr() for t in ts], dtype=np.uint64)  # noqa: E731
    c_t, l_t, m_t, o_t = tab(curs), tab(lasts), tab(ms), tab(outs)
    v_t = None if vs is None else tab(vs)
    P = np.asarray(Ps, dtype=np.int64)
    st = (ctypes.c_void_p * n)(*streams)
    NS.call("fso_step_parts", n, r, c_t.ctypes.data, l_t.ctypes.data, m_t.ctypes.data,
            None if v_t is None else v_t.ctypes.data, o_t.ctypes.data, P.ctypes.data,
            *_hp(eta, tau, beta, omb, beta2, omb2, v0), _flags(init, nt), st)


def plan(rule, P: int, *, init: bool = False, nt: Optional[bool] = None) -> dict:
    """What ``step(rule, ..., P, init=init, nt=nt)`` launches (fso_step_plan; host only): ``blocks`` workgroups of
    256 threads, the ``trips`` of the grid-stride loop, ``nt`` whether the loads and stores are non-temporal, and the
    ``bytes`` read plus written."""
    import numpy as np

    f = np.zeros(NS.PLAN_FIELDS, dtype=np.int64)
    NS.call("fso_step_plan", rule_id(rule), int(P), _flags(init, nt), f.ctypes.data)
    return dict(blocks=int(f[0]), trips=int(f[1]), nt=bool(f[2]), bytes=int(f[3]))
