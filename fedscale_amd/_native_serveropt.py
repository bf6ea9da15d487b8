"""ctypes binding of include/fedserveropt.h — the adaptive server optimizer entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1  # include/fedserveropt.h FSO_ABI_VERSION
ADAM, ADAGRAD, AVGM = 0, 1, 2            # FSO_ADAM, FSO_ADAGRAD, FSO_AVGM
FSO_INIT, FSO_NT_ON, FSO_NT_OFF = 1, 2, 4
NT_MIN_BYTES = 256 << 20                 # FSO_NT_MIN_BYTES
PLAN_FIELDS = 4                          # FSO_PLAN_FIELDS

_c_void_p, _i32, _i64, _f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float

# name -> (restype, argtypes);  must list every symbol of include/fedserveropt.h
SIGNATURES = {
    "fso_abi_version": (_i32, []),
    "fso_step": (_i32, [_i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _f32, _f32, _f32, _f32,
                        _f32, _f32, _f32, _i32, _c_void_p]),
    "fso_step_parts": (_i32, [_i32, _i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _f32,
                              _f32, _f32, _f32, _f32, _f32, _f32, _i32, _c_void_p]),
    "fso_step_plan": (_i32, [_i32, _i64, _i32, _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the fso_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "fso_abi_version", ABI_VERSION, "fedserveropt")
    return _lib


def call(name: str, *args):
    """Call an fso_* entry point; raise on a non-zero return code."""
    return _native.checked_call(load(), name, args)
