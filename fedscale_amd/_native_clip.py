"""ctypes binding of include/fedclip.h — the norm-clipped FedAvg entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1  # include/fedclip.h FCL_ABI_VERSION
PLAN_FIELDS = 6  # FCL_PLAN_FIELDS

_c_void_p, _i32, _i64, _f32, _f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double

# name -> (restype, argtypes);  must list every symbol of include/fedclip.h
SIGNATURES = {
    "fcl_abi_version": (_i32, []),
    "fcl_workspace_bytes": (_i64, [_i32, _i64]),
    "fcl_row_sqnorms": (_i32, [_c_void_p, _i64, _i32, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p]),
    "fcl_norm_plan": (_i64, [_i32, _i64, _c_void_p]),
    "fcl_clip_coefs": (_i32, [_c_void_p, _i32, _f64, _c_void_p, _c_void_p, _c_void_p]),
    "fcl_reduce": (_i32, [_c_void_p, _i64, _i32, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i32, _c_void_p]),
    "fcl_reduce_plan": (_i64, [_i32, _i32, _i64, _c_void_p, _i32]),
    "fcl_finish": (_i32, [_c_void_p, _c_void_p, _c_void_p, _f32, _f32, _i64, _c_void_p, _c_void_p, _c_void_p,
                          _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the fcl_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "fcl_abi_version", ABI_VERSION, "fedclip")
    return _lib


def call(name: str, *args):
    """Call an fcl_* entry point; raise on a negative return code (counts are returned)."""
    return _native.checked_call(load(), name, args, negative_only=True)
