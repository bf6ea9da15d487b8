"""ctypes binding of include/fedsketch.h — the Count-Sketch upload entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1    # include/fedsketch.h FCS_ABI_VERSION
PLAN_FIELDS = 4    # FCS_PLAN_FIELDS
TILE = 1024        # FCS_TILE
U = 8              # FCS_U
SUBTRACT_FROM = 1  # FCS_SUBTRACT_FROM

_c_void_p, _i32, _i64, _u64, _f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float

# name -> (restype, argtypes);  must list every symbol of include/fedsketch.h
SIGNATURES = {
    "fcs_abi_version": (_i32, []),
    "fcs_table_floats": (_i64, [_i32, _i64]),
    "fcs_sketch_plan": (_i64, [_i32, _i64, _i32, _i64, _c_void_p]),
    "fcs_sketch_row": (_i32, [_c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i64, _u64, _c_void_p, _i32, _i32,
                              _c_void_p]),
    "fcs_estimate": (_i32, [_c_void_p, _i64, _i32, _i64, _u64, _c_void_p, _c_void_p]),
    "fcs_state_step": (_i32, [_c_void_p, _c_void_p, _c_void_p, _f32, _i64, _c_void_p, _c_void_p, _c_void_p,
                              _c_void_p]),
    "fcs_apply": (_i32, [_c_void_p, _c_void_p, _i64, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the fcs_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "fcs_abi_version", ABI_VERSION, "fedsketch")
    return _lib


def call(name: str, *args):
    """Call an fcs_* entry point; raise on a negative return code (counts and sizes are returned)."""
    return _native.checked_call(load(), name, args, negative_only=True)
