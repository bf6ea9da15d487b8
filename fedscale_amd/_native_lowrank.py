"""ctypes binding of include/fedlowrank.h — the low-rank delta-upload entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1   # include/fedlowrank.h FLR_ABI_VERSION
MAX_RANK = 64     # FLR_MAX_RANK
PLAN_FIELDS = 4   # FLR_PLAN_FIELDS
DEPTH = 8         # FLR_DEPTH
DENSE_COLS = 256  # FLR_DENSE_COLS
KIND_DENSE, KIND_SMALL, KIND_LARGE = 0, 1, 2  # FLR_KIND_*

_c_void_p, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64

# name -> (restype, argtypes);  must list every symbol of include/fedlowrank.h
SIGNATURES = {
    "flr_abi_version": (_i32, []),
    "flr_row_layout": (_i64, [_i32, _i32, _c_void_p, _c_void_p]),
    "flr_reduce_plan": (_i64, [_i32, _i32, _i32, _c_void_p, _i32, _c_void_p]),
    "flr_reduce_table": (_i64, [_i32, _i32, _i32, _c_void_p, _i32, _c_void_p, _i64]),
    "flr_reduce": (_i32, [_c_void_p, _i64, _i32, _i32, _i32, _c_void_p, _i32, _c_void_p, _c_void_p, _i64, _c_void_p,
                          _c_void_p, _i32, _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the flr_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "flr_abi_version", ABI_VERSION, "fedlowrank")
    return _lib


def call(name: str, *args):
    """Call an flr_* entry point; raise on a negative return code (counts and sizes are returned)."""
    return _native.checked_call(load(), name, args, negative_only=True)
