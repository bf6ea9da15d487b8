"""ctypes binding of include/fedvote.h — the majority-vote sign entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1       # include/fedvote.h FVT_ABI_VERSION
PLAN_FIELDS = 7       # FVT_PLAN_FIELDS
MAX_ROWS = 65535      # FVT_MAX_ROWS
MAX_CLIENTS = 1 << 24  # FVT_MAX_CLIENTS
MODES = {"majority": 0, "mean": 1}  # FVT_MAJORITY, FVT_MEAN

_c_void_p, _i32, _i64, _f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float

# name -> (restype, argtypes);  must list every symbol of include/fedvote.h
SIGNATURES = {
    "fvt_abi_version": (_i32, []),
    "fvt_count": (_i32, [_c_void_p, _i64, _i32, _i64, _c_void_p, _i32, _c_void_p]),
    "fvt_count_plan": (_i64, [_i32, _i32, _i64, _c_void_p, _i32]),
    "fvt_finish": (_i32, [_c_void_p, _c_void_p, _i64, _i32, _f32, _i32, _c_void_p, _c_void_p, _c_void_p]),
    "fvt_sign_row": (_i32, [_c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the fvt_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "fvt_abi_version", ABI_VERSION, "fedvote")
    return _lib


def call(name: str, *args):
    """Call an fvt_* entry point; raise on a negative return code (counts are returned)."""
    return _native.checked_call(load(), name, args, negative_only=True)
