"""ctypes binding of include/fedhalf.h — the 16-bit client-upload entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1  # include/fedhalf.h FH_ABI_VERSION
FH_F16, FH_BF16 = 0, 1
PLAN_FIELDS = 6  # FH_PLAN_FIELDS

_c_void_p, _i32, _i64, _f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float

# name -> (restype, argtypes);  must list every symbol of include/fedhalf.h
SIGNATURES = {
    "fh_abi_version": (_i32, []),
    "fh_reduce": (_i32, [_c_void_p, _i32, _i64, _i32, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _f32, _i32,
                         _c_void_p]),
    "fh_reduce_plan": (_i64, [_i32, _i32, _i64, _i32, _c_void_p, _i32]),
    "fh_reduce_launches": (_i64, [_i32, _i64, _i32]),
    "fh_pack_row": (_i32, [_c_void_p, _c_void_p, _c_void_p, _i32, _c_void_p, _i32, _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the fh_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "fh_abi_version", ABI_VERSION, "fedhalf")
    return _lib


def call(name: str, *args):
    """Call an fh_* entry point; raise on a negative return code (counts are returned)."""
    return _native.checked_call(load(), name, args, negative_only=True)
