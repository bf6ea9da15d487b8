"""ctypes binding of include/fedsign.h — the 1-bit sign delta-upload entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1  # include/fedsign.h FSG_ABI_VERSION
PLAN_FIELDS = 6  # FSG_PLAN_FIELDS
BLOCK = 256      # FSG_BLOCK

_c_void_p, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64

# name -> (restype, argtypes);  must list every symbol of include/fedsign.h
SIGNATURES = {
    "fsg_abi_version": (_i32, []),
    "fsg_reduce": (_i32, [_c_void_p, _c_void_p, _i64, _i64, _i32, _i64, _c_void_p, _c_void_p, _i32, _c_void_p]),
    "fsg_reduce_plan": (_i64, [_i32, _i32, _i64, _c_void_p, _i32]),
    "fsg_sign_row": (_i32, [_c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the fsg_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "fsg_abi_version", ABI_VERSION, "fedsign")
    return _lib


def call(name: str, *args):
    """Call an fsg_* entry point; raise on a negative return code (counts are returned)."""
    return _native.checked_call(load(), name, args, negative_only=True)
