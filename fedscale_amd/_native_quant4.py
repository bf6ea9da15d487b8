"""ctypes binding of include/fedquant4.h — the MXFP4 delta-upload entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1  # include/fedquant4.h FQ4_ABI_VERSION
PLAN_FIELDS = 6  # FQ4_PLAN_FIELDS
BLOCK = 32       # FQ4_BLOCK
SCALE_MIN, SCALE_MAX = 2, 252  # FQ4_SCALE_MIN, FQ4_SCALE_MAX

_c_void_p, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64

# name -> (restype, argtypes);  must list every symbol of include/fedquant4.h
SIGNATURES = {
    "fq4_abi_version": (_i32, []),
    "fq4_reduce": (_i32, [_c_void_p, _c_void_p, _i64, _i64, _i32, _i64, _c_void_p, _c_void_p, _i32, _c_void_p]),
    "fq4_reduce_plan": (_i64, [_i32, _i32, _i64, _c_void_p, _i32]),
    "fq4_quantize_row": (_i32, [_c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the fq4_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "fq4_abi_version", ABI_VERSION, "fedquant4")
    return _lib


def call(name: str, *args):
    """Call an fq4_* entry point; raise on a negative return code (counts are returned)."""
    return _native.checked_call(load(), name, args, negative_only=True)
