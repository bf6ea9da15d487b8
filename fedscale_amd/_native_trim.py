"""ctypes binding of include/fedtrim.h — the coordinate-wise trimmed-mean entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1  # include/fedtrim.h FT_ABI_VERSION
MAX_TRIM = 16    # FT_MAX_TRIM
PLAN_FIELDS = 7  # FT_PLAN_FIELDS
KERNEL_SELECT, KERNEL_REDUCE = 0, 1  # FT_KERNEL_SELECT, FT_KERNEL_REDUCE

_c_void_p, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64

# name -> (restype, argtypes);  must list every symbol of include/fedtrim.h
SIGNATURES = {
    "ft_abi_version": (_i32, []),
    "ft_max_trim": (_i32, []),
    "ft_select": (_i32, [_c_void_p, _i64, _i32, _i64, _i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "ft_reduce": (_i32, [_c_void_p, _i64, _i32, _i64, _i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                         _c_void_p, _c_void_p]),
    "ft_plan": (_i64, [_i32, _i32, _i64, _i32, _c_void_p, _i32]),
}

_lib = None


def load():
    """The loaded library with the ft_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "ft_abi_version", ABI_VERSION, "fedtrim")
    return _lib


def call(name: str, *args):
    """Call an ft_* entry point; raise on a negative return code (counts are returned)."""
    return _native.checked_call(load(), name, args, negative_only=True)
