"""ctypes binding of include/fedsparse.h — the top-k sparse delta-upload entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1  # include/fedsparse.h FS_ABI_VERSION
PLAN_FIELDS = 6  # FS_PLAN_FIELDS
TILE = 4096      # FS_TILE

_c_void_p, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64

# name -> (restype, argtypes);  must list every symbol of include/fedsparse.h
SIGNATURES = {
    "fs_abi_version": (_i32, []),
    "fs_row_offsets": (_i32, [_c_void_p, _i64, _c_void_p, _i32, _i64, _c_void_p, _i64, _c_void_p]),
    "fs_check_rows": (_i32, [_c_void_p, _i64, _c_void_p, _i32, _i64, _c_void_p, _c_void_p]),
    "fs_reduce": (_i32, [_c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _i32, _i64, _c_void_p,
                         _c_void_p, _i32, _c_void_p]),
    "fs_reduce_plan": (_i64, [_i32, _i32, _i64, _c_void_p, _i32]),
    "fs_topk_workspace": (_i64, [_i64]),
    "fs_topk_row": (_i32, [_c_void_p, _c_void_p, _c_void_p, _i64, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                           _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the fs_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "fs_abi_version", ABI_VERSION, "fedsparse")
    return _lib


def call(name: str, *args):
    """Call an fs_* entry point; raise on a negative return code (counts and sizes are returned)."""
    return _native.checked_call(load(), name, args, negative_only=True)
