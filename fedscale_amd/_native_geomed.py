"""ctypes binding of include/fedgeomed.h — the geometric-median (RFA) entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1  # include/fedgeomed.h FGM_ABI_VERSION
MAX_K = 4096     # FGM_MAX_K
MAX_ITERS = 64   # FGM_MAX_ITERS
CHUNK = 256      # FGM_CHUNK

_c_void_p, _i32, _i64, _f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double

# name -> (restype, argtypes);  must list every symbol of include/fedgeomed.h
SIGNATURES = {
    "fgm_abi_version": (_i32, []),
    "fgm_start": (_i32, [_c_void_p, _i64, _i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "fgm_weights": (_i32, [_c_void_p, _i32, _f64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "fgm_dist2_workspace_bytes": (_i64, [_i32]),
    "fgm_gram_dist2": (_i32, [_c_void_p, _i32, _c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p]),
    "fgm_finish": (_i32, [_c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the fgm_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "fgm_abi_version", ABI_VERSION, "fedgeomed")
    return _lib


def call(name: str, *args):
    """Call an fgm_* entry point; raise on a negative return code (sizes are returned)."""
    return _native.checked_call(load(), name, args, negative_only=True)
