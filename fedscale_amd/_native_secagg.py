"""ctypes binding of include/fedsecagg.h — the secure-aggregation entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1          # include/fedsecagg.h FSA_ABI_VERSION
PLAN_FIELDS = 6          # FSA_PLAN_FIELDS
MAX_KEYS = 1 << 20       # FSA_MAX_KEYS
MAX_FRAC_BITS = 30       # FSA_MAX_FRAC_BITS
MAX_MAG_BITS = 30        # FSA_MAX_MAG_BITS
MASK_TILE = 4096         # FSA_MASK_TILE
MASK_GRID_PER_CU = 8     # FSA_MASK_GRID_PER_CU

_c_void_p, _i32, _i64, _u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32

# name -> (restype, argtypes);  must list every symbol of include/fedsecagg.h
SIGNATURES = {
    "fsa_abi_version": (_i32, []),
    "fsa_encode_row": (_i32, [_c_void_p, _c_void_p, _i64, _i32, _i32, _c_void_p, _c_void_p, _c_void_p]),
    "fsa_mask_sum": (_i32, [_c_void_p, _i32, _i32, _u32, _u32, _u32, _i64, _i64, _c_void_p, _c_void_p, _c_void_p]),
    "fsa_reduce": (_i32, [_c_void_p, _i64, _i32, _i64, _c_void_p, _c_void_p, _i32, _c_void_p]),
    "fsa_reduce_plan": (_i64, [_i32, _i32, _i64, _c_void_p, _i32]),
    "fsa_finish": (_i32, [_c_void_p, _c_void_p, _i64, _i32, _i32, _i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the fsa_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "fsa_abi_version", ABI_VERSION, "fedsecagg")
    return _lib


def call(name: str, *args):
    """Call an fsa_* entry point; raise on a negative return code (counts are returned)."""
    return _native.checked_call(load(), name, args, negative_only=True)
