"""ctypes binding of include/fedkrum.h — the Krum / Multi-Krum entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1  # include/fedkrum.h FK_ABI_VERSION
MAX_K = 4096     # FK_MAX_K
PLAN_FIELDS = 6  # FK_PLAN_FIELDS

_c_void_p, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64

# name -> (restype, argtypes);  must list every symbol of include/fedkrum.h
SIGNATURES = {
    "fk_abi_version": (_i32, []),
    "fk_gram_plan": (_i64, [_i32, _i64, _c_void_p]),
    "fk_gram_workspace_bytes": (_i64, [_i32, _i64]),
    "fk_gram": (_i32, [_c_void_p, _i64, _i32, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p]),
    "fk_scores": (_i32, [_c_void_p, _i32, _i32, _c_void_p, _c_void_p]),
    "fk_select": (_i32, [_c_void_p, _i32, _i32, _c_void_p, _c_void_p, _c_void_p]),
    "fk_finish": (_i32, [_c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the fk_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "fk_abi_version", ABI_VERSION, "fedkrum")
    return _lib


def call(name: str, *args):
    """Call an fk_* entry point; raise on a negative return code (sizes are returned)."""
    return _native.checked_call(load(), name, args, negative_only=True)
