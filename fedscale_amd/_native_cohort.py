"""ctypes binding of include/fedcohort.h — the cohort-signature entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1  # include/fedcohort.h FC_ABI_VERSION
GRAM_MAX_K = 4096  # FC_GRAM_MAX_K

_c_void_p, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64

# name -> (restype, argtypes);  must list every symbol of include/fedcohort.h
SIGNATURES = {
    "fc_abi_version": (_i32, []),
    "fc_signature": (_i32, [_c_void_p, _i64, _i32, _c_void_p, _c_void_p, _i32, _c_void_p, _c_void_p, _i32, _c_void_p,
                            _i32, _c_void_p, _i64, _c_void_p]),
    "fc_center_workspace_bytes": (_i64, [_i32, _i64]),
    "fc_center": (_i32, [_c_void_p, _i64, _i32, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
    "fc_normalize": (_i32, [_c_void_p, _i64, _i32, _i64, _c_void_p, _c_void_p, _c_void_p]),
    "fc_gram_workspace_bytes": (_i64, [_i32, _i64]),
    "fc_gram": (_i32, [_c_void_p, _i64, _i32, _i64, _c_void_p, _c_void_p, _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the fc_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "fc_abi_version", ABI_VERSION, "fedcohort")
    return _lib


def call(name: str, *args):
    """Call an fc_* entry point; raise on a non-zero return code."""
    return _native.checked_call(load(), name, args)
