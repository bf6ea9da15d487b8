"""ctypes binding of include/fedrotate.h — the block Hadamard rotation entry points of libfedagg.so.

They are typed onto the library ``_native.load()`` has already loaded and verified (build id, ABI version of
include/fedagg.h); ``_native.SIGNATURES`` stays the table of fedagg.h / fedclient.h alone.  As there: no fallback,
a missing symbol or a failing call raises ``FedAggError``.
"""
from __future__ import annotations

import ctypes

from . import _native

ABI_VERSION = 1  # include/fedrotate.h FRT_ABI_VERSION
BLOCK = 4096     # FRT_BLOCK

_c_void_p, _i32, _i64, _u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64

# name -> (restype, argtypes);  must list every symbol of include/fedrotate.h
SIGNATURES = {
    "frt_abi_version": (_i32, []),
    "frt_padded": (_i64, [_i64]),
    "frt_rotate": (_i32, [_c_void_p, _c_void_p, _i64, _u64, _c_void_p, _c_void_p]),
    "frt_unrotate": (_i32, [_c_void_p, _i64, _u64, _c_void_p, _c_void_p]),
}

_lib = None


def load():
    """The loaded library with the frt_* entry points typed (once; a racing second typing sets the same types)."""
    global _lib
    if _lib is None:
        _lib = _native.bind_header(SIGNATURES, "frt_abi_version", ABI_VERSION, "fedrotate")
    return _lib


def call(name: str, *args):
    """Call an frt_* entry point; raise on a negative return code (counts are returned)."""
    return _native.checked_call(load(), name, args, negative_only=True)
