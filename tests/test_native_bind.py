"""The binding helpers every ctypes table goes through (fedscale_amd/_native.py: bind, check_abi, checked_call), on a
fake library object: no GPU and no real library."""
import ctypes

import pytest

from fedscale_amd import _native


class _Fn:
    def __init__(self, rc):
        self.rc, self.args = rc, None

    def __call__(self, *args):
        self.args = args
        return self.rc


class _FakeLib:
    def __init__(self, **rcs):
        self.fa_last_error_string = _Fn(b"the reason")
        for name, rc in rcs.items():
            setattr(self, name, _Fn(rc))


SIGS = {"fx_abi_version": (ctypes.c_int32, []), "fx_count": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_void_p])}


def test_bind_types_every_symbol():
    lib = _FakeLib(fx_abi_version=3, fx_count=0)
    _native.bind(lib, SIGS, "lib.so")
    assert lib.fx_count.restype is ctypes.c_int64 and lib.fx_count.argtypes == [ctypes.c_int32, ctypes.c_void_p]
    assert lib.fx_abi_version.restype is ctypes.c_int32 and lib.fx_abi_version.argtypes == []


def test_missing_symbol_is_an_error():
    with pytest.raises(_native.FedAggError, match=r"lib\.so: no symbol fx_count \(an older build"):
        _native.bind(_FakeLib(fx_abi_version=3), SIGS, "lib.so")


def test_wrong_abi_version_is_an_error():
    lib = _FakeLib(fx_abi_version=3)
    _native.check_abi(lib, "fx_abi_version", 3, "lib.so: fedx")
    with pytest.raises(_native.FedAggError, match=r"lib\.so: fedx ABI version 3, expected 4"):
        _native.check_abi(lib, "fx_abi_version", 4, "lib.so: fedx")


def test_checked_call_negative_only():
    """The rule of the modules whose functions return counts: a negative code raises, a count passes through."""
    lib = _FakeLib(fx_count=7, fx_bad=-1)
    assert _native.checked_call(lib, "fx_count", (1, None), negative_only=True) == 7
    assert lib.fx_count.args == (1, None)
    assert _native.checked_call(_FakeLib(fx_count=0), "fx_count", (), negative_only=True) == 0
    with pytest.raises(_native.FedAggError, match=r"fx_bad failed \(-1\): the reason"):
        _native.checked_call(lib, "fx_bad", (), negative_only=True)


@pytest.mark.parametrize("rc", [-1, 1, 7])
def test_checked_call_raises_on_any_non_zero_code(rc):
    with pytest.raises(_native.FedAggError, match=rf"fx_count failed \({rc}\): the reason"):
        _native.checked_call(_FakeLib(fx_count=rc), "fx_count", (2,))
    assert _native.checked_call(_FakeLib(fx_count=0), "fx_count", (2,)) == 0
