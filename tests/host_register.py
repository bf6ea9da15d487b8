"""Whether this machine can pin host memory a process already owns (hipHostRegister).

Some MI355X hosts (virtual machines among them) refuse every hipHostRegister with ``invalid argument``; pinned memory
can then only be allocated (hipHostMalloc, torch's pin_memory).  The registered ingress is built on registration, so
the tests whose subject it is ask here first and skip themselves where the facility is missing.
"""
import functools

import numpy as np

REASON = "hipHostRegister is not supported here"


@functools.lru_cache(maxsize=None)
def supported() -> bool:
    """Register and release one page through the library (fa_host_register clears the error HIP keeps of a refused
    call, so nothing is left behind for a later launch check).  Call it with the GPU initialised."""
    from fedscale_amd import _native

    lib = _native.load()
    page = 4096
    raw = np.zeros(2 * page, dtype=np.uint8)
    addr = raw.ctypes.data + (-raw.ctypes.data) % page
    if lib.fa_host_register(addr, page) != 0:
        return False
    _native.call("fa_host_unregister", addr)
    return True
