"""The one way from torch tensors into libsurfel_raster.so: what every wrapper module hands the C-ABI (_lib.PROTOTYPES) and how it calls.
(_lib itself stays free of torch; this module is where the two meet.)"""
from __future__ import annotations

import contextlib
import ctypes as C

import torch

from ._lib import check, load

_ALREADY = contextlib.nullcontext()


def ptr(t):
    """The address the library gets for a tensor: NULL for None and for a tensor without elements ("not given")."""
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def buf(t):
    """(address, size) of a state buffer or workspace, for `*buf(geom)`."""
    return ptr(t), t.numel()


def stream(dev=None):
    """The current stream of `dev` (None: of the current device) as the `void* stream` of the ABI."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def on(dev):
    """The device of the call as the current one: a context only where it is not already."""
    return _ALREADY if dev.index == torch.cuda.current_device() else torch.cuda.device(dev)


def call(name, dev, *args):
    """One launching entry point on the current stream of `dev`: every one of them takes `void* stream` last.  A refusal or a HIP error
    raises SurfelRasterError with the function's name and sr_last_error()."""
    with on(dev):
        check(getattr(load(), name)(*args, stream(dev)), name)


def workspace(bytes_fn_name, dev, *args):
    """The uint8 tensor on `dev` of the size the named sr_*_bytes function reports for `args`."""
    return torch.empty((getattr(load(), bytes_fn_name)(*args),), dtype=torch.uint8, device=dev)
