"""The one place where the Python host layer meets the device entries of the C ABI (``include/syconn_dense.h``): the device and its
current stream, argument conversion, uploads, output / counter / scratch allocation and the ctypes triples.  Imports torch, so the
modules that import torch lazily import this module where they need it.  Entries without a trailing stream (``*_bytes``,
``sd_host_*``, ``sd_snappy_*``, ``sd_plan_clip_window``) are called on ``_lib.load()`` directly."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

u8, i32, i64, f64 = torch.uint8, torch.int32, torch.int64, torch.float64
_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.bool_): np.uint8}


def device(device=None) -> torch.device:
    """The given (default: the current) ROCm device, with the library initialised on it.  There is no CPU fallback."""
    lib = L.load()
    if not torch.cuda.is_available():
        raise RuntimeError('syconn_amd: no MI355X visible to PyTorch-ROCm; this package has no CPU fallback')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    L.check(lib.sd_init(dev.index or 0), 'sd_init')
    return dev


def stream(dev) -> int:
    """The raw handle of the stream that is current on `dev` now."""
    return torch.cuda.current_stream(dev).cuda_stream


def pointers(args) -> list:
    """Tensors (slices included) -> their ``data_ptr()``; None, numbers and ctypes objects are passed on as they are.  Dtype,
    contiguity and device are the caller's business."""
    return [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]


def call(name: str, dev, *args):
    """``lib.<name>(*args, current stream of dev)`` in the argument order of the header; a library error raises (``_lib.check``)."""
    L.check(getattr(L.load(), name)(*pointers(args), stream(dev)), name)


def up(a, dev) -> torch.Tensor:
    """numpy -> contiguous device tensor with the same bits: uint64 / uint32 / bool travel as int64 / int32 / uint8."""
    a = np.ascontiguousarray(a)
    signed = _SIGNED.get(a.dtype)
    return torch.from_numpy(a if signed is None else a.view(signed)).to(dev)


def empty(shape, dtype, dev) -> torch.Tensor:
    """Uninitialised output of `shape` (a number or a tuple) with a first extent of at least 1: the entries reject null outputs."""
    if isinstance(shape, tuple):
        return torch.empty((max(shape[0], 1),) + shape[1:], dtype=dtype, device=dev)
    return torch.empty(max(shape, 1), dtype=dtype, device=dev)


def counters(dev, n: int = 8) -> torch.Tensor:
    return torch.zeros(n, dtype=torch.int64, device=dev)


def scratch(name: str, dev, *sizes) -> torch.Tensor:
    """A uint8 buffer of ``lib.<name>(*sizes)`` bytes (at least one: the entries compare sizes and reject null)."""
    return torch.empty(max(int(getattr(L.load(), name)(*sizes)), 1), dtype=torch.uint8, device=dev)


def down(t, n=None, view=None) -> np.ndarray:
    """``t[:n]`` on the host (one copy, waits for the device), optionally viewed as another dtype of the same width."""
    a = (t if n is None else t[:n]).cpu().numpy()
    return a if view is None else a.view(view)


def i32x3(v):
    return (C.c_int32 * 3)(*[int(x) for x in v])


def i64x3(v):
    return (C.c_int64 * 3)(*[int(x) for x in v])


def f64x3(v):
    return (C.c_double * 3)(*[float(x) for x in v])
