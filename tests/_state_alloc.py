"""Allocators that decide what an "uninitialised" device buffer holds, for tests/test_gpu_buffer_state.py: the host layer allocates every
output and scratch with ``torch.empty`` (``_dev.empty`` / ``_dev.scratch`` and direct calls), so a result may depend on what the caching
allocator hands back.  ``Fill(byte)`` serves buffers that hold `byte` everywhere; ``Arena(nbytes)`` serves views of one buffer at bump
offsets, so that after ``rewind()`` the same call sequence gets the same addresses with the bytes the previous sequence left there.
``install`` puts one of them behind ``syconn_amd._dev.empty`` / ``_dev.scratch`` and behind ``torch.empty`` / ``torch.empty_like`` for
requests on the allocator's device type (default 'cuda'); every other request (another device, pinned memory, ``out=``) passes through.
The device type is a parameter so that tests/test_state_alloc_cpu.py runs all of this on the CPU."""
import contextlib

import torch

ALIGN = 512
_EMPTY, _EMPTY_LIKE = torch.empty, torch.empty_like        # the originals: the allocators themselves never go through the patches


def _extent(meta) -> int:
    """Bytes from the first to behind the last element of a tensor with the shape and strides of `meta`."""
    if meta.numel() == 0:
        return 0
    return (1 + sum((n - 1) * s for n, s in zip(meta.shape, meta.stride()))) * meta.element_size()


class _Alloc:
    def __init__(self, device='cuda'):
        self.device_type = torch.device(device).type
        self.served = []            # (name given to _dev.scratch or None, bytes), in call order

    @property
    def calls(self) -> int:
        return len(self.served)

    @property
    def names(self) -> set:
        return {name for name, _ in self.served if name is not None}

    @property
    def bytes_served(self) -> int:
        return sum(n for _, n in self.served)

    def raw(self, nbytes: int, device) -> torch.Tensor:
        raise NotImplementedError

    def serve(self, meta, device, name=None) -> torch.Tensor:
        """A tensor on `device` with the shape, strides and dtype of `meta` (a tensor on the meta device) over bytes of this allocator."""
        nbytes = _extent(meta)
        self.served.append((name, nbytes))
        flat = self.raw(nbytes, device).view(meta.dtype)
        return flat.as_strided(tuple(meta.shape), tuple(meta.stride()))

    def wants(self, device) -> bool:
        return device.type == self.device_type


class Fill(_Alloc):
    """Every buffer is a fresh allocation set to `byte` on the current stream."""

    def __init__(self, byte: int, device='cuda'):
        super().__init__(device)
        self.byte = int(byte)

    def raw(self, nbytes, device):
        return _EMPTY(nbytes, dtype=torch.uint8, device=device).fill_(self.byte)


class Arena(_Alloc):
    """One uint8 buffer of `nbytes` on `device`, filled once with 0xFF; requests are views at offsets rounded up to ALIGN bytes.  A request
    that does not fit raises MemoryError: there is no fresh allocation behind it."""

    def __init__(self, nbytes: int, device='cuda'):
        device = torch.device(device)
        super().__init__(device)
        self.buf = _EMPTY(int(nbytes) + ALIGN, dtype=torch.uint8, device=device).fill_(0xFF)
        self.base = -self.buf.data_ptr() % ALIGN           # the first served address is a multiple of ALIGN whatever torch returned
        self.size = int(nbytes)
        self.offset = self.high = 0

    def rewind(self):
        """Serve from the start again; the contents stay."""
        self.offset = 0

    def raw(self, nbytes, device):
        if torch.device(device).type != self.buf.device.type or (device.index is not None and self.buf.device.index is not None
                                                                   and device.index != self.buf.device.index):
            raise RuntimeError(f'Arena on {self.buf.device} asked for a buffer on {device}')
        start = -(-self.offset // ALIGN) * ALIGN
        if start + nbytes > self.size:
            raise MemoryError(f'Arena of {self.size} bytes: {nbytes} more at offset {start} do not fit')
        self.offset = start + nbytes
        self.high = max(self.high, self.offset)
        return self.buf[self.base + start:self.base + start + nbytes]


def _device_of(device, like=None) -> torch.device:
    if device is None:
        return like.device if like is not None else torch.get_default_device()
    device = torch.device('cuda', device) if isinstance(device, int) else torch.device(device)
    if device.type == 'cuda' and device.index is None and torch.cuda.is_available():
        device = torch.device('cuda', torch.cuda.current_device())
    return device


def install(monkeypatch, alloc):
    """Patch `alloc` in until `monkeypatch` undoes it.  -> alloc"""
    from syconn_amd import _dev as D
    from syconn_amd import _lib as L

    def empty(*args, **kw):
        device = _device_of(kw.get('device'))
        if kw.get('out') is not None or kw.get('pin_memory') or not alloc.wants(device):
            return _EMPTY(*args, **kw)
        grad = kw.pop('requires_grad', False)
        t = alloc.serve(_EMPTY(*args, **{**kw, 'device': 'meta'}), device)
        return t.requires_grad_(True) if grad else t

    def empty_like(inp, *args, **kw):
        device = _device_of(kw.get('device'), inp)
        if kw.get('pin_memory') or not alloc.wants(device):
            return _EMPTY_LIKE(inp, *args, **kw)
        grad = kw.pop('requires_grad', False)
        t = alloc.serve(_EMPTY_LIKE(inp, *args, **{**kw, 'device': 'meta'}), device)
        return t.requires_grad_(True) if grad else t

    def dev_empty(shape, dtype, dev):
        shape = (max(shape[0], 1),) + shape[1:] if isinstance(shape, tuple) else (max(shape, 1),)
        return alloc.serve(_EMPTY(shape, dtype=dtype, device='meta'), _device_of(dev))

    def dev_scratch(name, dev, *sizes):
        n = max(int(getattr(L.load(), name)(*sizes)), 1)
        return alloc.serve(_EMPTY(n, dtype=torch.uint8, device='meta'), _device_of(dev), name=name)

    monkeypatch.setattr(torch, 'empty', empty)
    monkeypatch.setattr(torch, 'empty_like', empty_like)
    monkeypatch.setattr(D, 'empty', dev_empty)
    monkeypatch.setattr(D, 'scratch', dev_scratch)
    return alloc


@contextlib.contextmanager
def installed(alloc):
    """``with installed(Fill(0xFF)) as a: ...``: the patches hold inside the block only."""
    import pytest
    with pytest.MonkeyPatch.context() as mp:
        yield install(mp, alloc)
