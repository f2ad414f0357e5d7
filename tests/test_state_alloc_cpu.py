"""tests/_state_alloc.py on the CPU (the allocators take their device as a parameter): what is served has the shape, dtype and strides
of the original call and holds the fill; the arena's offsets, rewind and refusal; what passes through; and that the patches end."""
import numpy as np
import pytest
import torch

import _state_alloc as A
from syconn_amd import _dev as D
from syconn_amd import _lib as L

ORIGINALS = (torch.empty, torch.empty_like, D.empty, D.scratch)


def raw_bytes(t):
    """The bytes of the elements of `t`, whatever its dtype and strides."""
    return t.contiguous().view(-1).view(torch.uint8).numpy()


REQUESTS = [
    (lambda: torch.empty(7, dtype=torch.uint8, device='cpu'), (7,), torch.uint8, (1,)),
    (lambda: torch.empty((5, 6), dtype=torch.int32, device='cpu'), (5, 6), torch.int32, (6, 1)),
    (lambda: torch.empty(3, 4, 5, dtype=torch.float64, device=torch.device('cpu')), (3, 4, 5), torch.float64, (20, 5, 1)),
    (lambda: torch.empty((2, 3, 4, 5), dtype=torch.float16, device='cpu', memory_format=torch.channels_last), (2, 3, 4, 5), torch.float16,
     (60, 1, 15, 3)),
    (lambda: torch.empty(0, dtype=torch.int64, device='cpu'), (0,), torch.int64, (1,)),
    (lambda: torch.empty((0, 3), dtype=torch.int64, device='cpu'), (0, 3), torch.int64, (3, 1)),
    (lambda: torch.empty(4, device='cpu'), (4,), torch.float32, (1,)),
    (lambda: torch.empty_like(torch.zeros((4, 3), dtype=torch.int16)), (4, 3), torch.int16, (3, 1)),
    (lambda: torch.empty_like(torch.zeros((4, 3), dtype=torch.int16).t()), (3, 4), torch.int16, (1, 3)),
    (lambda: torch.empty_like(torch.zeros((4, 3)), dtype=torch.int64), (4, 3), torch.int64, (3, 1)),
    (lambda: D.empty(0, torch.int64, 'cpu'), (1,), torch.int64, (1,)),
    (lambda: D.empty((0, 6), torch.int32, torch.device('cpu')), (1, 6), torch.int32, (6, 1)),
    (lambda: D.empty((9, 2, 3), torch.float32, 'cpu'), (9, 2, 3), torch.float32, (6, 3, 1)),
]


@pytest.mark.parametrize('make', [lambda: A.Fill(0x00, 'cpu'), lambda: A.Fill(0xFF, 'cpu'), lambda: A.Fill(0xCD, 'cpu'), lambda: A.Arena(1 << 16, 'cpu')])
def test_served_tensors_have_the_requested_form_and_hold_the_fill(make):
    with A.installed(make()) as alloc:
        byte = getattr(alloc, 'byte', 0xFF)
        for k, (request, shape, dtype, strides) in enumerate(REQUESTS):
            t = request()
            assert tuple(t.shape) == shape and t.dtype == dtype and t.device.type == 'cpu', k
            if t.numel():
                assert tuple(t.stride()) == strides, k
            assert alloc.calls == k + 1 and alloc.served[-1] == (None, t.numel() * t.element_size()), k
            assert (raw_bytes(t) == byte).all(), k
            if t.numel():
                t.fill_(1)
                assert (t == 1).all()
        assert alloc.names == set() and alloc.bytes_served == sum(n for _, n in alloc.served)
    with A.installed(A.Fill(0xFF, 'cpu')):                                      # all bits set: NaN as a float, -1 as a signed integer
        assert torch.isnan(torch.empty(3, dtype=torch.float64, device='cpu')).all()
        assert (torch.empty(3, dtype=torch.int32, device='cpu') == -1).all()


def test_scratch_is_served_by_name_with_the_library_size():
    n = int(L.load().sd_propmerge_temp_bytes(1000))
    with A.installed(A.Fill(0xA5, 'cpu')) as alloc:
        t = D.scratch('sd_propmerge_temp_bytes', 'cpu', 1000)
        u = D.scratch('sd_skel_components_temp_bytes', 'cpu', 0)
        torch.empty(5, dtype=torch.uint8, device='cpu')
    assert t.dtype == torch.uint8 and t.shape == (n,) and (t.numpy() == 0xA5).all() and u.numel() >= 1
    assert alloc.served[0] == ('sd_propmerge_temp_bytes', n) and alloc.served[1][0] == 'sd_skel_components_temp_bytes'
    assert alloc.names == {'sd_propmerge_temp_bytes', 'sd_skel_components_temp_bytes'} and alloc.calls == 3


def test_arena_offsets_rewind_and_refusal():
    arena = A.Arena(8192, 'cpu')
    assert arena.buf.numel() >= 8192 and (arena.buf.numpy() == 0xFF).all()
    sizes = ((3, torch.uint8), (100, torch.int64), (0, torch.int32), (1, torch.float64), (513, torch.uint8), (5, torch.int16))
    with A.installed(arena):
        first = [torch.empty(n, dtype=t, device='cpu') for n, t in sizes]
        ptrs = [t.data_ptr() for t in first]
        live = [p for p, t in zip(ptrs, first) if t.numel()]
        assert all(p % A.ALIGN == 0 for p in live)
        assert all(b >= a + t.numel() * t.element_size() for a, b, t in zip(live, live[1:], [t for t in first if t.numel()]))   # no overlap
        assert [p - live[0] for p in live] == [0, 512, 1536, 2048, 3072]
        for k, t in enumerate(first):
            t.fill_(k + 1)
        arena.rewind()
        again = [torch.empty(n, dtype=t, device='cpu') for n, t in sizes]
        assert [t.data_ptr() for t in again] == ptrs
        for k, t in enumerate(again):                                           # the previous sequence's values, not the 0xFF of the start
            assert (t == k + 1).all()
        arena.rewind()
        shifted = torch.empty(700, dtype=torch.uint8, device='cpu')            # another sequence: its first bytes are the old first buffer's
        assert shifted.data_ptr() == ptrs[0] and (shifted[:3] == 1).all() and (shifted[3:512] == 0xFF).all() and (shifted[512::8] == 2).all()
        arena.rewind()
        torch.empty(8192, dtype=torch.uint8, device='cpu')                      # exactly full
        with pytest.raises(MemoryError):
            torch.empty(1, dtype=torch.uint8, device='cpu')
        arena.rewind()
        with pytest.raises(MemoryError):
            torch.empty(8193, dtype=torch.uint8, device='cpu')
        arena.rewind()
        torch.empty(7680, dtype=torch.uint8, device='cpu')
        with pytest.raises(MemoryError):
            D.empty(65, torch.int64, 'cpu')                                     # 520 bytes at offset 7680
        with pytest.raises(MemoryError):
            D.scratch('sd_propmerge_temp_bytes', 'cpu', 100000)
    assert arena.high == 8192


def test_what_passes_through_is_not_touched():
    with A.installed(A.Fill(0xFF, 'cuda')) as alloc:                            # the product setting, seen from the CPU
        a = torch.empty(1000, dtype=torch.uint8)
        b = torch.empty((3, 4), dtype=torch.float32, device='cpu')
        c = torch.empty_like(torch.zeros(5, dtype=torch.int64))
        assert a.device.type == b.device.type == c.device.type == 'cpu' and b.shape == (3, 4) and c.dtype == torch.int64
        m = torch.empty(5, device='meta')
        assert m.device.type == 'meta'
        assert alloc.calls == 0
    with A.installed(A.Fill(0xFF, 'cpu')) as alloc:
        out = torch.zeros(6, dtype=torch.int32)
        r = torch.empty(6, out=out)
        assert r.data_ptr() == out.data_ptr() and (out == 0).all()
        m = torch.empty((2, 2), device='meta')
        ml = torch.empty_like(m)
        assert m.device.type == ml.device.type == 'meta'
        assert alloc.calls == 0
        z = torch.zeros(4, dtype=torch.uint8, device='cpu')                     # not an uninitialised request: never patched
        f = torch.full((4,), 3, dtype=torch.uint8, device='cpu')
        assert (z == 0).all() and (f == 3).all() and alloc.calls == 0
        assert (np.asarray(torch.empty(2, dtype=torch.uint8, device='cpu')) == 0xFF).all() and alloc.calls == 1


def test_pinned_requests_pass_through(monkeypatch):
    """``pin_memory=True`` needs a device to run, so the original is replaced by a recorder here: the patch hands the call on unchanged."""
    seen = []
    monkeypatch.setattr(A, '_EMPTY', lambda *a, **k: seen.append((a, k)) or 'orig')
    monkeypatch.setattr(A, '_EMPTY_LIKE', lambda *a, **k: seen.append((a, k)) or 'orig_like')
    with A.installed(A.Fill(0xFF, 'cpu')) as alloc:
        assert torch.empty(4, dtype=torch.uint8, pin_memory=True) == 'orig'
        src = torch.zeros(3)
        assert torch.empty_like(src, pin_memory=True) == 'orig_like'
    assert seen == [((4,), dict(dtype=torch.uint8, pin_memory=True)), ((src,), dict(pin_memory=True))] and alloc.calls == 0


def test_patches_end_with_the_context(monkeypatch):
    assert (torch.empty, torch.empty_like, D.empty, D.scratch) == ORIGINALS
    with A.installed(A.Fill(0x11, 'cpu')):
        assert torch.empty is not ORIGINALS[0] and torch.empty_like is not ORIGINALS[1] and D.empty is not ORIGINALS[2] and D.scratch is not ORIGINALS[3]
    assert (torch.empty, torch.empty_like, D.empty, D.scratch) == ORIGINALS
    with pytest.raises(ZeroDivisionError):
        with A.installed(A.Fill(0x11, 'cpu')):
            1 / 0
    assert (torch.empty, torch.empty_like, D.empty, D.scratch) == ORIGINALS
    with pytest.MonkeyPatch.context() as mp:                                    # the fixture form
        alloc = A.install(mp, A.Fill(0x22, 'cpu'))
        assert (torch.empty(2, dtype=torch.uint8, device='cpu') == 0x22).all() and alloc.calls == 1
    assert (torch.empty, torch.empty_like, D.empty, D.scratch) == ORIGINALS
    assert A._EMPTY is ORIGINALS[0] and A._EMPTY_LIKE is ORIGINALS[1]
