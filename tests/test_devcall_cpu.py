"""``syconn_amd._dev``, the call layer between the Python host side and the device entries, on ``torch.device('cpu')``: the upload
rule, the output / counter allocators, the ctypes triples and the argument conversion of ``call``.  No library call, no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from syconn_amd import _dev as D

CPU = torch.device('cpu')


@pytest.mark.parametrize('src, want', [(np.uint64, torch.int64), (np.uint32, torch.int32), (np.bool_, torch.uint8), (np.int64, torch.int64)])
def test_up_keeps_the_bits(src, want):
    rng = np.random.default_rng(3)
    if src is np.bool_:
        a = rng.integers(0, 2, (5, 7)).astype(np.bool_)
    else:
        a = rng.integers(0, np.iinfo(src).max, (5, 7), dtype=src, endpoint=True)
        a[0, 0] = np.iinfo(src).max                          # the sign bit of the unsigned types
        a[0, 1] = np.iinfo(src).min
    t = D.up(a, CPU)
    assert t.dtype == want and tuple(t.shape) == a.shape and t.is_contiguous()
    assert t.numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def test_up_makes_a_strided_array_contiguous():
    base = np.arange(4 * 6 * 3, dtype=np.uint64).reshape(4, 6, 3) + np.uint64(2 ** 63)
    for a in (base.swapaxes(0, 2), base[::2, 1::2], base[:, ::-1]):
        assert not a.flags['C_CONTIGUOUS']
        t = D.up(a, CPU)
        assert t.dtype == torch.int64 and t.is_contiguous() and tuple(t.shape) == a.shape
        assert np.array_equal(t.numpy().view(np.uint64), a)


def test_empty_has_a_first_extent_of_at_least_one():
    assert tuple(D.empty(0, D.i64, CPU).shape) == (1,)
    assert tuple(D.empty((0, 3), D.i32, CPU).shape) == (1, 3)
    assert tuple(D.empty(np.int64(0), D.u8, CPU).shape) == (1,)
    t = D.empty((4, 6), D.f64, CPU)
    assert tuple(t.shape) == (4, 6) and t.dtype == torch.float64 and t.device == CPU
    assert tuple(D.empty(5, D.i32, CPU).shape) == (5,) and D.empty(5, D.i32, CPU).dtype == torch.int32


def test_counters_are_int64_zeros():
    for n, t in ((8, D.counters(CPU)), (3, D.counters(CPU, 3)), (1, D.counters(CPU, 1))):
        assert t.dtype == torch.int64 and tuple(t.shape) == (n,) and not t.any() and t.device == CPU


def test_triples():
    for make, ctype, values in ((D.i32x3, C.c_int32, (np.int32(-7), 2 ** 31 - 1, np.uint32(5))), (D.i64x3, C.c_int64, (-2 ** 63, np.int64(9), 2 ** 63 - 1)),
                                (D.f64x3, C.c_double, (np.float32(0.5), 1e300, -3))):
        for v in (values, list(values), np.array(values)):
            a = make(v)
            assert a._type_ is ctype and len(a) == 3
            assert list(a) == [ctype(x).value for x in np.array(values).tolist()]


def test_pointers_convert_tensors_only():
    t = torch.arange(24, dtype=torch.int32).view(3, 8)
    triple, number, real = D.i64x3((1, 2, 3)), 12345678901234, 0.25
    got = D.pointers((t, t[1, 2:], None, number, real, triple, t[2]))
    assert got[0] == t.data_ptr()
    assert got[1] == t.data_ptr() + (8 + 2) * 4 and got[6] == t.data_ptr() + 16 * 4          # a slice: the slice's own address
    assert got[2] is None and got[3] is number and got[4] is real and got[5] is triple
    assert D.pointers(()) == []
