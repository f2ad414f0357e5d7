"""The entries of csrc/sd_locations.hip through the C ABI, for tests/test_gpu_locations*.py: every call uploads numpy arrays and runs
over a scratch of exactly ``sd_locations_*_temp_bytes`` followed by a guard band that must stay untouched, and over outputs of exactly
the capacity given followed by guard bands of their own (``Guarded`` of tests/_glia_gpu.py).  Also the inputs the tests share."""
import ctypes as C

import numpy as np
import torch

from _glia_gpu import Guarded
from syconn_amd import _lib as L


def call(dev, rule, verts, vert_begin, ds=None, bins=None, r=None, cap=0, shrink=0, null_scratch=False, n_verts=None, n_obj=None):
    """One call with the capacity `cap` (0: the sizing call) -> (rc, counts (8), loc_begin uint64 (n_obj + 1), locations (cap, 3))."""
    lib = L.load()
    v = np.ascontiguousarray(verts).reshape(-1, 3)
    vb = np.ascontiguousarray(vert_begin, np.uint64).reshape(-1)
    nv = len(v) if n_verts is None else n_verts
    no = len(vb) - 1 if n_obj is None else n_obj
    v_d = torch.from_numpy(v).to(dev)
    vb_d = torch.from_numpy(vb.view(np.int64)).to(dev)
    voxel = rule == 'voxel'
    dt = np.float64 if voxel else np.float32
    begin, loc, counts = Guarded(dev, len(vb), np.uint64), Guarded(dev, 3 * cap, dt), Guarded(dev, 8, np.uint64)
    need = getattr(lib, f'sd_locations_{rule}_temp_bytes')(nv if nv < 2 ** 31 else 1, no if no < 2 ** 31 else 1)
    tmp = Guarded(dev, need, np.uint8)
    tail = (begin.ptr(), loc.ptr() if cap else None, cap, counts.ptr(), None if null_scratch else tmp.ptr(), max(need - shrink, 0),
            torch.cuda.current_stream(dev).cuda_stream)
    vp = v_d.data_ptr() if len(v) else None
    if voxel:
        rc = lib.sd_locations_voxel(vp, int(v.dtype == np.float32), vb_d.data_ptr(), no, nv, float(ds), *tail)
    else:
        assert v.dtype == np.float32
        rc = lib.sd_locations_surface(vp, vb_d.data_ptr(), no, nv, (C.c_float * 3)(*[float(b) for b in bins]), float(r), *tail)
    torch.cuda.synchronize(dev)
    assert begin.intact() and loc.intact() and counts.intact() and tmp.intact(), 'the device wrote behind a buffer it was given'
    return rc, counts.host(8).copy(), begin.host(len(vb)).copy(), loc.host(3 * cap).copy().reshape(-1, 3)


def run(dev, rule, verts, vert_begin, **kw):
    """The sizing call, then the emitting call with exactly the counted capacity -> (counts, loc_begin, locations)."""
    rc, c, begin0, _ = call(dev, rule, verts, vert_begin, cap=0, **kw)
    assert rc == L.SD_OK, L.load().sd_last_error()
    assert not c[1] and not c[4] and not c[5] and not c[7], c
    n = int(c[0])
    assert int(begin0[-1]) == n
    if n == 0:
        return c, begin0, np.zeros((0, 3), np.float64 if rule == 'voxel' else np.float32)
    rc, c, begin, loc = call(dev, rule, verts, vert_begin, cap=n, **kw)
    assert rc == L.SD_OK and int(c[0]) == n and not c[1] and np.array_equal(begin, begin0)
    return c, begin, loc


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- shared inputs ------------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 63, 0, 64, 65, 129, 40, 30, 0)                                # an empty object first, in the middle and last


def base_table(seed=5):
    """Objects of SIZES vertices, float32 multiples of 0.5 around the origin (negative coordinates included); object 8 has one axis,
    object 9 all three of zero extent."""
    rng = np.random.default_rng(seed)
    parts = []
    for k, n in enumerate(SIZES):
        p = rng.integers(-6000, 6001, (n, 3)).astype(np.float32) * np.float32(0.5) + np.float32(1000 * k - 4000)
        if k == 8:
            p[:, 1] = p[0, 1]
        if k == 9:
            p[:] = p[0]
        parts.append(p)
    begin = np.concatenate(([0], np.cumsum(SIZES))).astype(np.uint64)
    return begin, np.concatenate(parts).astype(np.float32)
