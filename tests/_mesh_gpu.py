"""The entries of csrc/sd_mesh.hip through the C ABI, for tests/test_gpu_meshes*.py: every call uploads numpy arrays, gives every
output exactly the rows the count pass reports (or the caller's capacity) and the scratch exactly ``*_temp_bytes``, each followed by a
guard band that must stay untouched, and returns numpy arrays."""
import ctypes as C

import numpy as np
import torch

from syconn_amd import _lib as L

GUARD = 4096


def _up(a, dev, dtype):
    a = np.ascontiguousarray(np.asarray(a), dtype=dtype)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a if signed is None else a.view(signed)).to(dev)


class Guarded:
    """`nbytes` usable bytes (at least one allocated) followed by a guard band."""

    def __init__(self, dev, nbytes):
        self.n = int(nbytes)
        self.t = torch.empty(self.n + GUARD, dtype=torch.uint8, device=dev)
        self.t[self.n:] = 0xA5
        self.t[:self.n] = 0xCD

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.t[self.n:] == 0xA5).all())

    def host(self, dtype, shape):
        return self.t[:self.n].cpu().numpy().view(dtype).reshape(shape)


def source_tables(shape, pad, ds):
    from syconn_amd.proc.meshes import _source_tables
    return _source_tables(shape, pad, None if ds is None else np.asarray(ds, np.float64))


def count(dev, vol, tabs, ids):
    """-> (rc, counts)"""
    lib = L.load()
    v = _up(vol, dev, np.uint64)
    t = [_up(x, dev, np.int32) for x in tabs]
    i = _up(ids, dev, np.uint64)
    counts = torch.zeros(8, dtype=torch.int64, device=dev)
    X, Y, Z = vol.shape
    rc = lib.sd_mesh_count(v.data_ptr(), X, Y, Z, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(tabs[0]), len(tabs[1]), len(tabs[2]),
                           i.data_ptr(), len(ids), counts.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return rc, counts.cpu().numpy()


def build(dev, vol, tabs, ids, scale, offset, vert_cap=None, tri_cap=None, shrink=0):
    """-> (rc, counts, dict of outputs).  Capacities default to the count pass's numbers."""
    lib = L.load()
    ids = np.asarray(ids, np.uint64)
    if vert_cap is None or tri_cap is None:
        rc, c = count(dev, vol, tabs, ids)
        assert rc == 0
        vert_cap, tri_cap = (int(c[0]) if vert_cap is None else vert_cap), (int(c[1]) if tri_cap is None else tri_cap)
    v = _up(vol, dev, np.uint64)
    t = [_up(x, dev, np.int32) for x in tabs]
    i = _up(ids, dev, np.uint64)
    n = len(ids)
    X, Y, Z = vol.shape
    N = [len(x) for x in tabs]
    vb, tb = Guarded(dev, 8 * (n + 1)), Guarded(dev, 8 * (n + 1))
    verts, tris = Guarded(dev, 12 * vert_cap), Guarded(dev, 12 * tri_cap)
    bb, area = Guarded(dev, 24 * n), Guarded(dev, 8 * n)
    need = lib.sd_mesh_build_temp_bytes(N[0], N[1], N[2], vert_cap, tri_cap)
    tmp = Guarded(dev, need)
    counts = torch.zeros(8, dtype=torch.int64, device=dev)
    f3 = lambda a: (C.c_double * 3)(*[float(x) for x in a])
    rc = lib.sd_mesh_build(v.data_ptr(), X, Y, Z, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), N[0], N[1], N[2], i.data_ptr(), n, f3(scale), f3(offset),
                           vert_cap, tri_cap, vb.ptr(), tb.ptr(), verts.ptr(), tris.ptr(), bb.ptr(), area.ptr(), counts.data_ptr(), tmp.ptr(),
                           max(need - shrink, 0), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    for g, name in ((vb, 'vert_begin'), (tb, 'tri_begin'), (verts, 'verts'), (tris, 'tris'), (bb, 'mesh_bb'), (area, 'area'), (tmp, 'scratch')):
        assert g.intact(), f'the device wrote behind {name}'
    return rc, counts.cpu().numpy(), dict(ids=ids, vert_begin=vb.host(np.uint64, -1), tri_begin=tb.host(np.uint64, -1), vertices=verts.host(np.float32, (-1, 3)),
                                          indices=tris.host(np.uint32, (-1, 3)), mesh_bb=bb.host(np.float32, (-1, 2, 3)), mesh_area=area.host(np.float64, -1))


def merge(dev, piece_ids, vert_begin, tri_begin, verts, tris, shrink=0):
    """-> (rc, counts, dict of outputs cut to the objects the device reports)"""
    lib = L.load()
    P, NV, NT = len(piece_ids), len(verts), len(tris)
    pi, pv, pt = _up(piece_ids, dev, np.uint64), _up(vert_begin, dev, np.uint64), _up(tri_begin, dev, np.uint64)
    v, t = _up(np.asarray(verts).reshape(-1, 3), dev, np.float32), _up(np.asarray(tris).reshape(-1, 3), dev, np.uint32)
    o_ids, o_vb, o_tb = Guarded(dev, 8 * P), Guarded(dev, 8 * (P + 1)), Guarded(dev, 8 * (P + 1))
    o_v, o_t, o_bb, o_area = Guarded(dev, 12 * NV), Guarded(dev, 12 * NT), Guarded(dev, 24 * P), Guarded(dev, 8 * P)
    need = lib.sd_mesh_merge_temp_bytes(P)
    tmp = Guarded(dev, need)
    counts = torch.zeros(8, dtype=torch.int64, device=dev)
    rc = lib.sd_mesh_merge(pi.data_ptr(), pv.data_ptr(), pt.data_ptr(), P, v.data_ptr(), NV, t.data_ptr(), NT, o_ids.ptr(), o_vb.ptr(), o_tb.ptr(), o_v.ptr(),
                           o_t.ptr(), o_bb.ptr(), o_area.ptr(), counts.data_ptr(), tmp.ptr(), max(need - shrink, 0), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    for g in (o_ids, o_vb, o_tb, o_v, o_t, o_bb, o_area, tmp):
        assert g.intact(), 'the device wrote behind an output or the scratch'
    c = counts.cpu().numpy()
    n = int(min(max(c[0], 0), P))
    return rc, c, dict(ids=o_ids.host(np.uint64, -1)[:n], vert_begin=o_vb.host(np.uint64, -1)[:n + 1], tri_begin=o_tb.host(np.uint64, -1)[:n + 1],
                       vertices=o_v.host(np.float32, (-1, 3)), indices=o_t.host(np.uint32, (-1, 3)), mesh_bb=o_bb.host(np.float32, (-1, 2, 3))[:n],
                       mesh_area=o_area.host(np.float64, -1)[:n])
