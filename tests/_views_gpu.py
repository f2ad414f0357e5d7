"""csrc/sd_views.hip through the C ABI for the GPU tests: every output and every scratch buffer is followed by a guard band that the call
must leave untouched (checked before anything is returned)."""
import ctypes as C

import numpy as np
import torch

import _views_ref as R
from syconn_amd import _lib as L

GUARD, FILL = 4096, 0xA5


class Buf:
    """`n` bytes on the device followed by a guard band."""

    def __init__(self, n, dev):
        self.n = int(n)
        self.t = torch.full((self.n + GUARD,), FILL, dtype=torch.uint8, device=dev)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def host(self, dtype, count=None):
        assert bool((self.t[self.n:] == FILL).all()), 'a write went past the capacity given'
        a = self.t[:self.n].cpu().numpy().view(dtype)
        return a if count is None else a[:count]


def up(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev) if a.size else torch.zeros(1, dtype=torch.uint8, device=dev)


def f32x3(v):
    return (C.c_float * 3)(*[float(x) for x in np.asarray(v, np.float32).reshape(3)])


def f64n(v):
    v = np.asarray(v, np.float64).reshape(-1)
    return (C.c_double * len(v))(*[float(x) for x in v])


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _counts(dev):
    L.check(L.load().sd_init(dev.index or 0), 'sd_init')
    return Buf(64, dev)


def rotations(dev, verts, coords, edge, center=(0, 0, 0), max_dist=1.0, stride=1, flag_only=False):
    """-> (rc, counts, rot (N, 16) or None, empty (N,) bool)."""
    lib = L.load()
    verts, coords = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(coords, np.float32).reshape(-1, 3)
    n_v, n = len(verts), len(coords)
    v_d, c_d, cnt = up(verts, dev), up(coords, dev), _counts(dev)
    tmp = Buf(lib.sd_views_rotations_temp_bytes(n_v, stride), dev)
    rot, empty = Buf(max(n, 1) * 128, dev), Buf(max(n, 1), dev)
    if flag_only:
        rc = lib.sd_views_flag_empty(v_d.data_ptr(), n_v, stride, c_d.data_ptr(), n, f32x3(center), float(max_dist), float(edge), empty.ptr, cnt.ptr, tmp.ptr,
                                     tmp.n, stream(dev))
    else:
        rc = lib.sd_views_rotations(v_d.data_ptr(), n_v, stride, c_d.data_ptr(), n, f32x3(center), float(max_dist), float(edge), rot.ptr, empty.ptr, cnt.ptr,
                                    tmp.ptr, tmp.n, stream(dev))
    torch.cuda.synchronize(dev)
    tmp.host(np.uint8)
    return rc, cnt.host(np.uint64, 8), (None if flag_only else rot.host(np.float64, n * 16).reshape(n, 16)), empty.host(np.uint8, n).astype(bool)


class Mesh:
    """Raw vertices / triangles on the device with their normalisation and the triangle grid."""

    def __init__(self, dev, verts, tris, center=None, max_dist=None):
        lib = L.load()
        self.dev = dev
        self.verts, self.tris = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(tris, np.uint32).reshape(-1, 3)
        if center is None:
            center, max_dist = (self.verts.mean(0), np.abs(self.verts - self.verts.mean(0)).max()) if len(self.verts) else (np.zeros(3), 1.0)
        self.center, self.max_dist = np.asarray(center, np.float32), np.float32(max_dist)
        self.v_d, self.t_d = up(self.verts, dev), up(self.tris, dev)
        self.index = Buf(lib.sd_views_index_bytes(len(self.tris)), dev)
        tmp, cnt = Buf(lib.sd_views_index_temp_bytes(len(self.tris)), dev), _counts(dev)
        self.rc = lib.sd_views_index(self.v_d.data_ptr(), len(self.verts), self.t_d.data_ptr(), len(self.tris), f32x3(self.center), float(self.max_dist),
                                     self.index.ptr, self.index.n, cnt.ptr, tmp.ptr, tmp.n, stream(dev))
        torch.cuda.synchronize(dev)
        tmp.host(np.uint8)
        self.index.host(np.uint8)
        self.counts = cnt.host(np.uint64, 8)

    @property
    def vn(self):
        return R.normalise(self.verts, self.center, self.max_dist)

    def cn(self, coords):
        return R.normalise(coords, self.center, self.max_dist)

    def E(self, comp_window):
        return R.edge_lengths(comp_window, self.max_dist)

    def candidates(self, coords, E, cap=None):
        """-> (rc, counts, begin (N + 1) uint64, cand uint32); cap None: the sizing call first, then the exact capacity."""
        lib = L.load()
        coords = np.asarray(coords, np.float32).reshape(-1, 3)
        n = len(coords)
        c_d = up(coords, self.dev)
        tmp = Buf(lib.sd_views_candidates_temp_bytes(n), self.dev)

        def call(cap):
            begin, cand, cnt = Buf((n + 1) * 8, self.dev), Buf(max(cap, 1) * 4, self.dev), _counts(self.dev)
            rc = lib.sd_views_candidates(self.index.ptr, len(self.tris), c_d.data_ptr(), n, f32x3(self.center), float(self.max_dist), f64n(E), begin.ptr,
                                         cand.ptr if cap else None, cap, cnt.ptr, tmp.ptr, tmp.n, stream(self.dev))
            torch.cuda.synchronize(self.dev)
            tmp.host(np.uint8)
            return rc, cnt.host(np.uint64, 8), begin.host(np.uint64, n + 1), cand.host(np.uint32, cap), begin, cand
        if cap is None:
            rc, c, _, _, _, _ = call(0)
            assert rc == 0
            cap = int(c[0])
        return call(cap)

    def render(self, coords, rot, comp_window, nb_views, ws, index=False, cos_sin=None, cand=None, E=None):
        """-> (rc, counts, views (N, nb_views, H, W))."""
        lib = L.load()
        coords, rot = np.asarray(coords, np.float32).reshape(-1, 3), np.asarray(rot, np.float64).reshape(-1, 16)
        n, (W, H) = len(coords), ws
        E = self.E(comp_window) if E is None else E
        rc, c, begin_h, cand_h, begin, cand_b = self.candidates(coords, E) if cand is None else cand
        assert rc == 0 and c[1] == 0
        n_cand = int(begin_h[-1]) if n else 0
        cos_v, sin_v = R.view_cos_sin(nb_views) if cos_sin is None else cos_sin
        c_d, r_d = up(coords, self.dev), up(rot, self.dev)
        item = 4 if index else 1
        views, cnt = Buf(max(n * nb_views * H * W, 1) * item, self.dev), _counts(self.dev)
        tmp = Buf(lib.sd_views_render_temp_bytes(n, nb_views), self.dev)
        head = (self.v_d.data_ptr(), len(self.verts), self.t_d.data_ptr(), len(self.tris), self.index.ptr, c_d.data_ptr(), n, r_d.data_ptr(), f32x3(self.center),
                float(self.max_dist), f64n(E), f64n(cos_v), f64n(sin_v), nb_views, W, H)
        tail = (begin.ptr, cand_b.ptr, n_cand, views.ptr, n * nb_views * H * W, cnt.ptr, tmp.ptr, tmp.n, stream(self.dev))
        if index:
            rc = lib.sd_views_render_index(*head, *tail)
        else:
            rc = lib.sd_views_render(*head, f64n(R.gauss_weights()), *tail)
        torch.cuda.synchronize(self.dev)
        tmp.host(np.uint8)
        return rc, cnt.host(np.uint64, 8), views.host(np.uint32 if index else np.uint8, n * nb_views * H * W).reshape(n, nb_views, H, W)


def vote(dev, index_arr, label_arr, bg, n_verts, n_labels, unpredicted, table=True):
    """-> (rc, counts, vertex labels, table or None)."""
    lib = L.load()
    idx, lab = np.asarray(index_arr, np.uint32).reshape(-1), np.asarray(label_arr, np.uint8).reshape(-1)
    i_d, l_d, cnt = up(idx, dev), up(lab, dev), _counts(dev)
    out, tab = Buf(max(n_verts, 1), dev), Buf(max(n_verts * n_labels, 1), dev)
    tmp = Buf(lib.sd_views_vote_temp_bytes(n_verts, n_labels), dev)
    rc = lib.sd_views_vote(i_d.data_ptr(), l_d.data_ptr(), len(idx), int(bg), n_verts, n_labels, unpredicted, out.ptr, tab.ptr if table else None, cnt.ptr, tmp.ptr,
                           tmp.n, stream(dev))
    torch.cuda.synchronize(dev)
    tmp.host(np.uint8)
    t = tab.host(np.uint8, n_verts * n_labels).reshape(n_verts, n_labels)
    if not table:
        assert (t == FILL).all()
    return rc, cnt.host(np.uint64, 8), out.host(np.uint8, n_verts), (t if table else None)
