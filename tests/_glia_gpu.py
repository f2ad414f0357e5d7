"""The entries of csrc/sd_glia.hip through the C ABI, for tests/test_gpu_glia_split*.py: every call uploads numpy arrays, runs over a
scratch of exactly ``sd_glia_split_temp_bytes`` followed by a guard band that must stay untouched, over outputs of exactly the capacities
given followed by guard bands of their own, and returns numpy arrays cut to the counts the device reports."""
import numpy as np
import torch

from syconn_amd import _lib as L

GUARD = 4096
FILL = 0xCD  # what the usable bytes of every output and scratch hold before a call (tests/test_gpu_buffer_state.py sets 0x00 / 0xFF)
U = np.uint64


def _up(a, dev, dtype):
    a = np.ascontiguousarray(np.asarray(a), dtype=dtype)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


class Guarded:
    """`n` items of `dtype` holding FILL bytes, followed by GUARD bytes of 0xA5 (all in one uint8 buffer)."""

    def __init__(self, dev, n, dtype):
        self.bytes = int(n) * np.dtype(dtype).itemsize
        self.dtype = dtype
        self.t = torch.empty(self.bytes + GUARD, dtype=torch.uint8, device=dev)
        self.t[:self.bytes] = FILL
        self.t[self.bytes:] = 0xA5

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.t[self.bytes:] == 0xA5).all())

    def host(self, n):
        return self.t[:int(n) * np.dtype(self.dtype).itemsize].cpu().numpy().view(self.dtype)


def split(dev, edges, sv_ids, boxes, glia, T, nodes=None, cell_size=None, min_cell_size=0.0, sv_sizes=None, node_cap=None, edge_cap=None, shrink=0,
          null_scratch=False):
    """-> (rc, counts (16), dict of outputs shaped like tests/_glia_ref.split_table's)."""
    lib = L.load()
    e = np.asarray(edges, U).reshape(-1, 2)
    x = np.zeros(0, U) if nodes is None else np.asarray(nodes, U).reshape(-1)
    ids = np.asarray(sv_ids, U).reshape(-1)
    n_e, n_x, n_ids = len(e), len(x), len(ids)
    m = 2 * n_e + n_x
    nc, ec = (m if node_cap is None else node_cap), (n_e if edge_cap is None else edge_cap)
    d = dict(e=_up(e, dev, U), x=_up(x, dev, U), ids=_up(ids, dev, U), boxes=_up(np.asarray(boxes).reshape(-1, 6), dev, np.float64), glia=_up(glia, dev, np.uint8))
    cs = None if cell_size is None else _up(cell_size, dev, np.float64)
    ss = None if sv_sizes is None else _up(sv_sizes, dev, np.int64)
    ptr = lambda t, n=1: t.data_ptr() if t is not None and n else None
    o = dict(node_ids=Guarded(dev, nc, U), node_cell=Guarded(dev, nc, U), node_class=Guarded(dev, nc, np.uint8), node_comp=Guarded(dev, nc, U),
             node_size1=Guarded(dev, nc, np.float64), node_size2=Guarded(dev, nc, np.float64), cell_ids=Guarded(dev, nc, U), cell_outcome=Guarded(dev, nc, np.uint8))
    tabs = [dict(cc_ids=Guarded(dev, nc, U), cc_cell=Guarded(dev, nc, U), sv_begin=Guarded(dev, nc + 1, np.int64), sv_ids=Guarded(dev, nc, U)) for _ in range(2)]
    e_n, e_g = Guarded(dev, 2 * ec, U), Guarded(dev, 2 * ec, U)
    counts = Guarded(dev, 16, np.int64)
    need = lib.sd_glia_split_temp_bytes(n_ids, n_e, n_x)
    tmp = Guarded(dev, need, np.uint8)
    order = ('node_ids', 'node_cell', 'node_class', 'node_comp', 'node_size1', 'node_size2', 'cell_ids', 'cell_outcome')
    rc = lib.sd_glia_split(ptr(d['e'], n_e), n_e, ptr(d['x'], n_x), n_x, ptr(d['ids'], n_ids), ptr(d['boxes'], n_ids), ptr(d['glia'], n_ids), n_ids, float(T),
                           ptr(cs), float(min_cell_size), ptr(ss), nc, ec, *[o[k].ptr() for k in order],
                           *[t[k].ptr() for t in tabs for k in ('cc_ids', 'cc_cell', 'sv_begin', 'sv_ids')], e_n.ptr(), e_g.ptr(), counts.ptr(),
                           None if null_scratch else tmp.ptr(), max(need - shrink, 0), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    every = list(o.values()) + [g for t in tabs for g in t.values()] + [e_n, e_g, counts, tmp]
    assert all(g.intact() for g in every), 'the device wrote behind a buffer it was given'
    c = counts.host(16).copy()
    cut = lambda v, cap: int(min(max(int(v), 0), cap))
    n, n_cells = cut(c[0], nc), cut(c[1], nc)
    out = {k: o[k].host(n if k.startswith('node') else n_cells).copy() for k in order}
    for key, t, a, b in (('neuron', tabs[0], 2, 3), ('glia', tabs[1], 4, 5)):
        n_cc, n_sv = cut(c[a], nc), cut(c[b], nc)
        out[key] = dict(cc_ids=t['cc_ids'].host(n_cc).copy(), cc_cell=t['cc_cell'].host(n_cc).copy(), sv_begin=t['sv_begin'].host(n_cc + 1).copy(),
                        sv_ids=t['sv_ids'].host(n_sv).copy())
    out['neuron_edges'] = e_n.host(2 * cut(c[6], ec)).copy().reshape(-1, 2)
    out['astrocyte_edges'] = e_g.host(2 * cut(c[8], ec)).copy().reshape(-1, 2)
    return rc, c, out


def pred(dev, probas, view_begin, thresh, point_model):
    """-> (rc, counts, classes, means)"""
    lib = L.load()
    p = np.ascontiguousarray(probas)
    vb = np.asarray(view_begin, np.int64)
    n = len(vb) - 1
    p_d, vb_d = torch.from_numpy(p).to(dev), torch.from_numpy(vb).to(dev)
    cls, mean, counts = Guarded(dev, n, np.uint8), Guarded(dev, n, np.float64), Guarded(dev, 8, np.int64)
    rc = lib.sd_glia_pred(p_d.data_ptr() if len(p) else None, int(p.dtype == np.float64), vb_d.data_ptr(), n, len(p), float(thresh), int(point_model), cls.ptr(),
                          mean.ptr(), counts.ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert cls.intact() and mean.intact() and counts.intact()
    return rc, counts.host(8).copy(), cls.host(n).copy(), mean.host(n).copy()
