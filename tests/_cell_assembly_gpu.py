"""The entries of csrc/sd_cell_assembly.hip through the C ABI, for tests/test_gpu_cell_assembly*.py: every call uploads numpy arrays,
runs over a scratch of exactly ``*_temp_bytes`` followed by a guard band that must stay untouched, and returns numpy arrays cut to
the counts the device reports (``raw=True``: the return code and the counts only matter)."""
import ctypes as C

import numpy as np
import torch

from syconn_amd import _lib as L

GUARD = 4096
FILL = 0xCD  # what every output and the usable scratch hold before a call (tests/test_gpu_buffer_state.py sets 0x00 / 0xFF)


def _up(a, dev, dtype):
    a = np.ascontiguousarray(np.asarray(a), dtype=dtype)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


def _scratch(dev, need, shrink=0):
    t = torch.empty(need + GUARD, dtype=torch.uint8, device=dev)
    t[:need] = FILL
    t[need:] = 0xA5
    return t, max(need - shrink, 0)


def _out(dev, shape, dtype):
    """An output of `shape` (first extent at least 1) whose every byte is FILL."""
    shape = shape if isinstance(shape, tuple) else (shape,)
    t = torch.empty((max(shape[0], 1),) + shape[1:], dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(FILL)
    return t


def _intact(t, need):
    assert bool((t[need:] == 0xA5).all()), 'the device wrote behind the scratch it asked for'


def _u64(t, n):
    return t[:n].cpu().numpy().view(np.uint64)


def table(dev, ids, sizes, rep, box_begin, boxes):
    """-> device columns of a supervoxel table in the dtypes of the C ABI (no checks: inconsistent tables are test inputs)."""
    return dict(ids=_up(ids, dev, np.uint64), sizes=_up(sizes, dev, np.int64), rep=_up(np.asarray(rep).reshape(-1, 3), dev, np.int32),
                box_begin=_up(box_begin, dev, np.int64), boxes=_up(np.asarray(boxes).reshape(-1, 6), dev, np.int32), n=len(ids),
                n_boxes=len(np.asarray(boxes).reshape(-1, 6)))


def components(dev, edges, tab, scaling, min_cc_size, strict=True, shrink=0):
    """-> (rc, counts, dict of outputs)"""
    lib = L.load()
    e = _up(np.asarray(edges, np.uint64).reshape(-1, 2), dev, np.uint64)
    n_e, m = len(e), tab['n'] + 2 * len(e)
    i64 = lambda k: _out(dev, k, torch.int64)
    node_ids, node_comp, ssv_ids, sv_begin, sv_ids, edges_out = i64(m), i64(m), i64(m), i64(m + 1), i64(m), i64(2 * n_e)
    node_size = _out(dev, m, torch.float64)
    counts = torch.zeros(8, dtype=torch.int64, device=dev)
    need = lib.sd_svgraph_components_temp_bytes(tab['n'], n_e)
    tmp, told = _scratch(dev, need, shrink)
    sc = (C.c_double * 3)(*[float(v) for v in scaling])
    rc = lib.sd_svgraph_components(e.data_ptr(), n_e, tab['ids'].data_ptr(), tab['sizes'].data_ptr(), tab['box_begin'].data_ptr(), tab['boxes'].data_ptr(),
                                   tab['n'], tab['n_boxes'], sc, float(min_cc_size), int(strict), node_ids.data_ptr(), node_comp.data_ptr(),
                                   node_size.data_ptr(), ssv_ids.data_ptr(), sv_begin.data_ptr(), sv_ids.data_ptr(), edges_out.data_ptr(), counts.data_ptr(),
                                   tmp.data_ptr(), told, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    _intact(tmp, need)
    c = counts.cpu().numpy()
    n, n_cells, n_sv, n_kept = (int(min(max(v, 0), m)) for v in c[:4])
    return rc, c, dict(node_ids=_u64(node_ids, n), node_comp=_u64(node_comp, n), node_size=node_size[:n].cpu().numpy(), ssv_ids=_u64(ssv_ids, n_cells),
                       sv_begin=sv_begin[:n_cells + 1].cpu().numpy(), sv_ids=_u64(sv_ids, n_sv), edges=_u64(edges_out, 2 * min(n_kept, n_e)).reshape(-1, 2),
                       total_size=int(c[4]))


def props(dev, sv_begin, sv_ids, tab):
    """-> (rc, counts, size, box (n, 2, 3), rep)"""
    lib = L.load()
    n = len(sv_begin) - 1
    sb, sv = _up(sv_begin, dev, np.int64), _up(sv_ids, dev, np.uint64)
    size = _out(dev, n, torch.int64)
    box = _out(dev, (n, 6), torch.int32)
    rep = _out(dev, (n, 3), torch.int32)
    counts = torch.zeros(8, dtype=torch.int64, device=dev)
    rc = lib.sd_cell_props(sb.data_ptr(), sv.data_ptr(), n, len(sv_ids), tab['ids'].data_ptr(), tab['sizes'].data_ptr(), tab['rep'].data_ptr(),
                           tab['box_begin'].data_ptr(), tab['boxes'].data_ptr(), tab['n'], tab['n_boxes'], size.data_ptr(), box.data_ptr(), rep.data_ptr(),
                           counts.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return rc, counts.cpu().numpy(), size[:n].cpu().numpy(), box[:n].cpu().numpy().reshape(n, 2, 3), rep[:n].cpu().numpy()


def mapping(dev, sv_begin, sv_ids, rec_sub, rec_sv, rec_count, org_ids, org_sizes, lower, upper, thresh, shrink=0):
    """-> (rc, counts, dict of outputs; org_first_cell as rows, -1 = none)"""
    lib = L.load()
    r, o, n, s = len(rec_sub), len(org_ids), len(sv_begin) - 1, len(sv_ids)
    d = [_up(a, dev, t) for a, t in ((rec_sub, np.uint64), (rec_sv, np.uint64), (rec_count, np.int64), (org_ids, np.uint64), (org_sizes, np.int64),
                                     (sv_begin, np.int64), (sv_ids, np.uint64))]
    i64 = lambda k: _out(dev, k, torch.int64)
    cell_begin, pair_org, acc_begin, acc_org = i64(n + 1), i64(r), i64(n + 1), i64(r)
    ratio = _out(dev, r, torch.float64)
    accepted = _out(dev, r, torch.uint8)
    org_n, org_first = (_out(dev, o, torch.int32) for _ in range(2))
    counts = torch.zeros(8, dtype=torch.int64, device=dev)
    need = lib.sd_cell_mapping_temp_bytes(r, s)
    tmp, told = _scratch(dev, need, shrink)
    rc = lib.sd_cell_mapping(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), r, d[3].data_ptr(), d[4].data_ptr(), o, d[5].data_ptr(), d[6].data_ptr(), n, s,
                             float(lower), float(upper), float(thresh), cell_begin.data_ptr(), pair_org.data_ptr(), ratio.data_ptr(), accepted.data_ptr(),
                             acc_begin.data_ptr(), acc_org.data_ptr(), org_n.data_ptr(), org_first.data_ptr(), counts.data_ptr(), tmp.data_ptr(), told,
                             torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    _intact(tmp, need)
    c = counts.cpu().numpy()
    n_pairs, n_acc = int(min(max(c[1], 0), r)), int(min(max(c[2], 0), r))
    return rc, c, dict(cell_begin=cell_begin[:n + 1].cpu().numpy(), ids=_u64(pair_org, n_pairs), ratios=ratio[:n_pairs].cpu().numpy(),
                       accepted=accepted[:n_pairs].cpu().numpy().astype(bool), acc_begin=acc_begin[:n + 1].cpu().numpy(), acc_ids=_u64(acc_org, n_acc),
                       org_n_cells=org_n[:o].cpu().numpy().astype(np.int64), org_first_cell=org_first[:o].cpu().numpy().astype(np.int64))


def synapses(dev, ssv_ids, partners, keep, syn_ids, shrink=0):
    """-> (rc, counts, syn_begin, out_ids)"""
    lib = L.load()
    n, n_cells = len(syn_ids), len(ssv_ids)
    d = [_up(a, dev, t) for a, t in ((np.asarray(partners).reshape(-1, 2), np.uint64), (keep, np.uint8), (syn_ids, np.uint64), (ssv_ids, np.uint64))]
    begin = _out(dev, n_cells + 1, torch.int64)
    out = _out(dev, 2 * n, torch.int64)
    counts = torch.zeros(8, dtype=torch.int64, device=dev)
    need = lib.sd_cell_synapses_temp_bytes(n)
    tmp, told = _scratch(dev, need, shrink)
    rc = lib.sd_cell_synapses(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, d[3].data_ptr(), n_cells, begin.data_ptr(), out.data_ptr(), counts.data_ptr(),
                              tmp.data_ptr(), told, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    _intact(tmp, need)
    c = counts.cpu().numpy()
    return rc, c, begin.cpu().numpy(), _u64(out, int(min(max(c[0], 0), 2 * n)))
