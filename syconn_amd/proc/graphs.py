"""Connected components of the supervoxel graph and their size filter: what ``run_create_rag`` (/root/reference/syconn/exec/
exec_init.py:299-367), the ``apply_ssv_size_threshold`` branch of ``run_create_neuron_ssd`` (:61-80) and ``create_ccsize_dict``
(/root/reference/syconn/proc/graphs.py:220-249) do with networkx, node by node, as one device call over tables in memory
(``sd_svgraph_components``).  No CPU fallback; no edge-list files: edges arrive as an ``(e, 2)`` uint64 array."""
import numpy as np

from .. import _dev as D

INT32_MAX = 2 ** 31 - 1


def _u64(what, a, cols=None):
    a = np.asarray(a)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f'{what} must be integers, got {a.dtype}')
    if a.size and a.dtype != np.uint64 and a.min() < 0:
        raise ValueError(f'{what} must not be negative')
    if cols is not None:
        if a.size % cols or (a.ndim == 2 and a.shape[1] != cols and a.size):
            raise ValueError(f'{what} must have the shape (n, {cols})')
        a = a.reshape(-1, cols)
    else:
        a = a.reshape(-1)
    return np.ascontiguousarray(a, dtype=np.uint64)


def _i32(what, a, shape):
    a = np.asarray(a).reshape(shape)
    if a.size and (a.min() <= -INT32_MAX or a.max() >= INT32_MAX):
        raise ValueError(f'{what} must fit int32')
    return np.ascontiguousarray(a, dtype=np.int32)


class SvTable:
    """The supervoxel table the device entries read, uploaded once: the columns of a ``PropTable`` (``ids`` strictly ascending,
    ``sizes``, ``rep_coords``, ``boxes`` with ``box_begin``) as device tensors in the dtypes of the C ABI."""

    def __init__(self, props, device):
        ids = _u64('supervoxel ids', props.ids)
        if len(ids) > 1 and not (ids[1:] > ids[:-1]).all():
            raise ValueError('supervoxel ids must ascend strictly')
        n = len(ids)
        sizes = np.ascontiguousarray(np.asarray(props.sizes).reshape(-1), dtype=np.int64)
        box_begin = np.ascontiguousarray(np.asarray(props.box_begin).reshape(-1), dtype=np.int64)
        boxes = _i32('bounding boxes', props.boxes, (-1, 6))
        rep = _i32('representative coordinates', props.rep_coords, (-1, 3))
        if len(sizes) != n or len(rep) != n or len(box_begin) != n + 1:
            raise ValueError(f'{n} supervoxel ids, but {len(sizes)} sizes, {len(rep)} representative coordinates and {len(box_begin)} box offsets')
        if box_begin[0] != 0 or box_begin[-1] != len(boxes) or (np.diff(box_begin) < 0).any():
            raise ValueError('box_begin must ascend from 0 to the number of boxes')
        self.n, self.n_boxes, self.ids_host, self.sizes_host = n, len(boxes), ids, sizes
        self.ids, self.sizes, self.rep, self.box_begin, self.boxes = (D.up(a, device) for a in (ids, sizes, rep, box_begin, boxes))


class SvGraphComponents:
    """Result of ``svgraph_components``.  ``node_ids`` (ascending) / ``node_comp`` (the smallest id of the node's component, 0 where it
    was dropped) / ``node_size`` (float64: ``create_ccsize_dict``'s value per node); the kept cells as CSR ``ssv_ids`` (ascending),
    ``sv_begin``, ``sv_ids`` (ascending inside a cell) with ``cc_sizes`` per cell; ``edges`` = the pruned graph in input order;
    ``total_size`` = the voxels of the kept supervoxels."""

    def __init__(self, **columns):
        self.__dict__.update(columns)

    def ccsize_dict(self) -> dict:
        """node id -> size of its component, the dictionary ``create_ccsize_dict`` returns."""
        return dict(zip(self.node_ids.tolist(), self.node_size.tolist()))


def svgraph_components(edges, sv_props, scaling, min_cc_size, strict: bool = True, device=None) -> SvGraphComponents:
    """Components of the graph over the table's supervoxels and every edge endpoint (node 0 and its edges removed, a table id without
    an edge is a component of its own), the bounding box diagonal of every component in nm (``np.linalg.norm`` of the scaled extent
    of all boxes of its supervoxels, in the reference's float64 arithmetic) and the filter: components with ``size <= min_cc_size``
    are dropped (``strict=False``: with ``size < min_cc_size``).  A component none of whose supervoxels is in the table raises
    ``ValueError`` as ``create_ccsize_dict`` does.  `sv_props`: a ``PropTable``."""
    what = 'svgraph_components'
    e = _u64(f'{what}: edges', edges, cols=2)
    scaling = np.ascontiguousarray(np.asarray(scaling, dtype=np.float64).reshape(-1))
    if scaling.shape != (3,) or not (np.isfinite(scaling).all() and (scaling > 0).all()):
        raise ValueError(f'{what}: scaling must hold three positive numbers')
    if isinstance(min_cc_size, bool) or not np.isscalar(min_cc_size) or np.isnan(float(min_cc_size)):
        raise ValueError(f'{what}: min_cc_size must be a number, got {min_cc_size!r}')
    dev = D.device(device)
    tab = sv_props if isinstance(sv_props, SvTable) else SvTable(sv_props, dev)
    n_e, m = len(e), tab.n + 2 * len(e)
    e_d = D.up(e, dev)
    node_ids, node_comp, ssv_ids, sv_begin, sv_ids, edges_out = (D.empty(k, D.i64, dev) for k in (m, m, m, m + 1, m, 2 * n_e))
    node_size = D.empty(m, D.f64, dev)
    counts_d = D.counters(dev)
    tmp = D.scratch('sd_svgraph_components_temp_bytes', dev, tab.n, n_e)
    D.call('sd_svgraph_components', dev, e_d, n_e, tab.ids, tab.sizes, tab.box_begin, tab.boxes, tab.n, tab.n_boxes, D.f64x3(scaling),
           float(min_cc_size), int(bool(strict)), node_ids, node_comp, node_size, ssv_ids, sv_begin, sv_ids, edges_out, counts_d, tmp, tmp.numel())
    counts = D.down(counts_d)
    if int(counts[7]):
        raise ValueError(f'{what}: the supervoxel table is inconsistent (ids or box offsets do not ascend)')
    if int(counts[6]):
        raise ValueError(f'Could not find a single bounding box for connected component with IDs: {{{int(counts.view(np.uint64)[5])}, ...}}.')
    n, n_cells, n_sv, n_kept = (int(counts[i]) for i in range(4))
    host = lambda t, k: D.down(t, k, np.uint64)
    out = SvGraphComponents(node_ids=host(node_ids, n), node_comp=host(node_comp, n), node_size=D.down(node_size, n), ssv_ids=host(ssv_ids, n_cells),
                            sv_begin=D.down(sv_begin, n_cells + 1), sv_ids=host(sv_ids, n_sv), edges=host(edges_out, 2 * n_kept).reshape(-1, 2),
                            total_size=int(counts[4]))
    out.cc_sizes = out.node_size[np.searchsorted(out.node_ids, out.ssv_ids)] if n_cells else np.zeros(0, np.float64)
    return out


def create_ccsize_dict(edges, sv_props, scaling, device=None) -> dict:
    """``create_ccsize_dict`` (graphs.py:220-249) over the tables: node id -> bounding box diagonal of its component in nm."""
    return svgraph_components(edges, sv_props, scaling, -np.inf, device=device).ccsize_dict()
