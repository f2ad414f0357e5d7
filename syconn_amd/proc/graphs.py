"""Connected components of the supervoxel graph and their size filter: what ``run_create_rag`` (/root/reference/syconn/exec/
exec_init.py:299-367), the ``apply_ssv_size_threshold`` branch of ``run_create_neuron_ssd`` (:61-80) and ``create_ccsize_dict``
(/root/reference/syconn/proc/graphs.py:220-249) do with networkx, node by node, as one device call over tables in memory
(``sd_svgraph_components``).  No CPU fallback; no edge-list files: edges arrive as an ``(e, 2)`` uint64 array.

Astrocyte splitting: ``remove_glia_nodes`` (graphs.py:278-360) behind ``split_glia_graph`` (:173-195) for ALL cells of a graph in one
device call (``sd_glia_split``, ``split_glia_table``), the supervoxel glia decision ``glia_pred_so`` / ``glia_proba_so`` (reps/
segmentation_helper.py:32-78, ``glia_pred``) and drop-ins of the two reference functions over one cell."""
import numpy as np

from .. import _dev as D
from .. import global_params

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


# ---- astrocyte splitting ---------------------------------------------------------------------------------------------------------
def glia_pred(probas, view_begin, thresh=None, use_point_models=None, device=None):
    """``SegmentationObject.glia_pred`` / ``glia_proba`` (segmentation.py:799-828, segmentation_helper.py:32-78) for a table of supervoxels:
    `probas` = column 1 of every supervoxel's ``glia_probas`` one after another (float32 or float64), supervoxel i owning
    ``probas[view_begin[i]:view_begin[i + 1]]``.  -> ``(classes uint8, means float64)``.  Multi-view models: glia when ``mean > thresh``
    and more than ``int(n_views * 0.7)`` views are ``> thresh``; point models (default ``config['use_point_models']``): ``mean >= thresh``.
    A supervoxel without views is a neuron with mean NaN.  The mean is the float64 sum in view order divided once (numpy: pairwise in the
    input dtype; the two agree whenever the sum is exact).  `thresh` defaults to ``config['glia']['glia_thresh']``."""
    what = 'glia_pred'
    p = np.asarray(probas)
    if p.dtype not in (np.float32, np.float64):
        raise ValueError(f'{what}: probabilities must be float32 or float64, got {p.dtype}')
    p = np.ascontiguousarray(p.reshape(-1))
    vb = np.ascontiguousarray(np.asarray(view_begin).reshape(-1), dtype=np.int64)
    if len(vb) < 1 or vb[0] != 0 or vb[-1] != len(p) or (np.diff(vb) < 0).any():
        raise ValueError(f'{what}: view_begin must ascend from 0 to the number of views')
    if thresh is None:
        thresh = global_params.config['glia']['glia_thresh']
    if isinstance(thresh, bool) or not np.isscalar(thresh) or np.isnan(float(thresh)):
        raise ValueError(f'{what}: thresh must be a number, got {thresh!r}')
    if use_point_models is None:
        use_point_models = bool(global_params.config['use_point_models'])
    n = len(vb) - 1
    dev = D.device(device)
    cls, mean, counts_d = D.empty(n, D.u8, dev), D.empty(n, D.f64, dev), D.counters(dev)
    D.call('sd_glia_pred', dev, D.up(p, dev) if len(p) else None, int(p.dtype == np.float64), D.up(vb, dev), n, len(p), float(thresh),
           int(bool(use_point_models)), cls, mean, counts_d)
    if int(D.down(counts_d)[7]):
        raise ValueError(f'{what}: view_begin must ascend from 0 to the number of views')
    return D.down(cls, n), D.down(mean, n)


class GliaSplit:
    """Result of ``split_glia_table``.  Per node, ascending by id: ``node_ids``, ``node_cell`` (the smallest id of its cell), ``node_class``
    (0 neuron, 1 glia), ``node_comp`` (the smallest id of its final component), ``node_size1`` (the size of its same-class component in
    steps 1 / 2 of ``remove_glia_nodes``), ``node_size2`` (its size among neurons and tiny glia fragments in step 3, NaN where it took no
    part).  Per cell, ascending: ``cell_ids``, ``cell_outcome`` (1: no significant neuron component, all glia; 2: no significant glia
    component, all neuron; 3: split).  ``neuron`` / ``glia``: ``GliaComponents`` (CSR).  ``neuron_edges`` / ``astrocyte_edges``: the input
    edges inside one class, in input order (a neuron node whose neighbours all became glia is in ``neuron`` and, without a self loop, in no
    edge).  ``n_cells_by_outcome`` (three numbers), ``astrocyte_size`` (voxels, 0 without `sv_sizes`)."""

    def __init__(self, **columns):
        self.__dict__.update(columns)

    def as_lists(self):
        """Per cell (ascending by id): ``(neuron_ccs, glia_ccs)`` as ``remove_glia_nodes(..., return_removed_nodes=True)`` gives them,
        every component a uint64 array ascending."""
        out = [([], []) for _ in self.cell_ids]
        for k, t in enumerate((self.neuron, self.glia)):
            for c, a, b in zip(np.searchsorted(self.cell_ids, t.cc_cell), t.sv_begin[:-1], t.sv_begin[1:]):
                out[c][k].append(t.sv_ids[a:b])
        return out


class GliaComponents:
    """Components of one class in CSR form: ``cc_ids`` (ascending; the smallest supervoxel id), ``cc_cell`` (the cell they came from),
    ``sv_begin``, ``sv_ids`` (ascending inside a component)."""

    def __init__(self, cc_ids, cc_cell, sv_begin, sv_ids):
        self.cc_ids, self.cc_cell, self.sv_begin, self.sv_ids = cc_ids, cc_cell, sv_begin, sv_ids

    def __len__(self):
        return len(self.cc_ids)


def _column(what, a, n, dtype):
    a = np.asarray(a).reshape(-1)
    if len(a) != n:
        raise ValueError(f'{what}: {len(a)} entries for {n} supervoxels')
    return np.ascontiguousarray(a, dtype=dtype)


def split_glia_table(edges, sv_ids, boxes_nm, glia, min_cc_size=None, nodes=None, cell_size=None, min_cell_size=None, sv_sizes=None,
                     device=None) -> GliaSplit:
    """``remove_glia_nodes`` for every cell (component) of the graph `edges` (+ `nodes` without an edge) in one device call.  The supervoxel
    table: `sv_ids` strictly ascending, `boxes_nm` ``(n, 2, 3)`` in nm (``mesh_bb``; float32 is widened, which is exact), `glia` 0 / 1.
    `min_cc_size` defaults to ``config['min_cc_size_ssv']``.  With `cell_size` (per table row: the size of the supervoxel's ORIGINAL cell)
    and `min_cell_size`, supervoxels of cells below it leave the edge arrays and component lists as in ``write_astrocyte_svgraph``
    (glia_splitting.py:125-127, :147-149).  `sv_sizes` (voxels per table row) gives ``astrocyte_size``.  A node that is not in the table
    raises ``KeyError`` as ``glia_dict[n]`` does."""
    what = 'split_glia_table'
    e = _u64(f'{what}: edges', edges, cols=2)
    extra = _u64(f'{what}: nodes', [] if nodes is None else nodes)
    ids = _u64(f'{what}: supervoxel ids', sv_ids)
    if len(ids) > 1 and not (ids[1:] > ids[:-1]).all():
        raise ValueError(f'{what}: supervoxel ids must ascend strictly')
    n_ids = len(ids)
    boxes = np.asarray(boxes_nm)
    if boxes.size != 6 * n_ids:
        raise ValueError(f'{what}: boxes must have the shape ({n_ids}, 2, 3), got {boxes.shape}')
    if boxes.size and not np.issubdtype(boxes.dtype, np.floating) and not np.issubdtype(boxes.dtype, np.integer):
        raise ValueError(f'{what}: boxes must be numbers, got {boxes.dtype}')
    boxes = np.ascontiguousarray(boxes.reshape(-1, 6), dtype=np.float64)
    if not np.isfinite(boxes).all():
        raise ValueError(f'{what}: boxes must be finite')
    g = (_column(f'{what}: glia', glia, n_ids, np.int64) != 0).astype(np.uint8)
    if min_cc_size is None:
        min_cc_size = global_params.config['min_cc_size_ssv']
    if isinstance(min_cc_size, bool) or not np.isscalar(min_cc_size) or np.isnan(float(min_cc_size)):
        raise ValueError(f'{what}: min_cc_size must be a number, got {min_cc_size!r}')
    if (cell_size is None) != (min_cell_size is None):
        raise ValueError(f'{what}: pass cell_size and min_cell_size together')
    if cell_size is not None:
        cell_size = _column(f'{what}: cell_size', cell_size, n_ids, np.float64)
        if np.isnan(cell_size).any() or np.isnan(float(min_cell_size)):
            raise ValueError(f'{what}: cell sizes must not be NaN')
    if sv_sizes is not None:
        sv_sizes = _column(f'{what}: sv_sizes', sv_sizes, n_ids, np.int64)
    dev = D.device(device)
    n_e, n_x = len(e), len(extra)
    m = 2 * n_e + n_x
    opt = lambda a: None if a is None or not len(a) else D.up(a, dev)
    u64s = lambda k: D.empty(k, D.i64, dev)
    node_ids, node_cell, node_comp, cell_ids = u64s(m), u64s(m), u64s(m), u64s(m)
    node_class, cell_outcome = D.empty(m, D.u8, dev), D.empty(m, D.u8, dev)
    size1, size2 = D.empty(m, D.f64, dev), D.empty(m, D.f64, dev)
    tables = [(u64s(m), u64s(m), u64s(m + 1), u64s(m)) for _ in range(2)]
    e_n, e_g = u64s(2 * n_e), u64s(2 * n_e)
    counts_d = D.counters(dev, 16)
    tmp = D.scratch('sd_glia_split_temp_bytes', dev, n_ids, n_e, n_x)
    D.call('sd_glia_split', dev, opt(e), n_e, opt(extra), n_x, opt(ids), opt(boxes), opt(g), n_ids, float(min_cc_size), opt(cell_size),
           float(0.0 if min_cell_size is None else min_cell_size), opt(sv_sizes), m, n_e, node_ids, node_cell, node_class, node_comp, size1, size2,
           cell_ids, cell_outcome, *tables[0], *tables[1], e_n, e_g, counts_d, tmp, tmp.numel())
    counts = D.down(counts_d)
    if int(counts[7]):
        raise ValueError(f'{what}: supervoxel ids must ascend strictly')
    if int(counts[10]):
        raise KeyError(int(counts.view(np.uint64)[11]))
    if int(counts[12]):
        raise RuntimeError(f'{what}: the device reports lost records')
    n, n_cells = int(counts[0]), int(counts[1])
    host = lambda t, k: D.down(t, k, np.uint64)
    comps = [GliaComponents(host(t[0], int(counts[a])), host(t[1], int(counts[a])), D.down(t[2], int(counts[a]) + 1), host(t[3], int(counts[b])))
             for t, a, b in ((tables[0], 2, 3), (tables[1], 4, 5))]
    return GliaSplit(node_ids=host(node_ids, n), node_cell=host(node_cell, n), node_class=D.down(node_class, n), node_comp=host(node_comp, n),
                     node_size1=D.down(size1, n), node_size2=D.down(size2, n), cell_ids=host(cell_ids, n_cells),
                     cell_outcome=D.down(cell_outcome, n_cells), neuron=comps[0], glia=comps[1],
                     neuron_edges=host(e_n, 2 * int(counts[6])).reshape(-1, 2), astrocyte_edges=host(e_g, 2 * int(counts[8])).reshape(-1, 2),
                     n_cells_by_outcome=tuple(int(v) for v in counts[13:16]), astrocyte_size=int(counts[9]))


def _graph_arrays(what, g):
    """-> (edges (e, 2) uint64, nodes uint64) of an ``nx.Graph`` with integer node keys or of an ``(e, 2)`` array."""
    if hasattr(g, 'edges') and hasattr(g, 'nodes'):
        return _u64(f'{what}: edges', [(int(a), int(b)) for a, b in g.edges()], cols=2), _u64(f'{what}: nodes', [int(n) for n in g.nodes()])
    e = _u64(f'{what}: edges', g, cols=2)
    return e, np.zeros(0, np.uint64)


def remove_glia_nodes(g, size_dict, glia_dict, return_removed_nodes=False, device=None):
    """Drop-in of ``remove_glia_nodes`` (graphs.py:278-360) for ONE connected cell `g` (an ``nx.Graph`` or an ``(e, 2)`` array, integer
    node keys): `size_dict` node -> ``(2, 3)`` box in nm, `glia_dict` node -> 0 / 1, the threshold ``config['min_cc_size_ssv']``.  Returns
    the neuron components (with `return_removed_nodes` also the glia components) as the reference does: ``[]`` / ``[all nodes]`` at the two
    early returns, else a list of sets per class.  Many cells at once: ``split_glia_table``."""
    what = 'remove_glia_nodes'
    e, nodes = _graph_arrays(what, g)
    universe = np.unique(np.concatenate([e.reshape(-1), nodes]))
    for n in universe.tolist():                                                    # a node without a box raises too (the reference leaves it out of the sizes)
        if n not in glia_dict or n not in size_dict:
            raise KeyError(n)
    boxes = np.array([np.asarray(size_dict[n], dtype=np.float64).reshape(2, 3) for n in universe.tolist()], np.float64).reshape(-1, 2, 3)
    res = split_glia_table(e, universe, boxes, [glia_dict[n] for n in universe.tolist()], nodes=nodes, device=device)
    if len(res.cell_ids) > 1:
        raise ValueError(f'{what}: the graph holds {len(res.cell_ids)} cells; it takes one connected cell (split_glia_table takes many)')
    all_nodes = [int(n) for n in g.nodes()] if hasattr(g, 'nodes') else universe.tolist()
    if len(res.cell_ids) == 0:
        neuron_ccs, glia_ccs = [], [all_nodes]                                    # np.all of nothing: the first early return
    elif res.cell_outcome[0] == 1:
        neuron_ccs, glia_ccs = [], [all_nodes]
    elif res.cell_outcome[0] == 2:
        neuron_ccs, glia_ccs = [all_nodes], []
    else:
        neuron_ccs, glia_ccs = ([set(x.tolist()) for x in k] for k in res.as_lists()[0])
    return (neuron_ccs, glia_ccs) if return_removed_nodes else neuron_ccs


def split_glia_graph(nx_g, thresh, sv_ids, boxes_nm, probas, view_begin, use_point_models=None, device=None):
    """``split_glia_graph`` (graphs.py:173-195) for one cell over tables instead of ``SegmentationObject`` storages: the glia decision of
    every supervoxel (``glia_pred`` with `thresh`) and its ``mesh_bb`` come from the table `sv_ids` / `boxes_nm` / `probas` / `view_begin`.
    -> ``(neuron_ccs, glia_ccs)``."""
    ids = _u64('split_glia_graph: supervoxel ids', sv_ids)
    cls, _ = glia_pred(probas, view_begin, thresh, use_point_models, device)
    boxes = np.asarray(boxes_nm).reshape(-1, 2, 3)
    if len(cls) != len(ids) or len(boxes) != len(ids):
        raise ValueError(f'split_glia_graph: {len(ids)} supervoxel ids, but {len(boxes)} boxes and {len(cls)} view lists')
    return remove_glia_nodes(nx_g, dict(zip(ids.tolist(), boxes)), dict(zip(ids.tolist(), cls.tolist())), return_removed_nodes=True, device=device)
