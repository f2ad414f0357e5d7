"""Drop-ins for the functions of ``syconn.reps.super_segmentation_helper`` that consume the dense path's output or smooth it along
the skeletons.  ``map_myelin2coords`` (/root/reference/syconn/reps/super_segmentation_helper.py:550-615; SURVEY.md
section 8f row 3): same name, arguments, return value and error behaviour; the per-node ``kd.load_raw`` + numpy
reduction of the reference (one 11x11x5 box read per skeleton node) becomes: read the region the nodes cover once,
keep it on the GPU, one wave per node (``sd_box_majority``).  ``majorityvote_skeleton_property`` (:1270-1302) and
``majority_vote_compartments`` (:1233-1266): one Dijkstra per node and one ``np.unique`` per node or component become
``skeleton_majority_vote`` / ``skeleton_compartment_majority`` over all cells of a call (``sd_skel_*``).  No CPU fallback.
"""
import os

import numpy as np
import torch

from .. import _dev as D
from .. import _lib as L
from .. import global_params
from ..handler.basics import kd_factory

_REGION_VOX = 768          # nodes are processed in spatial buckets of this many mag-voxels per axis (<= ~0.5 GB each)


def box_majority_device(vol: torch.Tensor, origins_zyx: torch.Tensor, edge_zyx, thresh_proba: float,
                        thresh_majority: float) -> torch.Tensor:
    """out[i] = (count(vol[box_i] > thresh_proba) / prod(edge) > thresh_majority) on the device; boxes may leave the
    volume (zeros outside).  vol: (D,H,W) uint8, origins_zyx: (n,3) int32, both on the same ROCm device."""
    L.load()                                   # (a library that was not built is reported first)
    if not (vol.is_cuda and origins_zyx.is_cuda):
        raise RuntimeError('box_majority_device needs device tensors (there is no CPU fallback)')
    assert vol.dtype == torch.uint8 and vol.dim() == 3 and vol.is_contiguous()
    origins_zyx = origins_zyx.to(torch.int32).contiguous()
    n = int(origins_zyx.shape[0])
    out = torch.empty((n,), dtype=torch.uint8, device=vol.device)
    # (dev None: the current stream of the current device)
    D.call('sd_box_majority', None, vol, *(int(v) for v in vol.shape), origins_zyx, n, int(edge_zyx[0]), int(edge_zyx[1]), int(edge_zyx[2]),
           float(thresh_proba), float(thresh_majority), out)
    return out


def map_myelin2coords(coords: np.ndarray, cube_edge_avg: np.ndarray = np.array([11, 11, 5]),
                      thresh_proba: float = 255 // 2, thresh_majority: float = 0.5, mag: int = 4) -> np.ndarray:
    """Myelin prediction (0 / 1, uint8) at every coordinate (mag-1 voxels, x,y,z): majority of ``myelin > thresh_proba``
    inside a box of `cube_edge_avg` mag-`mag` voxels around it, read from
    ``<working_dir>/knossosdatasets/myelin/`` (super_segmentation_helper.py:550-615)."""
    myelin_kd_p = global_params.config.working_dir + "/knossosdatasets/myelin/"
    if not os.path.isdir(myelin_kd_p):
        raise ValueError(f'Could not find myelin KnossosDataset at {myelin_kd_p}.')
    if not torch.cuda.is_available():
        raise RuntimeError('syconn_amd.map_myelin2coords needs an MI355X (there is no CPU fallback)')
    kd = kd_factory(myelin_kd_p)
    coords = np.asarray(coords)
    preds = np.zeros((len(coords)), dtype=np.uint8)
    if len(coords) == 0:
        return preds
    edge = np.asarray(cube_edge_avg, dtype=np.int64)
    # reference: offset = c - (edge*mag)//2 (mag-1 voxels); kd.load_raw(size=edge*mag, offset, mag) reads `edge`
    # voxels from floor(offset / mag) in the mag-`mag` volume
    off = np.floor_divide(coords.astype(np.int64) - (edge * mag) // 2, mag)          # (n,3) x,y,z at `mag`
    dev = torch.device('cuda', torch.cuda.current_device())
    _, inv = np.unique(np.floor_divide(off, _REGION_VOX), axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    for k in range(int(inv.max()) + 1):
        ix = np.nonzero(inv == k)[0]
        lo = off[ix].min(axis=0)
        hi = off[ix].max(axis=0) + edge
        vol = kd.load_raw(size=(hi - lo) * mag, offset=lo * mag, mag=mag)              # (z,y,x) uint8, zeros outside
        vol_dev = D.up(vol, dev)
        org = D.up((off[ix] - lo)[:, ::-1].astype(np.int32), dev)
        res = box_majority_device(vol_dev, org, edge[::-1], thresh_proba, thresh_majority)
        preds[ix] = res.cpu().numpy()
    return preds


def extract_spinehead_volume_mesh(sso, ctx_vol=(200, 200, 100)):
    """Drop-in for ``extract_spinehead_volume_mesh`` (/root/reference/syconn/reps/super_segmentation_helper.py:2068-2198): fills
    ``sso.attr_dict['spinehead_vol']`` = {syn_ssv id: spine head volume in um^3} for one cell.  Reads what the reference reads of a
    (duck-typed) ``sso``: ``attr_dict`` / ``load_attr_dict``, ``scaling``, ``id``, ``label_dict('vertex')['spiness']``, ``sv_ids``,
    ``syn_ssv`` (``rep_coord``, ``id``), ``mesh[1]``, ``skeleton`` (``nodes`` and the averaged axoness key, what ``attr_for_coords``
    looks up), ``config`` (``['spines']['semseg2coords_spines']``, ``['compartments']``, ``kd_seg_path``).  The windows run on the
    device (``cs_processing_steps.calculate_spinehead_volume``); no CPU fallback."""
    from ..extraction.cs_processing_steps import CellTable, calculate_spinehead_volume
    if len(sso.attr_dict) == 0:
        sso.load_attr_dict()
    sso.attr_dict['spinehead_vol'] = {}
    labels = sso.label_dict('vertex')
    if 'spiness' not in labels:
        raise ValueError(f'"spiness" not available in skeleton of SSO {sso.id}.')
    syns = list(sso.syn_ssv)
    if len(syns) == 0:
        return
    cfg = sso.config
    sp = cfg['spines']['semseg2coords_spines']
    ax_key = "{}_avg{}".format(cfg['compartments']['view_properties_semsegax']['semseg_key'], cfg['compartments']['dist_axoness_averaging'])
    skel = getattr(sso, 'skeleton', None) or {}
    nodes = np.asarray(skel.get('nodes', np.zeros((0, 3)))).reshape(-1, 3)
    attrs = {ax_key: np.asarray(skel[ax_key]).reshape(-1)} if ax_key in skel and len(nodes) else {}
    verts = np.asarray(sso.mesh[1]).reshape(-1, 3)
    cells = CellTable([sso.id], verts, [0, len(verts)], {'spiness': labels['spiness']}, nodes, [0, len(nodes)], attrs)
    sv = np.asarray(sso.sv_ids, dtype=np.uint64).reshape(-1)
    kd_path = cfg.kd_seg_path
    kd = kd_factory(kd_path) if isinstance(kd_path, (str, os.PathLike)) else kd_path
    syn_ids = np.array([syn.id for syn in syns], np.uint64)
    rep = np.array([syn.rep_coord for syn in syns]).reshape(-1, 3)
    partners = np.stack([np.full(len(syns), sso.id, np.uint64), np.full(len(syns), sso.id, np.uint64)], 1)
    _, ids, vols = calculate_spinehead_volume(cells, [0, len(sv)], sv, syn_ids, rep, partners, kd, scaling=sso.scaling, ctx_vol=ctx_vol, k=sp['k'],
                                              ignore_labels=sp['ignore_labels'], ds_vertices=sp['ds_vertices'], ax_key=ax_key)
    for i, v in zip(ids.tolist(), vols.tolist()):
        sso.attr_dict['spinehead_vol'][i] = v


# -- majority votes along skeletons ------------------------------------------------------------------------------------------
def _skel_graph(what, n_nodes, node_begin, edges, edge_begin):
    """Checked offsets and edges -> (node_begin int64, edges int64 (e, 2), edge_begin int64, row of the cell of every edge)."""
    from ..extraction.cs_processing_steps import _check_offsets
    node_begin = np.ascontiguousarray(node_begin, dtype=np.int64).reshape(-1)
    edge_begin = np.ascontiguousarray(edge_begin, dtype=np.int64).reshape(-1)
    n_cells = len(node_begin) - 1
    if n_cells < 0:
        raise ValueError(f'{what}: node_begin must hold cells + 1 offsets')
    e = np.asarray(edges)
    if e.size and not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f'{what}: edges must be integers, got {e.dtype}')
    if e.size % 2 or (e.ndim == 2 and e.shape[1] != 2 and e.size):
        raise ValueError(f'{what}: edges must have the shape (e, 2)')
    if e.size and e.dtype == np.uint64 and e.max() >= 2 ** 63:
        raise ValueError(f'{what}: an edge names a node outside its cell')
    e = np.ascontiguousarray(e.reshape(-1, 2), dtype=np.int64)
    _check_offsets(f'{what}: node_begin', node_begin, n_cells, n_nodes)
    _check_offsets(f'{what}: edge_begin', edge_begin, n_cells, len(e))
    cell_of = np.repeat(np.arange(n_cells), np.diff(edge_begin))
    size = np.diff(node_begin)[cell_of]
    if len(e) and ((e < 0) | (e >= size[:, None])).any():
        raise ValueError(f'{what}: an edge names a node outside its cell')
    return node_begin, e, edge_begin, cell_of


def _dense_classes(what, labels, n_nodes, extra=()):
    """Integer labels -> (their sorted distinct values, with `extra`; the uint8 class of every node)."""
    lab = np.asarray(labels)
    if lab.size and not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f'{what}: labels must be integers, got {lab.dtype} (float-valued properties are not supported)')
    if lab.size != n_nodes or (lab.ndim > 1 and lab.shape[0] != n_nodes):
        raise ValueError(f'{what}: {n_nodes} nodes, labels of shape {lab.shape}')
    lab = lab.reshape(-1)
    values = np.unique(lab)
    for x in extra:
        if x not in values:
            values = np.unique(np.concatenate([values, np.array([x], values.dtype)]))
    if len(values) > L.SD_SKEL_MAX_CLASSES:
        raise ValueError(f'{what}: {len(values)} distinct labels, at most {L.SD_SKEL_MAX_CLASSES} classes are supported')
    return values, np.searchsorted(values, lab).astype(np.uint8), lab


def skeleton_edge_weights(nodes, node_begin, edges, edge_begin, scaling) -> np.ndarray:
    """The edge weights of ``weighted_graph`` (super_segmentation_object.py:1440-1444) for all cells: ``np.linalg.norm`` of the
    difference of the end points of ``nodes * scaling``, in the dtypes the caller passes; `edges` index the nodes of their cell."""
    nodes = np.asarray(nodes)
    node_begin, e, edge_begin, cell_of = _skel_graph('skeleton_edge_weights', len(nodes), node_begin, edges, edge_begin)
    node_scaled = nodes * scaling
    edge_coords = node_scaled[e + node_begin[cell_of][:, None]]
    return np.linalg.norm(edge_coords[:, 0] - edge_coords[:, 1], axis=1)


def _skel_counts(name, counts_d):
    counts = D.down(counts_d)
    if int(counts[7]):
        raise RuntimeError(f'{name}: an offset, an edge or a weight was out of range')
    return counts


def skeleton_majority_vote(nodes, node_begin, edges, edge_begin, labels, scaling, max_dist=10000, device=None, return_reached=False,
                           return_counts=False):
    """``majorityvote_skeleton_property`` (:1270-1302) for all cells at once.  Cell c owns ``nodes[node_begin[c]:node_begin[c + 1]]``
    ((n, 3), voxels) and ``edges[edge_begin[c]:edge_begin[c + 1]]`` ((e, 2) integers: node indices INSIDE the cell).  An edge weighs
    ``np.linalg.norm`` of its end points in ``nodes * scaling`` (computed here on the host with the caller's dtypes, widened to
    float64); the window of a node holds the nodes whose shortest-path distance (float64 sums from the source on) is ``<= max_dist``;
    the result is the most frequent of the integer `labels` in the window, the smallest on equal counts, in the dtype of `labels`.
    At most 64 distinct labels.  With `return_reached` also the window sizes (uint32), with `return_counts` the device's counters."""
    what = 'skeleton_majority_vote'
    nodes = np.asarray(nodes)
    if nodes.ndim != 2 or nodes.shape[1] != 3:
        if nodes.size:
            raise ValueError(f'{what}: nodes must have the shape (n, 3), got {nodes.shape}')
        nodes = nodes.reshape(0, 3)
    scaling = np.asarray(scaling)
    if scaling.shape != (3,) or not np.isfinite(scaling.astype(np.float64)).all():
        raise ValueError(f'{what}: scaling must hold three finite numbers')
    if not np.isfinite(nodes.astype(np.float64)).all():
        raise ValueError(f'{what}: a node coordinate is not finite')
    if isinstance(max_dist, bool) or not np.isscalar(max_dist) or not float(max_dist) >= 0:
        raise ValueError(f'{what}: max_dist must be a number >= 0, got {max_dist!r}')
    n = len(nodes)
    node_begin, e, edge_begin, cell_of = _skel_graph(what, n, node_begin, edges, edge_begin)
    values, classes, lab = _dense_classes(what, labels, n)
    node_scaled = nodes * scaling
    edge_coords = node_scaled[e + node_begin[cell_of][:, None]]
    weights = np.ascontiguousarray(np.linalg.norm(edge_coords[:, 0] - edge_coords[:, 1], axis=1), dtype=np.float64).reshape(-1)
    if not np.isfinite(weights).all():
        raise ValueError(f'{what}: an edge length is not finite')
    if n == 0:
        out = [lab.copy(), np.zeros(0, np.uint32), dict(sources_redone=0, steps_lds=0, steps_redo=0)]
        return out[0] if not (return_reached or return_counts) else tuple(o for o, f in zip(out, (True, return_reached, return_counts)) if f)
    dev = D.device(device)
    n_cells, n_e = len(node_begin) - 1, len(e)
    nb_d, eb_d, e_d, w_d, cls_d = (D.up(a, dev) for a in (node_begin, edge_begin, e, weights, classes))
    adj_begin, adj_nbr, adj_w = D.empty(n + 1, D.i64, dev), D.empty(2 * n_e, D.i32, dev), D.empty(2 * n_e, D.f64, dev)
    counts_d = D.counters(dev)
    tmp = D.scratch('sd_skel_csr_temp_bytes', dev, n_e)
    D.call('sd_skel_csr', dev, e_d, eb_d, nb_d, n_cells, n, n_e, w_d, adj_begin, adj_nbr, adj_w, counts_d, tmp, tmp.numel())
    _skel_counts('sd_skel_csr', counts_d)
    max_cell = int(np.diff(node_begin).max())
    vote_d = D.empty(n, D.u8, dev)
    reached_d = D.empty(n, D.i32, dev) if return_reached else None
    tmp = D.scratch('sd_skel_vote_temp_bytes', dev, n, max_cell)
    D.call('sd_skel_vote', dev, adj_begin, adj_nbr, adj_w, 2 * n_e, nb_d, n_cells, n, max_cell, cls_d, len(values), float(max_dist), vote_d,
           reached_d, counts_d, tmp, tmp.numel())
    counts = _skel_counts('sd_skel_vote', counts_d)
    out = [values[D.down(vote_d)].astype(lab.dtype, copy=False)]
    if return_reached:
        out.append(D.down(reached_d, view=np.uint32))
    if return_counts:
        out.append(dict(sources_redone=int(counts[0]), steps_lds=int(counts[1]), steps_redo=int(counts[2])))
    return out[0] if len(out) == 1 else tuple(out)


def skeleton_compartment_majority(node_begin, edges, edge_begin, labels, soma_label=2, device=None):
    """``majority_vote_compartments`` (:1233-1266) for all cells at once (`node_begin`, `edges`, `edge_begin` as in
    ``skeleton_majority_vote``): the nodes labelled `soma_label` keep it; the connected components of the others get their most
    frequent label, the smallest on equal counts; where that is 1 with a share below 0.66 (``50 * c1 < 33 * total``, the reference's
    float32 test for every component below 2^24 nodes) they get 0.  -> labels in the dtype of `labels`."""
    what = 'skeleton_compartment_majority'
    lab0 = np.asarray(labels)
    n = int(lab0.shape[0]) if lab0.ndim else 0
    node_begin, e, edge_begin, _ = _skel_graph(what, n, node_begin, edges, edge_begin)
    values, classes, lab = _dense_classes(what, lab0, n, extra=(0,) if n and (lab0 == 1).any() else ())
    if n == 0:
        return lab.copy()
    find = lambda x: int(np.searchsorted(values, x)) if x in values else -1
    dev = D.device(device)
    nb_d, eb_d, e_d, cls_d = (D.up(a, dev) for a in (node_begin, edge_begin, e, classes))
    out_d = D.empty(n, D.u8, dev)
    counts_d = D.counters(dev)
    tmp = D.scratch('sd_skel_components_temp_bytes', dev, n)
    D.call('sd_skel_components', dev, e_d, eb_d, nb_d, len(node_begin) - 1, n, len(e), cls_d, find(soma_label), find(1), max(find(0), 0), out_d,
           counts_d, tmp, tmp.numel())
    counts = _skel_counts('sd_skel_components', counts_d)
    if int(counts[6]):
        raise ValueError(f'{what}: a component of 2^24 nodes or more: the share of label 1 is not pinned there')
    return values[D.down(out_d)].astype(lab.dtype, copy=False)


def majorityvote_skeleton_property(sso, prop_key: str, max_dist: int = 10000, return_res: bool = False):
    """Drop-in for ``majorityvote_skeleton_property`` (:1270-1302): the sliding-window majority vote of the integer property
    ``sso.skeleton[prop_key]`` along the skeleton, stored as ``"%s_avg%d" % (prop_key, max_dist)`` or returned.  Reads ``skeleton``
    (``nodes``, ``edges``, the property), ``scaling`` and ``id`` of a (duck-typed) ``sso``.  Does not call ``sso.save_skeleton()``."""
    if prop_key not in sso.skeleton:
        raise ValueError(f'Given property "{prop_key}" does not exist in '
                         f'skeleton of SSV {sso.id}.')
    nodes = np.asarray(sso.skeleton['nodes']).reshape(-1, 3)
    edges = np.array(sso.skeleton['edges'], dtype=np.int64).reshape(-1, 2)
    prop = np.asarray(sso.skeleton[prop_key])
    avg_prop = skeleton_majority_vote(nodes, [0, len(nodes)], edges, [0, len(edges)], prop, sso.scaling, max_dist)
    if return_res:
        return avg_prop
    sso.skeleton["%s_avg%d" % (prop_key, max_dist)] = avg_prop


def majority_vote_compartments(sso, ax_pred_key: str = 'axoness'):
    """Drop-in for ``majority_vote_compartments`` (:1233-1266): stores ``ax_pred_key + "_comp_maj"`` (float64, as the reference
    does) and calls ``sso.save_skeleton()``."""
    nodes = np.asarray(sso.skeleton['nodes']).reshape(-1, 3)
    edges = np.array(sso.skeleton['edges'], dtype=np.int64).reshape(-1, 2)
    pred = np.asarray(sso.skeleton[ax_pred_key])
    res = skeleton_compartment_majority([0, len(nodes)], edges, [0, len(edges)], pred)
    new_axoness_arr = np.zeros((len(nodes)))
    new_axoness_arr[:] = res
    sso.skeleton[ax_pred_key + "_comp_maj"] = new_axoness_arr
    sso.save_skeleton()


# ---------------------------------------------------------------------------------------------------------------------------------
# from pixels back to the mesh (reps/super_segmentation_helper.py:1527-1667)
def _vote_device(index_arr, label_arr, bg_label, n_verts, n_labels, unpredicted, want_table, device=None):
    """``sd_views_vote`` -> (vertex labels uint8, the wrapped count table uint8 or None)."""
    index_arr = index_arr if isinstance(index_arr, torch.Tensor) else np.asarray(index_arr).reshape(-1)
    label_arr = label_arr if isinstance(label_arr, torch.Tensor) else np.asarray(label_arr).reshape(-1)
    dev = D.device(device)
    if isinstance(index_arr, torch.Tensor):
        idx_d = index_arr.to(dev).reshape(-1).to(torch.int32).contiguous()
    else:
        if len(index_arr) and (index_arr.min() < 0 or index_arr.max() >= 2 ** 32):
            raise IndexError('semseg2mesh_counter: an index does not fit 32 bits')
        idx_d = D.up(index_arr.astype(np.uint32), dev)
    if isinstance(label_arr, torch.Tensor):
        lab_d = label_arr.to(dev).reshape(-1).to(torch.uint8).contiguous()
    else:
        if len(label_arr) and (label_arr.min() < 0 or label_arr.max() > 255):
            raise ValueError('semseg2mesh_counter: labels must fit uint8')
        lab_d = D.up(label_arr.astype(np.uint8), dev)
    n_px = int(idx_d.numel())
    if int(lab_d.numel()) != n_px:
        raise ValueError(f'semseg2mesh_counter: {n_px} indices, {int(lab_d.numel())} labels')
    labels_d = D.empty(n_verts, D.u8, dev)
    table_d = D.empty((n_verts, n_labels), D.u8, dev) if want_table else None
    cnt = D.counters(dev)
    tmp = D.scratch('sd_views_vote_temp_bytes', dev, n_verts, n_labels)
    D.call('sd_views_vote', dev, idx_d if n_px else None, lab_d if n_px else None, n_px, int(bg_label) & 0xffffffff, n_verts, n_labels, unpredicted,
           labels_d, table_d, cnt, tmp, tmp.numel())
    c = D.down(cnt)
    if c[3]:
        raise IndexError('semseg2mesh_counter: a pixel names a vertex the mesh does not have')
    if c[4]:
        raise IndexError('semseg2mesh_counter: a label is outside the count table')
    return D.down(labels_d, n_verts), (D.down(table_d, n_verts) if want_table else None)


def semseg2mesh_counter(index_arr: np.ndarray, label_arr: np.ndarray, bg_label: int, count_arr: np.ndarray, device=None) -> np.ndarray:
    """Drop-in of the reference's ``semseg2mesh_counter`` (:1527-1551): the per-vertex label counts of the pixels, added to `count_arr`
    ((M, labels), zero-initialised by the caller) in ITS dtype, so a uint8 table wraps at 256 as the reference's does."""
    count_arr = np.asarray(count_arr)
    if count_arr.ndim != 2:
        raise ValueError('semseg2mesh_counter: count_arr must have shape (vertices, labels)')
    if count_arr.dtype != np.uint8:
        raise NotImplementedError('semseg2mesh_counter: only the uint8 count table of semseg2mesh is built')
    n_verts, n_labels = count_arr.shape
    if n_verts == 0 or n_labels == 0:
        if len(np.asarray(index_arr).reshape(-1)) and (np.asarray(index_arr).reshape(-1) != bg_label).any():
            raise IndexError('semseg2mesh_counter: a pixel names a vertex the mesh does not have')
        return count_arr
    _, table = _vote_device(index_arr, label_arr, bg_label, n_verts, n_labels, 0, True, device)
    count_arr += table.reshape(count_arr.shape)
    return count_arr


def semseg2mesh(sso, semseg_key=None, nb_views=None, dest_path=None, k=1, colors=None, force_recompute=False, index_view_key=None,
                index_views=None, semseg_views=None, device=None):
    """The reference's ``semseg2mesh`` (:1554-1667) on arrays in memory: `index_views` (the output of ``render_sso_coords_index_views``)
    and `semseg_views` (pixel labels of the same shape) vote for the vertices of ``sso.mesh``; -> ``(indices, vertices, normals, col)``
    with col the per-vertex label, or ``colors[label]``.  ``background_id = max(index_views)``, ``background_l = max(semseg_views)``,
    unpredicted = background_l + 1.  k = 0 keeps unpredicted and background vertices; k > 0 spreads the labels of the predicted,
    non-background vertices to all vertices by the majority of the k nearest (the device kNN vote of the spine head path).  The view
    and label storages are not built: the views are arguments, `dest_path` raises ``NotImplementedError``."""
    if dest_path is not None:
        raise NotImplementedError('semseg2mesh: writing the coloured mesh to a k.zip is not built')
    if index_views is None or semseg_views is None:
        raise NotImplementedError('semseg2mesh: the view storage is not built; pass index_views and semseg_views')
    from ..extraction.cs_processing_steps import segmented_knn
    i_views, s_views = np.asarray(index_views).reshape(-1), np.asarray(semseg_views).reshape(-1)
    if len(i_views) != len(s_views):
        raise ValueError(f'semseg2mesh: {len(i_views)} index pixels, {len(s_views)} label pixels')
    if len(i_views) == 0:
        raise ValueError('semseg2mesh: no pixels')
    mesh = sso.mesh
    vertices = np.asarray(mesh[1]).reshape(-1, 3)
    background_id, background_l = int(np.max(i_views)), int(np.max(s_views))
    unpredicted_l = background_l + 1
    if unpredicted_l > 255:
        raise ValueError('Overflow in label view array.')
    pp = len(vertices)
    if pp:
        vertex_labels, _ = _vote_device(i_views, s_views, background_id, pp, background_l + 1, unpredicted_l, False, device)
    else:
        if (i_views != background_id).any():
            raise IndexError('semseg2mesh: a pixel names a vertex the mesh does not have')
        vertex_labels = np.zeros(0, np.uint8)
    if isinstance(k, bool) or int(k) != k or k < 0:
        raise ValueError(f'semseg2mesh: k must be a non-negative integer, got {k!r}')
    if k == 0:
        maj_vote = vertex_labels
    else:
        keep = (vertex_labels != unpredicted_l) & (vertex_labels != background_l)
        if not keep.any():
            raise ValueError('semseg2mesh: no vertex has a prediction to spread (the reference fails in cKDTree.query here)')
        pts = vertices[keep]
        maj_vote = segmented_knn(pts, np.array([0, len(pts)]), vertex_labels[keep].astype(np.int32), np.zeros(pp, np.int64),
                                 vertices.astype(np.float64), int(k), device).astype(np.int32)
    col = maj_vote if colors is None else np.asarray(colors)[maj_vote].astype(np.uint8)
    return mesh[0], mesh[1], (mesh[2] if len(mesh) > 2 else np.zeros(0, np.float32)), col


def sample_locations_sso(sso, ds_factor=None, device=None):
    """What ``SuperSegmentationObject.sample_locations`` returns (reps/super_segmentation_object.py, over
    ``SegmentationObject.sample_locations``, reps/segmentation.py:700-732) without the storages: the list of one float32 (k, 3) array of
    rendering locations per entry of ``sso.svs``, each anything with ``.mesh`` (``[indices, vertices, ...]``), ``.rep_coord`` and
    ``.scaling``.  One device call for the whole cell."""
    from ..proc.locations import sample_locations_table
    svs = list(sso.svs)
    verts = [np.asarray(sv.mesh[1], np.float32).reshape(-1, 3) for sv in svs]
    begin = np.concatenate(([0], np.cumsum([len(v) for v in verts]))).astype(np.uint64)
    if not svs:
        return []
    table = sample_locations_table((np.arange(len(svs), dtype=np.uint64), begin, np.concatenate(verts)), ds_factor,
                                   rep_coords=np.array([np.asarray(sv.rep_coord).reshape(3) for sv in svs]),
                                   scaling=np.array([np.asarray(sv.scaling).reshape(3) for sv in svs]), device=device)
    lb = table.loc_begin.astype(np.int64)
    return [table.locations[lb[k]:lb[k + 1]] for k in range(len(svs))]


# -- glia probabilities from supervoxel views (reps/super_segmentation_helper.py:956-958, :1495-1523) ---------------------------------
def glia_pred_exists(so) -> bool:
    """:956-958."""
    if hasattr(so, 'load_attr_dict'):
        so.load_attr_dict()
    return "glia_probas" in so.attr_dict


def gliapred_sso_nocache(sso, model, verbose: bool = True, device=None):
    """:1495-1523: the rendering locations of every supervoxel (``sample_locations_sso``), raw views of the whole cell at all of them
    (``render_sso_coords(add_cellobjects=False)``; they stay on the device), one ``predict_views`` call, and
    ``sso.svs[i].attr_dict['glia_probas']`` = float32 (n_i, 2) per supervoxel.  `sso`: anything with ``.mesh`` and ``.svs`` (each with
    ``.id``, ``.mesh``, ``.rep_coord``, ``.scaling``, ``.attr_dict``), as for ``render_sampled_views``; the reference's assertion on
    ``sso.version == 'tmp'`` belongs to its storage layer and is not made.  As there, a supervoxel without vertices is looked at from
    its representative coordinate."""
    from ..proc.rendering import render_sso_coords
    from ..proc.sd_proc import predict_views
    pred_key = "glia_probas"
    svs = list(sso.svs)
    coords = sample_locations_sso(sso, device=device)
    # len(part_views) == N + 1
    part_views = np.cumsum([0] + [len(c) for c in coords])
    flat_coords = np.concatenate(coords) if coords else np.zeros((0, 3), np.float32)
    # views are flat
    views = render_sso_coords(sso, flat_coords, verbose=verbose, add_cellobjects=False, return_rot_mat=False, device=device, return_device=True)
    sv_views = [views[part_views[ii]:part_views[ii + 1]] for ii in range(len(svs))]
    if not sv_views:
        return
    probas = predict_views(model, sv_views, None, return_proba=True, pred_key=pred_key, verbose=verbose)
    for ii, prob in enumerate(probas):
        svs[ii].attr_dict[pred_key] = prob


class GliaTable:
    """Glia probabilities of many supervoxels, one row per supervoxel, ascending by id: ``sv_ids`` uint64 (n_sv,), ``view_begin`` int64
    (n_sv + 1,) into ``glia_probas`` float32 (n_loc, 2) (neuron, glia; one row per rendering location), ``glia_proba`` float64 (n_sv,)
    the mean of column 1 (NaN without locations) and ``glia`` uint8 (n_sv,) the class of ``graphs.glia_pred``.
    ``glia_probas[:, 1]`` and ``view_begin`` are the arguments of ``run_astrocyte_splitting``."""

    def __init__(self, sv_ids, view_begin, glia_probas, glia_proba, glia):
        self.sv_ids, self.view_begin = np.asarray(sv_ids, np.uint64), np.asarray(view_begin, np.int64)
        self.glia_probas, self.glia_proba, self.glia = glia_probas, glia_proba, glia
        n = len(self.sv_ids)
        if len(self.view_begin) != n + 1 or self.view_begin[0] != 0 or self.view_begin[-1] != len(glia_probas) or (np.diff(self.view_begin) < 0).any() \
                or len(glia_proba) != n or len(glia) != n:
            raise ValueError('GliaTable: offsets do not match the arrays')

    def __len__(self):
        return len(self.sv_ids)

    def _rows(self, ids):
        ids = np.asarray(ids, np.uint64).reshape(-1)
        rows = np.searchsorted(self.sv_ids, ids)
        if len(ids) and ((rows >= len(self.sv_ids)) | (self.sv_ids[np.minimum(rows, max(len(self.sv_ids) - 1, 0))] != ids)).any():
            raise KeyError('GliaTable: an id is not in the table')
        return rows

    def probas_of(self, ids):
        """The (n_i, 2) probabilities of one id, or the list of them for several."""
        rows = self._rows(ids)
        out = [self.glia_probas[self.view_begin[r]:self.view_begin[r + 1]] for r in rows]
        return out[0] if np.ndim(ids) == 0 else out

    def as_dict(self) -> dict:
        """id -> (n_i, 2): what the reference stores as ``glia_probas`` per supervoxel."""
        return {int(i): self.glia_probas[self.view_begin[k]:self.view_begin[k + 1]] for k, i in enumerate(self.sv_ids)}


class _Svs:
    def __init__(self, svs):
        self.svs = svs


def predict_glia_table(cells, model, thresh=None, max_locs_per_batch=None, single_cc_only=False, ds_factor=None, device=None,
                       background=1) -> GliaTable:
    """``run_astrocyte_rendering`` and ``run_astrocyte_prediction`` (exec/exec_render.py:206, exec/exec_inference.py:290) for cells in
    memory -> ``GliaTable``.  `cells`: the connected components of the pruned supervoxel graph as objects with ``.mesh`` and ``.svs``
    (see ``gliapred_sso_nocache``): as in the reference every supervoxel is looked at in the context of its whole component.  Per cell
    the locations of its supervoxels are rendered (``render_sso_coords(add_cellobjects=False)``), optionally filtered
    (`single_cc_only`: ``sd_views_center_component`` with `background`, as ``predict_views`` does), predicted and turned into
    probabilities in batches of at most `max_locs_per_batch` locations -- default: what keeps the uint8 view tensor at or below 256 MiB,
    4096 locations of 2 x 128 x 256 --; the views never reach the host, a supervoxel may straddle two batches, and because every
    sample's arithmetic is its own the result does not depend on the batch size, bit for bit.  A supervoxel without vertices has no
    locations here (``gliapred_sso_nocache`` looks at it from its representative coordinate): a neuron with a NaN mean, as
    ``glia_pred`` states.  A cell whose mesh is empty raises.  `thresh` as in ``glia_pred``.  `model`: a
    ``handler.prediction.GliaViewModel``."""
    from ..proc import graphs
    from ..proc.image import center_component_planes
    from ..proc.rendering import _window_defaults, render_sso_coords
    what = 'predict_glia_table'
    cells = list(cells)
    dev = model.dev if device is None else D.device(device)
    if max_locs_per_batch is None:
        ws, nb_views, _ = _window_defaults(None, None, None)
        max_locs_per_batch = max(1, (256 << 20) // (nb_views * ws[0] * ws[1]))
    if isinstance(max_locs_per_batch, bool) or int(max_locs_per_batch) != max_locs_per_batch or max_locs_per_batch < 1:
        raise ValueError(f'{what}: max_locs_per_batch must be a positive integer, got {max_locs_per_batch!r}')
    B = int(max_locs_per_batch)
    ids, counts, parts = [], [], []                      # per supervoxel in cell order; per batch the device probabilities
    for k, cell in enumerate(cells):
        svs = list(cell.svs)
        if len(np.asarray(cell.mesh[1]).reshape(-1)) == 0:
            raise ValueError(f'{what}: cell {k} has an empty mesh')
        has = [len(np.asarray(sv.mesh[1]).reshape(-1)) > 0 for sv in svs]
        coords = iter(sample_locations_sso(_Svs([sv for sv, h in zip(svs, has) if h]), ds_factor, device=dev))
        coords = [next(coords) if h else np.zeros((0, 3), np.float32) for h in has]
        ids += [int(sv.id) for sv in svs]
        counts += [len(c) for c in coords]
        flat = np.concatenate(coords) if coords else np.zeros((0, 3), np.float32)
        for b0 in range(0, len(flat), B):
            views = render_sso_coords(cell, flat[b0:b0 + B], add_cellobjects=False, device=dev, return_device=True)
            if single_cc_only:
                center_component_planes(views, background, out=views)
            parts.append(model.predict_device(views))
    ids = np.array(ids, np.uint64)
    if len(np.unique(ids)) != len(ids):
        raise ValueError(f'{what}: a supervoxel id occurs twice')
    probas = (torch.cat(parts, 0) if parts else torch.zeros((0, 2), dtype=torch.float32, device=dev)).cpu().numpy()
    order = np.argsort(ids, kind='stable')
    begin = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    rows = np.concatenate([np.arange(begin[r], begin[r + 1]) for r in order]) if len(order) else np.zeros(0, np.int64)
    probas = np.ascontiguousarray(probas[rows.astype(np.int64)])
    view_begin = np.concatenate(([0], np.cumsum(np.asarray(counts, np.int64)[order]))).astype(np.int64)
    glia, mean = graphs.glia_pred(probas[:, 1], view_begin, thresh, False, dev)
    return GliaTable(ids[order], view_begin, probas, mean, glia)


# -- cell types from multi-views (reps/super_segmentation_helper.py:180-213, :1670-1755, :1981-2065) -------------------------------
def view_sample_table(n_loc: int, views_per_loc: int, nb_views: int) -> np.ndarray:
    """The draws of ``sso_views_to_modelinput`` (:199-212) as a table over the UNSHUFFLED views (n_loc, C, views_per_loc, H, W): int32
    (n_samples, nb_views), entry = plane ``loc * views_per_loc + view`` of that slot.  numpy's global generator is seeded and used exactly
    as the reference uses it: ``seed(0)``, ``shuffle`` along axis 0 (for an array: ``n_loc - 1`` bounded draws, whatever it holds),
    ``choice`` for the padding when there are fewer than `nb_views` planes."""
    if n_loc < 1 or views_per_loc < 1 or nb_views < 1:
        raise ValueError('view_sample_table: no views')
    np.random.seed(0)
    perm = np.arange(n_loc).reshape(n_loc, 1)      # shuffled as the 5-D view array is: rows along axis 0
    np.random.shuffle(perm)
    planes = (perm.astype(np.int64) * views_per_loc + np.arange(views_per_loc)[None]).reshape(-1)
    if len(planes) < nb_views:
        rand_ixs = np.random.choice(len(planes), nb_views - len(planes))
        planes = np.append(planes, planes[rand_ixs])
    nb_samples = int(np.floor(len(planes) / nb_views))
    return planes[:nb_samples * nb_views].reshape(nb_samples, nb_views).astype(np.int32)


def sso_views_to_modelinput(sso, nb_views: int, view_key=None, return_table: bool = False):
    """:180-213: random subsets of `nb_views` views, (n_samples, C, nb_views, H, W).  `sso`: the view array (n_loc, C, views_per_loc, H,
    W) itself -- numpy, or a device tensor --, or anything with ``load_views(view_key=...)``.  With `return_table` the views are not
    moved: -> ``ViewSamples(views, table)`` (``handler.prediction``), the form the view network reads in place."""
    views = sso if isinstance(sso, (np.ndarray, torch.Tensor)) else sso.load_views(view_key=view_key)
    if views.ndim != 5 or views.shape[0] < 1 or views.shape[2] < 1:
        raise ValueError('sso_views_to_modelinput: views must be (n_loc > 0, C, views_per_loc > 0, H, W)')
    table = view_sample_table(int(views.shape[0]), int(views.shape[2]), int(nb_views))
    if return_table:
        from ..handler.prediction import ViewSamples
        return ViewSamples(views, table)
    v = views.cpu().numpy() if isinstance(views, torch.Tensor) else np.asarray(views)
    n_loc, C, vpl, H, W = v.shape
    planes = v.swapaxes(1, 0).reshape(C, n_loc * vpl, H, W)
    return planes[:, table.reshape(-1)].reshape(C, table.shape[0], nb_views, H, W).swapaxes(1, 0)


def syn_sign_ratio_celltype(syn_sign, mesh_area, syn_axs, weighted: bool = True, comp_types=None) -> float:
    """:1981-2065 over arrays: `syn_sign` (+1 / -1), `mesh_area` and the compartment label at the synapse (``attr_for_coords`` of the
    axoness key) of every ``syn_ssv`` object of the cell.  Boutons count as axon (3, 4 -> 1), the size is ``mesh_area / 2``; -> the
    (area-weighted) share of symmetric synapses among those on `comp_types` (default [1]), -1 for no synapse or zero area."""
    comp_types = [1] if comp_types is None else list(comp_types)
    syn_sign, mesh_area, syn_axs = np.asarray(syn_sign), np.asarray(mesh_area, dtype=np.float64), np.array(syn_axs, copy=True)
    if not (len(syn_sign) == len(mesh_area) == len(syn_axs)):
        raise ValueError('syn_sign_ratio_celltype: arrays of different lengths')
    if len(syn_sign) == 0:
        return -1
    syn_axs[syn_axs == 3] = 1
    syn_axs[syn_axs == 4] = 1
    keep = np.isin(syn_axs, comp_types)
    syn_signs, syn_sizes = syn_sign[keep], mesh_area[keep] / 2
    if len(syn_signs) == 0 or np.sum(syn_sizes) == 0:
        return -1
    if weighted:
        return np.sum(syn_sizes[syn_signs == -1]) / float(np.sum(syn_sizes))
    return np.sum(syn_signs == -1) / float(len(syn_signs))


def celltype_vote(res: np.ndarray, da_equals_tan: bool = True, n_classes: int = 7):
    """The vote block of ``celltype_of_sso_nocache`` (:1733-1753) on the logits of all samples of a cell: -> ``(pred, res, certainty)``
    with `res` the (merged) float32 array the reference stores as ``_probas`` and the certainty of ``certainty_celltype`` (the entropy
    certainty of the softmax of `res`)."""
    from ..handler.prediction import certainty_estimate
    res = np.array(res, copy=True)
    if da_equals_tan:
        assert n_classes == 7
        res[:, 1] += res[:, 6]
        res = np.delete(res, [6], axis=1)
    clf = np.argmax(res, axis=1)
    if np.max(clf) >= n_classes:
        raise ValueError('Unknown cell type predicted.')
    major_dec = np.zeros(n_classes)
    for ii in range(len(major_dec)):
        major_dec[ii] = np.sum(clf == ii)
    major_dec /= np.sum(major_dec)
    pred = np.argmax(major_dec)
    return pred, res, certainty_estimate(res, is_logit=True)


def _celltype_store(sso, pred_key, pred, res, cert, save_to_attr_dict):
    sso.attr_dict[pred_key] = pred
    sso.attr_dict[f'{pred_key}_probas'] = res
    sso.attr_dict[f'{pred_key}_certainty'] = cert
    if save_to_attr_dict and hasattr(sso, 'save_attributes'):
        sso.save_attributes([pred_key, f'{pred_key}_probas', f'{pred_key}_certainty'], [pred, res, cert])


def _celltype_scalars(sso, n_samples, syn_props):
    """[[ratio on axon, ratio on dendrite]] * n_samples (:1726-1727); `syn_props` = (syn_sign, mesh_area, syn_axs), default
    ``sso.syn_props``."""
    props = sso.syn_props if syn_props is None else syn_props
    return np.array([[syn_sign_ratio_celltype(*props, comp_types=[1, ]), syn_sign_ratio_celltype(*props, comp_types=[0, ])]] * n_samples)


def _celltype_predict(sso, model, views, nb_views_model, use_syntype, pred_key, da_equals_tan, n_classes, save_to_attr_dict, syn_props):
    inp = sso_views_to_modelinput(sso if views is None else views, nb_views_model, return_table=True)
    n = len(inp.table)
    res = model.predict_proba((inp, _celltype_scalars(sso, n, syn_props)) if use_syntype else inp, bs=40)
    pred, res, cert = celltype_vote(res, da_equals_tan, n_classes)
    _celltype_store(sso, pred_key, pred, res, cert, save_to_attr_dict)
    return pred, res, cert


def predict_sso_celltype(sso, model, nb_views_model: int = 20, use_syntype=True, overwrite: bool = False, pred_key_appendix='',
                         da_equals_tan: bool = True, n_classes: int = 7, save_to_attr_dict: bool = True, views=None, syn_props=None):
    """:114-177 with the views passed in (host array or device tensor, (n_loc, C, views_per_loc, H, W)) or from ``sso.load_views()``:
    the samples are read in place through the sample table, the vote runs in numpy on the logits.  The ratios are used when
    ``config.syntype_available and use_syntype``, as there.  Also returns ``(pred, probas, certainty)``."""
    pred_key = 'celltype_cnn_e3' + pred_key_appendix
    if not overwrite and pred_key in sso.attr_dict:
        return
    return _celltype_predict(sso, model, views, nb_views_model, bool(global_params.config.syntype_available and use_syntype), pred_key,
                             da_equals_tan, n_classes, save_to_attr_dict, syn_props)


def celltype_of_sso_nocache(sso, model, ws, nb_views, comp_window, nb_views_model: int = 20, pred_key_appendix: str = '', verbose: bool = False,
                            overwrite: bool = True, use_syntype: bool = True, da_equals_tan: bool = True, n_classes: int = 7,
                            save_to_attr_dict: bool = True, syn_props=None, device=None):
    """:1670-1755: render the 4-channel views at ``generate_rendering_locs(verts, comp_window / 3)`` -- they stay on the device --, cut
    them into the reference's random subsets, run the view network with the two synapse-sign ratios, add logit 6 onto logit 1, vote.
    `sso`: anything with ``.mesh``, ``.load_mesh(name)``, ``.attr_dict`` and ``.syn_props`` (or `syn_props`)."""
    from ..handler.multiviews import generate_rendering_locs
    from ..proc.rendering import render_sso_coords
    pred_key = 'celltype_cnn_e3' + pred_key_appendix
    if not overwrite and pred_key in sso.attr_dict:
        return
    verts = np.asarray(sso.mesh[1]).reshape(-1, 3)
    rendering_locs = generate_rendering_locs(verts, comp_window / 3, device=device)
    sso._sample_locations = rendering_locs
    views = render_sso_coords(sso, rendering_locs, ws=ws, comp_window=comp_window, nb_views=nb_views, verbose=verbose, add_cellobjects=True,
                              return_rot_mat=False, device=device, return_device=True)
    return _celltype_predict(sso, model, views, nb_views_model, use_syntype, pred_key, da_equals_tan, n_classes, save_to_attr_dict, syn_props)


class CellTypeTable:
    """Cell types of many cells: ``ids``, ``pred`` int64 (n,), ``certainty`` float64 (n,), and the (merged) logits of all samples as one
    ragged array: ``probas`` float32 (n_samples_total, C) with the samples of cell k at ``sample_begin[k]:sample_begin[k + 1]``."""

    def __init__(self, ids, pred, certainty, probas, sample_begin):
        self.ids, self.pred, self.certainty, self.probas, self.sample_begin = ids, pred, certainty, probas, sample_begin

    def __len__(self):
        return len(self.ids)

    def probas_of(self, k: int) -> np.ndarray:
        return self.probas[self.sample_begin[k]:self.sample_begin[k + 1]]

    def as_dict(self, pred_key: str = 'celltype_cnn_e3') -> dict:
        """id -> the three attributes the reference stores per cell."""
        return {i: {pred_key: self.pred[k], f'{pred_key}_probas': self.probas_of(k), f'{pred_key}_certainty': self.certainty[k]}
                for k, i in enumerate(self.ids)}


def predict_celltypes_table(cells, model, views=None, nb_views_model: int = 20, use_syntype: bool = True, da_equals_tan: bool = True,
                            n_classes: int = 7, bs: int = 40, ids=None) -> CellTypeTable:
    """The cell type step for many cells with ONE pass over the view network: the samples of all cells go through ``predict_proba`` in
    launch sets of `bs`, whatever cell they belong to, and the votes are taken per cell afterwards.  `views[k]` (default
    ``cells[k].load_views()``): the view array of cell k, host or device, (n_loc_k, C, views_per_loc, H, W) with the same
    ``views_per_loc``, H, W for all; they are joined along the location axis and read through one sample table.  Every cell's draws are
    those of ``sso_views_to_modelinput`` on its own views, so the result equals one ``predict_sso_celltype`` per cell."""
    from ..handler.prediction import ViewSamples
    cells = list(cells)
    if not cells:
        raise ValueError('predict_celltypes_table: no cells')
    views = [c.load_views() for c in cells] if views is None else list(views)
    if len(views) != len(cells):
        raise ValueError('predict_celltypes_table: one view array per cell')
    if len({tuple(v.shape[1:]) for v in views}) != 1:
        raise ValueError('predict_celltypes_table: the view arrays differ in channels, views per location or window')
    dev = model.dev
    tens = [v.to(dev) if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in views]
    vpl = int(tens[0].shape[2])
    tables, scal, begin, plane0 = [], [], [0], 0
    for c, v in zip(cells, tens):
        t = view_sample_table(int(v.shape[0]), vpl, int(nb_views_model)) + np.int32(plane0)
        tables.append(t)
        if use_syntype:
            scal.append(_celltype_scalars(c, len(t), None))
        begin.append(begin[-1] + len(t))
        plane0 += int(v.shape[0]) * vpl
    inp = ViewSamples(tens[0] if len(tens) == 1 else torch.cat(tens, 0), np.concatenate(tables))
    res = model.predict_proba((inp, np.concatenate(scal)) if use_syntype else inp, bs=bs)
    votes = [celltype_vote(res[begin[k]:begin[k + 1]], da_equals_tan, n_classes) for k in range(len(cells))]
    ids = np.arange(len(cells)) if ids is None else np.asarray(ids)
    return CellTypeTable(ids, np.array([v[0] for v in votes], np.int64), np.array([v[2] for v in votes], np.float64),
                         np.concatenate([v[1] for v in votes]), np.array(begin, np.int64))


# -- morphology embeddings from multi-views (reps/super_segmentation_helper.py:1758-1817) --------------------------------------------
def _cell_locations(sso) -> np.ndarray:
    """``np.concatenate(sso.sample_locations())`` (:1814), or the ``_sample_locations`` a rendering call left on a cell without the
    method: (n_loc, 3), in the order of the views."""
    if hasattr(sso, 'sample_locations'):
        locs = sso.sample_locations()
    else:
        locs = getattr(sso, '_sample_locations', None)
        if locs is None:
            raise ValueError('no rendering locations: the cell has neither sample_locations() nor _sample_locations')
    locs = np.concatenate(locs) if isinstance(locs, (list, tuple)) or np.asarray(locs).ndim == 3 else np.asarray(locs)
    return locs.reshape(-1, 3)


def _node_queries(sso) -> np.ndarray:
    """``sso.skeleton['nodes'] * sso.scaling`` (:1815) as the float64 the tree makes of it."""
    if hasattr(sso, 'load_skeleton'):
        sso.load_skeleton()
    return np.asarray(np.asarray(sso.skeleton['nodes']).reshape(-1, 3) * np.asarray(sso.scaling), dtype=np.float64)


def nearest_locations(locations, loc_begin, q_cell, q_xyz, ids=None, device=None) -> np.ndarray:
    """The ``cKDTree(locations).query(nodes * scaling, k=1)`` of :1814-1815 for many cells in one ``sd_syn_props_knn`` call: for every
    query the row, inside its cell's ``locations[loc_begin[c]:loc_begin[c + 1]]``, of the nearest location; the smaller row on equal
    float64 distances (the entry's rule, as in ``attr_for_coords``).  int64.  ValueError for a cell with queries and no location."""
    from ..extraction.cs_processing_steps import segmented_knn
    loc_begin = np.asarray(loc_begin, np.int64).reshape(-1)
    q_cell = np.asarray(q_cell, np.int64).reshape(-1)
    if len(q_cell) == 0:
        return np.zeros(0, np.int64)
    empty = np.diff(loc_begin)[q_cell] == 0
    if empty.any():
        c = int(q_cell[np.flatnonzero(empty)[0]])
        raise ValueError(f'cell {c if ids is None else ids[c]} has skeleton nodes but no rendering location')
    rows = segmented_knn(locations, loc_begin, None, q_cell, q_xyz, 1, device)
    return rows.astype(np.int64) - loc_begin[q_cell]


def view_embedding_of_sso_nocache(sso, model, ws, nb_views, comp_window, pred_key_appendix: str = '', verbose: bool = False,
                                  overwrite: bool = True, add_cellobjects=True, device=None):
    """:1758-1817: render the views at ``generate_rendering_locs(verts, comp_window / 3)`` -- they stay on the device, and in
    ``sso.view_dict['tmp_views' + pred_key_appendix]``, which is reused unless `overwrite` --, embed view 0 of every location with
    `model` (a ``handler.prediction.EmbeddingModel``; the uint8 views go in, the normalisation is the first layer's), give every
    skeleton node the latent of its nearest rendering location and store that as ``sso.skeleton['latent_morph' + pred_key_appendix]``,
    float32 (n_nodes, z_dim); also returned.  `sso`: anything with ``.mesh``, ``.load_mesh(name)``, ``.view_caching``,
    ``.view_dict``, ``.skeleton`` (``'nodes'`` in voxels) and ``.scaling``; ``load_skeleton`` / ``save_skeleton`` are called if there."""
    from ..handler.multiviews import generate_rendering_locs
    from ..proc.rendering import render_sso_coords
    pred_key = 'latent_morph' + pred_key_appendix
    assert sso.view_caching, "'view_caching' of {} has to be True in order to run 'view_embedding_of_sso_nocache'.".format(sso)
    tmp_view_key = 'tmp_views' + pred_key_appendix
    if tmp_view_key not in sso.view_dict or overwrite:
        verts = np.asarray(sso.mesh[1]).reshape(-1, 3)
        rendering_locs = generate_rendering_locs(verts, comp_window / 3, device=device)
        sso._sample_locations = rendering_locs[None, ]
        views = render_sso_coords(sso, rendering_locs, ws=ws, comp_window=comp_window, nb_views=nb_views, verbose=verbose,
                                  add_cellobjects=add_cellobjects, return_rot_mat=False, device=device, return_device=True)
        sso.view_dict[tmp_view_key] = views
        locs = rendering_locs
    else:
        views = sso.view_dict[tmp_view_key]
        locs = _cell_locations(sso)
    return _embed_to_skeleton(sso, model, views, locs, pred_key, None)


def _embed_to_skeleton(sso, model, views, locs, pred_key, view_ixs_key):
    queries = _node_queries(sso)
    if len(locs) != len(views):
        raise ValueError(f'{len(views)} view locations, {len(locs)} rendering locations')
    if len(queries) and not len(views):
        raise ValueError('the cell has skeleton nodes but no rendering location')
    if view_ixs_key is not None and view_ixs_key in sso.skeleton:
        ixs = np.asarray(sso.skeleton[view_ixs_key], np.int64).reshape(-1)
        if len(ixs) != len(queries):
            raise IndexError(f'skeleton[{view_ixs_key!r}] holds {len(ixs)} entries for {len(queries)} nodes')
        if len(ixs) and (ixs.min() < 0 or ixs.max() >= len(views)):      # stale indices: the reference's latent[ixs] raises too
            raise IndexError(f'skeleton[{view_ixs_key!r}] names a location outside [0, {len(views)})')
    else:
        ixs = nearest_locations(locs, [0, len(locs)], np.zeros(len(queries), np.int64), queries, device=model.dev)
        if view_ixs_key is not None:
            sso.skeleton[view_ixs_key] = ixs
    if len(views):
        latent = model.predict_device(views)
        node_latent = latent[D.up(ixs, model.dev)].cpu().numpy()
    else:
        node_latent = np.zeros((0, model.spec.n_classes), np.float32)
    sso.skeleton[pred_key] = node_latent
    if hasattr(sso, 'save_skeleton'):
        sso.save_skeleton()
    return node_latent


class MorphologyTable:
    """Morphology embeddings of many cells: ``ids``; ``latent`` float32 (n_loc_total, z), the locations of cell k at
    ``loc_begin[k]:loc_begin[k + 1]``; ``node_latent`` float32 (n_nodes_total, z) with ``node_begin`` likewise -- what goes into
    ``CellTable(node_attrs={'latent_morph': ...})`` --; ``view_ixs`` int64 (n_nodes_total): the nearest location of every node as a row
    inside its own cell, so that ``node_latent = latent[loc_begin[cell] + view_ixs]``."""

    def __init__(self, ids, latent, loc_begin, node_latent, node_begin, view_ixs):
        self.ids, self.latent, self.loc_begin = np.asarray(ids), latent, np.asarray(loc_begin, np.int64)
        self.node_latent, self.node_begin, self.view_ixs = node_latent, np.asarray(node_begin, np.int64), np.asarray(view_ixs, np.int64)
        n = len(self.ids)
        if len(self.loc_begin) != n + 1 or len(self.node_begin) != n + 1:
            raise ValueError('MorphologyTable: loc_begin and node_begin hold one offset per cell and one more')
        mono = self.loc_begin[0] == 0 and self.node_begin[0] == 0 and (np.diff(self.loc_begin) >= 0).all() and (np.diff(self.node_begin) >= 0).all()
        if not mono or self.loc_begin[-1] != len(latent) or self.node_begin[-1] != len(node_latent) or len(self.view_ixs) != len(node_latent):
            raise ValueError('MorphologyTable: offsets do not match the arrays')

    def __len__(self):
        return len(self.ids)

    def latent_of(self, k: int) -> np.ndarray:
        return self.latent[self.loc_begin[k]:self.loc_begin[k + 1]]

    def node_latent_of(self, k: int) -> np.ndarray:
        return self.node_latent[self.node_begin[k]:self.node_begin[k + 1]]

    def view_ixs_of(self, k: int) -> np.ndarray:
        return self.view_ixs[self.node_begin[k]:self.node_begin[k + 1]]


def embed_cells_table(cells, model, views=None, locations=None, bs=None, ids=None) -> MorphologyTable:
    """``view_embedding_of_sso_nocache``'s embedding and node mapping for many cells at once: the locations of all cells go through the
    network in launch sets of `bs` planes, whatever cell they belong to, and one segmented nearest-neighbour call covers all nodes.
    `views[k]` (default ``cells[k].view_dict['tmp_views']``): the views of cell k, host or device, (n_loc_k, C, nb_views, H, W);
    `locations[k]` (default: the cell's rendering locations) (n_loc_k, 3) in their order.  Equals one single call per cell bit for
    bit: a sample's latent does not depend on its launch set or tile, and the node mapping is the same entry's."""
    cells = list(cells)
    if not cells:
        raise ValueError('embed_cells_table: no cells')
    views = [c.view_dict['tmp_views'] for c in cells] if views is None else list(views)
    locations = [_cell_locations(c) for c in cells] if locations is None else [np.asarray(l).reshape(-1, 3) for l in locations]
    if len(views) != len(cells) or len(locations) != len(cells):
        raise ValueError('embed_cells_table: one view array and one location array per cell')
    if len({tuple(v.shape[1:]) for v in views}) != 1:
        raise ValueError('embed_cells_table: the view arrays differ in channels, views per location or window')
    for k, (v, l) in enumerate(zip(views, locations)):
        if len(v) != len(l):
            raise ValueError(f'embed_cells_table: cell {k} has {len(v)} view locations and {len(l)} rendering locations')
    ids = np.arange(len(cells)) if ids is None else np.asarray(ids)
    dev = model.dev
    queries = [_node_queries(c) for c in cells]
    loc_begin = np.concatenate(([0], np.cumsum([len(l) for l in locations]))).astype(np.int64)
    node_begin = np.concatenate(([0], np.cumsum([len(q) for q in queries]))).astype(np.int64)
    z = model.spec.n_classes
    if loc_begin[-1] == 0:
        if node_begin[-1]:
            raise ValueError('embed_cells_table: a cell has skeleton nodes but no rendering location')
        return MorphologyTable(ids, np.zeros((0, z), np.float32), loc_begin, np.zeros((0, z), np.float32), node_begin, np.zeros(0, np.int64))
    loc_dtype = np.float32 if all(l.dtype == np.float32 for l in locations) else np.float64
    view_ixs = nearest_locations(np.concatenate(locations).astype(loc_dtype), loc_begin, np.repeat(np.arange(len(cells)), np.diff(node_begin)),
                                 np.concatenate(queries), ids=ids, device=dev)
    tens = [v.to(dev) if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in views if len(v)]
    latent = model.predict_device(tens[0] if len(tens) == 1 else torch.cat(tens, 0), bs)
    rows = view_ixs + np.repeat(loc_begin[:-1], np.diff(node_begin))
    node_latent = latent[D.up(rows, dev)].cpu().numpy()
    return MorphologyTable(ids, latent.cpu().numpy(), loc_begin, node_latent, node_begin, view_ixs)


# -- compartment labels from multi-views (reps/super_segmentation_helper.py:1353-1392, :1820-1905) ----------------------------------
def predict_views_semseg(views, model, batch_size=10, verbose=False):
    """Drop-in of ``predict_views_semseg`` (:1353-1392): `views` uint8 (N_LOCS, N_CH, N_VIEWS, H, W), host array or device tensor ->
    the pixel labels (N_LOCS, 1, N_VIEWS, H, W), ``argmax`` over the classes of ``model(views / 255)``, as the same kind.  `model`: a
    ``handler.prediction.SemsegViewModel``; it reads the views where they are (no swap of the channel and view axes is made) and takes
    the argmax on the device, where the first maximum wins as in ``np.argmax``.  Labels are uint8 (the reference's are int64; its
    consumer ``semseg2mesh`` reads them as uint8 counts)."""
    return model.predict_labels(views, bs=batch_size)


def semseg_of_sso_nocache(sso, model, semseg_key: str, ws, nb_views: int, comp_window: float, k: int = 1, dest_path=None, verbose: bool = False,
                          add_cellobjects=True, bs: int = 10, device=None):
    """:1820-1905 without the view storage: raw views at ``generate_rendering_locs(verts, comp_window / 3)`` (or ``sso._sample_locations``
    if set) -> pixel labels -> index views at the same locations -> ``semseg2mesh``.  Raw views and labels stay on the device.  The
    vertex labels are stored as ``sso.label_dict('vertex')[semseg_key]`` (pushed if the dict has ``push``) and returned.  `sso`:
    anything with ``.mesh``, ``.load_mesh(name)``, ``.label_dict('vertex')`` and a settable ``_sample_locations``."""
    from ..handler.multiviews import generate_rendering_locs
    from ..proc.rendering import render_sso_coords, render_sso_coords_index_views
    if dest_path is not None:
        raise NotImplementedError('semseg_of_sso_nocache: writing the coloured mesh to a k.zip is not built')
    verts = np.asarray(sso.mesh[1]).reshape(-1, 3)
    locs = getattr(sso, '_sample_locations', None)
    if locs is None:
        locs = generate_rendering_locs(verts, comp_window / 3, device=device)
        sso._sample_locations = [locs]
    locs = np.concatenate(locs) if isinstance(locs, (list, tuple)) else np.asarray(locs)
    views = render_sso_coords(sso, locs, ws=ws, comp_window=comp_window, nb_views=nb_views, verbose=verbose, add_cellobjects=add_cellobjects,
                              device=device, return_device=True)
    if len(views) != len(locs):
        raise ValueError('Unequal number of views and redering locations.')
    labeled = predict_views_semseg(views, model, batch_size=bs, verbose=verbose)
    assert labeled.shape[2] == nb_views, 'Predictions have wrong shape.'
    index_views = render_sso_coords_index_views(sso, locs, ws=ws, comp_window=comp_window, nb_views=nb_views, verbose=verbose, device=device)
    col = semseg2mesh(sso, semseg_key, k=k, force_recompute=True, index_views=index_views, semseg_views=labeled.cpu().numpy(), device=device)[3]
    ld = sso.label_dict('vertex')
    ld[semseg_key] = col
    if hasattr(ld, 'push'):
        ld.push()
    return col
