"""CPU restatement of the spine head volume estimate (``extract_spinehead_volume_mesh``, reference
``reps/super_segmentation_helper.py:2068-2198``) with scipy for zoom, fill holes, EDT, label and cKDTree, the ``peak_local_max`` rule
of skimage 0.18 / 0.19 in own words, ``oracle.objseg_ref.watershed_ref`` for the flood and the selection rule spelled out.  Pinned to
golden g22 (the reference's own statements run by tests/golden/make_golden_spinehead.py) by tests/test_spinehead_cpu.py.

A cell is a dict ``id, sv_ids, vertices (v, 3) float32 nm, vertex_labels {'spiness': (v)}, nodes (m, 3) voxels, node_attrs {key: (m)}``;
the segmentation is ``(vol (x, y, z) uint64, origin)``: zeros outside, as ``kd.load_seg`` pads."""
from collections import Counter

import numpy as np
from scipy import ndimage, spatial

from oracle.objseg_ref import watershed_ref

import _syn_props_ref as SP


def load_window(vol, origin, offset, size):
    """``kd.load_seg(offset=offset, size=size, mag=1).swapaxes(2, 0)``: (x, y, z), zeros outside the volume."""
    out = np.zeros(tuple(int(s) for s in size), vol.dtype)
    lo = np.asarray(offset, np.int64) - np.asarray(origin, np.int64)
    a = np.maximum(lo, 0)
    b = np.minimum(lo + np.asarray(size, np.int64), vol.shape)
    if np.all(b > a):
        out[tuple(slice(int(a[i] - lo[i]), int(b[i] - lo[i])) for i in range(3))] = vol[tuple(slice(int(a[i]), int(b[i])) for i in range(3))]
    return out


def in_bounding_box(verts, box):
    """in_bounding_boxC.pyx: strictly inside, differences in double, the half edges held in C ``float``."""
    v = np.asarray(verts).astype(np.float64).reshape(-1, 3)
    box = np.asarray(box, np.float64)
    edge = (box[1] / 2).astype(np.float32).astype(np.float64)
    d = v - box[0]
    return np.all((d > -edge) & (d < edge), axis=1)


def peak_local_max(d2, mask):
    """``peak_local_max(distance, footprint=np.ones((3, 3, 3)), labels=mask)`` on squared distances (the order of the values is all that
    counts) -> (n, 3) int64 in raster order.  Restated from skimage 0.18 / 0.19 (UNPINNED): the labels lose the outermost voxel layer of
    the array (exclude_border, min_distance 1); roi = the bounding box of what is left; inside roi the image is the distance where the
    object is and its minimum (0) elsewhere; a voxel of the object is a peak iff it equals the maximum of its 3x3x3 neighbourhood within
    roi (constant 0 outside) and exceeds the threshold (the image minimum, 0); if every voxel of the object equals its maximum there is
    no peak at all; a spacing of 1 culls nothing."""
    lab = np.array(mask, dtype=bool)
    for a in range(3):
        ix = [slice(None)] * 3
        for edge in (0, -1):
            ix[a] = edge
            lab[tuple(ix)] = False
    if not lab.any():
        return np.zeros((0, 3), np.int64)
    roi = ndimage.find_objects(lab.astype(np.int32))[0]
    obj = lab[roi]
    img = np.where(obj, np.asarray(d2)[roi], 0).astype(np.int64)
    out = img == ndimage.maximum_filter(img, footprint=np.ones((3, 3, 3)), mode='constant', cval=0)
    if np.all(out[obj]):
        return np.zeros((0, 3), np.int64)
    out &= obj & (img > 0)
    return np.transpose(np.nonzero(out)).astype(np.int64) + np.array([s.start for s in roi], np.int64)


def vote(queries, points, labels, k):
    """colorcode_vertices(..., return_color=False): the majority label of the min(k, points) nearest points (cKDTree order: by
    distance), on equal counts the label met first."""
    tree = spatial.cKDTree(points)
    k = min(int(k), len(points))
    _, ixs = tree.query(queries, k=k)
    ixs = np.asarray(ixs).reshape(len(queries), -1)
    return np.array([Counter(np.asarray(labels)[i].tolist()).most_common(1)[0][0] for i in ixs], np.int32).reshape(-1)


def nearest_d2(coords, c, offset, scaling):
    """The array form of what ``cKDTree((coords + offset) * scaling).query([(c + offset) * scaling])`` measures (:2189-2191): per axis
    ``(x + off) * s - (c + off) * s`` -- both points scaled in the dtype numpy gives the product, held as float64 (cKDTree's own copy),
    then subtracted -- squared and summed in axis order, float64 with every operation rounded.  -> (n) float64."""
    sc, off = np.asarray(scaling), np.asarray(offset)
    p = np.asarray((np.asarray(coords) + off) * sc, np.float64).reshape(-1, 3)
    q = np.asarray((np.asarray(c) + off) * sc, np.float64).reshape(3)
    d = p - q
    return ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def nearest_object(objects, nb_obj, c, offset, scaling):
    """The branch :2182-2192 in the reference's own words, `scaling` in the dtype it is given -> dict: ``ref_id`` the reference's pick
    (cKDTree), ``dist`` its returned distance, ``d2`` / ``ids`` the array form per object voxel (objects in id order, raster order
    inside one), ``decided``: the smallest d2 of the nearest object is strictly below that of every other object in this arithmetic,
    ``chosen``: ``ref_id`` if decided; else -- an exact float64 tie between objects, where cKDTree's pick is an artefact of its tree
    order -- THE PROJECT'S RULE, not the reference's: the lowest id among the tied objects."""
    coords, ids = [], []
    for ii in range(1, nb_obj + 1):
        curr_coords = np.transpose(np.nonzero(objects == ii))
        coords.append(curr_coords)
        ids.extend(len(curr_coords) * [ii])
    coords = np.concatenate(coords) + offset
    nn_kdt = spatial.cKDTree(coords * scaling)
    dist, nn_id = nn_kdt.query([(np.asarray(c) + offset) * scaling])
    ids = np.array(ids, np.int64)
    d2 = nearest_d2(coords - offset, c, offset, scaling)
    per_obj = np.array([d2[ids == ii].min() for ii in range(1, nb_obj + 1)])
    tied = 1 + np.flatnonzero(per_obj == per_obj.min())
    decided = len(tied) == 1
    ref_id = int(ids[nn_id[0]])
    return dict(ref_id=ref_id, dist=float(dist[0]), d2=d2, ids=ids, decided=decided, chosen=ref_id if decided else int(tied.min()))


def select_head(flood, c, offset, scaling, info=None):
    """:2171-2196 -> (objects, nb_obj, chosen id, its voxel count).  `info`: an optional dict that receives ``branch`` ('single',
    'slice' or 'nearest') and, for 'nearest', the entries of ``nearest_object``."""
    objects, nb_obj = ndimage.label(flood == 1)
    max_id = 1
    branch = 'single'
    if nb_obj > 1:
        c = [int(v) for v in c]
        ls = objects[(c[0] - 10):(c[0] + 11), (c[1] - 10):(c[1] + 11), (c[2] - 10):(c[2] + 11)]      # a negative start wraps: empty for c < 10
        ids, cnts = np.unique(ls, return_counts=True)
        cnts, ids = cnts[ids != 0], ids[ids != 0]
        if len(ids) == 0:
            near = nearest_object(objects, nb_obj, np.asarray(c, np.int64), np.asarray(offset, np.int64), scaling)
            max_id, branch = near['chosen'], 'nearest'
            if info is not None:
                info.update(near)
        else:
            max_id, branch = int(ids[np.argmax(cnts)]), 'slice'
    if info is not None:
        info['branch'] = branch
    return objects.astype(np.int32), int(nb_obj), max_id, int(np.sum(objects == max_id))


def window_stages(window, sv_ids, ds, verts, labels, offset, size, c, scaling, k):
    """One pass of the loop :2130-2198 on `window` (x, y, z) = the segmentation at `offset`, `verts` = mesh / scaling without the
    ignored labels.  -> dict of every stage; ``entry`` False: the reference writes nothing (no vertex in the box); raises the
    reference's ValueError for an empty mask."""
    seg = ndimage.zoom(window, 1 / np.asarray(ds), order=0)
    mask = np.isin(seg, np.asarray(sv_ids, np.uint64)).astype(np.uint8)
    filled = ndimage.binary_fill_holes(mask)
    if filled.sum() == 0:
        raise ValueError(f'Could not find segmentation at {offset} and size {size}')
    out = dict(mask=mask, filled=filled.astype(np.uint8))
    inb = in_bounding_box(verts, np.array([np.asarray(offset) + np.asarray(size) / 2, size]))
    pts = np.asarray(verts)[inb].astype(np.float64) - np.asarray(offset, np.int64)
    lab = np.asarray(labels)[inb].astype(np.int32)
    lab[lab == 0] = 9
    distance = ndimage.distance_transform_edt(filled)
    d2 = np.rint(distance * distance).astype(np.int32)
    peaks = peak_local_max(d2, filled)
    out.update(d2=d2, peaks=peaks, points=pts, point_labels=lab, entry=len(lab) > 0)
    if not out['entry']:
        return out
    votes = vote(peaks.astype(np.float64) * np.asarray(ds, np.float64), pts, lab, k) if len(peaks) else np.zeros(0, np.int32)
    markers = np.zeros(filled.shape, np.int32)
    markers[tuple(peaks.T)] = votes
    flood = watershed_ref(d2.astype(np.int64), markers, out['filled'])
    objects, nb_obj, max_id, n_vox = select_head(flood, c, offset, scaling)
    out.update(votes=votes, markers=markers, flood=flood, objects=objects, nb_obj=nb_obj, chosen=max_id, n_voxels=n_vox)
    return out


def spinehead_filter(cell, rep, scaling, k, ds_vertices, ignore_labels, ax_key):
    """(curr_sp == 1) & (curr_ax == 0) (:2114-2122): semseg_for_coords and attr_for_coords as tests/_syn_props_ref.py restates them."""
    s = SP.scale64(scaling)
    q = np.asarray(rep, np.float64).reshape(-1, 3) * s
    v, lab = SP.spine_points(cell, ds_vertices, ignore_labels)
    sp = SP.knn(v, [0, len(v)], lab, np.zeros(len(q), np.int64), q, min(k, len(v)))[0]
    nodes = np.asarray(cell.get('nodes', np.zeros((0, 3))), np.float64).reshape(-1, 3)
    ax = np.full(len(q), -1, np.int64)
    if len(nodes) and ax_key in cell.get('node_attrs', {}):
        j = SP.knn(nodes * s, [0, len(nodes)], None, np.zeros(len(q), np.int64), q, 1)[0]
        ax = np.asarray(cell['node_attrs'][ax_key]).reshape(-1)[j]
    return (sp == 1) & (ax == 0)


def extract_spinehead_volume(cell, syn_ids, syn_rep, seg, scaling, ctx_vol=(200, 200, 100), k=50, ds_vertices=1, ignore_labels=(4, 5),
                             ax_key='axoness_avg10000', stages=None):
    """The whole function for one cell -> {syn id: volume (float64, um^3)}."""
    scaling = np.array(scaling)
    ctx = np.array(ctx_vol)
    if 'spiness' not in cell.get('vertex_labels', {}):
        raise ValueError(f'"spiness" not available in skeleton of SSO {cell["id"]}.')
    res = {}
    if len(syn_rep) == 0:
        return res
    verts = np.asarray(cell['vertices'], np.float32).reshape(-1, 3) / scaling
    sem = np.asarray(cell['vertex_labels']['spiness']).reshape(-1)
    for l in ignore_labels:
        verts, sem = verts[sem != l], sem[sem != l]
    keep = spinehead_filter(cell, syn_rep, scaling, k, ds_vertices, ignore_labels, ax_key)
    ds = scaling[2] // scaling
    vol, origin = seg
    for c, sid in zip(np.asarray(syn_rep, np.int64)[keep], np.asarray(syn_ids)[keep]):
        offset = np.maximum(c - ctx, 0)
        size = (2 * ctx).astype(np.int32)
        st = window_stages(load_window(vol, origin, offset, size), cell['sv_ids'], ds, verts, sem, offset, size, c - offset, scaling, k)
        if stages is not None:
            stages[int(sid)] = st
        if st['entry']:
            res[int(sid)] = st['n_voxels'] * np.prod(scaling * ds) / 1e9
    return res


def blob_volume(shape, seed, n_blobs=3, n_sticks=3):
    """A seeded (x, y, z) 0/1 volume of balls joined and pierced by thin sticks, clear of nothing in particular: for the random cases."""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing='ij'), -1).astype(np.float64)
    m = np.zeros(shape, bool)
    centres = []
    for _ in range(n_blobs):
        c = rng.uniform(0.15, 0.85, 3) * shape
        r = rng.uniform(0.12, 0.3) * min(shape)
        m |= ((g - c) ** 2).sum(-1) <= r * r
        centres.append(c)
    for _ in range(n_sticks):
        a, b = rng.uniform(0, 1, 3) * shape, centres[int(rng.integers(len(centres)))]
        t = np.linspace(0, 1, 4 * max(shape))[:, None]
        p = np.rint(a + t * (b - a)).astype(int)
        p = p[np.all((p >= 0) & (p < np.array(shape)), 1)]
        m[tuple(p.T)] = True
    return m.astype(np.uint8)


AX_KEY = 'axoness_avg10000'


def case_from_golden(g, p):
    """Case `p` ('a_', ...) of golden g22 -> dict(scaling, ctx_vol, k, seg, cells (list of dicts), syn_ids, syn_rep, syn_cells, expected
    {cell id: {syn id: volume}}, err_cells)."""
    vb, nb, sb = g[p + 'cell_vert_begin'], g[p + 'cell_node_begin'], g[p + 'cell_sv_begin']
    cells = []
    for i, cid in enumerate(g[p + 'cell_ids'].tolist()):
        cells.append(dict(id=cid, sv_ids=g[p + 'cell_sv'][sb[i]:sb[i + 1]], vertices=g[p + 'cell_verts'][vb[i]:vb[i + 1]],
                          vertex_labels={'spiness': g[p + 'cell_spiness'][vb[i]:vb[i + 1]]}, nodes=g[p + 'cell_nodes'][nb[i]:nb[i + 1]],
                          node_attrs={AX_KEY: g[p + 'cell_ax'][nb[i]:nb[i + 1]]}))
    expected = {cid: {} for cid in g[p + 'cell_ids'].tolist() if cid not in g[p + 'err_cells'].tolist()}
    for c, s, v in zip(g[p + 'sh_cell'].tolist(), g[p + 'sh_syn'].tolist(), g[p + 'sh_vol']):
        expected[c][s] = v
    return dict(scaling=g[p + 'scaling'], ctx_vol=g[p + 'ctx_vol'], k=int(g[p + 'k']), seg=(g[p + 'vol'], (0, 0, 0)), cells=cells,
                syn_ids=g[p + 'syn_ids'], syn_rep=g[p + 'syn_rep'], syn_cells=g[p + 'syn_cells'], expected=expected,
                err_cells=g[p + 'err_cells'].tolist())


def synapses_of(case, cid):
    m = (case['syn_cells'] == np.uint64(cid)).any(1)
    return case['syn_ids'][m], case['syn_rep'][m]
