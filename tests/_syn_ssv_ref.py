"""CPU restatement of the synapse agglomeration for the tests (numpy / scipy; pinned to the reference by golden g19 in
tests/test_syn_ssv_cpu.py): the strict radius graph over the voxels of one cell pair and the attribute step of
``_combine_and_split_syn_thread`` (cs_processing_steps.py:453-513), written per component as the reference writes it."""
import numpy as np
import scipy.sparse
import scipy.sparse.csgraph
import scipy.spatial


def connected_cluster(voxel_lists, cs_gap_nm, scaling):
    """Components of "scaled distance strictly below the gap" over ``np.concatenate(voxel_lists)``: ``query_pairs`` (which includes
    distance == r) minus the pairs whose float64 squared distance is not below gap^2.  -> int32 labels, components numbered in ascending
    order of their smallest flat index."""
    flat = np.concatenate([np.asarray(v).reshape(-1, 3) for v in voxel_lists]).astype(np.int64) * np.asarray(scaling, np.float64)
    n = len(flat)
    pairs = scipy.spatial.cKDTree(flat).query_pairs(r=float(cs_gap_nm), output_type='ndarray')
    d2 = ((flat[pairs[:, 0]] - flat[pairs[:, 1]]) ** 2).sum(1)
    pairs = pairs[d2 < float(cs_gap_nm) * float(cs_gap_nm)]
    graph = scipy.sparse.coo_matrix((np.ones(len(pairs), bool), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, lab = scipy.sparse.csgraph.connected_components(graph, directed=False)
    _, first = np.unique(lab, return_index=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[lab].astype(np.int32)


def cell_model_labels(voxel_lists, cs_gap_nm, scaling):
    """A Python model of the device form (csrc/sd_syn_ssv.hip) for one group: voxels binned into ``choose_cell`` cells, the upper half
    of the neighbourhood within ``floor(gap / (c s)) + 1`` cells per axis, the three classes from the two tight boxes (too far /
    joined without looking / voxel test), union-find over the cells, numbering by smallest flat index.  It shows on the CPU that the
    cell size, the reach and the box rules give the restatement's partition."""
    from syconn_amd.extraction.cs_processing_steps import choose_cell
    s = np.asarray(scaling, np.float64)
    gap = float(cs_gap_nm)
    vox = np.concatenate([np.asarray(v).reshape(-1, 3) for v in voxel_lists]).astype(np.int64)
    c = choose_cell(s, gap)
    reach = (np.floor(gap / (c * s)) + 1).astype(int)
    cc = (vox - vox.min(0)) // c
    cells = {}
    for i, k in enumerate(map(tuple, cc.tolist())):
        cells.setdefault(k, []).append(i)
    keys = sorted(cells)
    index = {k: n for n, k in enumerate(keys)}
    parent = list(range(len(keys)))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a
    gap2 = gap * gap
    nbh = [(dx, dy, dz) for dx in range(-reach[0], reach[0] + 1) for dy in range(-reach[1], reach[1] + 1) for dz in range(-reach[2], reach[2] + 1)]
    for k in keys:
        A = vox[cells[k]]
        alo, ahi = A.min(0), A.max(0)
        for d in nbh[len(nbh) // 2 + 1:]:
            o = (k[0] + d[0], k[1] + d[1], k[2] + d[2])
            if o not in index:
                continue
            B = vox[cells[o]]
            blo, bhi = B.min(0), B.max(0)
            near = np.maximum(0, np.maximum(blo - ahi, alo - bhi)) * s
            far = np.maximum(bhi - alo, ahi - blo) * s
            if not (near ** 2).sum() < gap2 * (1 + 1e-9):
                continue
            hit = (far ** 2).sum() < gap2 * (1 - 1e-9)
            if not hit:
                hit = bool(((((A[:, None, :] * s) - (B[None, :, :] * s)) ** 2).sum(-1) < gap2).any())
            if hit:
                a, b = find(index[k]), find(index[o])
                if a != b:
                    parent[max(a, b)] = min(a, b)
    root = np.array([find(index[k]) for k in map(tuple, cc.tolist())])
    _, first, inv = np.unique(root, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inv.reshape(-1)].astype(np.int32)


def combine(groups, scaling, cs_gap_nm, min_obj_vx, sym_thresh, reference_indexing=True, labels=None):
    """`groups` = [(enc_key, [(syn_id, voxels (n, 3), sym_prop, asym_prop), ...]), ...] in processing order.  -> (rows, labels):
    one dict per stored synapse in storing order (the reference's attribute keys, ``voxels`` in ascending flat index, ``component`` =
    its count among all components, ``frag_ids`` / ``frag_counts`` = the true contributors) and the label array of every group.
    `labels` (one array per group) replaces the component search when given."""
    scaling32 = np.asarray(scaling, np.float32)
    rows, all_labels, component = [], [], 0
    for g, (key, frags) in enumerate(groups):
        voxel_list = [np.asarray(f[1], np.uint32).reshape(-1, 3) for f in frags]
        synix_list = np.concatenate([np.full(len(v), (max(j - 1, 0) if reference_indexing else j), np.int64) for j, v in enumerate(voxel_list)])
        true_ix = np.concatenate([np.full(len(v), j, np.int64) for j, v in enumerate(voxel_list)])
        lab = connected_cluster(voxel_list, cs_gap_nm, scaling) if labels is None else np.asarray(labels[g])
        all_labels.append(lab)
        flat = np.concatenate(voxel_list)
        key = int(key)
        for c in range(int(lab.max()) + 1):
            mask = np.flatnonzero(lab == c)
            ixs, cnt = np.unique(synix_list[mask], return_counts=True)
            component += 1
            if np.sum(cnt) < min_obj_vx:
                continue
            w = cnt / np.sum(cnt)
            this_vx = flat[mask]
            p = this_vx * scaling32
            d2 = ((p - np.mean(p, axis=0)) ** 2).sum(1)
            rep = (p[int(np.argmin(d2))] // scaling32).astype(np.int32)
            sym = np.sum(w * np.array([frags[i][2] for i in ixs]))
            asym = np.sum(w * np.array([frags[i][3] for i in ixs]))
            ratio = -1 if sym + asym == 0 else sym / float(asym + sym)
            t_ix, t_cnt = np.unique(true_ix[mask], return_counts=True)
            rows.append(dict(neuron_partners=np.array([key >> 32, key & 0xffffffff], np.uint64), rep_coord=rep,
                             bounding_box=np.array([np.min(this_vx, axis=0), np.max(this_vx, axis=0)]), size=len(this_vx),
                             cs_ids=[int(frags[i][0]) for i in ixs], sym_prop=sym, asym_prop=asym, syn_type_sym_ratio=ratio,
                             syn_sign=-1 if ratio > sym_thresh else 1, voxels=this_vx, component=component - 1, group=g,
                             frag_ids=[int(frags[i][0]) for i in t_ix], frag_counts=t_cnt.tolist()))
    return rows, all_labels


def groups_from_arrays(syn_ids, vox, vox_begin, sym_prop, asym_prop, enc_keys, group_begin, syn_rows):
    """The `groups` argument of ``combine`` from table columns and the filter's result."""
    out = []
    for g, key in enumerate(np.asarray(enc_keys).tolist()):
        rows = np.asarray(syn_rows)[group_begin[g]:group_begin[g + 1]].tolist()
        out.append((key, [(int(syn_ids[r]), np.asarray(vox)[vox_begin[r]:vox_begin[r + 1]], float(sym_prop[r]), float(asym_prop[r])) for r in rows]))
    return out


def filter_relevant_syn(syn_ids, mapping: dict):
    """The reference's loop form: -> ordered dict key -> list of rows of `syn_ids`."""
    top = max(mapping) if mapping else 0
    out = {}
    for r, i in enumerate(int(v) for v in np.asarray(syn_ids).tolist()):
        svs = [i >> 32, i & 0xffffffff]
        cells = [mapping.get(s, 0) if s <= top else 0 for s in svs]
        if min(cells) > 0 and cells[0] != cells[1]:
            out.setdefault((max(cells) << 32) + min(cells), []).append(r)
    return out


def assert_rows_equal(got, want, what=''):
    """Two lists of row dicts (``SynSsvTable.as_dict()`` / ``combine``): integers and arrays exact, floats bit for bit."""
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        for k in ('neuron_partners', 'rep_coord', 'bounding_box', 'voxels'):
            assert np.array_equal(np.asarray(a[k]).astype(np.int64), np.asarray(b[k]).astype(np.int64)), (what, i, k)
        assert int(a['size']) == int(b['size']) and list(a['cs_ids']) == list(b['cs_ids']) and int(a['syn_sign']) == int(b['syn_sign']), (what, i)
        for k in ('sym_prop', 'asym_prop', 'syn_type_sym_ratio'):
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (what, i, k, a[k], b[k])


def stats_from_labels(vox, vox_frag, frag_group, labels, scaling, min_obj_vx):
    """Vectorised numpy: what the statistics launches hand to the host edge, from a partition.  `vox` (N, 3) in flat order, `labels` (N)
    = component numbers over the whole input, ascending in the smallest flat index.  -> the keyword arguments of
    ``build_syn_ssv_table`` that come from the device.  The representative is the voxel with the smallest float64 squared distance to
    ``(sum * scale) / n``, ties to the smallest flat index."""
    vox, labels = np.asarray(vox, np.int64), np.asarray(labels, np.int64)
    vox_frag = np.asarray(vox_frag, np.int64)
    s = np.asarray(scaling, np.float64)
    K = int(labels.max()) + 1 if len(labels) else 0
    order = np.argsort(labels, kind='stable')
    lab_s, vox_s = labels[order], vox[order]
    begin = np.searchsorted(lab_s, np.arange(K + 1))
    sizes = np.diff(begin)
    mean = (np.add.reduceat(vox_s, begin[:-1], axis=0).astype(np.float64) * s) / sizes[:, None].astype(np.float64)
    d = vox_s.astype(np.float64) * s - mean[lab_s]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    best = np.lexsort((order, d2, lab_s))[begin[:-1]]
    pair_key = lab_s * (int(vox_frag.max()) + 1) + vox_frag[order]
    heads = np.flatnonzero(np.concatenate(([True], pair_key[1:] != pair_key[:-1])))
    keep = np.repeat(sizes >= min_obj_vx, sizes)
    return dict(comp_group=np.asarray(frag_group, np.int64)[vox_frag[order][begin[:-1]]], comp_sizes=sizes,
                comp_bbox=np.stack([np.minimum.reduceat(vox_s, begin[:-1], axis=0), np.maximum.reduceat(vox_s, begin[:-1], axis=0)], 1),
                comp_rep_vox=vox_s[best], pair_comp=lab_s[heads], pair_frag=vox_frag[order][heads],
                pair_cnt=np.diff(np.concatenate((heads, [len(lab_s)]))), voxels=vox_s[keep])


class Table:
    """A stand-in for the ``SynTable`` columns ``combine_and_split_syn`` reads."""

    def __init__(self, ids, voxel_lists, sym_prop, asym_prop):
        self.ids = np.asarray(ids, np.uint64)
        self.voxels = np.concatenate([np.asarray(v).reshape(-1, 3) for v in voxel_lists]).astype(np.uint32) if len(voxel_lists) else np.zeros((0, 3), np.uint32)
        self.vox_begin = np.concatenate(([0], np.cumsum([len(v) for v in voxel_lists]))).astype(np.int64)
        self.sym_prop, self.asym_prop = np.asarray(sym_prop, np.float64), np.asarray(asym_prop, np.float64)


def assert_tables_equal(got, want, what=''):
    """Two ``SynSsvTable``: every column, integers exact, floats bit for bit."""
    for name in type(want).COLUMNS:
        a, b = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        if b.dtype.kind == 'f':
            assert a.astype(np.float64).tobytes() == b.astype(np.float64).tobytes(), (what, name)
        else:
            assert np.array_equal(a.astype(np.int64), b.astype(np.int64)), (what, name)
    assert got.n_components == want.n_components, what
