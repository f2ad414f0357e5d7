"""Brute-force numpy restatement of the synapse properties (``classify_synssv_objects``, ``collect_properties_from_ssv_partners``,
``export_matrix``), in own words and without scipy or sklearn, pinned to golden g21 by tests/test_syn_props_cpu.py.

Cells are dicts ``id, celltype, vertices (v, 3) float32 nm, vertex_labels {key: (v)}, nodes (m, 3) voxels, node_attrs {key: array}``
(a key may be missing), ``spinehead_vol {syn id: volume}``; a packed forest is a dict ``feature, threshold, left, right, proba,
tree_begin, n_features``.  A *side* is (synapse row i, partner slot p) = 2 i + p."""
import io
from collections import Counter

import numpy as np


def sq_dist(A, B):
    """((dx dx) + dy dy) + dz dz for every row of A (k, 3) against every row of B (l, 3): each product and sum rounded on its own."""
    d = A[:, None, :] - B[None, :, :]
    return ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def scale64(scaling):
    return np.asarray(scaling, np.float32).astype(np.float64)


def knn(points, begin, labels, q_cell, q_xyz, k, extra=0):
    """Segmented k nearest neighbours with vote.  -> vote (q) int32, rows (q, k) int32 padded with -1, d2 (q, k + extra) float64 padded
    with inf.  The neighbours of a query are the first min(k, points of its cell) points of the cell in the order of (d^2, row); the
    vote is ``Counter(labels in that order).most_common(1)``; -1 for a cell without points.  `extra` more d^2 are reported (for
    ``ambiguous``); labels None: the row is the label."""
    P = np.asarray(points).astype(np.float64).reshape(-1, 3)
    begin = np.asarray(begin, np.int64)
    q_xyz = np.asarray(q_xyz, np.float64).reshape(-1, 3)
    n_q = len(q_cell)
    vote, rows = np.full(n_q, -1, np.int32), np.full((n_q, k), -1, np.int32)
    d2 = np.full((n_q, k + extra), np.inf)
    for q in range(n_q):
        b0, b1 = int(begin[q_cell[q]]), int(begin[q_cell[q] + 1])
        if b1 == b0:
            continue
        d = sq_dist(P[b0:b1], q_xyz[q][None])[:, 0]
        order = np.argsort(d, kind='stable')                      # stable: equal d^2 stay in row order
        near = order[:k] + b0
        lab = near if labels is None else np.asarray(labels)[near]
        vote[q] = Counter(lab.tolist()).most_common(1)[0][0]      # most_common keeps first-seen order among equal counts
        rows[q, :len(near)] = near
        m = min(k + extra, len(order))
        d2[q, :m] = d[order[:m]]
    return vote, rows, d2


def ambiguous(d2, rel=1e-9):
    """Queries whose reported d^2 (ascending, k + 1 of them) hold two that are not further apart than a relative `rel`."""
    d2 = np.asarray(d2)
    a, b = d2[:, :-1], d2[:, 1:]
    both = np.isfinite(a) & np.isfinite(b)
    with np.errstate(invalid='ignore'):
        close = both & (b - a <= rel * np.maximum(b, np.finfo(np.float64).tiny))
    return close.any(1)


def forest_proba(f, X):
    """The forest's class probabilities (rows, classes) float64: every row as float32, in every tree left iff x[feature] <= threshold
    (float32 widened to float64), the leaves' class fractions summed in tree order, divided by the number of trees."""
    X32 = np.asarray(X, np.float64).astype(np.float32)
    n_trees = len(f['tree_begin']) - 1
    out = np.zeros((len(X32), f['proba'].shape[1]), np.float64)
    for r in range(len(X32)):
        acc = np.zeros(f['proba'].shape[1], np.float64)
        for t in range(n_trees):
            node = int(f['tree_begin'][t])
            while f['left'][node] >= 0:
                node = int(f['left'][node] if np.float64(X32[r, f['feature'][node]]) <= f['threshold'][node] else f['right'][node])
            acc = acc + f['proba'][node]
        out[r] = acc / n_trees
    return out


def spine_points(cell, ds_vertices, ignore_labels, key='spiness'):
    """The vertices and labels the vote of one cell runs over: every ds-th vertex (ds = max(1, ds_vertices // 10) below 5e6 vertices),
    then without the ignored labels."""
    v = np.asarray(cell.get('vertices', np.zeros((0, 3))), np.float32).reshape(-1, 3)
    ds = max(1, ds_vertices // 10) if len(v) < 5e6 else ds_vertices
    lab = np.asarray(cell['vertex_labels'][key]).reshape(-1)[::ds]
    v = v[::ds]
    keep = ~np.isin(lab, list(ignore_labels))
    return v[keep], lab[keep]


def collect_properties(partners, rep, ratio, syn_ids, cells, scaling, k=50, ds_vertices=1, ignore_labels=(4, 5), ax_key='axoness_avg10000',
                       n_embedding=10, sym_thresh=0.225):
    """-> dict of the six columns.  Per side: no mesh -> zeros everywhere; else spiness = the vote over the cell's spine points,
    celltype, spine-head volume of this synapse (-1 if the cell has none), and from the nearest skeleton node (scaled) the compartment
    and the embedding: -1 / inf without nodes or without the key."""
    s = scale64(scaling)
    by_id = {int(c['id']): c for c in cells}
    n = len(partners)
    out = dict(partner_axoness=np.zeros((n, 2), np.int32), partner_spiness=np.zeros((n, 2), np.int32), partner_celltypes=np.zeros((n, 2), np.int32),
               partner_spineheadvol=np.zeros((n, 2), np.float32), latent_morph=np.zeros((n, 2, n_embedding), np.float32),
               syn_sign=np.where(np.asarray(ratio) > sym_thresh, -1, 1).astype(np.int64))
    for i in range(n):
        q = (np.asarray(rep[i]).astype(np.float64) * s)[None]
        for p in (0, 1):
            if int(partners[i][p]) not in by_id:
                raise ValueError(f'Could not find the partner cell {int(partners[i][p])}')
            c = by_id[int(partners[i][p])]
            if len(np.asarray(c.get('vertices', np.zeros((0, 3)))).reshape(-1, 3)) == 0:
                continue
            v, lab = spine_points(c, ds_vertices, ignore_labels)
            if len(v) == 0:
                raise ValueError('all vertices ignored')
            out['partner_spiness'][i, p] = knn(v, [0, len(v)], lab, [0], q, min(k, len(v)))[0][0]
            out['partner_celltypes'][i, p] = c.get('celltype', -1)
            out['partner_spineheadvol'][i, p] = c.get('spinehead_vol', {}).get(int(syn_ids[i]), -1)
            nodes = np.asarray(c.get('nodes', np.zeros((0, 3))), np.float64).reshape(-1, 3)
            ax, lm = -1, np.full(n_embedding, np.inf, np.float32)
            if len(nodes):
                j = knn(nodes * s, [0, len(nodes)], None, [0], q, 1)[0][0]
                attrs = c.get('node_attrs', {})
                if ax_key in attrs:
                    ax = np.asarray(attrs[ax_key]).reshape(-1)[j]
                if 'latent_morph' in attrs:
                    lm = np.asarray(attrs['latent_morph'], np.float32).reshape(len(nodes), -1)[j]
            out['partner_axoness'][i, p] = ax
            out['latent_morph'][i, p] = lm
    return out


def conn_mat_bytes(rep, partners, props, syn_prob, mesh_area, threshold=0):
    """The bytes of conn_mat.csv: rows with syn_prob > threshold; columns x y z ssv1 ssv2 size comp1 comp2 celltype1 celltype2 spiness1
    spiness2 synprob spinehead_vol1 spinehead_vol2 latentmorph1_* latentmorph2_*; size = mesh_area / 2 * syn_sign; '%.18e', tabs."""
    syn_prob = np.asarray(syn_prob, np.float64)
    m = syn_prob > threshold
    e = props['latent_morph'].shape[2]
    size = (np.asarray(mesh_area, np.float64)[m] / 2 * props['syn_sign'][m])[:, None]
    cols = [np.asarray(rep)[m], np.asarray(partners)[m], size, props['partner_axoness'][m], props['partner_celltypes'][m], props['partner_spiness'][m],
            syn_prob[m][:, None], props['partner_spineheadvol'][m], props['latent_morph'][m].reshape(int(m.sum()), 2 * e)]
    table = np.concatenate([np.asarray(c, np.float64) for c in cols], 1)
    names = ['x', 'y', 'z', 'ssv1', 'ssv2', 'size', 'comp1', 'comp2', 'celltype1', 'celltype2', 'spiness1', 'spiness2', 'synprob',
             'spinehead_vol1', 'spinehead_vol2'] + [f'latentmorph{p}_{j}' for p in (1, 2) for j in range(e)]
    lines = ['# ' + '\t'.join(names)] + ['\t'.join('%.18e' % v for v in row) for row in table]
    return ('\n'.join(lines) + '\n').encode()


# -- the flat layout of golden g21 ----------------------------------------------------------------------------------------------------
def cells_from_case(c):
    """The cell dicts of one case of g21 (see tests/golden/make_golden_syn_props.py for the arrays)."""
    cells = []
    e = c['cell_latent'].shape[1]
    for j, cid in enumerate(c['cell_ids'].tolist()):
        v0, v1, n0, n1 = c['cell_vert_begin'][j], c['cell_vert_begin'][j + 1], c['cell_node_begin'][j], c['cell_node_begin'][j + 1]
        attrs = {}
        if c['cell_has_ax'][j]:
            attrs['axoness_avg10000'] = c['cell_ax'][n0:n1]
        if c['cell_has_latent'][j]:
            attrs['latent_morph'] = c['cell_latent'][n0:n1].reshape(n1 - n0, e)
        s0, s1 = c['cell_sh_begin'][j], c['cell_sh_begin'][j + 1]
        cells.append(dict(id=cid, celltype=int(c['cell_celltypes'][j]), vertices=c['cell_verts'][v0:v1], vertex_labels={'spiness': c['cell_spiness'][v0:v1]},
                          nodes=c['cell_nodes'][n0:n1], node_attrs=attrs,
                          spinehead_vol=dict(zip(c['cell_sh_ids'][s0:s1].tolist(), c['cell_sh_vol'][s0:s1].tolist()))))
    return cells


def forest_from_case(c):
    return dict(feature=c['rf_feature'], threshold=c['rf_threshold'], left=c['rf_left'], right=c['rf_right'], proba=c['rf_proba'],
                tree_begin=c['rf_tree_begin'], n_features=int(c['rf_n_features']))
