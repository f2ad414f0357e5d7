"""Golden vectors for the skeleton votes (``majorityvote_skeleton_property``, ``majority_vote_compartments``, ``semsegaxoness2skel``),
produced by the REFERENCE'S OWN code: the two functions of /root/reference/syconn/reps/super_segmentation_helper.py (:1270-1302,
:1233-1266), ``semsegaxoness2skel`` (reps/super_segmentation_object.py:3497-3557), the methods ``weighted_graph`` (:1420-1458) and
``semseg_for_coords`` (:2190-2240) and ``colorcode_vertices`` (reps/rep_helper.py:281-334) are lifted by AST at generation time and run
unchanged over networkx and scipy's cKDTree.  The cell object is an in-memory stand-in.  Nothing compiled and no reference text is
stored: inputs and outputs only, as flat arrays.

    python tests/golden/make_golden_skeleton.py      ->  tests/golden/g23_skeleton.npz

Notes.  ``weighted_graph`` indexes ``node_scaled[edges]``: a cell without edges works only with an edge array of shape (0, 2), which
the stand-in passes.  ``n_reached`` (the window sizes) is not a value the reference returns: it is ``len(nx.single_source_dijkstra_path
(g, n, max_dist))`` on the reference's graph, the call the reference makes.  The reference passes ``n_jobs=`` to ``cKDTree.query``,
which scipy 1.15 no longer accepts: the stand-in tree forwards it as ``workers``.

Three sets of cells, every cell run on its own through the reference.  Per set the cells are concatenated: ``*_nodes`` (n, 3) voxels,
``*_node_begin``, ``*_edges`` (e, 2) node indices inside the cell, ``*_edge_begin``, ``*_labels``, ``*_scaling``, ``*_max_dist``.
``a_`` scaling (10, 10, 20), integer nodes, max_dist 1000, outputs ``a_vote`` / ``a_reached``.  Cells (asserted in ``main``): 0 a path
on the 100 nm lattice with a node exactly at max_dist and the next edge beyond it; 1 a lattice cycle whose arcs differ in length; 2 a
zero-weight edge; 3 a duplicate edge and a self loop; 4 a vote tie decided by the smaller label; 5 a cell without edges; 6 one node;
7 an empty skeleton; 8, 9 two cells with identical coordinates; 10 a random tree with extra cycles.
``b_`` scaling (9, 9, 20) as float32, float64 nodes off every lattice, max_dist 1500: 0 a cycle, 1 a random graph.
``c_`` the compartment vote, outputs ``c_comp`` (float64): 0 label 1 with 33 of 50 nodes (share exactly 0.66: stays 1); 1 with 32 of
50 (becomes 0); 2 a soma node that splits a path in two components with different majorities; 3 a node whose neighbours are all
soma, and 4 a cell of soma nodes only; 5 a tie of counts; 6 a random graph with labels 0 .. 4.
``s_`` ``semsegaxoness2skel`` with map_properties k 20, ds_vertices 20 (every second vertex), ignore_labels [5], max_dist 2000:
``s_verts`` float32 nm on the 1/8 nm lattice / ``s_vert_begin`` / ``s_vert_labels``; outputs ``s_pred``, ``s_avg``, ``s_comp``.  Cell 0:
an axon with bouton predictions 3 and 4 (recovered in both smoothed keys), a soma, a dendrite with one bouton prediction (not
recovered); cell 1: random labels (no query has two equal d^2 among its first k + 1 neighbours); cell 2: nodes but no mesh, cell 3:
mesh but no nodes -- the reference's zero branch, ``s_zero_shapes`` = the shapes it stored."""
import os
import sys
import types
from collections import Counter

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_cs import lift_function  # noqa: E402
from make_golden_syn_props import lift_method  # noqa: E402

REF = '/root/reference/syconn'
MAP = dict(k=20, ds_vertices=20, ignore_labels=[5])
S_MAX_DIST = 2000


def lifted():
    import scipy.spatial

    class Tree:
        def __init__(self, data):
            self.t = scipy.spatial.cKDTree(data)

        def query(self, x, k=1, n_jobs=1, **kw):
            return self.t.query(x, k=k, workers=n_jobs, **kw)
    log = types.SimpleNamespace(debug=lambda *a: None, info=lambda *a: None, error=lambda *a: None, warning=lambda *a: None, warn=lambda *a: None)
    helper_ns = {'np': np, 'spatial': types.SimpleNamespace(cKDTree=Tree), 'Counter': Counter, 'log_reps': log}
    ssh_ns = {'np': np, 'nx': nx, 'log_reps': log}
    exec('from typing import *', ssh_ns)
    ssh_path, sso_path = f'{REF}/reps/super_segmentation_helper.py', f'{REF}/reps/super_segmentation_object.py'
    ssh = types.SimpleNamespace(majorityvote_skeleton_property=lift_function(ssh_path, 'majorityvote_skeleton_property', ssh_ns),
                                majority_vote_compartments=lift_function(ssh_path, 'majority_vote_compartments', ssh_ns))
    sso_ns = {'np': np, 'nx': nx, 'log_reps': log, 'ssh': ssh, 'SuperSegmentationObject': object}
    exec('from typing import *', sso_ns)
    sso_ns['colorcode_vertices'] = lift_function(f'{REF}/reps/rep_helper.py', 'colorcode_vertices', helper_ns)

    class SSO:
        weighted_graph = lift_method(sso_path, 'SuperSegmentationObject', 'weighted_graph', sso_ns)
        semseg_for_coords = lift_method(sso_path, 'SuperSegmentationObject', 'semseg_for_coords', sso_ns)

        def __init__(self, cid, nodes, edges, scaling, attrs=None, verts=None, vert_labels=None):
            self.id, self.scaling, self.nb_cpus, self._weighted_graph, self.saved = cid, scaling, 1, None, 0
            self.skeleton = dict(nodes=nodes, edges=np.asarray(edges, np.int64).reshape(-1, 2), **(attrs or {}))
            verts = np.zeros((0, 3), np.float32) if verts is None else verts
            self.mesh = (np.zeros(0, np.uint32), verts.reshape(-1).copy(), np.zeros(0, np.float32))
            self._labels = vert_labels or {}

        def load_skeleton(self):
            pass

        def save_skeleton(self):
            self.saved += 1

        def label_dict(self, what):
            assert what == 'vertex'
            return self._labels
    return SSO, ssh, lift_function(sso_path, 'semsegaxoness2skel', sso_ns)


def random_graph(rng, n, extra, lo, hi, integer):
    nodes = rng.uniform(lo, hi, (n, 3))
    nodes = np.round(nodes).astype(np.int64) if integer else nodes
    edges = [(int(rng.integers(0, i)), i) for i in range(1, n)] + [tuple(int(v) for v in rng.integers(0, n, 2)) for _ in range(extra)]
    return nodes, np.array(edges, np.int64).reshape(-1, 2)


def path_edges(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)], 1).astype(np.int64).reshape(-1, 2)


def set_a(rng):
    cells = []
    # 0: path along x, 10 voxels = 100 nm per edge; from node 0 node 10 is exactly at 1000 nm, node 11 beyond
    cells.append((np.stack([10 * np.arange(24), np.zeros(24), np.zeros(24)], 1).astype(np.int64), path_edges(24), (np.arange(24) // 5) % 3))
    # 1: lattice cycle 0-1-2-3-4-0, arcs from 0 to 3: 300 + 400 + 300 nm one way, 200 + 200 the other
    cells.append((np.array([(0, 0, 0), (30, 0, 0), (30, 40, 0), (0, 40, 0), (0, 20, 0)], np.int64),
                  np.array([(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)], np.int64), np.array([0, 1, 1, 2, 2])))
    # 2: nodes 1 and 2 on one coordinate
    cells.append((np.array([(0, 0, 0), (40, 0, 0), (40, 0, 0), (40, 60, 0), (40, 100, 0)], np.int64), path_edges(5), np.array([3, 1, 1, 3, 3])))
    # 3: edge (0, 1) twice, a self loop at 2
    cells.append((np.array([(0, 0, 0), (50, 0, 0), (50, 50, 0), (50, 50, 30)], np.int64),
                  np.array([(0, 1), (1, 0), (1, 2), (2, 2), (2, 3)], np.int64), np.array([2, 0, 0, 2])))
    # 4: two nodes, labels 3 and 1: one each, the smaller wins
    cells.append((np.array([(0, 0, 0), (5, 0, 0)], np.int64), path_edges(2), np.array([3, 1])))
    cells.append((np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0)], np.int64), np.zeros((0, 2), np.int64), np.array([4, 0, 2])))      # 5: no edges
    cells.append((np.array([(7, 7, 7)], np.int64), np.zeros((0, 2), np.int64), np.array([1])))                                  # 6: one node
    cells.append((np.zeros((0, 3), np.int64), np.zeros((0, 2), np.int64), np.zeros(0, np.int64)))                               # 7: empty
    nodes, edges = random_graph(rng, 40, 3, 0, 150, True)
    cells.append((nodes, edges, rng.integers(0, 3, 40)))                                                                        # 8
    cells.append((nodes.copy(), edges.copy(), rng.integers(0, 3, 40)))                                                          # 9: the same place
    nodes, edges = random_graph(rng, 120, 8, 0, 260, True)
    cells.append((nodes, edges, rng.integers(0, 5, 120)))                                                                       # 10
    return cells, np.array([10, 10, 20]), 1000


def set_b(rng):
    cells = []
    ang = np.sort(rng.uniform(0, 2 * np.pi, 30))
    ring = np.stack([300 + 250 * np.cos(ang), 300 + 250 * np.sin(ang), rng.uniform(0, 40, 30)], 1)
    cells.append((ring, np.concatenate([path_edges(30), [(29, 0)]]), rng.integers(0, 4, 30)))
    nodes, edges = random_graph(rng, 150, 12, -50.5, 320.25, False)
    cells.append((nodes, edges, rng.integers(0, 6, 150)))
    return cells, np.array([9, 9, 20], np.float32), 1500


def set_c(rng):
    z = lambda n: np.zeros((n, 3), np.int64)
    cells = []
    for ones in (33, 32):
        lab = np.zeros(50, np.int64)
        lab[rng.permutation(50)[:ones]] = 1
        cells.append((z(50), path_edges(50), lab))
    cells.append((z(9), path_edges(9), np.array([1, 1, 1, 1, 2, 0, 0, 1, 0])))                      # 2: 1 1 1 1 | soma | 0 0 1 0
    cells.append((z(4), np.array([(0, 1), (1, 2), (1, 3)], np.int64), np.array([2, 3, 2, 2])))      # 3: node 1 between soma nodes
    cells.append((z(3), path_edges(3), np.array([2, 2, 2])))                                        # 4: soma only
    cells.append((z(6), path_edges(6), np.array([4, 1, 4, 1, 3, 3])))                               # 5: 1, 3, 4 twice each -> 1 at share 1/3 -> 0
    nodes, edges = random_graph(rng, 160, 6, 0, 100, True)
    cells.append((nodes, edges, rng.choice(5, 160, p=[0.3, 0.35, 0.15, 0.1, 0.1])))                 # 6
    return cells


def set_s(rng):
    scaling = np.array([10, 10, 20])

    def cloud(centre_nm, spread, n):
        return (np.round((np.asarray(centre_nm, np.float64) + rng.uniform(-spread, spread, (n, 3))) * 8) / 8).astype(np.float32)
    # cell 0: 30 nodes 100 voxels = 1000 nm apart along x; 2 k vertices within 30 nm of every node, all with the node's label
    want = np.array([1, 1, 3, 1, 1, 4, 1, 1, 1, 3, 1, 1, 2, 2, 2, 0, 0, 0, 3, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0])
    nodes0 = np.stack([100 * np.arange(30), np.full(30, 50), np.full(30, 25)], 1).astype(np.int64)
    v0 = np.concatenate([cloud(p * scaling, 30, 2 * MAP['k']) for p in nodes0])
    l0 = np.repeat(want, 2 * MAP['k'])
    l0[1::2] = 5                                                                    # the skipped half: the ignored label, never seen
    l0[::14] = 5                                                                    # and some of the kept ones are ignored
    # cell 1: a random graph inside a cloud of randomly labelled vertices
    nodes1, edges1 = random_graph(rng, 60, 4, 0, 120, True)
    v1 = cloud((600, 600, 1200), 700, 900)
    l1 = rng.integers(0, 6, 900)
    nodes2 = np.array([(0, 0, 0), (10, 0, 0)], np.int64)
    cells = [(nodes0, path_edges(30), v0, l0), (nodes1, edges1, v1, l1), (nodes2, path_edges(2), np.zeros((0, 3), np.float32), np.zeros(0, np.int64)),
             (np.zeros((0, 3), np.int64), np.zeros((0, 2), np.int64), cloud((0, 0, 0), 50, 10), np.ones(10, np.int64))]
    return cells, scaling, want


def concat(cells, cols):
    out = {}
    for name, i, width in cols:
        parts = [np.asarray(c[i]).reshape((-1, width) if width else (-1,)) for c in cells]
        out[name] = np.concatenate(parts)
        out[name + '_begin'] = np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.int64)
    return out


def main():
    SSO, ssh, semsegaxoness2skel = lifted()
    rng = np.random.default_rng(2301)
    g = {}
    for prefix, (cells, scaling, max_dist) in (('a_', set_a(rng)), ('b_', set_b(rng))):
        votes, reached, dists = [], [], []
        for cid, (nodes, edges, lab) in enumerate(cells):
            sso = SSO(cid, nodes, edges, scaling, dict(prop=np.asarray(lab)))
            res = ssh.majorityvote_skeleton_property(sso, 'prop', max_dist, return_res=True)
            votes.append(np.asarray(res, np.int64).reshape(-1))
            graph = sso.weighted_graph()
            reached.append(np.array([len(nx.single_source_dijkstra_path(graph, n, max_dist)) for n in range(len(nodes))], np.int64))
            dists.append([nx.single_source_dijkstra_path_length(graph, n) for n in range(len(nodes))])
            assert sso.saved == 0
        c = concat(cells, (('nodes', 0, 3), ('edges', 1, 2)))
        g.update({prefix + 'nodes': c['nodes'], prefix + 'node_begin': c['nodes_begin'], prefix + 'edges': c['edges'],
                  prefix + 'edge_begin': c['edges_begin'], prefix + 'labels': np.concatenate([np.asarray(x[2], np.int64) for x in cells]),
                  prefix + 'scaling': scaling, prefix + 'max_dist': np.int64(max_dist), prefix + 'vote': np.concatenate(votes),
                  prefix + 'reached': np.concatenate(reached)})
        if prefix == 'a_':
            d0 = dists[0][0]
            assert d0[10] == 1000.0 and d0[11] == 1100.0 and reached[0][0] == 11 and reached[0][12] == 21
            d1 = dists[1][0]
            assert d1[3] == 400.0 and d1[2] == 700.0                               # the short arc 0-4-3
            assert dists[2][1][2] == 0.0 and reached[2][0] == 4
            assert reached[3].tolist() == [3, 3, 4, 2]
            assert votes[4].tolist() == [1, 1]
            assert votes[5].tolist() == [4, 0, 2] and reached[5].tolist() == [1, 1, 1] and votes[6].tolist() == [1] and len(votes[7]) == 0
            assert np.array_equal(reached[8], reached[9]) and not np.array_equal(votes[8], votes[9])
            assert reached[10].min() < reached[10].max() < 120
        else:
            assert reached[0].min() >= 3 and reached[0].max() < 30 and reached[1].max() < 150
    cells = set_c(rng)
    comp = []
    for cid, (nodes, edges, lab) in enumerate(cells):
        sso = SSO(cid, nodes, edges, np.array([10, 10, 20]), dict(axoness_avg10000=np.asarray(lab)))
        ssh.majority_vote_compartments(sso, 'axoness_avg10000')
        assert sso.saved == 1 and sso.skeleton['axoness_avg10000_comp_maj'].dtype == np.float64
        comp.append(sso.skeleton['axoness_avg10000_comp_maj'])
    assert (comp[0] == 1).all() and (comp[1] == 0).all()
    assert comp[2].tolist() == [1, 1, 1, 1, 2, 0, 0, 0, 0] and comp[3].tolist() == [2, 3, 2, 2] and comp[4].tolist() == [2, 2, 2]
    assert (comp[5] == 0).all()
    c = concat(cells, (('nodes', 0, 3), ('edges', 1, 2)))
    g.update(c_node_begin=c['nodes_begin'], c_edges=c['edges'], c_edge_begin=c['edges_begin'],
             c_labels=np.concatenate([np.asarray(x[2], np.int64) for x in cells]), c_comp=np.concatenate(comp))
    cells, scaling, want = set_s(rng)
    keys = ('axoness', 'axoness_avg%d' % S_MAX_DIST, 'axoness_avg%d_comp_maj' % S_MAX_DIST)
    outs, zero_shapes = [[], [], []], []
    for cid, (nodes, edges, verts, vlab) in enumerate(cells):
        sso = SSO(cid, nodes, edges, scaling, None, verts, dict(axoness=np.asarray(vlab)))
        semsegaxoness2skel(sso, dict(MAP), 'axoness', S_MAX_DIST)
        assert sso.saved >= 1
        if cid >= 2:
            zero_shapes.append([sso.skeleton[k].shape for k in keys[1:]])
            assert not sso.skeleton[keys[1]].any() and keys[0] not in sso.skeleton
            for o in outs:
                o.append(np.zeros(len(nodes)))
            continue
        for o, k in zip(outs, keys):
            o.append(np.asarray(sso.skeleton[k]).reshape(-1))
        if cid == 0:
            pred, avg, cm = (o[-1] for o in outs)
            merged = np.where(want >= 3, 1, want)
            assert np.array_equal(pred, merged)
            assert avg[2] == 3 and avg[5] == 4 and avg[9] == 3 and cm[2] == 3 and cm[5] == 4 and avg[18] == 0 and cm[18] == 0 and cm[24] == 0
            assert (avg[12:15] == 2).all()
        else:
            import scipy.spatial
            ds = max(1, MAP['ds_vertices'] // 10)
            kept = verts[::ds][np.asarray(vlab)[::ds] != 5].astype(np.float64)
            d, _ = scipy.spatial.cKDTree(kept).query(nodes * scaling, k=MAP['k'] + 1)
            assert (np.diff(d, axis=1) > 0).all()
    c = concat(cells, (('nodes', 0, 3), ('edges', 1, 2), ('verts', 2, 3)))
    g.update(s_nodes=c['nodes'], s_node_begin=c['nodes_begin'], s_edges=c['edges'], s_edge_begin=c['edges_begin'], s_verts=c['verts'].astype(np.float32),
             s_vert_begin=c['verts_begin'], s_vert_labels=np.concatenate([np.asarray(x[3], np.int64) for x in cells]), s_scaling=scaling,
             s_max_dist=np.int64(S_MAX_DIST), s_k=np.int64(MAP['k']), s_ds_vertices=np.int64(MAP['ds_vertices']),
             s_ignore_labels=np.array(MAP['ignore_labels'], np.int64), s_pred=np.concatenate(outs[0]).astype(np.int32),
             s_avg=np.concatenate(outs[1]).astype(np.int32), s_comp=np.concatenate(outs[2]).astype(np.float64),
             s_zero_shapes=np.array(zero_shapes, np.int64))
    out = os.path.join(HERE, 'g23_skeleton.npz')
    np.savez_compressed(out, **g)
    print('wrote', out, os.path.getsize(out), 'bytes;', {k: v.shape for k, v in g.items()})


if __name__ == '__main__':
    main()
