"""Golden vectors for the astrocyte splitting, produced by the REFERENCE'S OWN code: ``remove_glia_nodes`` and ``create_ccsize_dict``
(/root/reference/syconn/proc/graphs.py:278-360, :220-249), ``glia_pred_so`` and ``glia_proba_so`` (reps/segmentation_helper.py:32-78) and
the ``SegmentationObject`` members ``glia_pred`` / ``glia_proba`` (reps/segmentation.py:799-828) are lifted by AST at generation time and
run unchanged over networkx, with a stand-in namespace for ``global_params.config['min_cc_size_ssv']``.  Nothing compiled and no
reference text is stored: inputs and outputs only, as flat arrays.

    python tests/golden/make_golden_glia_split.py      ->  tests/golden/g26_glia_split.npz

What cannot be lifted (the file-bound ``write_astrocyte_svgraph``, proc/glia_splitting.py:96-103, :125-129, :147-154) is done here over
networkx with the reference's own calls (``g.copy()``, ``remove_node``, ``nx.connected_components``, the ``ccsize_dict[ix] <
min_ssv_size`` loops).  The per-node sizes of steps 1 / 2 and of step 3 are the lifted ``create_ccsize_dict`` over sub-graphs made the
way ``remove_glia_nodes`` makes them.

``e_edges`` (e, 2) uint64 and ``e_nodes`` (nodes without an edge): the graph of all cells; ``t_ids`` / ``t_boxes`` (n, 2, 3) float64 /
``t_f32`` (the row's cell was run with float32 boxes; widening is exact) / ``t_glia`` / ``t_sizes`` (voxels): the table; ``T``.
``o_``: per node ``node_ids`` / ``node_cell`` / ``node_class`` / ``node_comp`` / ``node_size1`` / ``node_size2``, per cell ``cell_ids`` /
``cell_outcome``, the tables ``ncc_`` / ``gcc_`` + ``ids`` / ``cell`` / ``begin`` / ``sv``, ``neuron_edges`` / ``astrocyte_edges``.
``w_``: the same split graphs and tables after the size filter of write_astrocyte_svgraph with ``w_cell_size`` (per table row) and
``w_min``, and ``w_total_size``.  ``p_``: glia_pred inputs ``p_probas`` (float64, multiples of 2^-12) / ``p_view_begin`` / ``p_thresh`` and
per dtype d in (f32, f64), threshold k and mode m (0 multi-view, 1 point models) ``p_cls_{d}_{k}_{m}``, per dtype ``p_mean_{d}``."""
import os
import sys
import types
import warnings

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _glia_ref as R  # noqa: E402
from make_golden_cs import lift_function  # noqa: E402
from make_golden_syn_props import lift_method  # noqa: E402

REF = '/root/reference/syconn'
U = np.uint64
T = 2600


class Cells:
    def __init__(self):
        self.edges, self.extra, self.table, self.cells, self.next_id = [], [], {}, [], 10

    def cell(self, nodes, edges, f32=False, ids=None, extra=()):
        """nodes: list of (glia, (lo, hi)) with lo / hi a number (a box on the x axis) or a 3-vector; edges: index pairs."""
        ids = list(range(self.next_id, self.next_id + len(nodes))) if ids is None else list(ids)
        self.next_id = max(self.next_id, 0 if ids[0] >= 2 ** 62 else max(ids) + 1) + 3
        for i, (g, (lo, hi)) in zip(ids, nodes):
            lo, hi = (np.array([v, 0, 0]) if np.isscalar(v) else np.array(v) for v in (lo, hi))
            self.table[i] = (int(g), np.array([lo, hi], np.float32 if f32 else np.float64))
        e = [(ids[a], ids[b]) for a, b in edges]
        self.edges += e
        self.extra += [ids[k] for k in extra]
        self.cells.append(dict(ids=ids, edges=e, f32=f32))
        return ids


def build(rng):
    c, name = Cells(), {}
    N, G = 0, 1
    path = lambda k: [(a, a + 1) for a in range(k - 1)]
    for f32 in (False, True):
        s = '_f32' if f32 else ''
        name['out1' + s] = c.cell([(N, (0, 1000)), (G, (1000, 4000)), (N, (3000, 3500))], path(3), f32)
        name['out2' + s] = c.cell([(N, (0, 3000)), (G, (3000, 3500))], path(2), f32)
        name['out3' + s] = c.cell([(N, (0, 3000)), (G, (0, 3000))], path(2), f32)
        # a tiny glia fragment (1) rejoins two neuron pieces (0, 2) below T each, 3100 together; 4 is the significant neuron piece behind the glia 3
        name['rejoin' + s] = c.cell([(N, (0, 1500)), (G, (1500, 1600)), (N, (1600, 3100)), (G, (0, 3000)), (N, (0, 3000))], [(0, 1), (1, 2), (0, 3), (3, 4)], f32)
        # an orphan neuron piece (2) behind the glia: it goes to the glia set
        name['orphan' + s] = c.cell([(N, (0, 3000)), (G, (0, 3000)), (N, (100, 600))], path(3), f32)
        # ties: extent (600, 800, 2400) is exactly 2600
        tie = ((100, 100, 100), (700, 900, 2500))
        name['tie1' + s] = c.cell([(N, tie), (G, (0, 3000))], path(2), f32)        # a neuron component of exactly T in step 1: not significant
        # a glia component (2) of exactly T in step 3: not tiny, so the neuron piece 3 behind it is an orphan
        name['tie_glia' + s] = c.cell([(N, (0, 3000)), (G, (0, 3000)), (G, tie), (N, (100, 600))], [(0, 1), (0, 2), (2, 3)], f32)
        # a neuron piece (2) of exactly T behind the glia: not below T, it stays
        name['tie_stay' + s] = c.cell([(N, (0, 3000)), (G, (0, 3000)), (N, tie)], path(3), f32)
    name['no_neuron'] = c.cell([(G, (0, 3000)), (G, (10, 20))], path(2))
    name['no_glia_big'] = c.cell([(N, (0, 3000)), (N, (10, 20))], path(2))
    name['no_glia_small'] = c.cell([(N, (0, 100)), (N, (10, 20))], path(2))
    name['loop_neuron'] = c.cell([(N, (0, 3000))], [(0, 0)])
    name['loop_neuron_small'] = c.cell([(N, (0, 30))], [(0, 0)])
    name['loop_glia'] = c.cell([(G, (0, 3000))], [(0, 0)], True)
    name['node_only'] = c.cell([(N, (0, 3000))], [], extra=(0,))
    name['dup'] = c.cell([(N, (0, 3000)), (G, (0, 3000)), (N, (0, 2000))], [(0, 1), (1, 0), (0, 1), (1, 2), (2, 2), (1, 1)])
    name['big_ids'] = c.cell([(N, (0, 3000)), (G, (0, 3000))], [(1, 0)], ids=(2 ** 63, 2 ** 64 - 1))
    for k in range(60):                                                            # random connected cells on a 100 nm lattice
        n = int(rng.integers(2, 30))
        x0 = rng.integers(0, 30, n) * 100
        nodes = [(int(rng.random() < 0.45), (int(a), int(a + rng.integers(1, 12) * 100))) for a in x0]
        edges = [(int(rng.integers(0, b)), b) for b in range(1, n)] + [tuple(rng.integers(0, n, 2).tolist()) for _ in range(int(rng.integers(0, n)))]
        edges = [e[::-1] if rng.random() < 0.5 else e for e in edges]
        c.cell(nodes, [edges[i] for i in rng.permutation(len(edges))], f32=bool(k % 2))
    return c, name


def run_cells(c, remove_glia_nodes, create_ccsize_dict):
    """-> per node dicts (cell, class, comp, size1, size2), outcome per cell id, the lists per cell."""
    node = {}
    outcome, lists = {}, {}
    for cell in c.cells:
        g = nx.Graph()
        g.add_nodes_from(cell['ids'])
        g.add_edges_from(cell['edges'])
        assert nx.is_connected(g)
        size_dict = {i: c.table[i][1] for i in cell['ids']}
        glia_dict = {i: c.table[i][0] for i in cell['ids']}
        n_ccs, g_ccs = remove_glia_nodes(g, size_dict, glia_dict, return_removed_nodes=True)
        assert remove_glia_nodes(g, size_dict, glia_dict) == n_ccs
        oc = 1 if not n_ccs else (2 if not g_ccs else 3)
        cid = min(cell['ids'])
        outcome[cid], lists[cid] = oc, (sorted(sorted(x) for x in n_ccs), sorted(sorted(x) for x in g_ccs))
        # sizes of steps 1 / 2: the two sub-graphs as remove_glia_nodes makes them
        s1 = {}
        for keep in (0, 1):
            sub = g.copy()
            for n in g.nodes():
                if (glia_dict[n] != 0) != bool(keep):
                    sub.remove_node(n)
            s1.update(create_ccsize_dict(sub, size_dict))
        s2 = {}
        if oc == 3:
            tiny = [n for n in g.nodes() if glia_dict[n] != 0 and s1[n] < T]
            sub = g.copy()
            for n in g.nodes():
                if glia_dict[n] != 0 and n not in tiny:
                    sub.remove_node(n)
            s2 = create_ccsize_dict(sub, size_dict)
        for k, ccs in enumerate((n_ccs, g_ccs)):
            for cc in ccs:
                for n in cc:
                    node[n] = dict(cell=cid, cls=k, comp=min(cc), size1=float(s1[n]), size2=float(s2.get(n, np.nan)))
        for v in list(s1.values()) + list(s2.values()):                            # sizes exact in the box dtype, none next to T
            assert float(v) == float(int(v)) and (v == T or abs(float(v) - T) > 1e-6 * T), v
            assert isinstance(v, np.float32 if cell['f32'] else np.float64)
    return node, outcome, lists


def csr(ccs):
    ccs = sorted((sorted(int(n) for n in cc) for cc in ccs), key=lambda cc: cc[0])
    return (np.array([cc[0] for cc in ccs], U), np.concatenate(([0], np.cumsum([len(cc) for cc in ccs]))).astype(np.int64),
            np.array([n for cc in ccs for n in cc], U))


def split_graph(c, node, create_ccsize_dict, cell_size_of=None, min_ssv_size=None):
    """write_astrocyte_svgraph :96-103, :125-129, :147-154 with the reference's calls."""
    g = nx.Graph()
    g.add_nodes_from(c.extra)
    g.add_edges_from(c.edges)
    astrocyte_svs = [n for n in g.nodes() if node[n]['cls'] == 1]
    neuron_g = g.copy()
    for ix in astrocyte_svs:
        neuron_g.remove_node(ix)
    astrocyte_g = g.copy()
    for ix in neuron_g.nodes():
        astrocyte_g.remove_node(ix)
    if cell_size_of is not None:
        for graph in (neuron_g, astrocyte_g):
            for ix in list(graph.nodes()):
                if cell_size_of[ix] < min_ssv_size:
                    graph.remove_node(ix)
    out = {}
    for key, graph in (('n', neuron_g), ('g', astrocyte_g)):
        ccs = list(nx.connected_components(graph))
        ids, begin, sv = csr(ccs)
        kept = np.array([graph.has_node(a) and graph.has_node(b) for a, b in c.edges], bool)
        edges = np.array(c.edges, dtype=object)[kept]
        assert {frozenset(e) for e in edges.tolist()} == {frozenset(e) for e in graph.edges()}
        out[f'{key}cc_ids'], out[f'{key}cc_begin'], out[f'{key}cc_sv'] = ids, begin, sv
        out[f'{key}cc_cell'] = np.array([node[int(i)]['cell'] for i in ids], U)
        out['neuron_edges' if key == 'n' else 'astrocyte_edges'] = np.array([[int(a), int(b)] for a, b in edges], U).reshape(-1, 2)
    total_size = 0
    for n in astrocyte_g.nodes():
        total_size += c.table[n][2]
    return out, total_size, neuron_g


def pred_set(rng):
    views = [np.zeros(0), np.array([0.5]), np.array([0.125]), np.full(10, 0.25), np.full(7, 0.1875),      # 0 views, 1 view, mean == thresh
             np.array([0.5] * 7 + [0.] * 3), np.array([0.5] * 8 + [0.] * 2),                              # votes == int(10 * 0.7) and one more
             np.array([0.75] * 14 + [0.] * 6), np.array([0.75] * 15 + [0.] * 5),                          # int(20 * 0.7) = 14
             np.array([1.0] * 2 + [0.] * 1), np.array([0.25, 0.25, 0.25 + 2 ** -12])]
    for _ in range(60):
        views.append(rng.integers(0, 4097, int(rng.integers(1, 80))) / 4096.)
    views.append(rng.integers(0, 1200, 4000) / 4096.)
    assert all(len(v) < 4096 for v in views)
    return np.concatenate(views), np.concatenate(([0], np.cumsum([len(v) for v in views]))).astype(np.int64)


def run_pred(probas, view_begin, thresholds):
    ns = {'np': np}
    exec('from typing import *', ns)
    p = f'{REF}/reps/segmentation_helper.py'
    ns['glia_pred_so'], ns['glia_proba_so'] = lift_function(p, 'glia_pred_so', ns), lift_function(p, 'glia_proba_so', ns)
    p = f'{REF}/reps/segmentation.py'
    m_pred, m_proba = lift_method(p, 'SegmentationObject', 'glia_pred', ns), lift_method(p, 'SegmentationObject', 'glia_proba', ns)

    class SO:
        type = 'sv'
        glia_pred, glia_proba = m_pred, m_proba

        def __init__(self, col, point):
            self.attr_dict = {'glia_probas': np.stack([1 - col, col], 1)}
            self.config = types.SimpleNamespace(use_point_models=point)
    out = {}
    for d, dt in (('f32', np.float32), ('f64', np.float64)):
        arr = probas.astype(dt)
        assert (arr.astype(np.float64) == probas).all()
        means = []
        for k, thresh in enumerate(thresholds):
            assert float(dt(thresh)) == thresh
            for m in (0, 1):
                cls = []
                for a, b in zip(view_begin[:-1], view_begin[1:]):
                    so = SO(arr[a:b], bool(m))
                    with warnings.catch_warnings():
                        warnings.simplefilter('ignore')                            # the mean of no views
                        cls.append(int(so.glia_pred(thresh)))
                        if k == 0 and m == 0:
                            means.append(so.glia_proba())
                out[f'p_cls_{d}_{k}_{m}'] = np.array(cls, np.uint8)
                mine, mean64 = R.glia_pred(arr, view_begin, thresh, m)             # the lifted functions agree with a float64 evaluation
                assert (mine == out[f'p_cls_{d}_{k}_{m}']).all(), (d, k, m)
        out[f'p_mean_{d}'] = np.array(means, dt)
        assert all(isinstance(v, dt) for v in means[1:])
        assert np.array_equal(mean64.astype(dt), out[f'p_mean_{d}'], equal_nan=True)
    return out


def main():
    rng = np.random.default_rng(2601)
    c, name = build(rng)
    for i in c.table:                                                              # voxels per supervoxel
        c.table[i] = c.table[i] + (int(rng.integers(1, 10 ** 6)),)
    ns = {'np': np, 'nx': nx, 'global_params': types.SimpleNamespace(config={'min_cc_size_ssv': T})}
    ccsize = lift_function(f'{REF}/proc/graphs.py', 'create_ccsize_dict', ns)
    ns['create_ccsize_dict'] = ccsize
    remove = lift_function(f'{REF}/proc/graphs.py', 'remove_glia_nodes', ns)
    node, outcome, lists = run_cells(c, remove, ccsize)
    ids = np.array(sorted(c.table), U)
    out = dict(e_edges=np.array([[int(a), int(b)] for a, b in c.edges], U), e_nodes=np.array(c.extra, U), t_ids=ids,
               t_boxes=np.array([c.table[int(i)][1].astype(np.float64) for i in ids]), t_f32=np.array([c.table[int(i)][1].dtype == np.float32 for i in ids]),
               t_glia=np.array([c.table[int(i)][0] for i in ids], np.uint8), t_sizes=np.array([c.table[int(i)][2] for i in ids], np.int64), T=np.float64(T))
    col = lambda k, dt: np.array([node[int(i)][k] for i in ids], dt)
    cells = np.array(sorted(outcome), U)
    out.update(o_node_ids=ids, o_node_cell=col('cell', U), o_node_class=col('cls', np.uint8), o_node_comp=col('comp', U),
               o_node_size1=col('size1', np.float64), o_node_size2=col('size2', np.float64), o_cell_ids=cells,
               o_cell_outcome=np.array([outcome[int(i)] for i in cells], np.uint8))
    graph, total, neuron_g = split_graph(c, node, ccsize)
    out.update({f'o_{k}': v for k, v in graph.items()})
    out['o_total_size'] = np.int64(total)
    # the per-cell lists of remove_glia_nodes are the components of the dataset-wide split graphs
    flat = lambda k: sorted(cc for i in cells for cc in lists[int(i)][k])
    for k, key in ((0, 'n'), (1, 'g')):
        b = graph[f'{key}cc_begin']
        assert flat(k) == sorted(graph[f'{key}cc_sv'][a:e].tolist() for a, e in zip(b[:-1], b[1:]))
    # the size filter: sizes of the original cells from the lifted create_ccsize_dict over the whole graph
    g_all = nx.Graph()
    g_all.add_nodes_from(c.extra)
    g_all.add_edges_from(c.edges)
    cell_size_of = ccsize(g_all, {i: c.table[i][1].astype(np.float64) for i in c.table})
    w_min = 3000.0
    graph_w, total_w, _ = split_graph(c, node, ccsize, cell_size_of, w_min)
    out.update({f'w_{k}': v for k, v in graph_w.items()})
    out.update(w_cell_size=np.array([cell_size_of[int(i)] for i in ids], np.float64), w_min=np.float64(w_min), w_total_size=np.int64(total_w))
    assert 0 < len(graph_w['ncc_sv']) < len(graph['ncc_sv']) and 0 < total_w < total and (out['w_cell_size'] == w_min).any()
    # the cases
    oc = lambda k: outcome[min(name[k])]
    cls = lambda k: [node[i]['cls'] for i in name[k]]
    for s in ('', '_f32'):
        assert (oc('out1' + s), oc('out2' + s), oc('out3' + s)) == (1, 2, 3)
        assert oc('rejoin' + s) == 3 and cls('rejoin' + s) == [0, 0, 0, 1, 0] and node[name['rejoin' + s][1]]['size2'] == 3100
        assert node[name['rejoin' + s][0]]['size1'] == 1500 and node[name['rejoin' + s][2]]['size1'] == 1500
        assert oc('orphan' + s) == 3 and cls('orphan' + s) == [0, 1, 1]
        assert oc('tie1' + s) == 1 and node[name['tie1' + s][0]]['size1'] == T
        assert oc('tie_glia' + s) == 3 and node[name['tie_glia' + s][2]]['size1'] == T and cls('tie_glia' + s) == [0, 1, 1, 1]
        assert oc('tie_stay' + s) == 3 and node[name['tie_stay' + s][2]]['size2'] == T and cls('tie_stay' + s) == [0, 1, 0]
    assert oc('no_neuron') == 1 and oc('no_glia_big') == 2 and oc('no_glia_small') == 1
    assert (oc('loop_neuron'), oc('loop_neuron_small'), oc('loop_glia'), oc('node_only')) == (2, 1, 1, 2)
    e = out['e_edges']
    assert (e[:, 0] == e[:, 1]).sum() >= 4 and len(np.unique(np.sort(e, 1), axis=0)) < len(e) and name['node_only'][0] not in e
    assert oc('dup') == 3 and oc('big_ids') == 3 and (e == U(2 ** 63)).any() and (e == U(2 ** 64 - 1)).any()
    assert out['t_f32'].any() and not out['t_f32'].all()
    # a neuron node all of whose neighbours became glia: in the lists, in no edge
    lone = name['orphan'][0]
    assert lone in out['o_ncc_sv'] and not (out['o_neuron_edges'] == U(lone)).any() and neuron_g.has_node(lone) and neuron_g.degree(lone) == 0
    assert sorted(np.bincount(out['o_cell_outcome'])[1:].tolist())[0] >= 10
    # glia_pred
    probas, view_begin = pred_set(rng)
    thresholds = (0.1875, 0.25)
    out.update(p_probas=probas, p_view_begin=view_begin, p_thresh=np.array(thresholds, np.float64))
    out.update(run_pred(probas, view_begin, thresholds))
    assert out['p_cls_f32_1_0'][3] == 0 and out['p_cls_f32_1_1'][3] == 1 and out['p_cls_f64_0_0'][4] == 0 and out['p_cls_f64_0_1'][4] == 1
    assert out['p_cls_f64_1_0'][5] == 0 and out['p_cls_f64_1_0'][6] == 1 and out['p_cls_f64_1_0'][7] == 0 and out['p_cls_f64_1_0'][8] == 1
    assert out['p_cls_f64_1_0'][0] == 0 and out['p_cls_f64_1_1'][0] == 0 and np.isnan(out['p_mean_f64'][0])
    path = os.path.join(HERE, 'g26_glia_split.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays; outcomes', np.bincount(out['o_cell_outcome'])[1:])


if __name__ == '__main__':
    main()
