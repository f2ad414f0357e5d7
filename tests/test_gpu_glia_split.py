"""GPU: csrc/sd_glia.hip through the C ABI (tests/_glia_gpu.py: the scratch and every output followed by a guard band) and through the host
layer (proc/graphs.py, proc/glia_splitting.py, exec/exec_inference.py) -- the golden of the reference's own functions (tests/golden/
g26_glia_split.npz) and random multi-cell datasets against the restatement (tests/_glia_ref.py), bit for bit: classes, outcomes, component
ids, both component tables, both split graphs, float64 sizes (every squared diagonal of the inputs is exact, so the ordered sum and a
BLAS dot agree), glia_pred classes and means; every count slot, every device flag, the drop-ins and the chain of the three drivers."""
import os

import networkx as nx
import numpy as np
import pytest

import _cell_assembly_ref as CA
import _glia_gpu as D
import _glia_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g26_glia_split.npz')
U = np.uint64
SD_OK, SD_ERR_INVALID = 0, -1
NODE_KEYS = ('node_ids', 'node_cell', 'node_class', 'node_comp', 'node_size1', 'node_size2', 'cell_ids', 'cell_outcome')
TABLE_KEYS = ('cc_ids', 'cc_cell', 'sv_begin', 'sv_ids')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def same(a, b):
    """Same shape, dtype and values, NaN == NaN (the payload of a NaN is no part of the contract); integers bit for bit."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def assert_same_result(got, want, nodes=True):
    """got / want: dicts shaped like _glia_ref.split_table's."""
    for k in NODE_KEYS if nodes else ():
        assert same(got[k], want[k]), k
    for t in ('neuron', 'glia'):
        for k in TABLE_KEYS:
            assert same(got[t][k], want[t][k]), (t, k)
    assert same(got['neuron_edges'], want['neuron_edges']) and same(got['astrocyte_edges'], want['astrocyte_edges'])


def gold_result(g, prefix='o_'):
    out = {k: g[f'o_{k}'] for k in NODE_KEYS}
    for t, key in (('neuron', 'ncc'), ('glia', 'gcc')):
        out[t] = dict(cc_ids=g[f'{prefix}{key}_ids'], cc_cell=g[f'{prefix}{key}_cell'], sv_begin=g[f'{prefix}{key}_begin'], sv_ids=g[f'{prefix}{key}_sv'])
    out['neuron_edges'], out['astrocyte_edges'] = g[f'{prefix}neuron_edges'], g[f'{prefix}astrocyte_edges']
    return out


def host_result(s):
    """A ``GliaSplit`` as such a dict."""
    out = {k: getattr(s, k) for k in NODE_KEYS}
    for t in ('neuron', 'glia'):
        out[t] = {k: getattr(getattr(s, t), k) for k in TABLE_KEYS}
    out['neuron_edges'], out['astrocyte_edges'] = s.neuron_edges, s.astrocyte_edges
    return out


# ---- the golden ----------------------------------------------------------------------------------------------------------------------
def test_golden_split(gpu, gold):
    from syconn_amd.proc.graphs import split_glia_table
    g = gold
    rc, c, got = D.split(gpu, g['e_edges'], g['t_ids'], g['t_boxes'], g['t_glia'], float(g['T']), g['e_nodes'], sv_sizes=g['t_sizes'])
    assert rc == SD_OK and c[7] == 0 and not c[10:13].any()
    assert_same_result(got, gold_result(g))
    assert c[9] == int(g['o_total_size']) and c[13:16].tolist() == np.bincount(g['o_cell_outcome'], minlength=4)[1:].tolist()
    for boxes in (g['t_boxes'], g['t_boxes'].astype(np.float32)):                   # float32 boxes are widened, which is exact
        assert (boxes.astype(np.float64) == g['t_boxes']).all()
        s = split_glia_table(g['e_edges'], g['t_ids'], boxes, g['t_glia'], float(g['T']), nodes=g['e_nodes'], sv_sizes=g['t_sizes'], device=gpu)
        assert_same_result(host_result(s), gold_result(g))
        assert s.astrocyte_size == int(g['o_total_size']) and s.n_cells_by_outcome == tuple(c[13:16].tolist())


def test_golden_size_filter(gpu, gold):
    from syconn_amd.proc import glia_splitting
    g = gold
    rc, c, got = D.split(gpu, g['e_edges'], g['t_ids'], g['t_boxes'], g['t_glia'], float(g['T']), g['e_nodes'], g['w_cell_size'], float(g['w_min']), g['t_sizes'])
    assert rc == SD_OK and not c[10:13].any() and c[9] == int(g['w_total_size'])
    assert_same_result(got, gold_result(g, 'w_'))                                  # the per-node outputs do not see the filter
    s = glia_splitting.run_glia_splitting(g['e_edges'], g['t_ids'], g['t_boxes'], g['t_glia'], float(g['T']), g['e_nodes'], g['w_cell_size'], float(g['w_min']),
                                          g['t_sizes'], gpu)
    assert_same_result(host_result(s), gold_result(g, 'w_'))
    w = glia_splitting.write_astrocyte_svgraph(s, scaling=(10, 10, 20))
    assert same(w.neuron_edges, g['w_neuron_edges']) and same(w.astrocyte_edges, g['w_astrocyte_edges'])
    assert (w.n_neuron_ccs, w.n_neuron_svs, w.n_astrocyte_ccs, w.n_astrocyte_svs) == (len(g['w_ncc_ids']), len(g['w_ncc_sv']), len(g['w_gcc_ids']), len(g['w_gcc_sv']))
    assert w.total_size == int(g['w_total_size']) and w.total_size_cmm == np.prod(np.array([10., 10., 20.])) * int(g['w_total_size']) / 1e18
    # collect_glia_sv with table ids outside the graph
    ids = np.concatenate([g['t_ids'], np.array([2 ** 63 + 7, 2 ** 63 + 9], U)])
    ids.sort()
    svs = glia_splitting.collect_glia_sv(s, ids)
    assert same(svs['astrocyte_svs'], g['t_ids'][g['o_node_class'] == 1]) and same(svs['neuron_svs'], g['t_ids'][g['o_node_class'] == 0])
    assert same(svs['pruned_svs'], np.array([2 ** 63 + 7, 2 ** 63 + 9], U))


@pytest.mark.parametrize('d, dt', [('f32', np.float32), ('f64', np.float64)])
def test_golden_glia_pred(gpu, gold, d, dt):
    from syconn_amd.proc.graphs import glia_pred
    g = gold
    p = g['p_probas'].astype(dt)
    for k, thresh in enumerate(g['p_thresh']):
        for m in (0, 1):
            rc, c, cls, mean = D.pred(gpu, p, g['p_view_begin'], float(thresh), m)
            assert rc == SD_OK and not c.any()
            assert same(cls, g[f'p_cls_{d}_{k}_{m}']), (k, m)
            assert same(mean.astype(dt), g[f'p_mean_{d}']) and same(mean, R.glia_pred(p, g['p_view_begin'], float(thresh), m)[1])
            h_cls, h_mean = glia_pred(p, g['p_view_begin'], float(thresh), bool(m), gpu)
            assert same(h_cls, cls) and same(h_mean, mean)


def test_glia_pred_flags_and_defaults(gpu, monkeypatch):
    from syconn_amd import global_params
    from syconn_amd.proc.graphs import glia_pred
    p = np.array([0.25, 0.25, 0.5], np.float32)
    rc, c, _, _ = D.pred(gpu, p, [0, 2, 1, 3], 0.25, 0)
    assert rc == SD_OK and c[7] == 1
    rc, c, _, _ = D.pred(gpu, p, [0, 1, 2], 0.25, 0)
    assert rc == SD_OK and c[7] == 1
    assert D.pred(gpu, p, [0, 3], np.nan, 0)[0] == SD_ERR_INVALID
    rc, c, cls, mean = D.pred(gpu, np.zeros(0, np.float64), [0, 0, 0], 0.25, 1)
    assert rc == SD_OK and not c.any() and cls.tolist() == [0, 0] and np.isnan(mean).all()
    # thresh and the mode from the config: mean 0.25 is above 0.161489; with point models mean == thresh counts
    assert glia_pred(p, [0, 2, 3], device=gpu)[0].tolist() == [1, 1]
    monkeypatch.setitem(global_params.config._entries, 'glia', {'glia_thresh': 0.25})
    assert glia_pred(p, [0, 2, 3], device=gpu)[0].tolist() == [0, 1]
    monkeypatch.setitem(global_params.config._entries, 'use_point_models', True)
    assert glia_pred(p, [0, 2, 3], device=gpu)[0].tolist() == [1, 1]


# ---- random datasets against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed, n_cells, filtered', [(1, 1, False), (2, 150, False), (3, 200, True), (4, 40, True)])
def test_random_datasets_against_the_restatement(gpu, seed, n_cells, filtered):
    rng = np.random.default_rng(seed)
    edges, ids, boxes, glia, cells = R.random_cells(rng, n_cells)
    if seed == 4:                                                                  # ids that use all 64 bits
        remap = np.sort(rng.choice(2 ** 62, len(ids), replace=False).astype(U) * U(4) + U(3))
        edges, ids = remap[np.searchsorted(ids, edges)], remap
    # single-node cells of this input have a self loop; some nodes are named twice: as an endpoint and in `nodes`
    nodes = ids[rng.integers(0, len(ids), 7)]
    sv_sizes = rng.integers(1, 10 ** 9, len(ids))
    kw = {}
    if filtered:
        full = R.split_table(edges, ids, boxes, glia, -1.0)                        # T = -1: every cell has outcome 3 or 1; only the cells matter here
        cell_size = rng.integers(0, 40, len(ids))[np.searchsorted(ids, full['node_cell'])] * 100.0
        kw = dict(cell_size=cell_size, min_cell_size=2000.0)
    for T in (2600.0, 1000.0):
        want = R.split_table(edges, ids, boxes, glia, T, nodes, sv_sizes=sv_sizes, **kw)
        rc, c, got = D.split(gpu, edges, ids, boxes, glia, T, nodes, sv_sizes=sv_sizes, **kw)
        assert rc == SD_OK
        assert_same_result(got, want)
        assert c.tolist() == want['counts'].tolist()
    assert n_cells < 100 or want['counts'][13:16].min() > 5


def test_empty_inputs(gpu):
    rc, c, got = D.split(gpu, np.zeros((0, 2), U), np.zeros(0, U), np.zeros((0, 2, 3)), np.zeros(0, np.uint8), 10.0)
    assert rc == SD_OK and not c.any() and len(got['node_ids']) == 0 and got['neuron']['sv_begin'].tolist() == [0] and got['glia']['sv_begin'].tolist() == [0]
    rc, c, got = D.split(gpu, np.zeros((0, 2), U), [5, 9], np.zeros((2, 2, 3)), [0, 1], 10.0)                # a table, but no graph
    assert rc == SD_OK and not c.any()
    rc, c, got = D.split(gpu, np.zeros((0, 2), U), [5, 9], [[[0, 0, 0], [30, 0, 0]], [[0, 0, 0], [1, 0, 0]]], [0, 1], 10.0, nodes=[9, 5, 9])
    assert rc == SD_OK and c[:6].tolist() == [2, 2, 1, 1, 1, 1] and got['cell_outcome'].tolist() == [2, 1] and got['node_class'].tolist() == [0, 1]


# ---- flags and argument checks ---------------------------------------------------------------------------------------------------------
def small_case():
    ids = np.array([3, 5, 8, 13], U)
    boxes = np.array([[[0, 0, 0], [3000, 0, 0]], [[0, 0, 0], [3000, 0, 0]], [[100, 0, 0], [600, 0, 0]], [[0, 0, 0], [5, 0, 0]]], np.float64)
    return np.array([[5, 3], [8, 5], [13, 13]], U), ids, boxes, np.array([0, 1, 0, 0], np.uint8)


def test_unknown_node(gpu):
    from syconn_amd.proc.graphs import remove_glia_nodes, split_glia_table
    edges, ids, boxes, glia = small_case()
    e2 = np.concatenate([edges, np.array([[8, 21], [34, 3]], U)])
    rc, c, _ = D.split(gpu, e2, ids, boxes, glia, 2600.0)
    assert rc == SD_OK and c[10] == 1 and c[11] == 21 and c[7] == 0
    rc, c, _ = D.split(gpu, edges, ids, boxes, glia, 2600.0, nodes=[2 ** 64 - 1])
    assert rc == SD_OK and c[10] == 1 and int(c.view(U)[11]) == 2 ** 64 - 1
    rc, c, _ = D.split(gpu, edges, ids, boxes, glia, 2600.0)
    assert rc == SD_OK and c[10] == 0 and c[11] == 0
    with pytest.raises(KeyError, match='21'):
        split_glia_table(e2, ids, boxes, glia, 2600.0, device=gpu)
    g = nx.Graph([(1, 2)])
    with pytest.raises(KeyError):
        remove_glia_nodes(g, {1: boxes[0], 2: boxes[1]}, {1: 0}, device=gpu)
    with pytest.raises(KeyError):
        remove_glia_nodes(g, {1: boxes[0]}, {1: 0, 2: 1}, device=gpu)


def test_table_that_does_not_ascend(gpu):
    edges, ids, boxes, glia = small_case()
    for bad in (np.array([3, 8, 5, 13], U), np.array([3, 5, 5, 13], U)):
        rc, c, _ = D.split(gpu, edges, bad, boxes, glia, 2600.0)
        assert rc == SD_OK and c[7] == 1


def test_scratch_and_argument_checks(gpu):
    from syconn_amd import _lib
    edges, ids, boxes, glia = small_case()
    lib = _lib.load()
    assert D.split(gpu, edges, ids, boxes, glia, 2600.0, shrink=1)[0] == SD_ERR_INVALID
    assert b'sd_glia_split_temp_bytes(n_ids, n_edges, n_nodes)' in lib.sd_last_error()
    assert D.split(gpu, edges, ids, boxes, glia, 2600.0, null_scratch=True)[0] == SD_ERR_INVALID
    assert D.split(gpu, edges, ids, boxes, glia, np.nan)[0] == SD_ERR_INVALID
    assert D.split(gpu, edges, ids, boxes, glia, 2600.0, cell_size=np.ones(4), min_cell_size=np.nan)[0] == SD_ERR_INVALID
    assert lib.sd_glia_split_temp_bytes(4, 3, 0) == lib.sd_glia_split_temp_bytes(400, 3, 0) > 0


def test_capacity_one_short(gpu):
    edges, ids, boxes, glia = small_case()
    want = R.split_table(edges, ids, boxes, glia, 2600.0)
    assert want['counts'][0] == 4 and want['counts'][6] == 0 and want['counts'][8] == 2 and want['cell_outcome'].tolist() == [3, 1]
    rc, c, got = D.split(gpu, edges, ids, boxes, glia, 2600.0, node_cap=4, edge_cap=2)                       # exactly enough
    assert rc == SD_OK and c[12] == 0 and c.tolist() == want['counts'].tolist()
    assert_same_result(got, want)
    rc, c, got = D.split(gpu, edges, ids, boxes, glia, 2600.0, node_cap=3, edge_cap=2)                       # D.split checks every guard band
    assert rc == SD_OK and c[12] == 1 and c[0] == 4
    assert same(got['node_ids'], want['node_ids'][:3]) and same(got['node_class'], want['node_class'][:3])
    rc, c, got = D.split(gpu, edges, ids, boxes, glia, 2600.0, node_cap=4, edge_cap=1)
    assert rc == SD_OK and c[12] == 1 and c[8] == 2 and same(got['node_comp'], want['node_comp']) and same(got['astrocyte_edges'], want['astrocyte_edges'][:1])
    rc, c, got = D.split(gpu, edges, ids, boxes, glia, 2600.0, node_cap=0, edge_cap=0)
    assert rc == SD_OK and c[12] == 1 and c[0] == 4


# ---- drop-ins --------------------------------------------------------------------------------------------------------------------------
def test_drop_ins_against_the_golden_lists(gpu, gold, monkeypatch):
    from syconn_amd import global_params
    from syconn_amd.proc.graphs import remove_glia_nodes, split_glia_graph, split_glia_table
    g = gold
    monkeypatch.setitem(global_params.config._entries, 'min_cc_size_ssv', float(g['T']))
    lists = R.as_lists(gold_result(g))
    s = split_glia_table(g['e_edges'], g['t_ids'], g['t_boxes'], g['t_glia'], nodes=g['e_nodes'], device=gpu)          # the threshold from the config
    mine = s.as_lists()
    assert [[[x.tolist() for x in k] for k in cell] for cell in mine] == [[k for k in cell] for cell in lists]
    box, cls = dict(zip(g['t_ids'].tolist(), g['t_boxes'])), dict(zip(g['t_ids'].tolist(), g['t_glia'].tolist()))
    seen = set()
    for k in list(range(34)) + [len(lists) - 1]:                                   # the named cases and a random cell
        cid, oc = int(g['o_cell_ids'][k]), int(g['o_cell_outcome'][k])
        seen.add(oc)
        members = g['o_node_ids'][g['o_node_cell'] == U(cid)].tolist()
        e = g['e_edges'][np.isin(g['e_edges'][:, 0], members)]
        graph = nx.Graph()
        graph.add_nodes_from(members)
        graph.add_edges_from(e.tolist())
        n_ccs, g_ccs = remove_glia_nodes(graph, box, cls, return_removed_nodes=True, device=gpu)
        assert remove_glia_nodes(graph, box, cls, device=gpu) == n_ccs
        norm = lambda ccs: sorted(sorted(cc) for cc in ccs)
        assert (norm(n_ccs), norm(g_ccs)) == (sorted(lists[k][0]), sorted(lists[k][1]))
        if oc == 1:
            assert n_ccs == [] and g_ccs == [list(graph.nodes())]
        elif oc == 2:
            assert n_ccs == [list(graph.nodes())] and g_ccs == []
        else:
            assert all(isinstance(cc, set) for cc in n_ccs + g_ccs)
        if len(e):                                                                 # the (e, 2) array form
            assert norm(remove_glia_nodes(e, box, cls, device=gpu)) == sorted(lists[k][0])
    assert seen == {1, 2, 3}
    with pytest.raises(ValueError, match='one connected cell'):
        remove_glia_nodes(g['e_edges'][:6], box, cls, device=gpu)
    # split_glia_graph: classes from probabilities
    ids = np.array([3, 5, 8], U)
    boxes = np.array([[[0, 0, 0], [3000, 0, 0]], [[0, 0, 0], [3000, 0, 0]], [[100, 0, 0], [600, 0, 0]]], np.float32)
    probas = np.array([0.1, 0.2, 0.9, 0.8, 0.9, 0.3], np.float32)
    n_ccs, g_ccs = split_glia_graph(nx.Graph([(3, 5), (5, 8)]), 0.5, ids, boxes, probas, [0, 2, 5, 6], device=gpu)
    assert n_ccs == [{3}] and g_ccs == [{5, 8}]


# ---- the isolated neuron node ------------------------------------------------------------------------------------------------------------
def test_isolated_neuron_node(gpu):
    """3 is a neuron whose only neighbour became glia: in the component table, in no edge; 13 has a self loop, which stays."""
    edges, ids, boxes, glia = small_case()
    boxes[3] = [[0, 0, 0], [3000, 0, 0]]
    rc, c, got = D.split(gpu, edges, ids, boxes, glia, 2600.0)
    assert rc == SD_OK and got['cell_outcome'].tolist() == [3, 2] and got['node_class'].tolist() == [0, 1, 1, 0]
    assert got['neuron']['cc_ids'].tolist() == [3, 13] and got['neuron']['sv_ids'].tolist() == [3, 13]
    assert got['neuron_edges'].tolist() == [[13, 13]] and got['astrocyte_edges'].tolist() == [[8, 5]]
    assert got['glia']['cc_ids'].tolist() == [5] and got['glia']['sv_ids'].tolist() == [5, 8] and got['glia']['cc_cell'].tolist() == [3]


# ---- the drivers --------------------------------------------------------------------------------------------------------------------------
def test_rag_to_astrocyte_splitting_to_neuron_ssd(gpu):
    from syconn_amd.exec.exec_inference import run_astrocyte_splitting
    from syconn_amd.exec.exec_init import run_create_neuron_ssd, run_create_rag
    from syconn_amd.proc.sd_proc import PropTable
    rng = np.random.default_rng(7)
    scaling, T = (10., 10., 20.), 2600.0
    edges, ids, boxes_nm, glia, cells = R.random_cells(rng, 120)
    n = len(ids)
    vox = (boxes_nm / np.array(scaling)).astype(np.int64)                            # lattice of 100 nm: whole voxels
    assert (vox * np.array(scaling) == boxes_nm).all()
    sizes, rep = rng.integers(1, 10 ** 6, n), vox[:, 0].copy()
    props = PropTable(ids, sizes, rep, vox, np.arange(n + 1))
    extra = np.array([[0, ids[0]], [ids[5], 0]], U)                                # node 0 leaves in run_create_rag
    rag = run_create_rag(np.concatenate([edges, extra]), props, scaling=scaling, min_cc_size=T, device=gpu)
    want_rag = CA.components(np.concatenate([edges, extra]), ids, sizes, np.arange(n + 1), vox, scaling, T, True)
    assert same(rag.edges, want_rag['edges']) and 0 < len(rag.ssv_ids) < len(cells)
    # the views: four per supervoxel, all 0.75 for glia and 0.0625 for neurons
    probas = np.repeat(np.where(glia != 0, 0.75, 0.0625), 4).astype(np.float32)
    res = run_astrocyte_splitting(rag, props, glia_probas=probas, view_begin=np.arange(n + 1) * 4, thresh=0.25, scaling=scaling, min_cc_size=T, device=gpu)
    assert same(res.glia, glia) and same(res.glia_proba, np.where(glia != 0, 0.75, 0.0625))
    row = np.searchsorted(ids, want_rag['node_ids'])
    cell_size = np.full(n, np.inf)
    cell_size[row] = want_rag['node_size']
    want = R.split_table(want_rag['edges'], ids, boxes_nm, glia, T, want_rag['sv_ids'], cell_size, T, sizes)
    assert_same_result(host_result(res.split), want)
    assert res.graph.total_size == want['counts'][9] and same(res.neuron_edges, want['neuron_edges'])
    assert same(res.svs['pruned_svs'], np.setdiff1d(ids, want_rag['sv_ids'])) and len(res.svs['pruned_svs']) > 0
    assert len(res.svs['astrocyte_svs']) + len(res.svs['neuron_svs']) + len(res.svs['pruned_svs']) == n
    assert want['counts'][13:16].min() > 0
    by_classes = run_astrocyte_splitting(rag, props, glia=glia, scaling=scaling, min_cc_size=T, device=gpu)
    assert_same_result(host_result(by_classes.split), want)
    assert by_classes.glia_proba is None
    # mesh boxes given: a table whose boxes differ from bounding_box * scaling
    mesh_bb = boxes_nm + np.array([[[0, 0, 0], [100, 0, 0]]])
    meshed = run_astrocyte_splitting(rag, props, mesh_bb=mesh_bb.astype(np.float32), glia=glia, scaling=scaling, min_cc_size=T, device=gpu)
    assert_same_result(host_result(meshed.split), R.split_table(want_rag['edges'], ids, mesh_bb, glia, T, want_rag['sv_ids'], cell_size, T, sizes))
    # the neuron graph into run_create_neuron_ssd
    ssd = run_create_neuron_ssd(props, {}, {}, edges=res.neuron_edges, apply_ssv_size_threshold=True, scaling=scaling, min_cc_size=T, obj_types=[], device=gpu)
    comp = CA.components(want['neuron_edges'], ids, sizes, np.arange(n + 1), vox, scaling, T, False)
    assert same(ssd.cells.ssv_ids, comp['ssv_ids']) and same(ssd.cells.sv_begin, comp['sv_begin']) and same(ssd.cells.sv_ids, comp['sv_ids'])
    size, box, rep_c = CA.cell_props(comp['sv_begin'], comp['sv_ids'], ids, sizes, rep, np.arange(n + 1), vox)
    assert same(ssd.props.size, size) and same(ssd.props.bounding_box, box) and same(ssd.props.rep_coord, rep_c)
