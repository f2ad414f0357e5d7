"""CPU: the restatement of the astrocyte splitting (tests/_glia_ref.py) against the golden of the reference's own functions (tests/golden/
g26_glia_split.npz) and against a networkx statement of the rule on random connected graphs; the argument checks of the host layer that
need no device; the config defaults."""
import os

import networkx as nx
import numpy as np
import pytest

import _glia_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g26_glia_split.npz')
U = np.uint64
NODE_KEYS = ('node_ids', 'node_cell', 'node_class', 'node_comp', 'node_size1', 'node_size2', 'cell_ids', 'cell_outcome')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_values(a, b):
    """Equal with NaN == NaN (the sign and payload of a NaN are no part of the contract)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def check_against_gold(res, g, prefix='o_', nodes=True):
    if nodes:
        for k in NODE_KEYS:
            assert same_values(res[k], g[f'o_{k}']), k
    for key, t in (('ncc', res['neuron']), ('gcc', res['glia'])):
        assert same_bits(t['cc_ids'], g[f'{prefix}{key}_ids']) and same_bits(t['cc_cell'], g[f'{prefix}{key}_cell']), key
        assert same_bits(t['sv_begin'], g[f'{prefix}{key}_begin']) and same_bits(t['sv_ids'], g[f'{prefix}{key}_sv']), key
    assert same_bits(res['neuron_edges'], g[f'{prefix}neuron_edges']) and same_bits(res['astrocyte_edges'], g[f'{prefix}astrocyte_edges'])


def test_restatement_equals_the_golden(gold):
    g = gold
    res = R.split_table(g['e_edges'], g['t_ids'], g['t_boxes'], g['t_glia'], float(g['T']), g['e_nodes'], sv_sizes=g['t_sizes'])
    check_against_gold(res, g)
    c = res['counts']
    assert c[0] == len(g['t_ids']) and c[1] == len(g['o_cell_ids']) and c[9] == int(g['o_total_size'])
    assert c[13:16].tolist() == np.bincount(g['o_cell_outcome'], minlength=4)[1:].tolist() and c[13:16].min() > 0


def test_restatement_size_filter_equals_the_golden(gold):
    g = gold
    res = R.split_table(g['e_edges'], g['t_ids'], g['t_boxes'], g['t_glia'], float(g['T']), g['e_nodes'], g['w_cell_size'], float(g['w_min']), g['t_sizes'])
    check_against_gold(res, g, 'w_', nodes=False)
    assert same_values(res['node_class'], g['o_node_class']) and res['counts'][9] == int(g['w_total_size'])


def test_restatement_glia_pred_equals_the_golden(gold):
    g = gold
    for d, dt in (('f32', np.float32), ('f64', np.float64)):
        for k, thresh in enumerate(g['p_thresh']):
            for m in (0, 1):
                cls, mean = R.glia_pred(g['p_probas'].astype(dt), g['p_view_begin'], float(thresh), m)
                assert same_bits(cls, g[f'p_cls_{d}_{k}_{m}']), (d, k, m)
                assert same_values(mean.astype(dt), g[f'p_mean_{d}'])


# ---- the rule over networkx (the issue's wording, one cell at a time) ---------------------------------------------------------------
def nx_sizes(sub, box):
    out = {}
    for cc in nx.connected_components(sub):
        corners = np.concatenate([box[n] for n in cc])
        size = float(R.ordered_norm(corners.max(0) - corners.min(0)))
        out.update({n: size for n in cc})
    return out


def nx_rule(g, box, glia, T):
    """-> (outcome, neuron set, neuron_ccs, glia_ccs) of ONE connected cell."""
    every = set(g.nodes())
    neuron = {n for n in every if glia[n] == 0}
    s_n = nx_sizes(g.subgraph(neuron), box)
    if not any(v > T for v in s_n.values()):
        return 1, set(), [], [sorted(every)]
    s_g = nx_sizes(g.subgraph(every - neuron), box)
    if not any(v > T for v in s_g.values()):
        return 2, every, [sorted(every)], []
    tiny = {n for n, v in s_g.items() if v < T}
    s_2 = nx_sizes(g.subgraph(neuron | tiny), box)
    stays = {n for n, v in s_2.items() if not v < T}
    ccs = lambda nodes: sorted(sorted(cc) for cc in nx.connected_components(g.subgraph(nodes)))
    return 3, stays, ccs(stays), ccs(every - stays)


def test_restatement_equals_the_networkx_rule():
    rng = np.random.default_rng(26)
    T = 2600.0
    edges, ids, boxes, glia, cells = R.random_cells(rng, 300)
    res = R.split_table(edges, ids, boxes, glia, T)
    lists = R.as_lists(res)
    assert len(lists) == len(cells) == 300
    box, cls = dict(zip(ids.tolist(), boxes)), dict(zip(ids.tolist(), glia.tolist()))
    g_all = nx.Graph()
    g_all.add_edges_from(edges.tolist())
    seen = [0, 0, 0]
    for k, cid in enumerate(cells):
        oc, neuron, n_ccs, g_ccs = nx_rule(g_all.subgraph(cid.tolist()), box, cls, T)
        seen[oc - 1] += 1
        assert res['cell_ids'][k] == cid[0] and res['cell_outcome'][k] == oc
        rows = np.searchsorted(res['node_ids'], cid)
        assert set(cid[res['node_class'][rows] == 0].tolist()) == neuron
        assert (sorted(lists[k][0]), sorted(lists[k][1])) == (n_ccs, g_ccs)
    assert min(seen) >= 30, seen


# ---- host layer: what is checked before the device is touched ----------------------------------------------------------------------
def test_split_glia_table_argument_checks():
    from syconn_amd.proc.graphs import split_glia_table
    ids, boxes, glia, e = np.array([1, 2], U), np.zeros((2, 2, 3)), [0, 1], [[1, 2]]
    bad = [dict(edges=[[1, 2, 3]]), dict(edges=[[1.5, 2]]), dict(edges=[[-1, 2]]), dict(sv_ids=[2, 1]), dict(sv_ids=[1, 1]), dict(boxes_nm=np.zeros((3, 2, 3))),
           dict(boxes_nm=np.full((2, 2, 3), np.nan)), dict(boxes_nm=np.full((2, 2, 3), np.inf)), dict(boxes_nm=np.zeros((2, 2, 3), 'U1')), dict(glia=[0]),
           dict(min_cc_size=np.nan), dict(min_cc_size='a'), dict(cell_size=[1., 2.]), dict(min_cell_size=1.), dict(cell_size=[1.], min_cell_size=1.),
           dict(cell_size=[np.nan, 1.], min_cell_size=1.), dict(sv_sizes=[1]), dict(nodes=[-3])]
    for kw in bad:
        args = dict(edges=e, sv_ids=ids, boxes_nm=boxes, glia=glia, min_cc_size=10.)
        args.update(kw)
        with pytest.raises(ValueError):
            split_glia_table(**args)


def test_glia_pred_and_driver_argument_checks():
    from syconn_amd.exec.exec_inference import run_astrocyte_splitting
    from syconn_amd.proc.graphs import glia_pred
    for kw in (dict(probas=np.zeros(3, np.int64)), dict(view_begin=[0, 2]), dict(view_begin=[1, 3]), dict(view_begin=[0, 2, 1, 3]), dict(thresh=np.nan),
               dict(thresh='x'), dict(view_begin=[])):
        args = dict(probas=np.zeros(3, np.float32), view_begin=[0, 3], thresh=0.25)
        args.update(kw)
        with pytest.raises(ValueError):
            glia_pred(**args)
    with pytest.raises(ValueError, match='either glia or glia_probas'):
        run_astrocyte_splitting(None, None)
    with pytest.raises(ValueError, match='either glia or glia_probas'):
        run_astrocyte_splitting(None, None, glia=[0], glia_probas=[0.])
    with pytest.raises(ValueError, match='view_begin'):
        run_astrocyte_splitting(None, None, glia_probas=[0.])


def test_config_defaults():
    from syconn_amd.handler.config import DEFAULTS, DynConfig
    assert DEFAULTS['glia'] == {'prior_astrocyte_removal': True, 'glia_thresh': 0.161489} and DEFAULTS['use_point_models'] is False
    cfg = DynConfig()
    assert cfg['glia']['prior_astrocyte_removal'] is True and cfg['glia']['glia_thresh'] == 0.161489 and cfg['use_point_models'] is False
    assert cfg['min_cc_size_ssv'] == 5000


def test_grid_constant_matches_the_header():
    import re
    from syconn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'syconn_dense.h')).read()
    assert int(re.search(r'#define SD_GLIA_GRID (\d+)', header).group(1)) == _lib.SD_GLIA_GRID
