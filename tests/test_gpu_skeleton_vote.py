"""GPU: csrc/sd_skeleton.hip through the Python API and the C ABI -- the golden vectors of the reference's own functions bit for bit,
random forests and graphs with cycles against the restatement (tests/_skeleton_ref.py), and the edges of the kernels' structure: the
LDS table of SD_SKEL_LDS_NODES nodes per wave (exactly full, one node more: the second pass), adjacency rows of 63, 64 and 65 entries
(a wave walks 64 per step), 1, 2 and 64 classes, max_dist 0, and an edge that names a node outside its cell."""
import os
import types

import numpy as np
import pytest

import _skeleton_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g23_skeleton.npz')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def chain(n):
    return np.stack([np.arange(n), np.zeros(n, np.int64), np.zeros(n, np.int64)], 1), np.stack([np.arange(n - 1), np.arange(1, n)], 1)


def chain_expect(labels, r):
    """Window [i - r, i + r] clipped, two classes 0 / 1: -> (vote, size)."""
    n = len(labels)
    i = np.arange(n)
    lo, hi = np.maximum(i - r, 0), np.minimum(i + r, n - 1)
    ones = np.concatenate(([0], np.cumsum(labels)))
    c1 = ones[hi + 1] - ones[lo]
    size = hi - lo + 1
    return (c1 > size - c1).astype(labels.dtype), size


# ---- golden ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', ['a_', 'b_'])
def test_golden_votes(gpu, gold, p):
    from syconn_amd.reps.super_segmentation_helper import skeleton_majority_vote
    vote, reached, counts = skeleton_majority_vote(gold[p + 'nodes'], gold[p + 'node_begin'], gold[p + 'edges'], gold[p + 'edge_begin'],
                                                   gold[p + 'labels'], gold[p + 'scaling'], int(gold[p + 'max_dist']), gpu, True, True)
    assert np.array_equal(reached, gold[p + 'reached'])
    assert np.array_equal(vote, gold[p + 'vote']) and vote.dtype == gold[p + 'labels'].dtype
    assert counts['sources_redone'] == 0


def test_golden_compartments(gpu, gold):
    from syconn_amd.reps.super_segmentation_helper import skeleton_compartment_majority
    comp = skeleton_compartment_majority(gold['c_node_begin'], gold['c_edges'], gold['c_edge_begin'], gold['c_labels'], device=gpu)
    assert np.array_equal(comp.astype(np.float64), gold['c_comp'])


class _Sso:
    def __init__(self, g, c, with_edges=True):
        n0, n1, e0, e1, v0, v1 = (int(g[k][c + d]) for k in ('s_node_begin', 's_edge_begin', 's_vert_begin') for d in (0, 1))
        self.id, self.scaling, self.saved = c, g['s_scaling'], 0
        self.skeleton = dict(nodes=g['s_nodes'][n0:n1], edges=g['s_edges'][e0:e1])
        self.mesh = (np.zeros(0, np.uint32), g['s_verts'][v0:v1].reshape(-1), np.zeros(0, np.float32))
        self._lab = g['s_vert_labels'][v0:v1]

    def load_skeleton(self):
        pass

    def save_skeleton(self):
        self.saved += 1

    def label_dict(self, what):
        return {'axoness': self._lab}


def test_golden_semsegaxoness2skel(gpu, gold):
    """The three keys: the table form over all four cells (two of them take the zero branch) and the drop-in cell by cell."""
    from syconn_amd.extraction.cs_processing_steps import CellTable
    from syconn_amd.reps.super_segmentation_object import semsegaxoness2skel, semsegaxoness2skel_table
    g = gold
    props = dict(k=int(g['s_k']), ds_vertices=int(g['s_ds_vertices']), ignore_labels=g['s_ignore_labels'].tolist())
    md = int(g['s_max_dist'])
    keys = ('axoness', 'axoness_avg%d' % md, 'axoness_avg%d_comp_maj' % md)
    cells = CellTable(np.arange(4), g['s_verts'], g['s_vert_begin'], {'axoness': g['s_vert_labels']}, g['s_nodes'], g['s_node_begin'], {})
    res = semsegaxoness2skel_table(cells, g['s_edges'], g['s_edge_begin'], props, 'axoness', md, g['s_scaling'], gpu)
    for key, want in zip(keys, (g['s_pred'], g['s_avg'], g['s_comp'])):
        assert res[key].dtype == want.dtype and np.array_equal(res[key], want), key
    for c in (0, 1):
        sso = _Sso(g, c)
        semsegaxoness2skel(sso, props, 'axoness', md)
        n0, n1 = g['s_node_begin'][c], g['s_node_begin'][c + 1]
        assert sso.saved == 1
        for key, want in zip(keys, (g['s_pred'], g['s_avg'], g['s_comp'])):
            assert sso.skeleton[key].dtype == want.dtype and np.array_equal(sso.skeleton[key], want[n0:n1]), (c, key)


def test_drop_ins_store_the_reference_keys(gpu, gold):
    from syconn_amd.reps.super_segmentation_helper import majority_vote_compartments, majorityvote_skeleton_property
    g = gold
    n0, n1, e0, e1 = g['a_node_begin'][10], g['a_node_begin'][11], g['a_edge_begin'][10], g['a_edge_begin'][11]
    sso = types.SimpleNamespace(id=3, scaling=g['a_scaling'], skeleton=dict(nodes=g['a_nodes'][n0:n1], edges=g['a_edges'][e0:e1],
                                                                           prop=g['a_labels'][n0:n1].astype(np.int32)))
    res = majorityvote_skeleton_property(sso, 'prop', 1000, return_res=True)
    assert np.array_equal(res, g['a_vote'][n0:n1]) and res.dtype == np.int32 and 'prop_avg1000' not in sso.skeleton
    assert majorityvote_skeleton_property(sso, 'prop', 1000) is None and np.array_equal(sso.skeleton['prop_avg1000'], res)
    n0, n1, e0, e1 = g['c_node_begin'][6], g['c_node_begin'][7], g['c_edge_begin'][6], g['c_edge_begin'][7]
    saved = []
    sso = types.SimpleNamespace(id=4, scaling=g['a_scaling'], save_skeleton=lambda: saved.append(1),
                                skeleton=dict(nodes=np.zeros((n1 - n0, 3), np.int64), edges=g['c_edges'][e0:e1], ax=g['c_labels'][n0:n1]))
    majority_vote_compartments(sso, 'ax')
    assert saved == [1] and sso.skeleton['ax_comp_maj'].dtype == np.float64 and np.array_equal(sso.skeleton['ax_comp_maj'], g['c_comp'][n0:n1])


# ---- random graphs -----------------------------------------------------------------------------------------------------------------
def _random_cells(rng, n_cells, cycles):
    nodes, edges, nb, eb = [], [], [0], [0]
    for c in range(n_cells):
        n = int(rng.integers(150, 320))
        p = np.cumsum(rng.normal(0, 8, (n, 3)), 0) + rng.uniform(0, 500, 3)
        parent = np.array([int(rng.integers(max(0, i - 4), i)) for i in range(1, n)])
        e = np.stack([parent, np.arange(1, n)], 1)
        if cycles:
            e = np.concatenate([e, rng.integers(0, n, (n // 20, 2)), e[:3], np.array([(5, 5)])])
        e = e[rng.permutation(len(e))]
        flip = rng.random(len(e)) < 0.5
        e[flip] = e[flip][:, ::-1]
        nodes.append(np.round(p).astype(np.int64) if c % 2 else p)
        edges.append(e)
        nb.append(nb[-1] + n)
        eb.append(eb[-1] + len(e))
    return np.concatenate([np.asarray(x, np.float64) for x in nodes]), np.array(nb), np.concatenate(edges), np.array(eb)


@pytest.mark.parametrize('cycles', [False, True])
def test_random_cells_match_the_restatement(gpu, cycles):
    from syconn_amd.reps.super_segmentation_helper import skeleton_compartment_majority, skeleton_majority_vote
    rng = np.random.default_rng(77 + cycles)
    nodes, nb, edges, eb = _random_cells(rng, 14, cycles)
    labels = rng.integers(0, 6, len(nodes)).astype(np.int16) * 3 - 4                  # not dense, some negative
    scaling = np.array([9, 9, 20], np.float32)
    vote, reached = skeleton_majority_vote(nodes, nb, edges, eb, labels, scaling, 900, gpu, return_reached=True)
    want, want_reached = R.majority_vote(nodes, nb, edges, eb, labels, scaling, 900)
    assert 5 < np.median(want_reached) < 150
    assert np.array_equal(reached, want_reached) and np.array_equal(vote, want) and vote.dtype == np.int16
    lab = rng.choice(5, len(nodes), p=[0.3, 0.35, 0.15, 0.1, 0.1]).astype(np.uint8)
    assert np.array_equal(skeleton_compartment_majority(nb, edges, eb, lab, device=gpu), R.compartment_majority(nb, edges, eb, lab))


# ---- structure edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extra', [0, 1])
def test_window_fills_the_lds_table_and_one_more(gpu, extra):
    """A chain of 2 CAP + 40 nodes 1 nm apart with max_dist r: source i reaches min(i, r) + min(n - 1 - i, r) + 1 nodes.  With r = CAP - 1
    the two end nodes fill the table exactly (CAP nodes) and stay in LDS; with r = CAP they hold CAP + 1.  Every source with more than
    CAP nodes is redone by the second pass and counted."""
    from syconn_amd._lib import SD_SKEL_LDS_NODES as CAP
    from syconn_amd.reps.super_segmentation_helper import skeleton_majority_vote
    n, r = 2 * CAP + 40, CAP - 1 + extra
    nodes, edges = chain(n)
    labels = ((np.arange(n) // 50) % 2).astype(np.int64)
    vote, reached, counts = skeleton_majority_vote(nodes, [0, n], edges, [0, n - 1], labels, (1, 1, 1), r, gpu, True, True)
    want, size = chain_expect(labels, r)
    assert size[0] == CAP + extra and np.array_equal(reached, size) and np.array_equal(vote, want)
    assert counts['sources_redone'] == int((size > CAP).sum()) and (size <= CAP).sum() == (2 if extra == 0 else 0)


@pytest.mark.parametrize('leaves', [63, 64, 65])
def test_star_rows_of_63_64_65(gpu, leaves):
    """Node 0 has `leaves` neighbours (its adjacency row is walked 64 per step); leaf j sits j + 1 nm away.  With max_dist 40 the centre
    reaches the leaves 1 .. 40, leaf j the centre if j + 1 <= 40 and the leaves k with (j + 1) + (k + 1) <= 40."""
    from syconn_amd.reps.super_segmentation_helper import skeleton_majority_vote
    d = np.arange(1, leaves + 1)
    nodes = np.concatenate([np.zeros((1, 3), np.int64), np.stack([d, 0 * d, 0 * d], 1)])
    edges = np.stack([np.zeros(leaves, np.int64), d], 1)[::-1]
    labels = np.concatenate([[1], d % 3])
    vote, reached = skeleton_majority_vote(nodes, [0, leaves + 1], edges, [0, leaves], labels, (1, 1, 1), 40, gpu, return_reached=True)
    want_reached = np.concatenate([[41], np.where(d <= 40, 1 + np.maximum(40 - d, 0) - ((d <= 40) & (2 * d <= 40)) + 1, 1)])
    w, wr = R.majority_vote(nodes, [0, leaves + 1], edges, [0, leaves], labels, (1, 1, 1), 40)
    assert np.array_equal(wr, want_reached) and np.array_equal(reached, want_reached) and np.array_equal(vote, w)


def test_path_longer_than_the_table_with_a_larger_max_dist(gpu):
    from syconn_amd._lib import SD_SKEL_LDS_NODES as CAP
    from syconn_amd.reps.super_segmentation_helper import skeleton_majority_vote
    n = CAP + 100
    nodes, edges = chain(n)
    labels = np.where(np.arange(n) % 3 == 0, 7, 5)
    vote, reached, counts = skeleton_majority_vote(nodes, [0, n], edges, [0, n - 1], labels, (10, 10, 20), 10 * n + 5, gpu, True, True)
    assert (reached == n).all() and (vote == 5).all() and counts['sources_redone'] == n


@pytest.mark.parametrize('n_classes', [1, 2, 64])
def test_class_counts(gpu, n_classes):
    """Two nodes of every class and a third of the last one, on a chain that every window covers (it fits the LDS table): the last
    class wins; with a third node of the first class as well the counts tie and the smaller class wins."""
    from syconn_amd.reps.super_segmentation_helper import skeleton_majority_vote
    labels = np.concatenate([np.repeat(np.arange(n_classes), 2), [n_classes - 1]]) * 5 - 20
    labels = labels[np.random.default_rng(3).permutation(len(labels))]
    for tie in (False, True):
        lab = np.concatenate([labels, [-20]]) if tie else labels
        n = len(lab)
        nodes, edges = chain(n)
        vote, reached = skeleton_majority_vote(nodes, [0, n], edges, [0, n - 1], lab, (1, 1, 1), 10 ** 6, gpu, return_reached=True)
        assert (reached == n).all() and (vote == (-20 if tie else 5 * (n_classes - 1) - 20)).all()


def test_65_classes_raise(gpu):
    from syconn_amd.reps.super_segmentation_helper import skeleton_majority_vote
    nodes, edges = chain(65)
    with pytest.raises(ValueError, match='at most 64'):
        skeleton_majority_vote(nodes, [0, 65], edges, [0, 64], np.arange(65), (1, 1, 1), 10, gpu)


def test_max_dist_zero(gpu):
    """The source and what a zero-weight edge joins to it."""
    from syconn_amd.reps.super_segmentation_helper import skeleton_majority_vote
    nodes = np.array([(0, 0, 0), (3, 0, 0), (3, 0, 0), (3, 0, 0), (6, 0, 0)])
    edges = np.array([(0, 1), (1, 2), (2, 3), (3, 4)])
    vote, reached = skeleton_majority_vote(nodes, [0, 5], edges, [0, 4], np.array([4, 9, 2, 2, 1]), (1, 1, 1), 0, gpu, return_reached=True)
    assert reached.tolist() == [1, 3, 3, 3, 1] and vote.tolist() == [4, 2, 2, 2, 1]


def test_edge_outside_its_cell_sets_the_error_slot(gpu):
    """Through the C ABI: two cells of three nodes; the second cell's edge (1, 3) names a node the cell does not have (it would be node
    0 of nothing), (-1, 0) a negative one.  counts[7] is set, the rows hold the valid edges only, and the vote over them runs."""
    import torch
    from syconn_amd import _lib as L
    lib = L.load()
    L.check(lib.sd_init(gpu.index or 0), 'sd_init')
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    edges = np.array([(0, 1), (1, 2), (0, 1), (1, 3), (-1, 0)])
    e_d, eb_d, nb_d, w_d = up(edges, np.int64), up([0, 2, 5], np.int64), up([0, 3, 6], np.int64), up(np.ones(5), np.float64)
    adj_begin, adj_nbr, adj_w = (torch.zeros(k, dtype=t, device=gpu) for k, t in ((7, torch.int64), (10, torch.int32), (10, torch.float64)))
    counts = torch.zeros(8, dtype=torch.int64, device=gpu)
    tmp = torch.empty(lib.sd_skel_csr_temp_bytes(5), dtype=torch.uint8, device=gpu).fill_(0xCD)
    L.check(lib.sd_skel_csr(e_d.data_ptr(), eb_d.data_ptr(), nb_d.data_ptr(), 2, 6, 5, w_d.data_ptr(), adj_begin.data_ptr(), adj_nbr.data_ptr(),
                            adj_w.data_ptr(), counts.data_ptr(), tmp.data_ptr(), tmp.numel(), stream), 'sd_skel_csr')
    assert int(counts.cpu()[7]) != 0
    assert adj_begin.cpu().tolist() == [0, 1, 3, 4, 5, 6, 6] and adj_nbr.cpu().tolist()[:6] == [1, 0, 2, 1, 1, 0]
    cls = up([0, 1, 1, 1, 0, 0], np.uint8)
    vote, reached = torch.zeros(6, dtype=torch.uint8, device=gpu), torch.zeros(6, dtype=torch.int32, device=gpu)
    tmp = torch.empty(lib.sd_skel_vote_temp_bytes(6, 3), dtype=torch.uint8, device=gpu).fill_(0xCD)
    L.check(lib.sd_skel_vote(adj_begin.data_ptr(), adj_nbr.data_ptr(), adj_w.data_ptr(), 10, nb_d.data_ptr(), 2, 6, 3, cls.data_ptr(), 2, 5.0,
                             vote.data_ptr(), reached.data_ptr(), counts.data_ptr(), tmp.data_ptr(), tmp.numel(), stream), 'sd_skel_vote')
    assert int(counts.cpu()[7]) == 0 and reached.cpu().tolist() == [3, 3, 3, 2, 2, 1] and vote.cpu().tolist() == [1, 1, 1, 0, 0, 0]
    # the components ignore the same edges and say so
    out = torch.zeros(6, dtype=torch.uint8, device=gpu)
    tmp = torch.empty(lib.sd_skel_components_temp_bytes(6), dtype=torch.uint8, device=gpu).fill_(0xCD)
    L.check(lib.sd_skel_components(e_d.data_ptr(), eb_d.data_ptr(), nb_d.data_ptr(), 2, 6, 5, cls.data_ptr(), -1, 1, 0, out.data_ptr(), counts.data_ptr(),
                                   tmp.data_ptr(), tmp.numel(), stream), 'sd_skel_components')
    assert int(counts.cpu()[7]) != 0 and out.cpu().tolist() == [1, 1, 1, 0, 0, 0]


def test_map_myelin_global(gpu, tmp_path):
    """predict_myelin's two follow-up steps over a table: map_myelin2coords at the nodes (golden g7 of the reference's own function) and
    the vote along two chains with the config's dist_axoness_averaging and scaling."""
    from test_gpu_myelin import _make_wd
    from syconn_amd import global_params
    from syconn_amd.exec.exec_skeleton import map_myelin_global
    from syconn_amd.extraction.cs_processing_steps import CellTable
    g = np.load(os.path.join(os.path.dirname(GOLD), 'g7_myelin2coords.npz'))
    coords, mag = g['coords'], int(g['mag'])
    n = len(coords)
    nb = np.array([0, n // 3, n])
    edges = np.concatenate([chain(n // 3)[1], chain(n - n // 3)[1]])
    eb = np.array([0, n // 3 - 1, n - 2])
    cells = CellTable([5, 9], np.zeros((0, 3)), [0, 0, 0], {}, coords, nb, {})
    _make_wd(tmp_path, g['vol4'], mag)
    try:
        res = map_myelin_global(cells, edges, eb, mag=mag, device=gpu)
        near = map_myelin_global(cells, edges, eb, max_dist=4000, mag=mag, device=gpu)
    finally:
        global_params.wd = None
    assert sorted(res) == ['myelin', 'myelin_avg10000'] and np.array_equal(res['myelin'], g['default']) and res['myelin'].dtype == np.uint8
    for r, md in ((res, 10000), (near, 4000)):
        want, _ = R.majority_vote(coords, nb, edges, eb, g['default'], np.array((10., 10., 25.)), md)
        assert np.array_equal(r['myelin_avg%d' % md], want) and r['myelin_avg%d' % md].dtype == np.uint8
