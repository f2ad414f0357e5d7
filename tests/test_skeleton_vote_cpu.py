"""CPU: the skeleton votes without a device -- the restatement (tests/_skeleton_ref.py) against the golden vectors the reference's own
functions produced (tests/golden/g23_skeleton.npz), the integer form of the 0.66 rule against numpy, the argument checks of the table
API and the error paths of the drop-ins that need no device."""
import os
import types

import numpy as np
import pytest

import _skeleton_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g23_skeleton.npz')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


@pytest.mark.parametrize('p', ['a_', 'b_'])
def test_restatement_matches_golden_votes(gold, p):
    vote, reached = R.majority_vote(gold[p + 'nodes'], gold[p + 'node_begin'], gold[p + 'edges'], gold[p + 'edge_begin'], gold[p + 'labels'],
                                    gold[p + 'scaling'], int(gold[p + 'max_dist']))
    assert np.array_equal(reached, gold[p + 'reached'])
    assert np.array_equal(vote, gold[p + 'vote'])


def test_restatement_matches_golden_compartments(gold):
    comp = R.compartment_majority(gold['c_node_begin'], gold['c_edges'], gold['c_edge_begin'], gold['c_labels'])
    assert np.array_equal(comp.astype(np.float64), gold['c_comp'])


def test_restatement_smooths_golden_semseg(gold):
    """From the golden node predictions on: merge 3, 4 -> 1, vote, recover the boutons, compartment vote, recover again."""
    g = gold
    pred = g['s_pred']
    avg, _ = R.majority_vote(g['s_nodes'], g['s_node_begin'], g['s_edges'], g['s_edge_begin'], pred, g['s_scaling'], int(g['s_max_dist']))
    assert np.array_equal(avg[avg != 1], g['s_avg'][avg != 1]) and set(g['s_avg'][avg == 1].tolist()) <= {1, 3, 4}
    comp = R.compartment_majority(g['s_node_begin'], g['s_edges'], g['s_edge_begin'], g['s_avg'])
    assert np.array_equal(comp[comp != 1], g['s_comp'][comp != 1]) and set(g['s_comp'][comp == 1].tolist()) <= {1, 3, 4}


def test_integer_rule_is_the_numpy_expression():
    """50 c1 < 33 total  <=>  (float32(c1) / total < 0.66) with the comparison in float32 (numpy 1, the reference's environment, and
    numpy 2 with a Python scalar) and in float64, for every 1 <= c1 <= total <= 4096."""
    total = np.repeat(np.arange(1, 4097), np.arange(1, 4097))
    c1 = np.concatenate([np.arange(1, t + 1) for t in range(1, 4097)])
    want = R.share_below_066(c1, total)
    p32 = c1.astype(np.float32) / total                                           # np.array(cnts, float32) / np.sum(cnts): float64 in numpy
    assert np.array_equal(p32.astype(np.float32) < np.float32(0.66), want)
    assert np.array_equal(c1.astype(np.float32) / total.astype(np.float32) < np.float32(0.66), want)
    assert np.array_equal(c1.astype(np.float64) / total < 0.66, want)


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
def _ok():
    return dict(nodes=np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0)]), node_begin=[0, 3], edges=np.array([(0, 1), (1, 2)]), edge_begin=[0, 2],
                labels=np.array([0, 1, 1]), scaling=(10, 10, 20))


@pytest.mark.parametrize('change, match', [
    (dict(nodes=np.zeros((3, 2))), 'shape'),
    (dict(nodes=np.array([(0, 0, 0), (1, 0, np.nan), (2, 0, 0)])), 'finite'),
    (dict(scaling=(10, 10)), 'scaling'),
    (dict(scaling=(10, np.inf, 20)), 'scaling'),
    (dict(node_begin=[0, 2]), 'node_begin'),
    (dict(node_begin=[1, 3]), 'node_begin'),
    (dict(node_begin=[0, 4, 3]), 'node_begin'),
    (dict(edge_begin=[0, 1]), 'edge_begin'),
    (dict(edge_begin=[0, 1, 2]), 'edge_begin'),
    (dict(edges=np.array([(0, 1), (1, 3)])), 'outside its cell'),
    (dict(edges=np.array([(0, 1), (-1, 2)])), 'outside its cell'),
    (dict(edges=np.array([(0., 1.), (1., 2.)])), 'integers'),
    (dict(edges=np.array([0, 1, 2])), 'shape'),
    (dict(labels=np.array([0, 1])), 'labels'),
    (dict(labels=np.array([0., 1., 1.])), 'integers'),
    (dict(max_dist=-1), 'max_dist'),
    (dict(max_dist=float('nan')), 'max_dist'),
    (dict(max_dist=None), 'max_dist'),
])
def test_majority_vote_argument_checks(change, match):
    from syconn_amd.reps.super_segmentation_helper import skeleton_majority_vote
    with pytest.raises(ValueError, match=match):
        skeleton_majority_vote(**{**_ok(), **change})


def test_more_than_64_labels_raise():
    from syconn_amd.reps.super_segmentation_helper import skeleton_compartment_majority, skeleton_majority_vote
    n = 65
    nodes = np.stack([np.arange(n), np.zeros(n), np.zeros(n)], 1)
    edges = np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    with pytest.raises(ValueError, match='at most 64'):
        skeleton_majority_vote(nodes, [0, n], edges, [0, n - 1], np.arange(n), (1, 1, 1))
    with pytest.raises(ValueError, match='at most 64'):
        skeleton_compartment_majority([0, n], edges, [0, n - 1], np.arange(n) + 10)


@pytest.mark.parametrize('change, match', [
    (dict(node_begin=[0, 2]), 'node_begin'),
    (dict(edge_begin=[0, 3]), 'edge_begin'),
    (dict(edges=np.array([(0, 1), (1, 3)])), 'outside its cell'),
    (dict(labels=np.array([0., 1., 1.])), 'integers'),
])
def test_compartment_argument_checks(change, match):
    from syconn_amd.reps.super_segmentation_helper import skeleton_compartment_majority
    ok = {k: v for k, v in _ok().items() if k in ('node_begin', 'edges', 'edge_begin', 'labels')}
    with pytest.raises(ValueError, match=match):
        skeleton_compartment_majority(**{**ok, **change})


def test_empty_tables_need_no_device():
    from syconn_amd.reps.super_segmentation_helper import skeleton_compartment_majority, skeleton_edge_weights, skeleton_majority_vote
    z = np.zeros((0, 3))
    vote, reached = skeleton_majority_vote(z, [0, 0, 0], np.zeros((0, 2), np.int64), [0, 0, 0], np.zeros(0, np.int16), (10, 10, 20), return_reached=True)
    assert vote.shape == (0,) and vote.dtype == np.int16 and reached.shape == (0,) and reached.dtype == np.uint32
    assert skeleton_compartment_majority([0], np.zeros((0, 2), np.int64), [0], np.zeros(0, np.int8)).dtype == np.int8
    assert skeleton_edge_weights(z, [0, 0], np.zeros((0, 2), np.int64), [0, 0], (10, 10, 20)).shape == (0,)


def test_edge_weights_are_the_reference_expression(gold):
    from syconn_amd.reps.super_segmentation_helper import skeleton_edge_weights
    for p in ('a_', 'b_'):
        nb, eb = gold[p + 'node_begin'], gold[p + 'edge_begin']
        w = skeleton_edge_weights(gold[p + 'nodes'], nb, gold[p + 'edges'], eb, gold[p + 'scaling'])
        want = np.concatenate([R.edge_weights(gold[p + 'nodes'][nb[c]:nb[c + 1]], gold[p + 'edges'][eb[c]:eb[c + 1]], gold[p + 'scaling'])
                               for c in range(len(nb) - 1)])
        assert w.dtype == want.dtype and np.array_equal(w, want)


# ---- drop-ins ----------------------------------------------------------------------------------------------------------------------
class _Sso:
    def __init__(self, nodes, edges, verts=np.zeros((0, 3), np.float32), **attrs):
        self.id, self.scaling, self.saved = 7, np.array([10, 10, 20]), 0
        self.skeleton = dict(nodes=nodes, edges=edges, **attrs)
        self.mesh = (np.zeros(0, np.uint32), np.asarray(verts, np.float32).reshape(-1), np.zeros(0, np.float32))

    def load_skeleton(self):
        pass

    def save_skeleton(self):
        self.saved += 1

    def label_dict(self, what):
        return {'axoness': np.zeros(len(self.mesh[1]) // 3, np.int64)}


def test_missing_property_raises_the_reference_error():
    from syconn_amd.reps.super_segmentation_helper import majorityvote_skeleton_property
    sso = _Sso(np.zeros((2, 3), np.int64), np.array([(0, 1)]))
    with pytest.raises(ValueError, match='Given property "myelin" does not exist in skeleton of SSV 7.'):
        majorityvote_skeleton_property(sso, 'myelin')


def test_semsegaxoness2skel_zero_branch(gold):
    """No nodes or no mesh vertices: (n, 1) zeros under both smoothed keys, the skeleton saved once, pred_key untouched."""
    from syconn_amd.reps.super_segmentation_object import semsegaxoness2skel
    for case, (nodes, verts) in enumerate([(np.array([(0, 0, 0), (10, 0, 0)]), np.zeros((0, 3))), (np.zeros((0, 3), np.int64), np.ones((10, 3)))]):
        sso = _Sso(nodes, np.zeros((0, 2), np.int64), verts)
        semsegaxoness2skel(sso, dict(k=20, ds_vertices=20), 'axoness', 2000)
        assert sso.saved == 1 and 'axoness' not in sso.skeleton
        for j, key in enumerate(('axoness_avg2000', 'axoness_avg2000_comp_maj')):
            assert sso.skeleton[key].shape == tuple(gold['s_zero_shapes'][case][j]) == (len(nodes), 1) and not sso.skeleton[key].any()
    sso = _Sso(None, None)
    sso.skeleton = None
    assert semsegaxoness2skel(sso, dict(k=20, ds_vertices=20), 'axoness', 2000) is None and sso.saved == 0


def test_table_forms_check_their_arguments():
    from syconn_amd.reps.super_segmentation_object import semsegaxoness2skel_table
    from syconn_amd.extraction.cs_processing_steps import CellTable
    with pytest.raises(TypeError):
        semsegaxoness2skel_table(types.SimpleNamespace(), np.zeros((0, 2)), [0], dict(k=20, ds_vertices=20), 'axoness', 2000, (10, 10, 20))
    cells = CellTable([1], np.zeros((0, 3)), [0, 0], {}, np.zeros((0, 3)), [0, 0], {})
    with pytest.raises(ValueError, match='at most 64'):
        semsegaxoness2skel_table(cells, np.zeros((0, 2), np.int64), [0, 0], dict(k=65, ds_vertices=20), 'axoness', 2000, (10, 10, 20))
