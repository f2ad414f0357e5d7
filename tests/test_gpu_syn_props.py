"""GPU: the synapse properties (csrc/sd_syn_props.hip; ``classify_synssv_objects``, ``collect_properties_from_ssv_partners``,
``export_matrix`` of ``extraction.cs_processing_steps``).

1. golden g21 (the reference's own workers over scipy's cKDTree and sklearn's forest), both cases through the public functions:
   ``syn_prob`` bit for bit, every property column equal, the bytes of conn_mat.csv;
2. random cells against the restatement tests/_syn_props_ref.py (pinned to g21 on the CPU): votes, neighbour rows and d^2 equal for
   every query whose first k + 1 reference d^2 are pairwise further apart than a relative 1e-9; the others may be at most 1 %;
3. structure edges: k = 1, 50, 63, 64, k = 65 refused, a query far outside its cell's box, two cells that interleave in space,
   duplicate points, a cell of several tiles with all its points on one line, cells without points."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _syn_props_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
G21 = os.path.join(HERE, 'golden', 'g21_syn_props.npz')
COLUMNS = ('partner_axoness', 'partner_spiness', 'partner_celltypes', 'partner_spineheadvol', 'latent_morph', 'syn_sign')


@pytest.fixture(scope='module')
def g21():
    return dict(np.load(G21))


def case(g, prefix):
    return {k[2:]: v for k, v in g.items() if k.startswith(prefix + '_')}


class Syn:
    def __init__(self, c):
        self.neuron_partners, self.rep_coords, self.syn_type_sym_ratio = c['syn_partners'], c['syn_rep'], c['syn_ratio']

    def __len__(self):
        return len(self.syn_type_sym_ratio)


@pytest.mark.parametrize('prefix', ['a', 'b'])
def test_golden_end_to_end(gpu, g21, prefix, tmp_path):
    from syconn_amd.extraction.cs_processing_steps import (CellTable, PackedForest, classify_synssv_objects, collect_properties_from_ssv_partners,
                                                           export_matrix)
    c = case(g21, prefix)
    f = R.forest_from_case(c)
    forest = PackedForest(f['feature'], f['threshold'], f['left'], f['right'], f['proba'], f['tree_begin'], f['n_features'])
    syn_prob = classify_synssv_objects(c['features'], forest, device=gpu)
    assert syn_prob.dtype == np.float64 and syn_prob.tobytes() == c['syn_prob'].tobytes()
    assert forest.predict_proba(c['features'], gpu).tobytes() == c['rf_predict_proba'].tobytes()
    cells = CellTable.from_cells(R.cells_from_case(c))
    # k 50, ds_vertices 1, ignore [4, 5], the axoness key and sym_thresh come from the config: they are the golden's
    props = collect_properties_from_ssv_partners(Syn(c), cells, c['scaling'], syn_ids=c['syn_ids'], n_embedding=4, device=gpu)
    for key in COLUMNS:
        got = getattr(props, key)
        assert got.dtype == c[key].dtype and got.shape == c[key].shape and got.tobytes() == c[key].tobytes(), key
    path = export_matrix(Syn(c), props, syn_prob, c['mesh_area'], str(tmp_path))
    assert open(path, 'rb').read() == c['csv'].tobytes()


def random_cells(rng, sizes, cube=4000.0):
    pts = (rng.random((sum(sizes), 3)) * cube).astype(np.float32)
    begin = np.concatenate(([0], np.cumsum(sizes)))
    return pts, begin, rng.integers(0, 6, len(pts)).astype(np.int32)


def assert_knn_equal(got, want, keep, k, what=''):
    vote, rows, d2 = got
    assert np.array_equal(vote[keep], want[0][keep]), what
    assert np.array_equal(rows[keep], want[1][keep]), what
    assert d2[keep].tobytes() == want[2][keep][:, :k].tobytes(), what


def test_random_cells_against_the_restatement(gpu):
    from syconn_amd.extraction.cs_processing_steps import segmented_knn
    rng = np.random.default_rng(11)
    pts, begin, lab = random_cells(rng, [3000, 777, 0, 64, 65, 1])
    g = np.arange(0, 4000, 700.0)
    lattice = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)[:200]
    q_xyz = np.concatenate([lattice, lattice[:60] + 0.5, lattice[:30], lattice[:10]])
    q_cell = np.concatenate([np.zeros(200, np.int64), np.ones(60, np.int64), rng.integers(3, 6, 30), np.full(10, 2)])
    for k, labels in ((50, lab), (1, None), (7, lab)):
        want = R.knn(pts, begin, labels, q_cell, q_xyz, k, extra=1)
        flagged = R.ambiguous(want[2][:, :k + 1])
        assert flagged.mean() <= 0.01, (k, flagged.sum())
        got = segmented_knn(pts, begin, labels, q_cell, q_xyz, k, gpu, return_neighbours=True, return_counts=True)
        assert_knn_equal(got[:3], want, ~flagged, k, k)
        assert np.all(got[0][q_cell == 2] == -1) and np.all(got[1][q_cell == 2] == -1) and np.all(np.isinf(got[2][q_cell == 2]))
        assert got[3]['tiles_skipped'] > 0 and got[3]['tiles_visited'] > 0                   # cell 0 has 47 tiles: some are never read
    # float64 points: the same rows widened on the host give the same answer
    got64 = segmented_knn(pts.astype(np.float64), begin, lab, q_cell, q_xyz, 50, gpu, return_neighbours=True)
    want = R.knn(pts, begin, lab, q_cell, q_xyz, 50, extra=1)
    assert_knn_equal(got64, want, ~R.ambiguous(want[2]), 50)


def test_k_edges(gpu):
    """k = 1, 50, 63, 64 over a cell of several tiles and cells of 63, 64, 65 points; k = 65 is refused."""
    from syconn_amd.extraction.cs_processing_steps import segmented_knn
    rng = np.random.default_rng(12)
    pts, begin, lab = random_cells(rng, [500, 63, 64, 65], cube=1000.0)
    q_cell = np.tile(np.arange(4), 8)
    q_xyz = rng.random((32, 3)) * 1000
    for k in (1, 50, 63, 64):
        want = R.knn(pts, begin, lab, q_cell, q_xyz, k, extra=1)
        assert not R.ambiguous(want[2]).any()
        assert_knn_equal(segmented_knn(pts, begin, lab, q_cell, q_xyz, k, gpu, return_neighbours=True), want, np.ones(32, bool), k, k)
    for k in (65, 0, -1):
        with pytest.raises(ValueError, match='1 <= k <= 64'):
            segmented_knn(pts, begin, lab, q_cell, q_xyz, k, gpu)
    with pytest.raises(ValueError):
        segmented_knn(pts, begin, lab, [4], q_xyz[:1], 1, gpu)                             # a cell row outside the table
    with pytest.raises(ValueError):
        segmented_knn(pts, begin, lab[:-1], q_cell, q_xyz, 1, gpu)
    assert len(segmented_knn(pts, begin, lab, [], np.zeros((0, 3)), 5, gpu)) == 0


def test_far_query_and_interleaved_cells(gpu):
    from syconn_amd.extraction.cs_processing_steps import segmented_knn
    # two cells on one integer lattice, alternating like a checkerboard: a query's nearest lattice points belong to both
    g = np.arange(12.0)
    lat = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) * 10
    odd = (lat.sum(1) / 10).astype(np.int64) % 2
    pts = np.concatenate([lat[odd == 0], lat[odd == 1]])
    begin = [0, int((odd == 0).sum()), len(pts)]
    lab = np.concatenate([np.zeros(begin[1], np.int32), np.ones(begin[2] - begin[1], np.int32)])
    rng = np.random.default_rng(13)
    # queries on the quarter lattice, the last two far outside the box: every d^2 is exact in float64, so ties on d^2 (there are many on
    # a lattice) have one right answer, the smaller row, and every query is compared
    q_xyz = np.concatenate([rng.integers(0, 440, (60, 3)) * 0.25, [(1e7, -1e7, 3e6), (-5e5, 40, 40)]])
    for cell in (0, 1):
        q_cell = np.full(len(q_xyz), cell)
        want = R.knn(pts, begin, lab, q_cell, q_xyz, 9)
        got = segmented_knn(pts, begin, lab, q_cell, q_xyz, 9, gpu, return_neighbours=True)
        assert_knn_equal(got, want, np.ones(len(q_xyz), bool), 9, cell)
        assert np.all(got[0] == cell) and np.all((got[1] >= begin[cell]) & (got[1] < begin[cell + 1]))
        other = R.knn(pts, begin, lab, 1 - q_cell, q_xyz, 1)[2][:, 0]
        assert np.sum(other < want[2][:, 0]) > 10                  # for many queries a point of the other cell is the nearest of all


def test_duplicates_and_collinear_points(gpu):
    from syconn_amd.extraction.cs_processing_steps import segmented_knn
    rng = np.random.default_rng(14)
    # cell 0: 40 distinct positions, each five times, shuffled: among equal d^2 the smaller row wins, whatever the sorted order is
    pos = rng.integers(0, 50, (40, 3)).astype(np.float64) * 16
    dup = np.repeat(pos, 5, 0)[rng.permutation(200)]
    # cell 1: 300 points (five tiles) on one line, every tile box is degenerate; cell 2: 130 times the same point
    line = np.outer(rng.permutation(300), (3.0, 4.0, 12.0))
    same = np.tile((7.0, 7.0, 7.0), (130, 1))
    pts = np.concatenate([dup, line, same])
    begin = [0, 200, 500, 630]
    lab = rng.integers(0, 3, len(pts)).astype(np.int32)
    q_xyz = np.concatenate([pos[:10], rng.random((10, 3)) * 800, np.outer(np.arange(10) * 31.5, (3.0, 4.0, 12.0)), rng.random((10, 3)) * 100])
    q_cell = np.concatenate([np.zeros(20, np.int64), np.ones(10, np.int64), np.full(10, 2)])
    for k in (1, 6, 64):
        # ties are the point here: every query is compared, the restatement's stable sort is the (d^2, row) order
        want = R.knn(pts, begin, lab, q_cell, q_xyz, k)
        got = segmented_knn(pts, begin, lab, q_cell, q_xyz, k, gpu, return_neighbours=True)
        assert_knn_equal(got, want, np.ones(len(q_cell), bool), k, k)
    assert np.array_equal(segmented_knn(pts, begin, None, q_cell[30:], q_xyz[30:], 3, gpu, return_neighbours=True)[1], np.tile((500, 501, 502), (10, 1)))


def test_forest_edges(gpu):
    """A forest that holds a tree of a single leaf, values at a threshold, float32 rounding of the row."""
    from syconn_amd.extraction.cs_processing_steps import PackedForest
    third = float(np.float32(1 / 3))                             # the float32 nearest to 1/3, above 1/3
    # tree 0: x0 <= 1/3 (float64) ? [1, 0] : [0.25, 0.75]; tree 1: a leaf [0.5, 0.5]; tree 2: x1 <= 2 ? (x0 <= -1 ? [0, 1] : [1, 0]) : [0.125, 0.875]
    f = PackedForest(feature=[0, 0, 0, 0, 1, 0, 0, 0, 0], threshold=[1 / 3, 0, 0, 0, 2.0, -1.0, 0, 0, 0], left=[1, -1, -1, -1, 5, 6, -1, -1, -1],
                     right=[2, -1, -1, -1, 8, 7, -1, -1, -1],
                     proba=[[0, 0], [1, 0], [0.25, 0.75], [0.5, 0.5], [0, 0], [0, 0], [0, 1], [1, 0], [0.125, 0.875]], tree_begin=[0, 3, 4, 9], n_features=2)
    x = np.array([(1 / 3, 2.0), (third, 2.0), (0.0, 2.0000001), (-1.0, 2.0), (-1.0000001, 1e30), (5.0, -3.0)])
    packed = {k: getattr(f, k) for k in PackedForest._FIELDS}
    want = R.forest_proba(packed, x)
    # row 0: 1/3 rounds UP to float32, so it goes right in tree 0; row 2: 2.0000001 rounds to 2.0 in float32, so left in tree 2
    assert want[0].tolist() == [(0.25 + 0.5 + 1) / 3, (0.75 + 0.5 + 0) / 3] and want[2].tolist() == [(1 + 0.5 + 1) / 3, 0.5 / 3]
    assert f.predict_proba(x, gpu).tobytes() == want.tobytes()
    assert f.predict_proba(np.zeros((0, 2)), gpu).shape == (0, 2)
