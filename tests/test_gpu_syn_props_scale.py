"""GPU: csrc/sd_syn_props.hip on analytic lattices past every launch cap and one grid stride of its kernels.  One grid stride is
SD_SYN_PROPS_CELL_GRID = 4096 blocks of four waves (one cell per wave: 16384 cells) for the per-cell kernels, SD_SYN_PROPS_QUERY_GRID =
8192 blocks of four waves (one query per wave: 32768 queries) for the query kernel, SD_SYN_PROPS_FOREST_GRID = 1024 blocks of 256 rows
(262144 rows) for the forest, SD_SYN_PROPS_POINT_GRID = 1024 blocks of 256 points (262144 points) for the per-point kernels; a query
tests the tile boxes of its cell 64 at a time.  Every expected value is a closed form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_many_tiny_cells(gpu):
    """20000 cells of 1 + c % 3 points, more than one stride of the per-cell kernels; every third cell empty.  Cell c sits at x = 100 c:
    its points are (100 c, 10 j, 0), j = 0 .. size - 1, stored in descending j; the query (100 c + 1, 12, 0) has the point j at
    d^2 = 1 + (12 - 10 j)^2: j = 1 (5), j = 2 (65), j = 0 (145)."""
    from syconn_amd._lib import SD_SYN_PROPS_CELL_GRID
    from syconn_amd.extraction.cs_processing_steps import segmented_knn
    n = 20000
    assert n > SD_SYN_PROPS_CELL_GRID * 4
    c = np.arange(n)
    size = np.where(c % 4 == 3, 0, 1 + c % 3)
    begin = np.concatenate(([0], np.cumsum(size)))
    cell_of = np.repeat(c, size)
    j = size[cell_of] - 1 - (np.arange(begin[-1]) - begin[cell_of])               # descending inside the cell
    pts = np.stack([100.0 * cell_of, 10.0 * j, np.zeros(len(j))], 1)
    lab = (7 * cell_of + j).astype(np.int32)
    q_xyz = np.stack([100.0 * c + 1, np.full(n, 12.0), np.zeros(n)], 1)
    vote, rows, d2 = segmented_knn(pts, begin, lab, c, q_xyz, 2, gpu, return_neighbours=True)
    order = np.array([[0, -1, -1], [1, 0, -1], [1, 2, 0]])[np.maximum(size, 1) - 1][:, :2]        # j of the nearest two, by size
    order = np.where((size == 0)[:, None], -1, order)
    want_rows = np.where(order >= 0, begin[:-1, None] + size[:, None] - 1 - order, -1)
    want_d2 = np.where(order >= 0, 1.0 + (12.0 - 10.0 * order) ** 2, np.inf)
    assert np.array_equal(rows, want_rows) and np.array_equal(d2, want_d2)
    assert np.array_equal(vote, np.where(size == 0, -1, 7 * c + order[:, 0]))                        # one vote each: the nearest is first


def test_more_queries_than_one_stride_over_many_tiles(gpu):
    """40000 queries, more than one stride of the query kernel, on one cell of 67^3 = 300763 lattice points (more than one stride of
    the per-point kernels; 4700 tiles: more than the 64 boxes a wave tests at a time), spacing 10, stored shuffled.  The query at an interior lattice point + (1, 2, 3) has that point at
    d^2 = 14, then the neighbours one step on in z (1 + 4 + 49 = 54), y (1 + 64 + 9 = 74) and x (81 + 4 + 9 = 94), then the one a step
    on in y and z (1 + 64 + 49 = 114)."""
    from syconn_amd._lib import SD_SYN_PROPS_POINT_GRID, SD_SYN_PROPS_QUERY_GRID
    from syconn_amd.extraction.cs_processing_steps import segmented_knn
    n_q, side = 40000, 67
    assert n_q > SD_SYN_PROPS_QUERY_GRID * 4 and side ** 3 > SD_SYN_PROPS_POINT_GRID * 256 and side ** 3 > 64 * 64
    g = np.arange(side)
    lat = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    perm = np.random.default_rng(21).permutation(len(lat))
    pts = (lat[perm] * 10).astype(np.float32)
    row_of = np.empty(len(lat), np.int64)                                          # lattice index -> stored row
    row_of[perm] = np.arange(len(lat))
    flat = lambda p: (p[:, 0] * side + p[:, 1]) * side + p[:, 2]
    inner = lat[np.all((lat >= 1) & (lat <= side - 2), 1)]
    at = inner[np.arange(n_q) % len(inner)]
    q_xyz = at * 10.0 + np.array((1.0, 2.0, 3.0))
    lab = (lat[perm].sum(1) % 5).astype(np.int32)
    vote, rows, d2, counts = segmented_knn(pts, [0, len(pts)], lab, np.zeros(n_q, np.int64), q_xyz, 5, gpu, return_neighbours=True, return_counts=True)
    steps = np.array([(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 1, 1)])
    want_rows = np.stack([row_of[flat(at + s)] for s in steps], 1)
    assert np.array_equal(rows, want_rows) and np.array_equal(d2, np.tile((14.0, 54.0, 74.0, 94.0, 114.0), (n_q, 1)))
    # labels in list order: s, s + 1, s + 1, s + 1, s + 2 (mod 5) with s = the coordinate sum: three of a kind win
    assert np.array_equal(vote, (at.sum(1) + 1) % 5)
    assert counts['tiles_skipped'] > 0 and counts['tiles_visited'] >= n_q


def test_more_forest_rows_than_one_stride(gpu):
    """300000 rows of two features, more than one stride of the forest kernel, through four trees of depth 1: tree t goes left iff
    x[t % 2] <= t + 0.5, left leaf (1, 0), right leaf (0, 1).  Row r = (r % 5, (r // 5) % 7): column 1 = (trees gone right) / 4."""
    from syconn_amd._lib import SD_SYN_PROPS_FOREST_GRID
    from syconn_amd.extraction.cs_processing_steps import PackedForest
    n = 300000
    assert n > SD_SYN_PROPS_FOREST_GRID * 256
    t = np.arange(4)
    f = PackedForest(feature=np.stack([t % 2, 0 * t, 0 * t], 1).reshape(-1), threshold=np.stack([t + 0.5, 0.0 * t, 0.0 * t], 1).reshape(-1),
                     left=np.stack([3 * t + 1, -1 + 0 * t, -1 + 0 * t], 1).reshape(-1), right=np.stack([3 * t + 2, -1 + 0 * t, -1 + 0 * t], 1).reshape(-1),
                     proba=np.tile([(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)], (4, 1)), tree_begin=3 * np.arange(5), n_features=2)
    r = np.arange(n)
    x = np.stack([r % 5, (r // 5) % 7], 1).astype(np.float64)
    right = sum((x[:, k % 2] > k + 0.5).astype(np.float64) for k in range(4))
    got = f.predict_proba(x, gpu)
    assert np.array_equal(got[:, 1], right / 4) and np.array_equal(got[:, 0], (4 - right) / 4)
