"""GPU: sd_glia_split past one grid stride (SD_GLIA_GRID blocks of 256 items) of nodes, of edges that pass the filter of each of the four
passes, of cells and of final components, against closed-form answers.

60,000 path cells of 12 nodes: node p of a cell has the box [(1000 p, 0, 0), (1000 p + 600, 0, 0)], so a run of k consecutive nodes has the
size 1000 (k - 1) + 600 exactly, and T = 2600 is the size of a run of 3.  By c % 8:
  0      N N N g N N N g N N N g   every neuron run is exactly T, which is not significant: outcome 1, all glia, one component
  1      N N N N N N N N N N g g   a neuron run of 10, the glia run of 2 is 1600: outcome 2, all neuron, one component
  2..7   N N N N g N G G G G N N   neuron run {0..3} = 3600 and glia run {6..9} = 3600 are significant: outcome 3; g = {4} (600) is tiny, so
                                   {0..5} is one piece of 5600 and stays; {10, 11} = 1600 is below T and goes to the glia: neuron {0..5},
                                   glia {6..11}
and 210,000 single-node cells given as self loops, by s % 3: a neuron of 3600 (outcome 2), a neuron of 600 (outcome 1), a glia node of 3600
(outcome 1).  Edges are shuffled and half of them flipped with a fixed seed."""
import numpy as np
import pytest

import _glia_gpu as D
from syconn_amd import _lib

pytestmark = pytest.mark.gpu
U = np.uint64
STRIDE = _lib.SD_GLIA_GRID * 256
N_PATH, N_SINGLE, T = 60_000, 210_000, 2600.0
PATTERNS = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 1, 0, 1, 1, 1, 1, 0, 0]], np.uint8)
SIZE1 = np.array([[2600, 2600, 2600, 600, 2600, 2600, 2600, 600, 2600, 2600, 2600, 600], [9600] * 10 + [1600] * 2,
                  [3600, 3600, 3600, 3600, 600, 600, 3600, 3600, 3600, 3600, 1600, 1600]], np.float64)
NAN = np.nan
SIZE2 = np.array([[NAN] * 12, [NAN] * 12, [5600] * 6 + [NAN] * 4 + [1600] * 2], np.float64)
FINAL = np.array([[1] * 12, [0] * 12, [0] * 6 + [1] * 6], np.uint8)
COMP = np.array([[0] * 12, [0] * 12, [0] * 6 + [6] * 6])                           # the first node of the final component, within the cell


def test_past_one_grid_stride(gpu):
    rng = np.random.default_rng(260)
    kind = np.minimum(np.arange(N_PATH) % 8, 2)                                    # 0, 1, 2 = the three patterns
    base = U(1) + U(16) * np.arange(N_PATH, dtype=U)
    path_ids = (base[:, None] + np.arange(12, dtype=U)[None]).reshape(-1)
    s_kind = np.arange(N_SINGLE) % 3
    single_ids = U(16) * U(N_PATH) + U(100) + np.arange(N_SINGLE, dtype=U)
    ids = np.concatenate([path_ids, single_ids])
    n = len(ids)
    boxes = np.zeros((n, 2, 3))
    boxes[:12 * N_PATH, 0, 0] = np.tile(np.arange(12) * 1000.0, N_PATH)
    boxes[:12 * N_PATH, 1, 0] = boxes[:12 * N_PATH, 0, 0] + 600
    boxes[12 * N_PATH:, 1, 0] = np.where(s_kind == 1, 600.0, 3600.0)
    glia = np.concatenate([PATTERNS[kind].reshape(-1), (s_kind == 2).astype(np.uint8)])
    edges = np.concatenate([np.stack([path_ids.reshape(-1, 12)[:, :-1].reshape(-1), path_ids.reshape(-1, 12)[:, 1:].reshape(-1)], 1),
                            np.stack([single_ids, single_ids], 1)])
    edges = edges[rng.permutation(len(edges))]
    flip = rng.random(len(edges)) < 0.5
    edges[flip] = edges[flip][:, ::-1]
    # expected
    cls = np.concatenate([FINAL[kind].reshape(-1), np.where(s_kind == 0, 0, 1).astype(np.uint8)])
    comp = np.concatenate([(base[:, None] + COMP[kind].astype(U)).reshape(-1), single_ids])
    size1 = np.concatenate([SIZE1[kind].reshape(-1), np.where(s_kind == 1, 600.0, 3600.0)])
    size2 = np.concatenate([SIZE2[kind].reshape(-1), np.full(N_SINGLE, NAN)])
    cell = np.concatenate([np.repeat(base, 12), single_ids])
    outcome = np.concatenate([kind + 1, np.where(s_kind == 0, 2, 1)]).astype(np.uint8)
    row = lambda v: np.searchsorted(ids, v)
    a, b = row(edges[:, 0]), row(edges[:, 1])
    three = np.concatenate([np.repeat(kind == 2, 12), np.zeros(N_SINGLE, bool)])
    part = three & ((glia == 0) | (size1 < T))                                     # pass C: neuron or tiny, in outcome-3 cells
    n_cells = N_PATH + N_SINGLE
    n_final = int((kind == 2).sum()) + n_cells
    # the counts exceed one grid stride: nodes, the edges each pass unites or keeps, cells, final components
    for v in (n, len(edges), int((glia[a] == glia[b]).sum()), int((part[a] & part[b]).sum()), int((cls[a] == cls[b]).sum()), n_cells, n_final):
        assert v > STRIDE, (v, STRIDE)
    rc, c, got = D.split(gpu, edges, ids, boxes, glia, T, sv_sizes=np.ones(n, np.int64))
    assert rc == 0 and c[7] == 0 and not c[10:13].any()
    assert c[0] == n and c[1] == n_cells and c[2] + c[4] == n_final and c[3] + c[5] == n and c[9] == int((cls == 1).sum())
    assert c[13:16].tolist() == [int((outcome == k).sum()) for k in (1, 2, 3)]
    assert np.array_equal(got['node_ids'], ids) and np.array_equal(got['node_cell'], cell) and np.array_equal(got['node_class'], cls)
    assert np.array_equal(got['node_comp'], comp) and np.array_equal(got['node_size1'], size1) and np.array_equal(got['node_size2'], size2, equal_nan=True)
    assert np.array_equal(got['cell_ids'], np.concatenate([base, single_ids])) and np.array_equal(got['cell_outcome'], outcome)
    for k, t in ((0, got['neuron']), (1, got['glia'])):
        mine = cls == k
        heads = np.flatnonzero(mine & (comp == ids))
        assert np.array_equal(t['sv_ids'], ids[mine]) and np.array_equal(t['cc_ids'], ids[heads]) and np.array_equal(t['cc_cell'], cell[heads])
        assert np.array_equal(t['sv_begin'], np.concatenate([np.searchsorted(np.flatnonzero(mine), heads), [mine.sum()]]))
    assert np.array_equal(got['neuron_edges'], edges[(cls[a] == 0) & (cls[b] == 0)]) and c[6] == len(got['neuron_edges']) > STRIDE
    assert np.array_equal(got['astrocyte_edges'], edges[(cls[a] == 1) & (cls[b] == 1)]) and c[8] == len(got['astrocyte_edges']) > STRIDE
