"""GPU: csrc/sd_skeleton.hip past one grid stride of its kernels; every expected value is a closed form.  One grid stride is
SD_SKEL_VOTE_GRID blocks of four waves (one source per wave), SD_SKEL_NODE_GRID blocks of 256 nodes or cells, SD_SKEL_EDGE_GRID blocks
of 256 half edges or edges; a wave's LDS table holds SD_SKEL_LDS_NODES nodes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_chain_longer_than_one_stride_of_the_vote_kernel(gpu):
    """Nodes 100 nm apart (10 voxels at scaling 10), max_dist 10000: the window of node i is [i - 100, i + 100] clipped to the chain,
    201 nodes in the interior; labels (i // 50) % 2."""
    from syconn_amd._lib import SD_SKEL_VOTE_GRID
    from syconn_amd.reps.super_segmentation_helper import skeleton_majority_vote
    n = 4 * SD_SKEL_VOTE_GRID + 1003
    i = np.arange(n)
    nodes = np.stack([10 * i, 0 * i, 0 * i], 1)
    edges = np.stack([i[:-1], i[1:]], 1)
    labels = ((i // 50) % 2).astype(np.int32)
    vote, reached, counts = skeleton_majority_vote(nodes, [0, n], edges, [0, n - 1], labels, (10, 10, 20), 10000, gpu, True, True)
    lo, hi = np.maximum(i - 100, 0), np.minimum(i + 100, n - 1)
    ones = np.concatenate(([0], np.cumsum(labels)))
    c1, size = ones[hi + 1] - ones[lo], hi - lo + 1
    assert size[n // 2] == 201 and np.array_equal(reached, size) and np.array_equal(vote, (c1 > size - c1).astype(np.int32))
    assert counts['sources_redone'] == 0


def test_many_tiny_cells(gpu):
    """More three-node cells than one stride of the per-cell and the per-half-edge kernels, every fourth one empty.  A cell is a path
    0 - 1 - 2 with 100 nm edges and max_dist 100: the end nodes see themselves and the middle one, the middle one sees all three.
    The labels (c % 3, c // 3 % 3, c // 9 % 3) run through every combination."""
    from syconn_amd._lib import SD_SKEL_EDGE_GRID, SD_SKEL_NODE_GRID
    from syconn_amd.reps.super_segmentation_helper import skeleton_majority_vote
    n_cells = 256 * SD_SKEL_NODE_GRID + 4000
    c = np.arange(n_cells)
    full = c % 4 != 3
    cf = c[full]
    assert 4 * len(cf) > 256 * SD_SKEL_EDGE_GRID
    node_begin = np.concatenate(([0], np.cumsum(np.where(full, 3, 0))))
    edge_begin = np.concatenate(([0], np.cumsum(np.where(full, 2, 0))))
    nodes = np.stack([np.tile([0, 10, 20], len(cf)), np.repeat(cf % 1000, 3), np.zeros(3 * len(cf), np.int64)], 1)
    edges = np.tile([(1, 0), (1, 2)], (len(cf), 1))
    l0, l1, l2 = cf % 3, cf // 3 % 3, cf // 9 % 3
    labels = np.stack([l0, l1, l2], 1).reshape(-1).astype(np.int8)
    vote, reached = skeleton_majority_vote(nodes, node_begin, edges, edge_begin, labels, (10, 10, 20), 100, gpu, return_reached=True)
    mid = np.where(l0 == l1, l0, np.where(l1 == l2, l1, np.where(l0 == l2, l0, np.minimum(np.minimum(l0, l1), l2))))
    want = np.stack([np.minimum(l0, l1), mid, np.minimum(l1, l2)], 1).reshape(-1)
    assert np.array_equal(reached, np.tile([2, 3, 2], len(cf))) and np.array_equal(vote, want) and vote.dtype == np.int8


def test_grid_graph_takes_the_second_pass(gpu):
    """A 4-connected 48 x 48 grid, 100 nm apart, max_dist r * 100 with the smallest r whose diamond 2 r^2 + 2 r + 1 outgrows the LDS
    table: the window of (x, y) is the Manhattan diamond clipped to the grid.  Label 1 where x >= 24."""
    from syconn_amd._lib import SD_SKEL_LDS_NODES as CAP
    from syconn_amd.reps.super_segmentation_helper import skeleton_majority_vote
    side = 48
    r = next(r for r in range(1, side) if 2 * r * r + 2 * r + 1 > CAP)
    assert side > 2 * r + 1
    x, y = (v.reshape(-1) for v in np.meshgrid(np.arange(side), np.arange(side), indexing='ij'))
    idx = lambda a, b: a * side + b
    edges = np.concatenate([np.stack([idx(x, y), idx(x + 1, y)], 1)[x < side - 1], np.stack([idx(x, y), idx(x, y + 1)], 1)[y < side - 1]])
    edges = edges[np.random.default_rng(5).permutation(len(edges))]
    nodes = np.stack([10 * x, 10 * y, 0 * x], 1)
    labels = (x >= side // 2).astype(np.int64)
    size, ones = np.zeros(side * side, np.int64), np.zeros(side * side, np.int64)
    for dx in range(-r, r + 1):
        ok = (x + dx >= 0) & (x + dx < side)
        col = np.where(ok, np.minimum(y + r - abs(dx), side - 1) - np.maximum(y - (r - abs(dx)), 0) + 1, 0)
        size += col
        ones += np.where(x + dx >= side // 2, col, 0)
    vote, reached, counts = skeleton_majority_vote(nodes, [0, side * side], edges, [0, len(edges)], labels, (10, 10, 20), 100 * r, gpu, True, True)
    inner = (x >= r) & (x < side - r) & (y >= r) & (y < side - r)
    assert inner.sum() > 0 and (size[inner] == 2 * r * r + 2 * r + 1).all()
    assert np.array_equal(reached, size) and np.array_equal(vote, (ones > size - ones).astype(np.int64))
    assert counts['sources_redone'] == int((size > CAP).sum()) >= inner.sum()


def test_compartments_every_share_up_to_100(gpu):
    """One component per (c1, total), 1 <= c1 <= total <= 100: a chain of `total` nodes, c1 of them labelled 1 and the rest 3 and 4 in
    turn, shuffled; the components hang on one chain, separated by soma nodes.  5050 components, more nodes than one stride of the
    per-node kernels.  Expected: the smallest most frequent label, 0 where that is 1 and 50 c1 < 33 total."""
    from syconn_amd._lib import SD_SKEL_NODE_GRID
    from syconn_amd.reps.super_segmentation_helper import skeleton_compartment_majority
    rng = np.random.default_rng(9)
    total = np.repeat(np.arange(1, 101), np.arange(1, 101))
    c1 = np.concatenate([np.arange(1, t + 1) for t in range(1, 101)])
    parts, want = [], []
    for c, t in zip(c1.tolist(), total.tolist()):
        rest = t - c
        n3, n4 = (rest + 1) // 2, rest // 2
        lab = np.concatenate([np.full(c, 1), np.full(n3, 3), np.full(n4, 4)])
        maj = 1 if c >= n3 else 3
        if maj == 1 and 50 * c < 33 * t:
            maj = 0
        parts += [lab[rng.permutation(t)], [2]]
        want += [np.full(t, maj), [2]]
    labels, want = np.concatenate(parts).astype(np.int32), np.concatenate(want)
    n = len(labels)
    assert n > 256 * SD_SKEL_NODE_GRID and len(c1) == 5050
    edges = np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    edges = edges[rng.permutation(n - 1)]
    out = skeleton_compartment_majority([0, n], edges, [0, n - 1], labels, device=gpu)
    assert np.array_equal(out, want) and out.dtype == np.int32 and (want == 0).any() and (want == 1).any()
