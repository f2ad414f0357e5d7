"""GPU: the skeletonisation chain past one grid stride of every kernel (closed forms, no CPU restatement at this size) and a relaxation
that needs more global sweeps than one call of the sweep entry enqueues."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_lattice_of_rods_past_every_grid_stride():
    """One-voxel rods along z on a pitch of 2, each its own label: every rod voxel is a node, n - 1 edges along the rod, radius = the
    smaller in-plane voxel size.  513 x 513 rods of 4 voxels: more components than one stride of the component kernels, more voxels than
    one stride of the voxel kernels, more tiles than the tile grid, more new nodes than the node grid."""
    from syconn_amd import _lib as L
    from syconn_amd.proc.skeleton import trace_chunk
    nx = ny = 513
    Z = 4
    seg = np.zeros((2 * nx, 2 * ny, Z), np.uint64)
    ids = (np.arange(nx * ny, dtype=np.uint64) + 1).reshape(nx, ny)
    seg[::2, ::2, :] = ids[:, :, None]
    n = nx * ny
    T = L.SD_SKELETONIZE_TILE
    assert n > 256 * L.SD_SKELETONIZE_COMP_GRID and seg.size > 256 * L.SD_SKELETONIZE_VOX_GRID and n * Z > L.SD_SKELETONIZE_NODE_GRID
    assert -(-seg.shape[0] // T) * -(-seg.shape[1] // T) > L.SD_SKELETONIZE_TILE_GRID
    o = trace_chunk(seg, (10, 9, 20), dict(scale=0, const=0), dust_threshold=1, max_paths=3)
    assert np.array_equal(o['labels'], ids.reshape(-1)) and (o['sizes'] == Z).all() and not o['void'].any() and o['absorbed'] == 0
    assert np.array_equal(o['node_begin'], np.arange(n + 1) * Z) and np.array_equal(o['edge_begin'], np.arange(n + 1) * (Z - 1))
    x, y = np.divmod(np.arange(n), ny)
    want = (((2 * x) * seg.shape[1] + 2 * y) * Z)[:, None] + np.arange(Z)[None, :]
    assert np.array_equal(o['node_voxel'].reshape(n, Z), want)
    assert (o['radii'] == np.float32(9)).all()
    e = o['edges'].reshape(n, Z - 1, 2)
    assert (np.abs(e[:, :, 0] - e[:, :, 1]) == 1).all()      # every edge joins neighbours along the rod
    assert all(np.array_equal(np.sort(np.unique(e[k])), np.arange(Z)) for k in (0, n // 2, n - 1))
    assert np.array_equal(o['vertices'][-1], np.array([2 * (nx - 1) * 10, 2 * (ny - 1) * 9, (Z - 1) * 20], np.float32))


def test_long_serpentine_needs_many_sweeps():
    """A one-voxel path (rows two voxels apart, joined by diagonal turns, so no voxel can be skipped) that snakes through 5 x 5 tiles: the field crosses a tile seam a hundred times, one sweep each, which is more than
    the first call of the sweep entry enqueues -- the host continues from the reported dirty tiles.  Every path voxel is a node."""
    from syconn_amd.proc.skeleton import trace_chunk
    X = Y = 67
    seg = np.zeros((X, Y, 3), np.uint64)
    path = []
    for k, x in enumerate(range(1, X - 1, 2)):
        ys = list(range(2, Y - 2))
        if k % 2:
            ys.reverse()
        path += [(x, y) for y in ys]
        if x + 2 < X - 1:
            path.append((x + 1, 1 if k % 2 else Y - 2))      # a diagonal turn: with a square corner the path would cut the corner voxel
    for x, y in path:
        seg[x, y, 1] = 8
    o = trace_chunk(seg, (1, 1, 1), dict(scale=0, const=0), dust_threshold=1, max_paths=2)
    assert len(o['labels']) == 1 and o['sizes'][0] == len(path)
    assert max(sw for sw, _ in o['stats']) > 24      # more sweeps than the first two calls enqueue
    idx = np.array([(x * Y + y) * 3 + 1 for x, y in path])
    assert np.array_equal(o['node_voxel'], np.sort(idx)) and len(o['edges']) == len(path) - 1
    rank = {int(v): k for k, v in enumerate(o['node_voxel'])}
    want = {frozenset((rank[int(a)], rank[int(b)])) for a, b in zip(idx[:-1], idx[1:])}
    assert {frozenset(map(int, e)) for e in o['edges']} == want
    assert (o['radii'] == np.float32(1)).all()
