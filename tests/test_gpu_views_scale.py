"""GPU: csrc/sd_views.hip past one grid stride of its kernels -- more (location, view) items than SD_VIEWS_RASTER_GRID workgroups and
more locations than the waves of one stride of the candidate kernels, more triangles than one stride of the index kernels, more pixels
than one stride of the vote, more locations than the waves of one stride of the rotation solver and more vertices than one stride of
the rotation's key and place kernels."""
import os

import numpy as np
import pytest

import _views_gpu as G
import _views_ref as R
from syconn_amd import _lib as L
from test_gpu_views import ROT_BOUND

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g27_views.npz')


def test_locations_past_the_raster_stride(gpu):
    """4097 locations x 1 view x 1 tile > SD_VIEWS_RASTER_GRID, and 4097 waves > the 4096 of one stride of the candidate kernels."""
    n = L.SD_VIEWS_RASTER_GRID + 1
    assert n > L.SD_VIEWS_GRID * 4
    v, t = R.edge_cases()['shared_edge']
    m = G.Mesh(gpu, v, t, np.zeros(3), 1.0)
    shifts = np.array([(0.0, 0.0, 0.0), (0.25, 0.0, 0.0), (0.0, 0.125, 0.0), (-0.5, 0.25, 0.25), (0.125, -0.125, -0.5), (3.0, 0.0, 0.0), (0.0, 0.0, 0.9),
                       (0.0625, 0.0625, 0.0)], np.float32)
    coords = shifts[np.arange(n) % len(shifts)]
    rot = np.tile(R.IDENTITY, (n, 1))
    rot[5::16] = 0
    for index in (False, True):
        uniq, _ = R.render(v, t, shifts, np.tile(R.IDENTITY, (len(shifts), 1)), R.edge_lengths(2.0, 1.0), 1, (8, 4), index=index)
        want = uniq[np.arange(n) % len(shifts)].copy()
        want[5::16] = R.BG_INDEX if index else 255
        rc, c, got = m.render(coords, rot, 2.0, 1, (8, 4), index=index)
        assert rc == 0 and np.array_equal(got, want)
        assert len(np.unique(want[:8].reshape(8, -1), axis=0)) >= 5                 # the shifts give different views


def test_triangles_past_the_index_stride(gpu):
    """A lattice of 2 * 363^2 = 263,538 triangles > 262,144 = one stride of the index kernels, in the plane Zf = 0.375: every pixel of a
    window inside the lattice holds the byte 96, which the filter keeps (a constant image stays constant)."""
    k = 363
    assert 2 * k * k > L.SD_VIEWS_GRID * 256
    gx, gy = np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing='ij')
    verts = np.stack([gx * 0.05 - 9.0, gy * 0.05 - 9.0, np.full(gx.shape, R.z_of(0.375))], -1).reshape(-1, 3).astype(np.float32)
    a = (gx[:-1, :-1] * (k + 1) + gy[:-1, :-1]).reshape(-1)
    tris = np.concatenate([np.stack([a, a + k + 1, a + k + 2], 1), np.stack([a, a + k + 2, a + 1], 1)]).astype(np.uint32)
    m = G.Mesh(gpu, verts, tris, np.zeros(3), 1.0)
    assert m.rc == 0 and not m.counts.any()
    coords = np.array([(0.0, 0.0, 0.0), (3.03, -2.51, 0.0), (8.6, 8.6, 0.0)], np.float32)      # the last one looks over the lattice's corner
    rot = np.tile(R.IDENTITY, (3, 1))
    rc, c, got = m.render(coords, rot, 2.0, 1, (32, 16))
    assert rc == 0 and c[2] == 0 and (got[:2] == 96).all()
    x_edge = int(np.floor((9.15 - 8.6 + 1.0) / 2.0 * 32 - 0.5))                     # the last column whose sample lies inside x <= 9.15
    assert (got[2][0, :, :x_edge - 3] == 96).all() and (got[2][0, :, x_edge + 4:] == 255).all()
    rc, c, ix = m.render(coords[:2], rot[:2], 2.0, 1, (32, 16), index=True)
    assert rc == 0 and (ix != R.BG_INDEX).all()
    cx = (np.arange(32) + 0.5) / 16 - 1.0                                           # the lattice cell under every sample of view 0
    cy = (np.arange(16) + 0.5) / 16 - 0.5
    cell_x, cell_y = np.floor((cx + 9.0) / 0.05 + 1e-9).astype(int), np.floor((cy + 9.0) / 0.05 + 1e-9).astype(int)
    corner = (cell_x[None, :] * (k + 1) + cell_y[:, None])
    last = ix[0, 0].astype(np.int64) - corner                                      # the last vertex of either triangle of that cell
    assert np.isin(last, (k + 2, 1)).all()


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope='module')
def rot_small(gpu, gold):
    """The 52 clouds of the golden, which test_rotations_against_golden compares with the reference."""
    g = gold
    rc, c, rot, empty = G.rotations(gpu, g['r_verts'], g['r_coords'], g['r_edge'])
    assert rc == 0 and not c.any()
    rot.setflags(write=False)
    return rot, empty


def test_rotation_locations_past_one_stride(gpu, gold, rot_small):
    """4201 locations > the 4096 waves of one stride of k_vw_rot_solve: a location's result does not depend on the others (its sums go
    through one fixed butterfly), so every repeat equals the 52-location call bit for bit."""
    g = gold
    n = L.SD_VIEWS_GRID * 4 + 105
    rep = np.arange(n) % 52
    rot, empty = rot_small
    rc, c, big, empty_big = G.rotations(gpu, g['r_verts'], g['r_coords'][rep], g['r_edge'])
    assert rc == 0 and not c.any()
    assert np.array_equal(big, rot[rep]) and np.array_equal(empty_big, empty[rep])
    assert big[-1].any() and big[L.SD_VIEWS_GRID * 4].any()                         # the second trip wrote matrices
    rc, c, none, empty_flag = G.rotations(gpu, g['r_verts'], g['r_coords'][rep], g['r_edge'], flag_only=True)
    assert rc == 0 and none is None and np.array_equal(empty_flag, empty[rep]) and empty[48] and not empty[49]


@pytest.mark.parametrize('fill', [50.0, -50.0])
def test_rotation_vertices_past_one_stride(gpu, gold, rot_small, fill):
    """266,006 vertices > 262,144 = one stride of k_vw_rot_keys / k_vw_rot_place, the cloud across the stride's end behind a filler
    that is no inlier anywhere: the inliers are the same, their order in the sums need not be.  The filler at 50 has the largest
    Morton code and is sorted behind the cloud; the one at -50 has code 0 and is sorted in front of it, so the cloud lies across the
    stride's end in the sorted order that k_vw_rot_place writes as well."""
    g = gold
    verts = np.concatenate([np.full((255000, 3), fill, np.float32), g['r_verts']])
    assert len(verts) > L.SD_VIEWS_GRID * 256 > 255000
    rot, empty = rot_small
    rc, c, big, empty_big = G.rotations(gpu, verts, g['r_coords'], g['r_edge'])
    assert rc == 0 and not c.any()
    assert np.array_equal(empty_big, empty) and np.array_equal(big.any(1), rot.any(1))           # <= 2 inliers: 16 zeros
    fixed = [3, 7, 11, 12, 13, 14, 15]                                              # the last row and column of every matrix
    assert np.array_equal(big[:, fixed], rot[:, fixed])
    ok = g['r_gap_ok']
    worst = np.abs(big - rot)[ok].max()
    print(f'rotations with 255,000 filler vertices at {fill}: largest |difference| of an entry = {worst:.3e} over {int(ok.sum())} clouds')
    assert worst <= ROT_BOUND                                                       # sign included


def test_rotation_stride_with_a_remainder(gpu, gold):
    g = gold
    v = g['m_vn'][:1021]
    assert len(v) % 8 == 5
    rc, c, rot8, empty8 = G.rotations(gpu, v, g['m_cn'], g['m_edge'], stride=8)
    rc2, c2, sub, empty_sub = G.rotations(gpu, v[::8], g['m_cn'], g['m_edge'])
    assert rc == rc2 == 0 and not c.any() and np.array_equal(rot8, sub) and np.array_equal(empty8, empty_sub) and rot8.any()


def test_vote_past_one_stride(gpu):
    n_px, n_verts, n_labels = L.SD_VIEWS_GRID * 256 + 1001, 5000, 4
    rng = np.random.default_rng(11)
    idx = rng.integers(0, n_verts, n_px).astype(np.uint32)
    idx[rng.random(n_px) < 0.3] = R.BG_INDEX
    idx[-1] = 17
    lab = rng.integers(0, n_labels, n_px).astype(np.uint8)
    rc, c, labels, table = G.vote(gpu, idx, lab, R.BG_INDEX, n_verts, n_labels, n_labels)
    keep = idx != R.BG_INDEX
    count = np.bincount(idx[keep].astype(np.int64) * n_labels + lab[keep], minlength=n_verts * n_labels).reshape(n_verts, n_labels)
    assert rc == 0 and count.max() < 256 and np.array_equal(table, count.astype(np.uint8))
    assert np.array_equal(labels, np.where(count.sum(1) == 0, n_labels, count.argmax(1)).astype(np.uint8))
