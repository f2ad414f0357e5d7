"""CPU: the numpy restatement of the view raster rule (tests/_views_ref.py) against hand-computed answers and scipy, its normalisation,
rotations, ids and vote against the golden of the reference's own functions (tests/golden/g27_views.npz), and the host-side rules of
syconn_amd.proc.rendering / proc.meshes / reps.super_segmentation_helper that need no device."""
import os

import numpy as np
import pytest
import scipy.ndimage

import _views_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g27_views.npz')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def edge_view(name, index=False, dense=None):
    v, t = R.edge_cases()[name]
    out, dropped = R.render(v, t, np.zeros((1, 3), np.float32), R.IDENTITY[None], R.edge_lengths(R.EDGE_CW, 1.0), 1, R.EDGE_WS, index=index, dense=dense)
    return out[0, 0], dropped


def raw_bytes(name):
    v, t = R.edge_cases()[name]
    D, tb, _ = R.raster_view(v, t, np.zeros(3, np.float32), R.IDENTITY, R.edge_lengths(R.EDGE_CW, 1.0), 1.0, 0.0, *R.EDGE_WS)
    return np.where(D < R.D_ONE, D >> 16, 255).astype(np.uint8), tb


# ---- the raster rule against hand-computed answers -------------------------------------------------------------------------------------
def test_square_on_pixel_centres_exact_bytes():
    """Corners on the centres of pixels (4, 3) and (12, 10) at Zf = 0.5: D = 2^23, byte 128.  With y pointing down the bias rule gives the
    samples on the bottom and right edges to the square and those on the top and left edges not: columns 5 .. 12, rows 4 .. 10."""
    b, _ = raw_bytes('pixel_centres')
    want = np.full((16, 32), 255, np.uint8)
    want[4:11, 5:13] = 128
    assert np.array_equal(b, want)


def test_whole_window_and_flip():
    b, _ = raw_bytes('border')
    assert (b == 64).all()                                                         # Zf = 0.25 -> D = 2^22 -> 64, every sample once
    # y orientation: a triangle in the upper half of eye space (y' > 0) lands in the LOWER rows (Y = (y'/E1 + 0.5) H), glOrtho's
    # inverted y followed by the top-bottom flip of screen_shot
    v = np.array([(R.px_x(2), 0.1, 0.0), (R.px_x(30), 0.1, 0.0), (R.px_x(16), 0.4, 0.0)], np.float32)
    D, _, _ = R.raster_view(v, [(0, 1, 2)], np.zeros(3, np.float32), R.IDENTITY, R.edge_lengths(2.0, 1.0), 1.0, 0.0, 32, 16)
    rows = np.flatnonzero((D < R.D_ONE).any(1))
    assert len(rows) and rows.min() >= 8 and rows.max() <= 14


@pytest.mark.parametrize('name', ['shared_edge', 'shared_edge_flipped'])
def test_shared_edge_covers_every_sample_once(name):
    """The diagonal of the quad runs through pixel centres: with both triangles drawn every sample of the quad is covered, and each
    triangle alone covers disjoint sets (whichever way either is wound)."""
    v, t = R.edge_cases()[name]
    E, c = R.edge_lengths(2.0, 1.0), np.zeros(3, np.float32)
    both = R.raster_view(v, t, c, R.IDENTITY, E, 1.0, 0.0, 32, 16)[0] < R.D_ONE
    a = R.raster_view(v, t[:1], c, R.IDENTITY, E, 1.0, 0.0, 32, 16)[0] < R.D_ONE
    b = R.raster_view(v, t[1:], c, R.IDENTITY, E, 1.0, 0.0, 32, 16)[0] < R.D_ONE
    want = np.zeros((16, 32), bool)
    want[4:12, 5:13] = True
    assert np.array_equal(both, want) and not (a & b).any() and np.array_equal(a | b, want) and a.sum() + b.sum() == 64
    assert a[np.arange(4, 12), np.arange(5, 13)].all() != b[np.arange(4, 12), np.arange(5, 13)].all()      # the diagonal belongs to exactly one


def test_rule_edges_by_hand():
    ix, _ = edge_view('coplanar', index=True)
    assert set(np.unique(ix)) == {2, 7, R.BG_INDEX}                                # triangle 0 (last vertex 2) beats 1 on one half ...
    b, tb = raw_bytes('coplanar')
    assert set(np.unique(tb)) == {-1, 0, 2}                                        # ... and 2 (last vertex 7) beats 3 on the other
    near, _ = raw_bytes('near_plane')
    far, _ = raw_bytes('far_plane')
    assert (near == 255).any() and (near < 64).any() and near[3, 3] == 255          # the part in front of the near plane is cut
    assert (far[far != 255] >= 192).all() and (far != 255).any() and far[3, 3] == 255
    d0, _ = raw_bytes('d_zero')
    assert (d0 == 0).all()
    out, _ = edge_view('d_zero')
    assert (out == 255).all()                                                      # an image whose sum is 0 becomes all 255
    za, tb = raw_bytes('zero_area')
    assert set(np.unique(tb)) == {-1, 3}
    huge, _ = raw_bytes('huge')
    assert (huge == 128).all()
    bb, dropped = edge_view('beyond_bound', index=True)
    assert dropped == 1 and set(np.unique(bb)) == {2, 3, R.BG_INDEX}


@pytest.mark.parametrize('name', sorted(R.edge_cases()))
def test_dense_and_per_triangle_restatements_agree(name):
    for index in (False, True):
        a, da = edge_view(name, index, dense=True)
        b, db = edge_view(name, index, dense=False)
        assert np.array_equal(a, b) and da == db


def test_skipped_locations_and_empty_shapes():
    v, t = R.edge_cases()['border']
    E = R.edge_lengths(2.0, 1.0)
    for index, bg in ((False, 255), (True, R.BG_INDEX)):
        out, _ = R.render(v, t, np.zeros((2, 3)), np.stack([np.zeros(16), R.IDENTITY]), E, 2, (8, 4), index=index)
        assert (out[0] == bg).all() and not (out[1] == bg).all() and out.shape == (2, 2, 4, 8)
        assert (R.render(np.zeros_like(v), t, np.zeros((1, 3)), R.IDENTITY[None], E, 1, (8, 4), index=index)[0] == bg).all()
        assert R.render(v, t, np.zeros((0, 3)), np.zeros((0, 16)), E, 3, (8, 4), index=index)[0].shape == (0, 3, 4, 8)
        assert (R.render(np.zeros((0, 3)), np.zeros((0, 3), np.uint32), np.zeros((1, 3)), R.IDENTITY[None], E, 1, (8, 4), index=index)[0] == bg).all()


# ---- the filter against scipy, bit for bit ---------------------------------------------------------------------------------------------
def scipy_filter(img):
    return scipy.ndimage.gaussian_filter(img, .7)


def test_filter_equals_scipy_on_random_image():
    img = np.random.default_rng(7).integers(0, 256, (128, 256), dtype=np.uint8)
    w = R.gauss_weights()
    assert np.array_equal(R.filter_axis(R.filter_axis(img, 0, w), 1, w), scipy_filter(img))
    assert not np.array_equal(R.filter_axis(R.filter_axis(img, 1, w), 0, w), scipy_filter(img))          # the order of the axes matters
    for shape in ((4, 8), (1, 5), (2, 2), (129, 257)):
        img = np.random.default_rng(8).integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(R.filter_axis(R.filter_axis(img, 0, w), 1, w), scipy_filter(img)), shape


def test_filter_equals_scipy_on_constants():
    w = R.gauss_weights()
    for c in range(256):
        img = np.full((16, 32), c, np.uint8)
        assert np.array_equal(R.filter_axis(R.filter_axis(img, 0, w), 1, w), scipy_filter(img)), c


def test_weights_are_the_package_s():
    from syconn_amd.proc import rendering
    assert np.array_equal(rendering.gauss_weights(), R.gauss_weights()) and len(R.gauss_weights()) == 7
    assert np.array_equal(R.gauss_weights(), R.gauss_weights()[::-1])


# ---- against the golden of the reference's functions -------------------------------------------------------------------------------------
def test_normalisation_equals_meshobject(gold):
    g = gold
    assert np.array_equal(R.normalise(g['m_verts'], g['m_center'], g['m_max_dist']), g['m_vn'])
    assert np.array_equal(R.normalise(g['m_coords'], g['m_center'], g['m_max_dist']), g['m_cn'])
    from syconn_amd.proc.meshes import MeshObject
    mo = MeshObject('raw', g['m_tris'].reshape(-1), g['m_verts'].reshape(-1).copy())
    assert np.array_equal(mo.vert_resh, g['m_vn']) and np.array_equal(mo.center, g['m_center']) and mo.max_dist == g['m_max_dist']
    assert mo.center.dtype == np.float32 and mo.max_dist.dtype == np.float32 and mo.vertices.dtype == np.float32
    assert np.array_equal(mo.transform_external_coords(g['m_coords']), g['m_cn'])
    mo2 = MeshObject('raw', g['m_tris'], g['m_verts'], bounding_box=[g['m_center'] + 1, g['m_max_dist'] * 2])
    assert np.array_equal(mo2.vert_resh, R.normalise(g['m_verts'], g['m_center'] + 1, g['m_max_dist'] * 2))


def sine(a, b):
    return np.linalg.norm(np.cross(a, b), axis=-1)


def test_rotations_restatement_against_golden(gold):
    g = gold
    for key, verts, coords in (('m', g['m_vn'], g['m_cn']), ('r', g['r_verts'], g['r_coords'])):
        rot, empty = R.rot_matrices(coords, verts, g[f'{key}_edge'])
        ref = g[f'{key}_rot']
        assert np.array_equal(empty, g[f'{key}_empty']) and np.array_equal(rot.any(1), ref.any(1))
        a, b = rot.reshape(-1, 4, 4, order='F')[:, :3, :3], ref.reshape(-1, 4, 4, order='F')[:, :3, :3]
        ok = g['r_gap_ok'] if key == 'r' else ref.any(1)
        assert sine(a, b)[ok].max() < 1e-5
        assert np.array_equal(rot[:, 15], ref[:, 15]) and not rot.reshape(-1, 4, 4)[:, 3, :3].any()
    assert g['r_gap_ok'].sum() >= 40
    rows = R.sign_rows([[0.5, -0.5, 0.1], [-0.2, 0.1, 0.2], [0.1, 0.2, -0.9]])
    assert rows[0, 0] > 0 and rows[1, 0] > 0 and rows[1, 2] < 0 and rows[2, 2] > 0      # ties: the lowest index decides


def test_ids_and_vote_against_golden(gold):
    g = gold
    assert np.array_equal(g['i_ids'], np.arange(int(g['i_n']))) and int(g['i_bg'][0]) == R.BG_INDEX
    labels, table = R.vote(g['v_index'], g['v_labels'], int(g['v_bg']), int(g['v_n_verts']), int(g['v_bg_l']) + 1, int(g['v_bg_l']) + 1)
    assert np.array_equal(labels, g['v_vertex_labels']) and np.array_equal(table, g['v_table']) and np.array_equal(labels, g['v_k0'])
    with pytest.raises(IndexError):
        R.vote([0, 300], [0, 0], int(g['v_bg']), 300, 5, 5)


# ---- host-side rules -----------------------------------------------------------------------------------------------------------------
def test_view_angles_and_stride():
    from syconn_amd.proc import meshes, rendering
    assert rendering.view_angles(2).tolist() == [-25.0, 25.0] and rendering.view_angles(3).tolist() == [0.0, 120.0, 240.0]
    assert rendering.view_angles(1).tolist() == [0.0] and np.array_equal(rendering.view_angles(4), R.view_angles(4))
    assert meshes.rot_vertex_stride(100000) == 1 and meshes.rot_vertex_stride(100001) == 8
    assert rendering.BG_INDEX == R.BG_INDEX == 256 ** 4 - 2


def test_config_and_argument_checks():
    from syconn_amd import global_params
    from syconn_amd.proc import rendering
    cfg = global_params.config['views']
    assert cfg['view_properties'] == {'comp_window': 8000, 'ws': [256, 128], 'nb_views': 2} and cfg['subcell_objects'] == ['mi', 'vc', 'sj']
    assert rendering._subcell_objects(None) == ['mi', 'vc', 'syn_ssv'] and cfg['subcell_objects'] == ['mi', 'vc', 'sj']
    assert rendering._window_defaults(None, None, None) == ((256, 128), 2, 8000.0)
    for bad in (dict(ws=(0, 4)), dict(ws=(4, 4, 4)), dict(ws=(9000, 4)), dict(nb_views=0), dict(nb_views=17), dict(comp_window=0),
                dict(comp_window=np.nan), dict(comp_window=[1, 2, 3])):
        kw = dict(ws=(8, 4), nb_views=2, comp_window=100.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            rendering._check_window(**kw)
    for flag in ('clahe', 'wire_frame'):
        with pytest.raises(NotImplementedError):
            rendering.render_mesh_coords(np.zeros((1, 3)), np.zeros(3, np.uint32), np.zeros(9, np.float32), **{flag: True})
    with pytest.raises(NotImplementedError):
        rendering.render_mesh_coords(np.zeros((1, 3)), np.zeros(3, np.uint32), np.zeros(9, np.float32), depth_map=False)


def test_semseg2mesh_argument_checks():
    from syconn_amd.reps import super_segmentation_helper as ssh

    class Cell:
        mesh = [np.zeros(3, np.uint32), np.zeros(9, np.float32), np.zeros(0, np.float32)]
    with pytest.raises(NotImplementedError):
        ssh.semseg2mesh(Cell(), 'spiness', dest_path='x.k.zip', index_views=np.zeros(4, np.uint32), semseg_views=np.zeros(4, np.uint8))
    with pytest.raises(NotImplementedError):
        ssh.semseg2mesh(Cell(), 'spiness')
    with pytest.raises(ValueError, match='Overflow'):
        ssh.semseg2mesh(Cell(), 'spiness', index_views=np.array([0, R.BG_INDEX], np.uint32), semseg_views=np.array([1, 255], np.uint8))
    with pytest.raises(ValueError):
        ssh.semseg2mesh(Cell(), 'spiness', index_views=np.zeros(4, np.uint32), semseg_views=np.zeros(3, np.uint8))
    with pytest.raises(NotImplementedError):
        ssh.semseg2mesh_counter(np.zeros(1, np.uint32), np.zeros(1, np.uint8), 5, np.zeros((3, 2), np.int64))


def test_mesh_table_row_as_cell_mesh():
    from syconn_amd.proc.meshes import MeshTable
    v = np.arange(27, dtype=np.float32).reshape(9, 3)
    t = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 2], [2, 3, 4]], np.uint32)
    table = MeshTable([5, 9], [0, 4, 9], [0, 2, 4], v, t, np.zeros((2, 2, 3), np.float32), np.zeros(2))
    ind, vert, norm = table.mesh_of(9)
    assert np.array_equal(ind, t[2:].reshape(-1)) and np.array_equal(vert, v[4:].reshape(-1)) and len(norm) == 0
    assert all(len(a) == 0 for a in table.mesh_of(7)) and all(len(a) == 0 for a in table.mesh_of(10))
