"""CPU: every input of tests/_views_edge_cases.py sits on the structure edge of csrc/sd_views.hip that it claims, shown with the numpy
restatement (tests/_views_ref.py) alone -- an input that stops exercising its branch fails here, without a device."""
import os

import numpy as np
import pytest
import scipy.ndimage

import _views_edge_cases as EC
import _views_ref as R
from syconn_amd import _lib as L

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g27_views.npz')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def tiles_of(img, tile):
    """-> {(tx, ty): the part of img [H, W] in that tile}."""
    H, W = img.shape
    return {(tx, ty): img[ty * tile[1]:(ty + 1) * tile[1], tx * tile[0]:(tx + 1) * tile[0]]
            for ty in range(-(-H // tile[1])) for tx in range(-(-W // tile[0]))}


# ---- 1. the tiled all-zero rule -----------------------------------------------------------------------------------------------------------
def test_tiled_windows_have_the_tiles_the_cases_assume():
    W, H = EC.TILED_WS
    assert W * H > L.SD_VIEWS_TILE_PX                                               # more than one depth tile, so also more than one index tile
    assert len(tiles_of(np.zeros((H, W)), EC.DEPTH_TILE)) == 4 and len(tiles_of(np.zeros((H, W)), EC.INDEX_TILE)) == 6
    assert 32 * 16 <= L.SD_VIEWS_TILE_PX // 2                                       # the small window is one tile in both modes


def test_all_zero_and_corner_nonzero():
    c = EC.cases('zero_rule')
    raw, _, dropped = c['all_zero'].raw()
    assert (raw == 0).all() and dropped == 0
    out, dropped = c['all_zero'].ref(False)
    assert (out == 255).all() and dropped == 0                                      # every tile is all zero: k_vw_zero_rule writes the whole view
    out, dropped = c['corner_nonzero'].ref(False)
    img = out[0, 0]
    rows, cols = np.nonzero(img)
    assert dropped == 0 and sorted(set(rows)) == list(range(123, 129)) and sorted(set(cols)) == list(range(251, 257))
    assert (img == 0).sum() == 33120 and img.size == 33153
    t = tiles_of(img, EC.DEPTH_TILE)
    assert t[1, 1].any() and not t[0, 0].any() and not t[1, 0].any() and not t[0, 1].any()       # three tiles that a rule per tile would turn to 255


@pytest.mark.parametrize('name,nv', [('three_locations', 1), ('three_locations_two_views', 2)])
def test_three_locations_in_one_call(name, nv):
    c = EC.cases('zero_rule')
    out, dropped = c[name].ref(False)
    assert out.shape == (3, nv, 129, 257) and dropped == 0
    assert (c[name].raw(0)[0] == 0).all() and (out[0] == 255).all()                 # all zero before the rule
    for m in range(nv):
        assert np.array_equal(out[1, m], c['corner_nonzero'].ref(False)[0][0, 0])   # mostly zero, and it stays so
    assert (out[2] == 255).all() and not c[name].rot[2].any()                       # skipped


# ---- 2. the bounds, exactly ---------------------------------------------------------------------------------------------------------------
def test_snap_bound_exact():
    c = EC.cases('bound')
    assert float(np.float32(R.px_x(16384.0))) == 1023.0 and float(np.float32(R.px_x(16384.0 - 1.0 / 256))) == 1022.999755859375
    for name, xs_far in (('at_bound', R.SNAP_LIM), ('below_bound', R.SNAP_LIM - 1)):
        X = (float(c[name].v[5, 0]) / 2.0 + 0.5) * 32.0
        assert int(np.floor(X * 256.0 + 0.5)) == xs_far
    ix, dropped = c['at_bound'].ref(True)
    assert dropped == 1 and (ix != R.BG_INDEX).sum() == 36 and set(np.unique(ix)) == {2, 3, R.BG_INDEX}
    ix, dropped = c['below_bound'].ref(True)
    assert dropped == 0 and (ix != R.BG_INDEX).all() and ix.size == 512 and (ix == 6).sum() >= 512 - 36      # at equal depth triangle 1 beats 2
    assert c['at_bound'].ref(False)[1] == 1 and c['below_bound'].ref(False)[1] == 0


def test_snap_bound_counted_once_per_view():
    case = EC.cases('bound')['at_bound_tiled']
    n_lv = len(case.coords) * case.nb_views
    per_view = [case.raw(n, m)[2] for n in range(len(case.coords)) for m in range(case.nb_views)]
    assert per_view == [1] * n_lv                                                   # every angle meets the window
    for index in (False, True):
        assert case.ref(index)[1] == n_lv >= 2                                      # 4 or 6 tiles per view: a count per tile gives another number
    ix = case.ref(True)[0]
    assert set(np.unique(ix)) <= {2, 3, R.BG_INDEX} and (ix != R.BG_INDEX).any()


def test_depth_cut_off_exact():
    c = EC.cases('bound')
    assert float(c['last_depth'].v[0, 2]) == -1.0 + 2.0 ** -22 and float(c['past_last_depth'].v[0, 2]) == -1.0 + 2.0 ** -23
    for name, D in (('last_depth', 2 ** 24 - 2), ('past_last_depth', 2 ** 24 - 1)):
        Zf = 0.5 - float(c[name].v[0, 2]) / 2.0
        assert np.floor(Zf * 16777216.0) == D
    ix, _ = c['last_depth'].ref(True)
    assert (ix != R.BG_INDEX).sum() == 36 and (c['last_depth'].ref(False)[0] == 255).all()
    assert (c['past_last_depth'].ref(True)[0] == R.BG_INDEX).all() and (c['past_last_depth'].ref(False)[0] == 255).all()


# ---- 3. lane or wave ----------------------------------------------------------------------------------------------------------------------
def test_pixel_boxes_of_64_and_65():
    c = EC.cases('split')
    assert c['box_64'].pixel_boxes().tolist() == [EC.NARROW_MAX, EC.NARROW_MAX]
    assert c['box_65'].pixel_boxes().tolist() == [EC.NARROW_MAX + 1, EC.NARROW_MAX + 1]
    for name, n in (('box_64', 64), ('box_65', 65)):
        ix, dropped = c[name].ref(True)
        assert dropped == 0 and (ix != R.BG_INDEX).sum() == n and set(np.unique(ix)) == {2, 3, R.BG_INDEX}      # both triangles draw
        assert (c[name].raw()[0] != 255).sum() == n and len(np.unique(c[name].raw()[0])) > 4                 # the depth differs per pixel


# ---- 4. seams under large triangles -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', EC.NAMES['seam'])
def test_seams_have_drawn_pixels_on_both_sides(name):
    case = EC.cases('seam')[name]
    raw, t, dropped = case.raw()
    drawn = t >= 0
    assert dropped == 0 and (case.pixel_boxes() > EC.NARROW_MAX).all()              # drawn by the whole wave
    first, second = sorted(set(np.unique(t)) - {-1})
    assert (first, second) == ((0, 2) if name == 'coplanar' else (0, 1))            # coplanar: the lower-numbered triangle of each pair wins
    for col in EC.SEAM_COLS:
        for tri in (first, second):
            assert (t[:, col - 1] == tri).any() and (t[:, col] == tri).any(), (col, tri)
    for row in EC.SEAM_ROWS:
        for tri in (first, second):
            assert (t[row - 1] == tri).any() and (t[row] == tri).any(), (row, tri)
    x0, y0, x1, y1 = EC.SEAM_QUAD
    want = np.zeros_like(drawn)
    want[int(y0 + 0.5):int(y1 + 0.5), int(x0 + 0.5):int(x1 + 0.5)] = True           # a square owns its bottom and right edges; clipped by the window
    assert np.array_equal(drawn, want)                                              # every sample once: the diagonal through pixel centres has no gap
    diag = [(int(y0 + k), int(x0 + EC.SEAM_STEP * k)) for k in range(1, 67)]        # samples exactly on the shared diagonal, down to the last row
    assert diag[-1][0] == case.ws[1] - 1
    assert all(drawn[r, c] for r, c in diag) and len({t[r, c] for r, c in diag}) == 1
    assert len(np.unique(raw[drawn])) > 16                                          # the depth differs per vertex
    ix, _ = case.ref(True)
    assert set(np.unique(ix)) == ({2, 7, R.BG_INDEX} if name == 'coplanar' else {int(case.t[0, 2]), 3, R.BG_INDEX})


# ---- 5. more candidates than a block has threads ------------------------------------------------------------------------------------------
def test_lattice_on_the_reference():
    v, t = EC.lattice_mesh()
    assert len(t) == 9216 and len(v) == 2 * 49 * 49
    radius = 0.5 * np.linalg.norm(R.edge_lengths(R.EDGE_CW, 1.0))
    assert radius == 1.5
    n1 = (EC.LATTICE_K + 1) ** 2
    for ws in EC.LATTICE_WS:
        case = EC.lattice_case(ws)
        for cn in case.coords:                                                      # a lower bound of the candidate list (test_candidate_capacity: a superset)
            assert (np.linalg.norm(v[t.astype(np.int64)].astype(np.float64) - cn, axis=2) <= radius).any(1).sum() > 1024
        ix, dropped = case.ref(True)
        assert dropped == 0 and case.ref(False)[1] == 0
        drawn = ix != R.BG_INDEX
        share = (ix[drawn] < n1).mean()
        assert drawn.mean() > 0.9 and 0.3 < share < 0.5                             # both sheets win pixels
        assert len(np.unique(case.ref(False)[0])) > 50                              # not flat
    W, H = EC.LATTICE_WS[1]
    assert 32 * 16 <= 4096 < W * H <= L.SD_VIEWS_TILE_PX // 2                       # one tile in both modes, 256 and 1024 threads


# ---- 6. windows narrower than the filter --------------------------------------------------------------------------------------------------
def test_tiny_windows_on_the_reference():
    for ws in EC.TINY_WS:
        out, dropped = EC.tiny_case('near_plane', ws).ref(False)
        n = len(np.unique(out))
        assert dropped == 0 and out.shape == (1, 1, ws[1], ws[0])
        assert (n == 1) if ws == (1, 1) else (2 <= n <= 21), (ws, n)                 # the filter has something to fold
        for name in EC.TINY_NAMES:
            for index in (False, True):
                a = R.render(*R.edge_cases()[name], np.zeros((1, 3)), R.IDENTITY[None], R.edge_lengths(R.EDGE_CW, 1.0), 1, ws, index=index, dense=False)
                b = EC.tiny_case(name, ws).ref(index)
                assert np.array_equal(a[0], b[0]) and a[1] == b[1]                  # the two restatements agree
    assert any((EC.tiny_case('pixel_centres', ws).ref(True)[0] != R.BG_INDEX).any() for ws in EC.TINY_WS)


def test_depth_filter_equals_scipy_on_narrow_images():
    rng = np.random.default_rng(23)
    for shape in ((1, 5), (2, 7), (3, 3), (5, 1), (1, 1)):
        for img in (rng.integers(0, 256, shape, dtype=np.uint8), np.zeros(shape, np.uint8), rng.integers(0, 2, shape, dtype=np.uint8)):
            want = scipy.ndimage.gaussian_filter(img, .7)
            if want.sum() == 0:
                want = np.full_like(want, 255)
            assert np.array_equal(R.depth_filter(img), want), shape


# ---- 7. view counts -----------------------------------------------------------------------------------------------------------------------
def test_sixteen_views_differ(gold):
    assert L.SD_VIEWS_MAX_VIEWS == 16
    for index in (False, True):
        out, dropped = EC.tube_ref(gold, 16, index)
        assert dropped == 0 and out.shape == (2, 16, 16, 32)
        for n in range(2):
            assert len(np.unique(out[n].reshape(16, -1), axis=0)) == 16
        two, dropped = EC.tube_ref(gold, 2, index)
        assert dropped == 0 and not np.array_equal(two[:, 0], two[:, 1]) and not np.array_equal(two[:, 0], out[:, 0])      # +/- 25 degrees, not 0 and 180
    assert R.view_angles(2).tolist() == [-25.0, 25.0]


# ---- 8. rotations past one stride ---------------------------------------------------------------------------------------------------------
def test_rotation_inputs_pass_one_stride(gold):
    g = gold
    assert len(g['r_coords']) == 52 and len(g['r_verts']) == 11006
    assert L.SD_VIEWS_GRID * 4 + 105 > L.SD_VIEWS_GRID * 4                          # k_vw_rot_solve: 4 waves per block
    n_fill = 255000
    assert n_fill < L.SD_VIEWS_GRID * 256 < n_fill + len(g['r_verts'])              # the cloud straddles the end of the first stride
    for fill in (50.0, -50.0):                                                      # the largest Morton code and code 0: behind and in front of the cloud
        filler = np.full((1, 3), fill, np.float32)
        assert not any(R.in_bounding_box(filler, c, g['r_edge'])[0] for c in g['r_coords'])              # the filler is no inlier anywhere
        assert (np.abs(g['r_verts']) < 50).all() and ((fill + 1.0) * 512.0 >= 1023.0 or (fill + 1.0) * 512.0 <= 0.0)
    assert len(g['m_vn']) == 1024 and 1021 % 8 != 0 and len(g['m_vn'][:1021][::8]) == -(-1021 // 8)
