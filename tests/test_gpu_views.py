"""GPU: csrc/sd_views.hip through the C ABI (tests/_views_gpu.py: every output and scratch followed by a guard band) and through the host
layer (proc/rendering.py, proc/meshes.py, reps/super_segmentation_helper.py) -- depth and index views against the numpy restatement of the
raster rule (tests/_views_ref.py) bit for bit, rotations against the golden of the reference's own functions (tests/golden/g27_views.npz)
up to sign within the bound derived below, the vote against the golden bit for bit."""
import os

import numpy as np
import pytest

import _views_gpu as G
import _views_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g27_views.npz')
SD_OK, SD_ERR_INVALID = 0, -1
# |v_dev x v_ref| on clouds whose eigenvalue gaps are >= 0.05 of the largest eigenvalue: the float32 centring perturbs the covariance
# by at most 2 x 2^-24 relative; divided by the gap that is 2.4e-6; a factor 4 covers the solver and three axes
ROT_BOUND = 1e-5


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope='module')
def tube(gpu, gold):
    g = gold
    return G.Mesh(gpu, g['m_verts'], g['m_tris'], g['m_center'], g['m_max_dist'])


_ref_cache = {}


def tube_ref(gold, ws, nb_views, n_loc, index):
    """The restatement's views of the tube, computed once per shape and never changed."""
    key = (ws, nb_views, n_loc, index)
    if key not in _ref_cache:
        g = gold
        out, dropped = R.render(g['m_vn'], g['m_tris'], g['m_cn'][:n_loc], g['m_rot'][:n_loc], R.edge_lengths(float(g['m_comp_window']), g['m_max_dist']),
                                nb_views, ws, index=index)
        out.setflags(write=False)
        _ref_cache[key] = (out, dropped)
    return _ref_cache[key]


# ---- depth and index views of the tube ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ws,nb_views,n_loc', [((32, 16), 1, 1), ((32, 16), 3, 3), ((32, 16), 3, 40), ((256, 128), 1, 3), ((256, 128), 3, 1),
                                               ((257, 129), 3, 1), ((257, 129), 1, 3)])
@pytest.mark.parametrize('index', [False, True])
def test_tube_views(gold, tube, ws, nb_views, n_loc, index):
    g = gold
    want, dropped = tube_ref(g, ws, nb_views, n_loc, index)
    rc, c, got = tube.render(g['m_coords'][:n_loc], g['m_rot'][:n_loc], float(g['m_comp_window']), nb_views, ws, index=index)
    assert rc == SD_OK and c[2] == dropped == 0 and c[3] == 0
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), f'{(got != want).sum()} of {got.size} pixels differ'
    bg = R.BG_INDEX if index else 255
    assert (want != bg).any()                                                      # the case draws something
    if n_loc == 40:
        assert (got[-1] == bg).all()                                               # the last location has a zero matrix


# ---- rule edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(R.edge_cases()))
@pytest.mark.parametrize('index', [False, True])
def test_rule_edges(gpu, name, index):
    v, t = R.edge_cases()[name]
    m = G.Mesh(gpu, v, t, np.zeros(3), 1.0)
    assert m.rc == SD_OK and not m.counts.any()
    coords, rot = np.zeros((1, 3), np.float32), R.IDENTITY[None]
    want, dropped = R.render(v, t, coords, rot, R.edge_lengths(R.EDGE_CW, 1.0), 1, R.EDGE_WS, index=index)
    rc, c, got = m.render(coords, rot, R.EDGE_CW, 1, R.EDGE_WS, index=index)
    assert rc == SD_OK and c[2] == dropped and c[3] == 0
    assert np.array_equal(got, want)
    if name == 'beyond_bound':
        assert dropped == 1
    if name == 'huge':
        assert (got != (R.BG_INDEX if index else 255)).all()                       # the widening by the largest half extent found it
    if name == 'd_zero' and not index:
        assert (got == 255).all()


def test_skipped_and_empty(gpu):
    v, t = R.edge_cases()['border']
    E = R.edge_lengths(2.0, 1.0)
    for index, bg in ((False, 255), (True, R.BG_INDEX)):
        m = G.Mesh(gpu, v, t, np.zeros(3), 1.0)
        rot = np.stack([np.zeros(16), R.IDENTITY, np.zeros(16)])
        rc, c, got = m.render(np.zeros((3, 3)), rot, 2.0, 2, (8, 4), index=index)
        want, _ = R.render(v, t, np.zeros((3, 3)), rot, E, 2, (8, 4), index=index)
        assert rc == SD_OK and np.array_equal(got, want) and (got[0] == bg).all() and (got[2] == bg).all() and not (got[1] == bg).all()
        rc, c, got = m.render(np.zeros((0, 3)), np.zeros((0, 16)), 2.0, 3, (8, 4), index=index)     # zero locations
        assert rc == SD_OK and got.shape == (0, 3, 4, 8)
        z = G.Mesh(gpu, np.zeros_like(v), t, np.zeros(3), 1.0)                      # all normalised vertices zero
        rc, c, got = z.render(np.zeros((1, 3)), R.IDENTITY[None], 2.0, 1, (8, 4), index=index)
        assert rc == SD_OK and (got == bg).all()
        e = G.Mesh(gpu, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(3), 1.0)       # an empty mesh
        rc, c, got = e.render(np.zeros((2, 3)), np.stack([R.IDENTITY] * 2), 2.0, 1, (8, 4), index=index)
        assert e.rc == SD_OK and rc == SD_OK and (got == bg).all()
    bad = G.Mesh(gpu, v, np.array([[0, 1, 9]], np.uint32), np.zeros(3), 1.0)        # a vertex number outside the mesh
    assert bad.rc == SD_OK and bad.counts[3] == 1


# ---- rotations -------------------------------------------------------------------------------------------------------------------------
def sine(a, b):
    return np.linalg.norm(np.cross(a, b), axis=-1)


def rows_of(rot):
    return rot.reshape(-1, 4, 4, order='F')[:, :3, :3]


def test_rotations_against_golden(gpu, gold):
    g = gold
    worst = 0.0
    for key, verts, coords in (('m', g['m_vn'], g['m_cn']), ('r', g['r_verts'], g['r_coords'])):
        rc, c, rot, empty = G.rotations(gpu, verts, coords, g[f'{key}_edge'])
        ref = g[f'{key}_rot']
        assert rc == SD_OK and not c.any()
        assert np.array_equal(empty, g[f'{key}_empty'])                             # flag_empty_spaces, exactly
        assert np.array_equal(rot.any(1), ref.any(1))                               # <= 2 inliers: 16 zeros
        nz = ref.any(1)
        assert (rot[nz, 15] == 1).all() and not rot.reshape(-1, 4, 4)[:, 3, :3].any() and not rot.reshape(-1, 4, 4)[:, :3, 3].any()
        ok = g['r_gap_ok'] if key == 'r' else nz
        s = sine(rows_of(rot), rows_of(ref))[ok]
        worst = max(worst, float(s.max()))
        print(f'rotations {key}: largest |v_dev x v_ref| = {s.max():.3e} over {int(ok.sum())} clouds')
        assert s.max() <= ROT_BOUND
        a = rows_of(rot)[nz]                                                        # the sign convention and orthonormal rows
        big = np.take_along_axis(a, np.abs(a).argmax(2)[..., None], 2)
        assert (big > 0).all() and np.abs(a @ a.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12
        mine, _ = R.rot_matrices(coords, verts, g[f'{key}_edge'])
        assert np.abs(rows_of(rot) - rows_of(mine))[ok].max() <= ROT_BOUND          # against the restatement, sign included
        rc, c, none, empty2 = G.rotations(gpu, verts, coords, g[f'{key}_edge'], flag_only=True)
        assert rc == SD_OK and none is None and np.array_equal(empty2, g[f'{key}_empty'])
    assert g['r_n_in'][48:51].tolist() == [0, 2, 3] and g['r_n_in'][51] == 60      # 0 / 2 / 3 inliers and the points on the box faces


def test_rotations_raw_vertices_and_stride(gpu, gold):
    """Raw vertices with the normalisation applied by the kernel equal normalised input; the stride takes every 8th vertex."""
    g = gold
    rc, c, rot, empty = G.rotations(gpu, g['m_verts'], g['m_coords'], g['m_edge'], g['m_center'], g['m_max_dist'])
    rc2, c2, rot2, empty2 = G.rotations(gpu, g['m_vn'], g['m_cn'], g['m_edge'])
    assert rc == rc2 == SD_OK and np.array_equal(rot, rot2) and np.array_equal(empty, empty2)
    rc, c, rot8, _ = G.rotations(gpu, g['m_vn'], g['m_cn'], g['m_edge'], stride=8)
    rc2, c2, sub, _ = G.rotations(gpu, g['m_vn'][::8], g['m_cn'], g['m_edge'])
    assert rc == rc2 == SD_OK and np.array_equal(rot8, sub) and not np.array_equal(rot8, rot2)
    rc, c, rot0, empty0 = G.rotations(gpu, np.zeros((0, 3)), g['m_cn'][:3], g['m_edge'])                # no vertices
    assert rc == SD_OK and not rot0.any() and empty0.all()


def test_rotation_dropins(gpu, gold):
    from syconn_amd.proc import meshes
    g = gold
    rot = meshes.calc_rot_matrices(g['r_coords'], g['r_verts'], g['r_edge'], device=gpu)
    rc, c, want, empty = G.rotations(gpu, g['r_verts'], g['r_coords'], g['r_edge'])
    assert rot.shape == (len(g['r_coords']), 16) and rot.dtype == np.float64 and np.array_equal(rot, want)
    flags = meshes.flag_empty_spaces(g['r_coords'], g['r_verts'], g['r_edge'], device=gpu)
    assert flags.dtype == bool and np.array_equal(flags, g['r_empty'])
    assert meshes.calc_rot_matrices(np.zeros((0, 3)), g['r_verts'], g['r_edge'], device=gpu).shape == (0, 16)


# ---- the vote --------------------------------------------------------------------------------------------------------------------------
def test_vote_against_golden(gpu, gold):
    from syconn_amd.reps import super_segmentation_helper as ssh
    g = gold
    n, nl = int(g['v_n_verts']), int(g['v_bg_l']) + 1
    rc, c, labels, table = G.vote(gpu, g['v_index'], g['v_labels'], int(g['v_bg']), n, nl, nl)
    assert rc == SD_OK and c[3] == 0 and c[4] == 0 and c[0] == (g['v_table'].sum(1) != 0).sum()
    assert np.array_equal(table, g['v_table']) and np.array_equal(labels, g['v_vertex_labels'])
    assert table[0, 1] == 255 and table[1, 1] == 0 and table[2, 2] == 1 and labels[1] == nl and labels[3] == 1      # 255 / 256 / 257 hits, the tie
    rc, c, labels2, none = G.vote(gpu, g['v_index'], g['v_labels'], int(g['v_bg']), n, nl, nl, table=False)
    assert rc == SD_OK and none is None and np.array_equal(labels2, labels)
    rc, c, only_bg, _ = G.vote(gpu, np.full(100, g['v_bg']), np.full(100, 4), int(g['v_bg']), 7, nl, nl)          # only background
    assert rc == SD_OK and (only_bg == nl).all() and c[0] == 0
    rc, c, _, _ = G.vote(gpu, [1, n, 2], [0, 0, 0], int(g['v_bg']), n, nl, nl)                                     # a bad index
    assert rc == SD_OK and c[3] == 1
    count = ssh.semseg2mesh_counter(g['v_index'], g['v_labels'], int(g['v_bg']), np.zeros((n, nl), np.uint8), device=gpu)
    assert count.dtype == np.uint8 and np.array_equal(count, g['v_table'])
    with pytest.raises(IndexError):
        ssh.semseg2mesh_counter(np.array([1, n], np.uint32), np.zeros(2, np.uint8), int(g['v_bg']), np.zeros((n, nl), np.uint8), device=gpu)


class Cell:
    """What the host layer reads of a cell: ``mesh`` and ``load_mesh(name)``."""

    def __init__(self, mesh, organelles=None):
        self.mesh, self.organelles, self.nb_cpus, self.id = mesh, organelles or {}, 1, 1

    def load_mesh(self, name):
        return self.organelles.get(name, [np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.float32)])


def test_semseg2mesh_against_golden(gpu, gold):
    from syconn_amd.reps import super_segmentation_helper as ssh
    g = gold
    cell = Cell([np.zeros(0, np.uint32), g['v_verts'].reshape(-1), np.zeros(0, np.float32)])
    for k, key in ((0, 'v_k0'), (1, 'v_k1')):
        ind, vert, norm, col = ssh.semseg2mesh(cell, 'spiness', k=k, index_views=g['v_index'], semseg_views=g['v_labels'], device=gpu)
        assert np.array_equal(col, g[key]) and vert is cell.mesh[1]
    colors = np.arange(24).reshape(6, 4)
    col = ssh.semseg2mesh(cell, 'spiness', k=0, colors=colors, index_views=g['v_index'], semseg_views=g['v_labels'], device=gpu)[3]
    assert col.dtype == np.uint8 and np.array_equal(col, colors[g['v_k0']])
    with pytest.raises(IndexError):
        ssh.semseg2mesh(cell, 'spiness', k=0, index_views=np.array([0, 300, g['v_bg']], np.uint32), semseg_views=np.array([0, 1, 4], np.uint8), device=gpu)
    with pytest.raises(ValueError, match='Overflow'):
        ssh.semseg2mesh(cell, 'spiness', k=0, index_views=np.array([0, g['v_bg']], np.uint32), semseg_views=np.array([0, 255], np.uint8), device=gpu)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cell(gold):
    g = gold
    verts, tris = g['m_verts'], g['m_tris']
    mi = R.bent_tube(12, 8, 120.0, 2500.0, 300.0, offset=verts[200].astype(np.float64) + [0, 40, 0])
    vc = R.bent_tube(10, 6, 80.0, 1500.0, 100.0, offset=verts[500].astype(np.float64) - [0, 30, 10])
    flat = lambda m: [m[1].reshape(-1), m[0].reshape(-1), np.zeros(0, np.float32)]
    return Cell([tris.reshape(-1), verts.reshape(-1), np.zeros(0, np.float32)], {'mi': flat(mi), 'vc': flat(vc)})


def test_render_sso_coords(gpu, gold, cell):
    from syconn_amd.proc import rendering
    g = gold
    coords = g['m_verts'][[200, 500]] + np.float32(25)                              # next to the two organelles
    views, rot = rendering.render_sso_coords(cell, coords, return_rot_mat=True, device=gpu)
    assert views.shape == (2, 4, 2, 128, 256) and views.dtype == np.uint8 and rot.shape == (2, 16)
    assert (views[:, 3] == 255).all()                                               # 'syn_ssv' is missing: a channel of 255
    assert (views[:, 0] != 255).any() and (views[:, 1] != 255).any()
    E = R.edge_lengths(8000.0, g['m_max_dist'])
    want, _ = R.render(g['m_vn'], g['m_tris'], R.normalise(coords, g['m_center'], g['m_max_dist']), rot, E, 2, (256, 128))
    assert np.array_equal(views[:, 0], want)
    mo = G.Mesh(gpu, cell.organelles['mi'][1], cell.organelles['mi'][0])            # an organelle has its own normalisation
    want_mi, _ = R.render(mo.vn, mo.tris, mo.cn(coords), rot, mo.E(8000.0), 2, (256, 128))
    assert np.array_equal(views[:, 1], want_mi)
    again = rendering.render_sso_coords(cell, coords, rot_mat=rot, device=gpu)      # rot_mat is accepted
    assert np.array_equal(again, views)
    only = rendering.render_sso_coords(cell, coords, cellobjects_only=True, ws=(32, 16), nb_views=3, device=gpu)
    full = rendering.render_sso_coords(cell, coords, ws=(32, 16), nb_views=3, device=gpu)
    assert only.shape == (2, 3, 3, 16, 32) and np.array_equal(only, full[:, 1:])
    empty = rendering.render_sso_coords(cell, np.zeros((0, 3)), ws=(32, 16), device=gpu)
    assert empty.shape == (0, 4, 2, 16, 32)
    raw = rendering.render_mesh_coords(coords, cell.mesh[0], cell.mesh[1], ws=(32, 16), rot_matrices=rot, device=gpu)
    assert np.array_equal(raw, rendering.render_sso_coords(cell, coords, add_cellobjects=False, ws=(32, 16), rot_mat=rot, device=gpu)[:, 0])


def test_index_views_to_vertex_labels(gpu, gold, cell):
    from syconn_amd.proc import rendering
    from syconn_amd.reps import super_segmentation_helper as ssh
    g = gold
    coords = g['m_coords'][[3, 12, 20, 31]]
    ix, rot = rendering.render_sso_coords_index_views(cell, coords, ws=(64, 32), nb_views=3, return_rot_matrices=True, device=gpu)
    assert ix.shape == (4, 1, 3, 32, 64) and ix.dtype == np.uint32
    want, _ = R.render(g['m_vn'], g['m_tris'], g['m_cn'][[3, 12, 20, 31]], rot, R.edge_lengths(8000.0, g['m_max_dist']), 3, (64, 32), index=True)
    assert np.array_equal(ix[:, 0], want) and (ix == R.BG_INDEX).any() and (ix != R.BG_INDEX).any()
    n_verts = len(g['m_verts'])
    label_of = (np.arange(n_verts) // 16 % 3).astype(np.uint8)                      # a known function of the vertex: the ring it is on
    semseg = np.where(ix == R.BG_INDEX, 3, label_of[np.minimum(ix, n_verts - 1)]).astype(np.uint8)
    seen = np.zeros(n_verts, bool)
    seen[ix[ix != R.BG_INDEX]] = True
    k0 = ssh.semseg2mesh(cell, 'spiness', k=0, index_views=ix, semseg_views=semseg, device=gpu)[3]
    assert np.array_equal(k0[seen], label_of[seen]) and (k0[~seen] == 4).all() and 0 < seen.sum() < n_verts
    want0, _ = R.vote(ix, semseg, R.BG_INDEX, n_verts, 4, 4)
    assert np.array_equal(k0, want0)
    k1 = ssh.semseg2mesh(cell, 'spiness', k=1, index_views=ix, semseg_views=semseg, device=gpu)[3]
    assert np.array_equal(k1[seen], label_of[seen]) and k1.max() <= 2 and len(k1) == n_verts
    import scipy.spatial
    verts = g['m_verts'].astype(np.float64)
    near = scipy.spatial.cKDTree(verts[seen]).query(verts, k=1)[1]
    d_near = np.linalg.norm(verts - verts[seen][near], axis=1)
    d_all = np.sort(scipy.spatial.distance.cdist(verts[~seen], verts[seen]), axis=1)[:, :2] if (~seen).any() else np.zeros((0, 2))
    unique = np.ones(n_verts, bool)
    unique[~seen] = d_all[:, 0] < d_all[:, 1]                                       # where the nearest predicted vertex is not tied
    assert np.array_equal(k1[unique], label_of[seen][near][unique]) and d_near[seen].max() == 0


# ---- capacities ----------------------------------------------------------------------------------------------------------------------
def test_candidate_capacity(gpu, gold, tube):
    g = gold
    E = tube.E(float(g['m_comp_window']))
    rc, c, begin, cand, _, _ = tube.candidates(g['m_coords'], E)
    total = int(c[0])
    assert rc == SD_OK and c[1] == 0 and begin[0] == 0 and begin[-1] == total == len(cand) and (np.diff(begin.astype(np.int64)) >= 0).all()
    assert begin[-1] == begin[-2]                                                   # the far location sees nothing
    # a superset of what any view needs: every triangle with a vertex inside the sphere around the location
    vn, cn = g['m_vn'].astype(np.float64), g['m_cn'].astype(np.float64)
    radius = 0.5 * np.linalg.norm(E)
    for n in (0, 7, 38):
        mine = set(cand[int(begin[n]):int(begin[n + 1])].tolist())
        assert len(mine) == int(begin[n + 1] - begin[n])                            # no triangle twice
        need = np.flatnonzero((np.linalg.norm(vn[g['m_tris'].astype(np.int64)] - cn[n], axis=2) <= radius).any(1))
        assert set(need.tolist()) <= mine
    rc, c2, begin2, short, _, _ = tube.candidates(g['m_coords'], E, cap=total - 1)  # one short: the flag, and nothing past the capacity
    assert rc == SD_OK and c2[1] == 1 and c2[0] == total and np.array_equal(short, cand[:total - 1]) and np.array_equal(begin2, begin)
    rc, c3, begin3, _, _, _ = tube.candidates(g['m_coords'], E, cap=0)               # the sizing call
    assert rc == SD_OK and c3[0] == total and c3[1] == 0 and np.array_equal(begin3, begin)


def test_bad_arguments(gpu, gold, tube):
    from syconn_amd import _lib as L
    lib = L.load()
    g = gold
    assert lib.sd_views_render_temp_bytes(3, 2) >= 24 and lib.sd_views_vote_temp_bytes(10, 5) >= 200
    rc, c, _ = tube.render(g['m_coords'][:1], g['m_rot'][:1], 8000.0, 1, (8, 4), cos_sin=(np.array([2.0]), np.array([0.0])))
    assert rc == SD_ERR_INVALID and b'cos' in lib.sd_last_error()
    rc, c, _ = tube.render(g['m_coords'][:1], g['m_rot'][:1], 8000.0, 1, (8, 4), E=np.array([1.0, 0.0, 1.0]),
                           cand=tube.candidates(g['m_coords'][:1], tube.E(8000.0)))
    assert rc == SD_ERR_INVALID
    rc, c, _, _ = G.rotations(gpu, g['m_vn'], g['m_cn'], g['m_edge'], max_dist=0.0)
    assert rc == SD_ERR_INVALID
    rc, c, _, _ = G.vote(gpu, [0], [0], 5, 4, 300, 1)
    assert rc == SD_ERR_INVALID
