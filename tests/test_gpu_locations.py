"""GPU: the rendering locations of csrc/sd_locations.hip against the golden (the reference's own ``surface_samples``) and the restatement
(tests/_locations_ref.py), BIT FOR BIT, through the C ABI (guard bands behind every buffer) and through the host layer.  No case is left
out for a tie or a boundary: the stated rule decides every input."""
import os

import numpy as np
import pytest

import _locations_gpu as G
import _locations_ref as R
from syconn_amd import _lib as L

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(HERE, 'golden', 'g28_locations.npz'))


def one(v):
    return np.array([0, len(v)], np.uint64)


def check_table(gpu, rule, begin, verts, **kw):
    want_begin, want = R.sample_table(begin, verts, rule, **kw)
    _, got_begin, got = G.run(gpu, rule, verts, begin, **({'ds': kw['ds']} if rule == 'voxel' else {'bins': kw['bin_sizes'], 'r': kw['r']}))
    assert np.array_equal(got_begin, want_begin)
    assert G.same_bits(got, want)
    return got_begin, got


# ---- the golden ---------------------------------------------------------------------------------------------------------------------
def test_surface_golden_every_cloud_and_as_one_table(gpu, gold):
    from syconn_amd.reps.rep_helper import surface_samples
    n = int(gold['n'])
    for k in range(n):
        v, bins, r, want = gold[f's{k}_verts'], gold[f's{k}_bins'], float(gold[f's{k}_r']), gold[f's{k}_out']
        _, begin, got = G.run(gpu, 'surface', v, one(v), bins=bins, r=r)
        assert begin.tolist() == [0, len(want)] and G.same_bits(got, want), f'cloud {k}'
        assert G.same_bits(surface_samples(v, bins, r=r, device=gpu), want)
        assert G.same_bits(surface_samples(v, bins, max_nb_samples=1, r=r, device=gpu), want)
    # the clouds with the default bins as ONE table: every segment starts at an offset of its own
    ks = [k for k in range(n) if gold[f's{k}_bins'].tolist() == [2000, 2000, 2000] and float(gold[f's{k}_r']) == 1000]
    assert len(ks) >= 2
    verts = np.concatenate([gold[f's{k}_verts'] for k in ks])
    begin = np.concatenate(([0], np.cumsum([len(gold[f's{k}_verts']) for k in ks]))).astype(np.uint64)
    _, got_begin, got = G.run(gpu, 'surface', verts, begin, bins=(2000, 2000, 2000), r=1000)
    assert G.same_bits(got, np.concatenate([gold[f's{k}_out'] for k in ks]))
    assert got_begin.tolist() == np.concatenate(([0], np.cumsum([len(gold[f's{k}_out']) for k in ks]))).tolist()


# ---- the table of odd sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ds', [700.0, 1000.1, 0.25, 1e6])
def test_voxel_table_of_odd_sizes(gpu, ds):
    """0, 1, 2, 63, 64, 65, 129 vertices, empty objects first, in the middle and last, negative coordinates, zero extents; ds = 1000.1 is
    no float32, 0.25 gives one voxel per distinct vertex, 1e6 one voxel per object."""
    begin, verts = G.base_table()
    got_begin, got = check_table(gpu, 'voxel', begin, verts, ds=ds)
    per = np.diff(got_begin.astype(np.int64))
    assert (per[np.array(G.SIZES) == 0] == 0).all() and (per[np.array(G.SIZES) > 0] >= 1).all()
    if ds == 1e6:
        assert per.tolist() == [int(n > 0) for n in G.SIZES]
    if ds == 0.25:
        assert per[7] == len(np.unique(verts[int(begin[7]):int(begin[8])], axis=0)) and per[9] == 1
    check_table(gpu, 'voxel', begin, verts.astype(np.float64) + 0.125, ds=ds)         # float64 vertices


@pytest.mark.parametrize('bins,r', [((2000, 2000, 2000), 1000), ((1500, 700, 2600), 433.5), ((100000, 100000, 100000), 0)])
def test_surface_table_of_odd_sizes(gpu, bins, r):
    begin, verts = G.base_table()
    got_begin, _ = check_table(gpu, 'surface', begin, verts, bin_sizes=bins, r=r)
    per = np.diff(got_begin.astype(np.int64))
    assert (per[np.array(G.SIZES) == 0] == 0).all() and (per[np.array(G.SIZES) > 0] >= 1).all() and per[9] == 1


# ---- voxel rule ---------------------------------------------------------------------------------------------------------------------
def test_voxel_boundary_and_order(gpu):
    v = np.array([[15, 0, 0], [0, 0, 0], [5, 0, 0], [4.5, 0, 0], [14.5, 0, 0]], np.float64)
    _, _, got = G.run(gpu, 'voxel', v, one(v), ds=10)
    assert np.array_equal(got, [[2.25, 0, 0], [9.75, 0, 0], [15, 0, 0]])          # x = 5: p - vmin = 10 = 1 ds, the upper voxel
    v = np.array([[0, 0, 20], [0, 20, 0], [20, 0, 0], [0, 0, 0]], np.float32)
    _, _, got = G.run(gpu, 'voxel', v, one(v), ds=10)
    assert np.array_equal(got, [[0, 0, 0], [0, 0, 20], [0, 20, 0], [20, 0, 0]])


def test_voxel_sum_is_in_vertex_order(gpu):
    rng = np.random.default_rng(1)
    p = rng.uniform(0, 1, (5000, 3)) + 1e6
    want = R.generate_rendering_locs(p, 10.0)
    pair = np.array([np.sum(np.ascontiguousarray(p[:, a])) for a in range(3)]) / 5000.0
    assert len(want) == 1 and not np.array_equal(want[0], pair)                   # the teeth: a pairwise sum is another number
    _, _, got = G.run(gpu, 'voxel', p, one(p), ds=10.0)
    assert G.same_bits(got, want)


def test_voxel_extent_limit(gpu):
    from syconn_amd.handler.multiviews import generate_rendering_locs
    v = np.array([[0, 0, 0], [0, L.SD_LOCATIONS_MAX_CELLS - 1, 0]], np.float64)
    _, _, got = G.run(gpu, 'voxel', v, one(v), ds=1.0)                              # one below the limit: voxel 2^21 - 1
    assert np.array_equal(got, v) and G.same_bits(got, R.generate_rendering_locs(v, 1.0))
    v[1, 1] = L.SD_LOCATIONS_MAX_CELLS
    rc, c, _, _ = G.call(gpu, 'voxel', v, one(v), ds=1.0)
    assert rc == L.SD_OK and c[4] != 0
    with pytest.raises(ValueError, match='voxels'):
        generate_rendering_locs(v, 1.0, device=gpu)
    with pytest.raises(ValueError):
        R.generate_rendering_locs(v, 1.0)


# ---- surface rule -------------------------------------------------------------------------------------------------------------------
def edge_cloud(mx, bs, j):
    """Vertices on a line along x with extent `mx`: 0, mx, the interior float32 edge j of numpy's histogram and its float32
    neighbour below."""
    nb = max(1, int(np.ceil(F(mx) / F(bs))))
    step = F(F(mx) / F(nb))
    e = F(F(j) * step)
    x = np.array([0, mx, e, np.nextafter(e, F(0))], F)
    return np.stack([x, np.zeros(4, F), np.zeros(4, F)], 1), nb


@pytest.mark.parametrize('mx,bs,j,nb', [(3000, 1000, 1, 3), (6500, 1000, 3, 7), (7000.5, 1000, 5, 8), (1900, 1000, 1, 2), (900, 1000, 0, 1)])
def test_surface_histogram_edges(gpu, mx, bs, j, nb):
    """c == mx goes to the last bin, a vertex equal to an interior float32 edge to the upper bin, its float32 neighbour below to the
    lower one; nb of 1, 2, 3, 7, 8."""
    v, n = edge_cloud(mx, bs, j)
    assert n == nb
    c = v - v.min(0)
    bins = R.surface_bins(c, c.max(0), np.array([nb, 1, 1]))[:, 0]
    if nb > 1:
        assert bins.tolist() == [0, nb - 1, j, j - 1]
    _, occupied, _, _, got_nb = R.surface_samples(v, (bs, bs, bs), r=10, return_parts=True)
    assert got_nb.tolist() == [nb, 1, 1] and len(occupied) == len(np.unique(bins))
    check_table(gpu, 'surface', one(v), v, bin_sizes=(bs, bs, bs), r=10)
    check_table(gpu, 'surface', one(v), v + F(12345.5), bin_sizes=(bs, bs, bs), r=10)


def test_surface_two_bins_pick_the_same_vertex(gpu):
    v = np.array([[0, 0, 50000], [600, 450, 50000], [1001, 0, 0]], F)
    bins = (1000, 1000, 100000)
    want, occupied, nearest, _, _ = R.surface_samples(v, bins, r=100, return_parts=True)
    assert occupied.tolist() == [[0, 0, 0], [1, 0, 0]] and nearest.tolist() == [1, 1]    # both are kept
    assert np.array_equal(want, [v[1], v[1]])
    check_table(gpu, 'surface', one(v), v, bin_sizes=bins, r=100)


def test_surface_tie_for_the_nearest_vertex_takes_the_lowest_index(gpu):
    # both vertices are as far from the only centre (500, 500, 500): index 0 wins, whichever way a spatial order would put them
    for v in (np.array([[1000, 0, 0], [0, 0, 0]], F), np.array([[0, 0, 0], [1000, 0, 0]], F)):
        want = R.surface_samples(v, (1000, 1000, 1000), r=100)
        assert np.array_equal(want, v[:1])
        check_table(gpu, 'surface', one(v), v, bin_sizes=(1000, 1000, 1000), r=100)
    # the same across tiles: 200 vertices, the two nearest ones at rows 70 and 150
    v = np.zeros((200, 3), F)
    v[:, 0] = 3000
    v[0, 0], v[150, 0], v[70, 0] = 0, 400, 600
    want, _, nearest, _, _ = R.surface_samples(v, (1000, 1000, 1000), r=10, return_parts=True)
    assert nearest[0] == 70
    check_table(gpu, 'surface', one(v), v, bin_sizes=(1000, 1000, 1000), r=10)


def test_surface_ball_is_inclusive(gpu):
    # the only bin's centre is the vertex (1000, 1000, 1000) itself; (600, 800, 0) further is at exactly d == r, half a unit more is outside
    p = np.array([1000, 1000, 1000], F)
    v = np.stack([p, p + F([600, 800, 0]), p + F([600, 800.5, 0]), np.zeros(3, F)])
    want, _, nearest, sizes, nb = R.surface_samples(v, (2000, 2000, 2000), r=1000, return_parts=True)
    assert nb.tolist() == [1, 1, 1] and nearest.tolist() == [0] and sizes.tolist() == [2]
    assert np.array_equal(want, [(v[0] + v[1]) / F(2)])
    check_table(gpu, 'surface', one(v), v, bin_sizes=(2000, 2000, 2000), r=1000)


def test_surface_sum_is_in_vertex_order_in_float32(gpu):
    rng = np.random.default_rng(2)
    v = rng.uniform(0, 50, (5000, 3)).astype(F)
    v[0] = 0                                                                       # the minimum: the last addition does not hide the sum
    want, _, _, sizes, _ = R.surface_samples(v, r=100, return_parts=True)
    assert sizes.tolist() == [5000]
    c = (v - v.min(0)).astype(F)
    pair = (np.array([np.sum(np.ascontiguousarray(c[:, a])) for a in range(3)]) / F(5000) + v.min(0)).astype(F)
    wide = (c.astype(np.float64).sum(0) / 5000).astype(F) + v.min(0)
    assert (want[0] != pair).all() and (want[0] != wide).all()                    # the teeth
    check_table(gpu, 'surface', one(v), v, bin_sizes=(2000, 2000, 2000), r=100)


# ---- capacities, scratch, arguments, flags --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rule', ['voxel', 'surface'])
def test_capacity_and_scratch_one_short(gpu, rule):
    begin, verts = G.base_table()
    kw = dict(ds=700.0) if rule == 'voxel' else dict(bins=(2000, 2000, 2000), r=1000)
    c, want_begin, want = G.run(gpu, rule, verts, begin, **kw)
    n = int(c[0])
    rc, c, got_begin, got = G.call(gpu, rule, verts, begin, cap=n - 1, **kw)         # the guard behind the output stays intact
    assert rc == L.SD_OK and c[1] != 0 and int(c[0]) == n and np.array_equal(got_begin, want_begin)
    assert G.same_bits(got, want[:n - 1])
    rc, _, _, _ = G.call(gpu, rule, verts, begin, cap=n, shrink=1, **kw)
    assert rc == L.SD_ERR_INVALID and b'temp_bytes' in L.load().sd_last_error()
    rc, _, _, _ = G.call(gpu, rule, verts, begin, cap=n, null_scratch=True, **kw)
    assert rc == L.SD_ERR_INVALID


def test_argument_errors_and_device_flags(gpu):
    begin, verts = G.base_table()
    for ds in (0.0, -1.0, np.nan, np.inf):
        assert G.call(gpu, 'voxel', verts, begin, ds=ds)[0] == L.SD_ERR_INVALID
    for kw in (dict(bins=(0, 1, 1), r=1), dict(bins=(1, np.inf, 1), r=1), dict(bins=(1, 1, 1), r=-1), dict(bins=(1, 1, 1), r=np.nan)):
        assert G.call(gpu, 'surface', verts, begin, **kw)[0] == L.SD_ERR_INVALID
    for rule, kw in (('voxel', dict(ds=1.0)), ('surface', dict(bins=(1, 1, 1), r=1))):
        assert G.call(gpu, rule, verts, begin, n_verts=2 ** 31, **kw)[0] == L.SD_ERR_INVALID
        assert G.call(gpu, rule, verts, begin, n_obj=2 ** 31, **kw)[0] == L.SD_ERR_INVALID
        rc, c, b, _ = G.call(gpu, rule, verts[:0], np.zeros(1, np.uint64), **kw)     # no objects
        assert rc == L.SD_OK and not c.any() and b.tolist() == [0]
        rc, c, b, _ = G.call(gpu, rule, verts[:0], np.zeros(4, np.uint64), **kw)     # objects without any vertex
        assert rc == L.SD_OK and not c.any() and b.tolist() == [0, 0, 0, 0]
        bad = begin.copy()
        bad[3], bad[4] = bad[4], bad[3] + 1                                        # descending offsets
        rc, c, _, _ = G.call(gpu, rule, verts, bad, **kw)
        assert rc == L.SD_OK and c[7] != 0
        short = begin.copy()
        short[-1] -= 1                                                             # does not end at n_verts
        assert G.call(gpu, rule, verts, short, **kw)[1][7] != 0
        for wild in (np.nan, np.inf, -np.inf):
            w = verts.copy()
            w[100, 1] = wild
            rc, c, _, _ = G.call(gpu, rule, w, begin, **kw)
            assert rc == L.SD_OK and c[5] != 0
    far = np.array([[0, 0, 0], [3e6, 0, 0]], F)                                    # 3e6 bins of size 1 along x
    assert G.call(gpu, 'surface', far, one(far), bins=(1, 1, 1), r=1)[1][4] != 0


def test_host_layer_raises_on_device_flags(gpu):
    import torch
    from syconn_amd.proc.locations import sample_locations_table
    from syconn_amd.reps.rep_helper import surface_samples
    far = np.array([[0, 0, 0], [3e6, 0, 0]], F)
    with pytest.raises(ValueError, match='bins'):
        surface_samples(far, (1, 1, 1), r=1, device=gpu)
    w = torch.zeros((4, 3), dtype=torch.float32, device=gpu)
    w[1, 2] = float('nan')                                                         # a device tensor: only the device can see it
    for new in (True, False):
        with pytest.raises(ValueError, match='NaN'):
            sample_locations_table((np.arange(1), [0, 4], w), use_new_renderings_locs=new, device=gpu)


# ---- the host layer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('new', [True, False])
def test_sample_locations_table_against_the_dropins(gpu, new):
    import torch
    from syconn_amd.handler.multiviews import generate_rendering_locs
    from syconn_amd.proc.locations import sample_locations_table
    from syconn_amd.reps.rep_helper import surface_samples
    begin, verts = G.base_table()
    n = len(G.SIZES)
    ids = np.arange(n, dtype=np.uint64) * 3 + 5
    rep = np.arange(3 * n).reshape(n, 3) + 17
    scaling = np.array([10., 10., 20.])
    ds = 1500
    t = sample_locations_table((ids, begin, verts), ds, use_new_renderings_locs=new, rep_coords=rep, scaling=scaling, device=gpu)
    assert t.locations.dtype == F and np.array_equal(t.ids, ids) and len(t) == n
    d = t.as_dict()
    b = begin.astype(np.int64)
    for k in range(n):
        v = verts[b[k]:b[k + 1]]
        want = R.sample_locations(v, rep[k], scaling, ds, new)
        assert G.same_bits(d[int(ids[k])], want), k
        if len(v):
            drop = generate_rendering_locs(v, ds, device=gpu).astype(F) if new else surface_samples(v, [ds] * 3, r=ds / 2, device=gpu).astype(F)
            assert G.same_bits(drop, want)
        else:
            assert G.same_bits(want, (np.array([rep[k]], F) * scaling).astype(F))
    pick = ids[[10, 3, 0, 3]]
    loc, lb = t.locations_of(pick)
    assert G.same_bits(loc, np.concatenate([d[int(i)] for i in pick])) and lb.tolist() == np.concatenate(([0], np.cumsum([len(d[int(i)]) for i in pick]))).tolist()
    # the tensors stay on the device; default ds_factor and the configuration's rule
    td = sample_locations_table((ids, begin, torch.from_numpy(verts).to(gpu)), ds, use_new_renderings_locs=new, rep_coords=rep, scaling=scaling,
                                device=gpu, return_device=True)
    assert td.on_device and td.locations.is_cuda and td.loc_begin.is_cuda
    assert G.same_bits(td.locations.cpu().numpy(), t.locations) and np.array_equal(td.loc_begin.cpu().numpy(), t.loc_begin.astype(np.int64))
    keep = np.array(G.SIZES) > 0
    full = sample_locations_table((ids[keep], np.concatenate(([0], np.cumsum(np.array(G.SIZES)[keep]))), verts), device=gpu)
    want = np.concatenate([R.sample_locations(verts[b[k]:b[k + 1]], None, None) for k in np.flatnonzero(keep)])
    assert G.same_bits(full.locations, want)


def test_sample_locations_sso_and_mesh_table(gpu):
    from syconn_amd.proc.locations import sample_locations_table
    from syconn_amd.proc.meshes import MeshTable
    from syconn_amd.reps.super_segmentation_helper import sample_locations_sso
    begin, verts = G.base_table()
    b = begin.astype(np.int64)

    class Sv:
        def __init__(self, k):
            self.mesh = [np.zeros(0, np.uint32), verts[b[k]:b[k + 1]].reshape(-1), np.zeros(0, F)]
            self.rep_coord, self.scaling = np.array([k, 2 * k, 3 * k + 1]), np.array([10, 10, 20], F)

    class Cell:
        svs = [Sv(k) for k in range(len(G.SIZES))]

    got = sample_locations_sso(Cell(), device=gpu)
    assert len(got) == len(G.SIZES)
    for sv, g in zip(Cell.svs, got):
        assert G.same_bits(g, R.sample_locations(sv.mesh[1], sv.rep_coord, sv.scaling))
    got = sample_locations_sso(Cell(), ds_factor=900, device=gpu)
    for sv, g in zip(Cell.svs, got):
        assert G.same_bits(g, R.sample_locations(sv.mesh[1], sv.rep_coord, sv.scaling, 900))
    n = len(G.SIZES)
    mt = MeshTable(np.arange(1, n + 1), begin, np.zeros(n + 1, np.uint64), verts, np.zeros((0, 3), np.uint32), np.zeros((n, 2, 3), F), np.zeros(n))
    t = sample_locations_table(mt, 900, rep_coords=np.array([sv.rep_coord for sv in Cell.svs]), scaling=(10, 10, 20), device=gpu)
    assert G.same_bits(t.locations, np.concatenate(got))


# ---- end to end: labels -> meshes -> locations -> views -------------------------------------------------------------------------------
def test_labels_to_meshes_to_locations_to_views(gpu):
    from syconn_amd.proc.locations import sample_locations_table
    from syconn_amd.proc.meshes import find_meshes_table
    from syconn_amd.proc.rendering import render_sampled_views, render_views_table
    x, y, z = np.meshgrid(np.arange(64), np.arange(48), np.arange(32), indexing='ij')
    vol = np.zeros((64, 48, 32), np.uint64)
    vol[((x - 20) / 14.) ** 2 + ((y - 24) / 10.) ** 2 + ((z - 16) / 9.) ** 2 < 1] = 3
    vol[(abs(x - 50) < 8) & (abs(y - 20) < 12) & (abs(z - 14) < 6)] = 8
    vol[60:62, 40:42, 28:30] = 11
    scaling = (10., 10., 20.)
    meshes = find_meshes_table(vol, (0, 0, 0), pad=1, scaling=scaling, device=gpu)
    assert meshes.ids.tolist() == [3, 8, 11]
    kw = dict(ws=(64, 32), nb_views=2, comp_window=400.0)
    for new in (True, False):
        t = sample_locations_table(meshes, 120, use_new_renderings_locs=new, device=gpu)
        want_begin, want = [0], []
        for k in range(3):
            want.append(R.sample_locations(meshes.vertices[int(meshes.vert_begin[k]):int(meshes.vert_begin[k + 1])], None, None, 120, new))
            want_begin.append(want_begin[-1] + len(want[-1]))
        assert t.loc_begin.tolist() == want_begin and len(t.locations) == want_begin[-1] >= 3
        assert G.same_bits(t.locations, np.concatenate(want))
        for k, i in enumerate(meshes.ids):
            m = meshes.mesh_of(i)
            views, rot = render_views_table([(m[0], m[1])], t.as_dict()[int(i)], device=gpu, **kw)
            ref_views, ref_rot = render_views_table([(m[0], m[1])], want[k], device=gpu, **kw)
            assert views.shape == (len(want[k]), 1, 2, 32, 64) and np.array_equal(views, ref_views) and np.array_equal(rot, ref_rot)
            if k == 0:
                assert (views != 255).any()

    class Sv:
        def __init__(self, i):
            self.mesh, self.rep_coord, self.scaling = meshes.mesh_of(i), (0, 0, 0), scaling

    class Cell:
        svs = [Sv(3)]
        mesh = meshes.mesh_of(3)

        def load_mesh(self, name):
            return [np.zeros(0, np.uint32), np.zeros(0, F), np.zeros(0, F)]

    views, locs = render_sampled_views(Cell(), 120, return_locations=True, add_cellobjects=False, device=gpu, **kw)
    want = R.sample_locations(meshes.mesh_of(3)[1], None, None, 120)
    assert G.same_bits(locs, want) and views.shape == (len(want), 1, 2, 32, 64)
    assert np.array_equal(views[:, 0], render_views_table([(Cell.mesh[0], Cell.mesh[1])], want, device=gpu, **kw)[0][:, 0])
    iv = render_sampled_views(Cell(), 120, index_views=True, device=gpu, **kw)
    assert iv.dtype == np.uint32 and iv.shape == (len(want), 1, 2, 32, 64)
