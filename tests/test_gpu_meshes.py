"""GPU: csrc/sd_mesh.hip through the C ABI (tests/_mesh_gpu.py: every output and the scratch exactly as large as asked for, each followed
by a guard band) and through the host layer (syconn_amd/proc/meshes.py, proc/sd_proc.py mesh_objects), against the golden of the
reference's own functions (tests/golden/g25_meshes.npz) and the numpy restatement (tests/_mesh_ref.py).  Vertices, indices, mesh_bb, ids
and offsets bit for bit; the area within n_tri * 2^-52 relative (positive terms, two summation orders)."""
import os

import numpy as np
import pytest

import _mesh_gpu as D
import _mesh_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g25_meshes.npz')
U = np.uint64
SCALING = np.array([10., 10., 20.])
SD_OK, SD_ERR_INVALID = 0, -1


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_table(got, want):
    """`got`: a dict of the C ABI helper or a MeshTable; `want`: the restatement's dict."""
    g = got if isinstance(got, dict) else {k: getattr(got, k) for k in want}
    for k in ('ids', 'vert_begin', 'tri_begin', 'vertices', 'indices', 'mesh_bb'):
        assert same_bits(g[k], want[k]), k
    n_tri = np.diff(want['tri_begin'].astype(np.int64))
    assert g['mesh_area'].shape == want['mesh_area'].shape
    assert (np.abs(g['mesh_area'] - want['mesh_area']) <= n_tri * 2.0 ** -52 * want['mesh_area']).all()


def scale_offset(offset, pad, ds, scaling=SCALING):
    s_ds = scaling * (np.asarray(ds, np.float64) if ds is not None else 1.0)
    return s_ds, np.asarray(offset, np.float64) * scaling - (pad * s_ds if pad > 0 else 0.0)


def run_abi(gpu, vol, offset=(0, 0, 0), pad=0, ds=None, ids=None):
    vol = np.ascontiguousarray(vol, U)
    if ids is None:
        ids = np.unique(vol)
        ids = ids[ids != 0]
    tabs = D.source_tables(vol.shape, pad, ds)
    s_ds, off = scale_offset(offset, pad, ds)
    rc, c, out = D.build(gpu, vol, tabs, ids, s_ds, off)
    assert rc == SD_OK and not c[2:].any() and c[0] == len(out['vertices']) and c[1] == len(out['indices']), c
    return out


def run_host(gpu, vol, offset=(0, 0, 0), pad=0, ds=None):
    from syconn_amd.proc.meshes import find_meshes_table
    return find_meshes_table(np.ascontiguousarray(vol, U), offset, pad=pad, ds=ds, scaling=SCALING, device=gpu)


def both(gpu, vol, offset=(0, 0, 0), pad=0, ds=None):
    """The C ABI and the host layer against the restatement; -> the restatement's dict."""
    want = R.find_meshes_table(vol, offset, pad=pad, ds=ds, scaling=SCALING)
    assert_table(run_abi(gpu, vol, offset, pad, ds), want)
    assert_table(run_host(gpu, vol, offset, pad, ds), want)
    return want


def obj(t, k):
    vb, tb = t['vert_begin'].astype(np.int64), t['tri_begin'].astype(np.int64)
    return t['vertices'][vb[k]:vb[k + 1]], t['indices'][tb[k]:tb[k + 1]]


# ---- the golden ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', ['a', 'b'])
def test_golden_chunks_and_merge(gpu, gold, r):
    from syconn_amd.proc.meshes import MeshTable, find_meshes, find_meshes_table
    tables = []
    for c in range(3):
        chunk = np.ascontiguousarray(gold['vol'][8 * c:8 * c + 8])
        offset = gold['origin'] + (8 * c, 0, 0)
        out = run_abi(gpu, chunk, offset, 1, gold[f'{r}_ds'])
        assert same_bits(out['ids'], gold[f'{r}{c}_ids'])
        assert same_bits(out['vertices'].reshape(-1), gold[f'{r}{c}_vert']) and same_bits(out['indices'].reshape(-1), gold[f'{r}{c}_ind'])
        assert np.array_equal(out['vert_begin'].astype(np.int64) * 3, gold[f'{r}{c}_vert_begin'])
        assert np.array_equal(out['tri_begin'].astype(np.int64) * 3, gold[f'{r}{c}_ind_begin'])
        d = find_meshes(chunk, offset, pad=1, ds=gold[f'{r}_ds'], scaling=gold['scaling'],
                        meshing_props=dict(normals=False, simplification_factor=50, max_simplification_error=40), device=gpu)
        assert [U(i) for i in d] == list(gold[f'{r}{c}_ids'])
        ib, vb = gold[f'{r}{c}_ind_begin'], gold[f'{r}{c}_vert_begin']
        for k, i in enumerate(d):
            assert same_bits(d[i][0], gold[f'{r}{c}_ind'][ib[k]:ib[k + 1]]) and same_bits(d[i][1], gold[f'{r}{c}_vert'][vb[k]:vb[k + 1]])
            assert d[i][2].dtype == np.float32 and d[i][2].shape == (0,)
        tables.append(find_meshes_table(chunk, offset, pad=1, ds=gold[f'{r}_ds'], scaling=gold['scaling'], device=gpu))
    want = dict(ids=gold[f'{r}_ids'], vert_begin=(gold[f'{r}_vert_begin'] // 3).astype(U), tri_begin=(gold[f'{r}_ind_begin'] // 3).astype(U),
                vertices=gold[f'{r}_vert'].reshape(-1, 3), indices=gold[f'{r}_ind'].reshape(-1, 3), mesh_bb=gold[f'{r}_bb'], mesh_area=gold[f'{r}_area'])
    assert_table(MeshTable.merge(tables, device=gpu), want)
    cat = lambda k: np.concatenate([getattr(t, k) for t in tables])
    v0 = np.cumsum([0] + [len(t.vertices) for t in tables]).astype(U)
    t0 = np.cumsum([0] + [len(t.indices) for t in tables]).astype(U)
    vb = np.concatenate([t.vert_begin[:-1] + v0[k] for k, t in enumerate(tables)] + [v0[-1:]])
    tb = np.concatenate([t.tri_begin[:-1] + t0[k] for k, t in enumerate(tables)] + [t0[-1:]])
    rc, c, out = D.merge(gpu, cat('ids'), vb, tb, cat('vertices'), cat('indices'))
    assert rc == SD_OK and c[0] == len(want['ids']) and not c[1:].any()
    assert_table(out, want)


# ---- shapes --------------------------------------------------------------------------------------------------------------------------
def test_eight_labels_in_one_cube(gpu):
    vol = np.array([3, 2 ** 63 + 5, 7, 11, 13, 2 ** 64 - 1, 19, 23], U).reshape(2, 2, 2)
    for pad in (0, 1):
        want = both(gpu, vol, pad=pad)
        assert len(want['ids']) == 8 and (np.diff(want['tri_begin'].astype(np.int64)) >= 1).all()
    want = R.find_meshes_table(vol, (0, 0, 0), pad=0, scaling=SCALING)
    assert np.diff(want['tri_begin'].astype(np.int64)).tolist() == [1] * 8 and np.diff(want['vert_begin'].astype(np.int64)).tolist() == [3] * 8


@pytest.mark.parametrize('density', [0.2, 0.5, 0.8])
def test_noise_is_closed_and_canonical(gpu, density):
    rng = np.random.default_rng(int(density * 100))
    labels = np.array([4, 9, 2 ** 33 + 1, 2 ** 63 + 2, 77], U)
    vol = np.zeros((17, 13, 9), U)
    vol[1:-1, 1:-1, 1:-1] = np.where(rng.random((15, 11, 7)) < density, labels[rng.integers(0, 5, (15, 11, 7))], U(0))   # no object touches a face
    want = both(gpu, vol, offset=(3, 5, 7))
    got = run_abi(gpu, vol, (3, 5, 7))
    for k, i in enumerate(got['ids']):
        v, t = obj(got, k)
        assert R.edge_balance(t)[0], f'object {i} is not closed'
        keys = R.vertex_keys(vol == i)
        pos = (np.maximum(R.key_positions(keys, vol.shape) * SCALING + np.array([3., 5, 7]) * SCALING, 0)).astype(np.float32)
        assert same_bits(v, pos)
    full = np.where(rng.random(vol.shape) < density, labels[rng.integers(0, 5, vol.shape)], U(0))     # objects on every face, padded
    both(gpu, full, offset=(1, 0, 2), pad=1)


def test_ball_and_box(gpu):
    g = np.indices((15, 15, 15)) - 7
    vol = np.zeros((22, 15, 15), U)
    vol[:15][(g ** 2).sum(0) <= 25] = 6
    vol[16:20, 1:4, 1:3] = 8
    from syconn_amd.proc.meshes import find_meshes_table
    t = find_meshes_table(vol, (0, 0, 0), scaling=(1, 1, 1), device=gpu)
    assert_table(t, R.find_meshes_table(vol, (0, 0, 0), scaling=(1., 1., 1.)))
    d = t.as_dict()
    for i, (nv, nt, volume) in {6: (486, 968, 503.25), 8: (52, 100, 20 + 1 / 6)}.items():
        ind, vert = d[i][0].reshape(-1, 3), d[i][1].reshape(-1, 3)
        assert (len(vert), len(ind)) == (nv, nt) and abs(R.signed_volume(vert, ind) - volume) < 1e-9
        assert R.euler(nv, ind) == 2 and R.edge_balance(ind) == (True, True)


def test_object_through_the_chunk_face_is_open_and_clamped(gpu):
    vol = np.zeros((6, 7, 5), U)
    vol[0:3, 2:5, 1:4] = 5                                  # reaches the face x = 0: the pad replicates it to x = -1
    vol[4, 4, 2] = 9
    want = both(gpu, vol, pad=1)
    v, t = obj(want, 0)
    assert not R.edge_balance(t)[0] and v[:, 0].min() == 0 and (v >= 0).all()
    assert R.edge_balance(obj(want, 1)[1]) == (True, True)
    tabs = D.source_tables(vol.shape, 1, None)
    assert tabs[0].tolist() == [0, 0, 1, 2, 3, 4, 5, 5]


def test_object_only_in_the_replicated_plane(gpu):
    vol = np.zeros((5, 6, 4), U)
    vol[4, 1:4, 1:3] = 12                                   # one voxel thick, on the face x = 4
    want = both(gpu, vol, offset=(2, 2, 2), pad=1)
    assert len(want['vertices']) and not R.edge_balance(want['indices'])[0]
    both(gpu, vol, offset=(2, 2, 2), pad=0)


def test_ds_that_removes_an_object_keeps_its_empty_entry(gpu):
    from syconn_amd.proc.meshes import find_meshes
    vol = np.zeros((8, 8, 6), U)
    vol[2:6, 2:6, 1:4] = 3
    vol[3, 7, 5] = 21
    assert 21 not in R.padded_volume(vol, 0, (2, 2, 1))
    want = both(gpu, vol, offset=(1, 1, 1), pad=1, ds=(2, 2, 1))
    assert want['ids'].tolist() == [3, 21] and want['vert_begin'][2] == want['vert_begin'][1] and want['mesh_area'][1] == 0
    d = find_meshes(vol, (1, 1, 1), pad=1, ds=(2, 2, 1), scaling=SCALING, device=gpu)
    assert list(d) == [3, 21] and [a.shape for a in d[21]] == [(0,), (0,), (0,)] and d[21][0].dtype == np.uint32 and d[21][1].dtype == np.float32


def test_non_cubic_ds(gpu):
    rng = np.random.default_rng(8)
    from scipy import ndimage
    lab, _ = ndimage.label(ndimage.gaussian_filter(rng.random((33, 31, 18)), 1.2) > 0.52)
    vol = lab.astype(U) * U(1000003)
    want = both(gpu, vol, offset=(64, 0, 32), pad=1, ds=(4, 4, 2))
    assert len(want['ids']) > 3 and len(want['vertices']) > 50


def test_volume_without_labels(gpu):
    from syconn_amd.proc.meshes import find_meshes, find_meshes_table
    vol = np.zeros((5, 4, 3), U)
    assert find_meshes(vol, (0, 0, 0), pad=1, scaling=SCALING, device=gpu) == {} and len(find_meshes_table(vol, (0, 0, 0), scaling=SCALING, device=gpu)) == 0
    tabs = D.source_tables(vol.shape, 1, None)
    rc, c, out = D.build(gpu, vol, tabs, np.zeros(0, U), SCALING, np.zeros(3))
    assert rc == SD_OK and not c.any() and out['vert_begin'].tolist() == [0] and out['tri_begin'].tolist() == [0]
    one = np.full((4, 4, 4), 7, U)                          # one label everywhere: no edge crosses without the pad's help either
    want = both(gpu, one, pad=1)
    assert want['ids'].tolist() == [7] and len(want['vertices']) == 0


def test_two_runs_have_identical_bytes(gpu):
    rng = np.random.default_rng(3)
    vol = np.where(rng.random((17, 13, 9)) < 0.5, rng.integers(1, 6, (17, 13, 9)), 0).astype(U)
    a, b = run_abi(gpu, vol, (1, 2, 3), 1, (2, 1, 1)), run_abi(gpu, vol, (1, 2, 3), 1, (2, 1, 1))
    for k in a:
        assert same_bits(a[k], b[k]), k


# ---- flags and argument checks ------------------------------------------------------------------------------------------------------------
def test_device_flags(gpu):
    vol = np.zeros((6, 6, 6), U)
    vol[1:4, 1:4, 1:4] = 5
    vol[4, 4, 4] = 8
    tabs = D.source_tables(vol.shape, 1, None)
    s, o = scale_offset((0, 0, 0), 1, None)
    rc, c = D.count(gpu, vol, tabs, [5])                                         # 8 is in the volume but not in ids
    assert rc == SD_OK and c[6] == 1 and c[7] == 0
    rc, c = D.count(gpu, vol, tabs, [8, 5])                                      # ids do not ascend
    assert rc == SD_OK and c[7] == 1
    bad = [t.copy() for t in tabs]
    bad[1][3] = 6                                                                # beyond the source extent: read as label 0, flagged
    rc, c = D.count(gpu, vol, bad, [5, 8])
    assert rc == SD_OK and c[7] == 1
    rc, c = D.count(gpu, vol, tabs, [5, 8])
    assert rc == SD_OK and not c[2:].any()
    nv, nt = int(c[0]), int(c[1])
    for vert_cap, tri_cap in ((nv - 1, nt), (nv, nt - 1), (0, 0), (3, 2)):       # too small: flagged, nothing behind the outputs (guard bands)
        rc, c, _ = D.build(gpu, vol, tabs, [5, 8], s, o, vert_cap=vert_cap, tri_cap=tri_cap)
        assert rc == SD_OK and c[2] == 1 and (c[0], c[1]) == (nv, nt)
    rc, c, out = D.build(gpu, vol, tabs, [5, 8], s, o, vert_cap=nv + 5, tri_cap=nt + 7)      # larger than needed: the same tables
    assert rc == SD_OK and not c[2:].any()
    want = R.find_meshes_table(vol, (0, 0, 0), pad=1, scaling=SCALING)
    out['vertices'], out['indices'] = out['vertices'][:nv], out['indices'][:nt]
    assert_table(out, want)
    minus = [t.copy() for t in tabs]
    minus[2][0] = -1                                                             # scipy's constant: that plane reads as label 0
    rc, c = D.count(gpu, vol, minus, [5, 8])
    assert rc == SD_OK and not c[2:].any()


def test_argument_errors(gpu):
    from syconn_amd import _lib as L
    lib = L.load()
    vol = np.zeros((4, 4, 4), U)
    vol[1, 1, 1] = 2
    tabs = D.source_tables(vol.shape, 0, None)
    s, o = scale_offset((0, 0, 0), 0, None)
    rc, _, _ = D.build(gpu, vol, tabs, [2], s, o, shrink=1)
    assert rc == SD_ERR_INVALID and b'sd_mesh_build_temp_bytes' in lib.sd_last_error()
    rc, _, _ = D.build(gpu, vol, tabs, [2], (10, 0, 20), o)
    assert rc == SD_ERR_INVALID
    assert lib.sd_mesh_build_temp_bytes(4, 4, 4, 2 ** 31, 1) == 0 and lib.sd_mesh_build_temp_bytes(2048, 2048, 513, 1, 1) == 0
    assert lib.sd_mesh_build_temp_bytes(2048, 2048, 512, 1, 1) > 0 and lib.sd_mesh_merge_temp_bytes(2 ** 31) == 0
    big = [np.zeros(n, np.int32) for n in (2048, 2048, 513)]                     # more than 2^31 padded voxels: refused before any launch
    rc, _ = D.count(gpu, vol, big, [2])
    assert rc == SD_ERR_INVALID and b'2^31' in lib.sd_last_error()
    import torch
    cnt = torch.zeros(8, dtype=torch.int64, device=gpu)
    assert lib.sd_mesh_count(None, 4, 4, 4, None, None, None, 4, 4, 4, None, 0, cnt.data_ptr(), 0) == SD_ERR_INVALID
    assert lib.sd_mesh_count(None, 4, 4, 4, None, None, None, 4, 4, 4, None, 0, None, 0) == SD_ERR_INVALID
    assert lib.sd_mesh_merge(None, None, None, 1, None, 0, None, 0, None, cnt.data_ptr(), cnt.data_ptr(), None, None, None, None, cnt.data_ptr(), None, 0, 0) == SD_ERR_INVALID
    rc, c, _ = D.merge(gpu, [4, 4], [0, 2, 1], [0, 0, 0], np.zeros((1, 3)), np.zeros((0, 3)))       # offsets that do not ascend to the total
    assert rc == SD_OK and c[7] == 1
    rc, _, _ = D.merge(gpu, [4, 4], [0, 0, 0], [0, 0, 0], np.zeros((0, 3)), np.zeros((0, 3)), shrink=1)
    assert rc == SD_ERR_INVALID
    from syconn_amd.proc.meshes import find_meshes
    with pytest.raises(ValueError):
        find_meshes(vol, (0, 0, 0), pad=2, scaling=SCALING, device=gpu)
    with pytest.raises(NotImplementedError):
        find_meshes(vol, (0, 0, 0), scaling=SCALING, meshing_props={'normals': True}, device=gpu)


# ---- the consumers -----------------------------------------------------------------------------------------------------------------------
def test_vertices_feed_the_organelle_table(gpu, gold):
    from syconn_amd.extraction.cs_processing_steps import OrganelleTable
    from syconn_amd.proc.meshes import find_meshes_table
    t = find_meshes_table(gold['vol'], gold['origin'], pad=1, ds=(2, 2, 1), scaling=gold['scaling'], device=gpu)
    ids = t.ids[::-1].copy()
    verts, begin = t.vertices_of(ids)
    table = OrganelleTable(ids, np.zeros(len(ids)), np.ones(len(ids)), np.zeros((len(ids), 3)), verts, begin)
    assert table.vertices is not None and same_bits(table.vertices, verts) and same_bits(table.vert_begin, begin)
    d = t.as_dict()
    for k, i in enumerate(ids):
        assert same_bits(table.vertices[begin[k]:begin[k + 1]].reshape(-1), d[int(i)][1])


def test_mesh_objects_merges_in_chunk_order(gpu, gold):
    import torch
    import syconn_amd.proc.sd_proc as sp
    from syconn_amd import global_params
    from syconn_amd.proc import meshes as M

    class KD:
        boundary = np.array([24, 10, 9])
    vol = gold['vol']
    dvol = torch.from_numpy(vol.view(np.int64)).to(gpu)
    seen = []

    def loader(name, off, size):
        seen.append((name, tuple(int(v) for v in off)))
        return dvol[off[0]:off[0] + size[0], off[1]:off[1] + size[1], off[2]:off[2] + size[2]].contiguous()
    orig = sp.kd_factory
    sp.kd_factory = lambda p: KD()
    try:
        out = sp.mesh_objects('', {'sj': ''}, chunk_size=(8, 10, 9), device=gpu, chunk_loader=loader, generate_sv_mesh=True, scaling=gold['scaling'])
    finally:
        sp.kd_factory = orig
    assert sorted(out) == ['sj', 'sv'] and len(seen) == 6
    for kind in ('sj', 'sv'):
        ds = global_params.config['meshes']['downsampling'][kind]
        parts = [R.find_meshes_table(np.ascontiguousarray(vol[8 * c:8 * c + 8]), (8 * c, 0, 0), pad=1, ds=ds, scaling=gold['scaling']) for c in range(3)]
        got = out[kind].as_dict()
        assert [U(i) for i in got] == list(np.unique(vol)[1:])
        for i in got:
            pieces = [obj(p, list(p['ids']).index(i)) for p in parts if i in p['ids']]
            ind, vert = M.merge_meshes([t.reshape(-1) for _, t in pieces], [v.reshape(-1) for v, _ in pieces])
            assert same_bits(got[i][0], ind) and same_bits(got[i][1], vert)
