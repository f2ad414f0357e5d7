"""CPU: the marching-cubes table (the committed header against the rule, the rule's numbers), the restatement of the device contract
against the golden of the reference's own ``find_meshes`` (tests/golden/g25_meshes.npz), the source-index tables against scipy's zoom
and numpy's pad, the numpy drop-ins and ``mesh_props`` against the golden bit for bit, the argument checks of the host layer, and the
project's usual error without a device."""
import os
import re

import numpy as np
import pytest

import _mesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'g25_meshes.npz')
U = np.uint64


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def header_table():
    src = open(os.path.join(ROOT, 'syconn_amd', 'csrc', 'sd_mc_table.h')).read()
    body = lambda name: src[src.index(name):].split('= {', 1)[1].split('};', 1)[0]
    count = [int(v) for v in re.findall(r'\d+', body('SD_MC_COUNT[256]'))]
    edges = [[int(v) for v in re.findall(r'\d+', row)] for row in re.findall(r'\{([^{}]*)\}', body('SD_MC_EDGES[256][15]'))]
    return count, edges


def test_committed_header_equals_the_rule_entry_for_entry():
    count, edges = header_table()
    assert len(count) == 256 and len(edges) == 256 and all(len(r) == 15 for r in edges)
    for mask, tris in enumerate(R.TABLE):
        flat = [e for t in tris for e in t]
        assert count[mask] == len(tris), mask
        assert edges[mask] == flat + [255] * (15 - len(flat)), mask


def test_generator_writes_the_committed_header():
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_mc_table', os.path.join(ROOT, 'tools', 'gen_mc_table.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.header_text(gen.build_table()) == open(os.path.join(ROOT, 'syconn_amd', 'csrc', 'sd_mc_table.h')).read()


def test_rule_table_numbers():
    assert sum(len(t) for t in R.TABLE) == 820 and max(len(t) for t in R.TABLE) == 5
    assert R.TABLE[0] == [] and R.TABLE[255] == []
    for mask in range(256):                                 # every crossing edge of a mask is used, and no other
        used = {e for t in R.TABLE[mask] for e in t}
        crossing = {k for k, (a, b) in enumerate(R.EDGES) if ((mask >> a) & 1) != ((mask >> b) & 1)}
        assert used == crossing, mask


def shape_numbers(m):
    keys, t = R.marching_cubes(m)
    closed, manifold = R.edge_balance(t)
    return len(keys), len(t), R.signed_volume(R.key_positions(keys, m.shape), t), closed, manifold, R.euler(len(keys), t)


def test_rule_shapes():
    one = np.zeros((3, 3, 3), bool); one[1, 1, 1] = True
    assert shape_numbers(one) == (6, 8, 1 / 6, True, True, 2)
    box = np.zeros((6, 5, 4), bool); box[1:5, 1:4, 1:3] = True
    nv, nt, vol, closed, manifold, chi = shape_numbers(box)
    assert (nv, nt, closed, chi) == (52, 100, True, 2) and abs(vol - (20 + 1 / 6)) < 1e-12
    g = np.indices((15, 15, 15)) - 7
    ball = (g ** 2).sum(0) <= 25
    assert ball.sum() == 515
    nv, nt, vol, closed, manifold, chi = shape_numbers(ball)
    assert (nv, nt, vol, closed, chi) == (486, 968, 503.25, True, 2)
    two = np.zeros((4, 4, 3), bool); two[1, 1, 1] = two[2, 2, 1] = True       # touching along a face diagonal: two octahedra
    assert shape_numbers(two)[:2] == (12, 16) and shape_numbers(two)[3:5] == (True, True)


@pytest.mark.parametrize('density', [0.2, 0.5, 0.8])
def test_rule_noise_is_closed_with_the_canonical_vertex_set(density):
    rng = np.random.default_rng(int(density * 10))
    m = np.zeros((10, 10, 10), bool)
    m[1:-1, 1:-1, 1:-1] = rng.random((8, 8, 8)) < density
    keys, t = R.marching_cubes(m)
    assert R.edge_balance(t)[0]
    assert np.array_equal(np.unique(t), np.arange(len(keys)))            # every vertex of the canonical set is used


def test_restatement_equals_the_reference_golden(gold):
    for r in 'ab':
        for c in range(3):
            chunk = np.ascontiguousarray(gold['vol'][8 * c:8 * c + 8])
            t = R.find_meshes_table(chunk, gold['origin'] + (8 * c, 0, 0), pad=1, ds=gold[f'{r}_ds'], scaling=gold['scaling'])
            assert same_bits(t['ids'], gold[f'{r}{c}_ids'])
            assert same_bits(t['vertices'].reshape(-1), gold[f'{r}{c}_vert']) and same_bits(t['indices'].reshape(-1), gold[f'{r}{c}_ind'])
            assert np.array_equal(t['vert_begin'].astype(np.int64) * 3, gold[f'{r}{c}_vert_begin'])
            assert np.array_equal(t['tri_begin'].astype(np.int64) * 3, gold[f'{r}{c}_ind_begin'])


@pytest.mark.parametrize('shape,ds,pad', [((8, 10, 9), (2, 2, 1), 1), ((33, 31, 18), (4, 4, 2), 1), ((33, 31, 18), (4, 4, 2), 0), ((7, 5, 3), None, 1),
                                          ((9, 9, 9), (3, 2, 1.5), 1)])
def test_source_tables_are_scipy_zoom_and_numpy_pad(shape, ds, pad):
    from syconn_amd.proc.meshes import _source_tables
    vol = np.arange(1, np.prod(shape) + 1, dtype=np.uint64).reshape(shape)
    tx, ty, tz = _source_tables(shape, pad, None if ds is None else np.asarray(ds, np.float64))
    assert tx.dtype == np.int32 and min(tx.min(), ty.min(), tz.min()) >= 0
    assert np.array_equal(vol[tx][:, ty][:, :, tz], R.padded_volume(vol, pad, ds))


def pieces_of(gold, r, i):
    out = []
    for c in range(3):
        ids = list(gold[f'{r}{c}_ids'])
        if i in ids:
            k = ids.index(i)
            ib, vb = gold[f'{r}{c}_ind_begin'], gold[f'{r}{c}_vert_begin']
            out.append([gold[f'{r}{c}_ind'][ib[k]:ib[k + 1]], gold[f'{r}{c}_vert'][vb[k]:vb[k + 1]], np.zeros((0,), np.float32)])
    return out


def test_numpy_drop_ins_equal_the_golden(gold):
    from syconn_amd.proc import meshes as M
    for r in 'ab':
        for k, i in enumerate(gold[f'{r}_ids']):
            parts = pieces_of(gold, r, i)
            ib, vb = gold[f'{r}_ind_begin'], gold[f'{r}_vert_begin']
            want = [gold[f'{r}_ind'][ib[k]:ib[k + 1]], gold[f'{r}_vert'][vb[k]:vb[k + 1]]]
            a = M.merge_meshes([p[0] for p in parts], [p[1] for p in parts])
            b = M.merge_meshes_incl_norm([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts])
            assert same_bits(a[0], want[0]) and same_bits(a[1], want[1]) and same_bits(b[0], want[0]) and same_bits(b[1], want[1]) and b[2].shape == (0,)
            if len(want[1]):
                assert np.float64(M.mesh_area_calc(b)).tobytes() == gold[f'{r}_area'][k].tobytes()
    e = M.merge_meshes([], [])
    assert e[0].dtype == np.uint64 and [len(x) for x in e] == [0, 0, 0] and len(M.merge_meshes_incl_norm([], [], [])) == 3
    c = np.array([[0., 0, 0], [2, 4, 6], [4, 2, 0]])
    mean, dist = M.get_bounding_box(c.reshape(-1))
    assert np.array_equal(mean, [2, 2, 2]) and dist == 4 and M.get_bounding_box(c)[1] == 4


def gold_table(gold, r):
    from syconn_amd.proc.meshes import MeshTable
    return MeshTable(gold[f'{r}_ids'], gold[f'{r}_vert_begin'] // 3, gold[f'{r}_ind_begin'] // 3, gold[f'{r}_vert'], gold[f'{r}_ind'], gold[f'{r}_bb'], gold[f'{r}_area'])


def test_mesh_props_equal_the_golden(gold):
    from syconn_amd.proc.meshes import mesh_props
    from syconn_amd.proc.sd_proc import PropTable
    props = PropTable(gold['p_ids'], gold['p_sizes'], np.zeros((len(gold['p_ids']), 3), np.int64), gold['p_boxes'], gold['p_box_begin'])
    for r in 'ab':
        t = mesh_props(gold_table(gold, r), props, gold['scaling'], int(gold['p_min_obj_vx']), int(gold['p_mesh_min_obj_vx']))
        assert same_bits(t.ids, gold['p_ids'])
        assert np.array_equal(np.diff(t.vert_begin.astype(np.int64)), gold[f'{r}_props_nvert']) and np.array_equal(np.diff(t.tri_begin.astype(np.int64)), gold[f'{r}_props_ntri'])
        assert same_bits(t.mesh_bb.astype(np.float64), gold[f'{r}_props_bb']) and same_bits(t.mesh_area, gold[f'{r}_props_area'])
        assert (gold[f'{r}_props_nvert'] == 0).any()
        full = gold_table(gold, r)
        for k, i in enumerate(t.ids):                       # kept objects keep their mesh
            if gold[f'{r}_props_nvert'][k]:
                assert same_bits(t.as_dict()[int(i)][1], full.as_dict()[int(i)][1]) and same_bits(t.as_dict()[int(i)][0], full.as_dict()[int(i)][0])


def test_mesh_table_views(gold):
    from syconn_amd.extraction.cs_processing_steps import OrganelleTable
    from syconn_amd.proc.meshes import MeshTable
    t = gold_table(gold, 'b')
    d = t.as_dict()
    assert list(d) == [int(i) for i in t.ids] and all(v[0].dtype == np.uint32 and v[1].dtype == np.float32 and v[2].shape == (0,) for v in d.values())
    ids = np.array([t.ids[2], 12345, t.ids[0]], U)
    verts, begin = t.vertices_of(ids)
    assert begin.dtype == np.int64 and begin[2] == begin[1] and same_bits(verts[:begin[1]].reshape(-1), d[int(ids[0])][1])
    assert same_bits(verts[begin[2]:].reshape(-1), d[int(ids[2])][1])
    OrganelleTable(ids, np.zeros(3), np.ones(3), np.zeros((3, 3)), verts, begin)
    assert len(MeshTable.empty()) == 0 and MeshTable.empty().vertices_of(ids)[1].tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        MeshTable(t.ids, t.vert_begin[:-1], t.tri_begin, t.vertices, t.indices, t.mesh_bb, t.mesh_area)


def test_argument_checks():
    from syconn_amd.proc.meshes import find_meshes
    z = np.zeros((4, 4, 4), np.uint64)
    kw = dict(scaling=(10, 10, 20))
    for bad in (dict(pad=2), dict(pad=-1), dict(ds=(2, 2)), dict(ds=(2, 0, 1)), dict(scaling=(10, 10)), dict(scaling=(10, -1, 20)),
                dict(meshing_props={'colour': 1})):
        with pytest.raises(ValueError):
            find_meshes(z, (0, 0, 0), **{**kw, **bad})
    with pytest.raises(ValueError):
        find_meshes(z[0], (0, 0, 0), **kw)
    with pytest.raises(ValueError):
        find_meshes(z, (0, 0), **kw)
    with pytest.raises(NotImplementedError):
        find_meshes(z, (0, 0, 0), meshing_props={'normals': True, 'simplification_factor': 50, 'max_simplification_error': 40}, **kw)


def test_config_has_the_meshes_block():
    from syconn_amd import global_params
    m = global_params.config['meshes']
    assert m['downsampling']['mi'] == [4, 4, 2] and m['downsampling']['sj'] == [2, 2, 1] and m['mesh_min_obj_vx'] == 100
    assert m['meshing_props'] == {'normals': False, 'simplification_factor': 50, 'max_simplification_error': 40}


def test_no_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is visible')
    from syconn_amd.proc.meshes import MeshTable, find_meshes
    one = np.zeros((3, 3, 3), np.uint64); one[1, 1, 1] = 4
    with pytest.raises(RuntimeError):
        find_meshes(one, (0, 0, 0), scaling=(10, 10, 20))
    t = MeshTable([4], [0, 1], [0, 0], np.zeros((1, 3)), np.zeros((0, 3)), np.zeros((1, 2, 3), np.float32), [0.])
    with pytest.raises(RuntimeError):
        MeshTable.merge([t, t])
