"""GPU: the spine head volumes on the device (``sd_spinehead_*``, ``sd_edt_squared``, ``extraction/spinehead.py``) against the CPU
restatement tests/_spinehead_ref.py, stage by stage and bit for bit: the window mask, the filled mask, the squared distances, the peak
list, the vertices in the box and the votes, the marker volume, the flood labels, the head objects, the chosen id and its voxel count --
on the windows of golden g22 and on random blobs-and-sticks volumes with ragged extents.  Then ``calculate_spinehead_volume``, the drop-in
``extract_spinehead_volume_mesh`` and the ``exec_syns`` form against g22 (the reference's own numbers), and the ``spinehead_vol`` columns
of conn_mat.csv through ``collect_properties_from_ssv_partners`` and ``export_matrix``."""
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _spinehead_ref as R  # noqa: E402
import _syn_props_ref as SP  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = ['a_', 'b_', 'c_', 'd_']
IGNORE = (4, 5)


@pytest.fixture(scope='module')
def g22():
    return dict(np.load(os.path.join(HERE, 'golden', 'g22_spinehead.npz')))


def cell_inputs(cell, scaling):
    verts = np.asarray(cell['vertices'], np.float32).reshape(-1, 3) / np.array(scaling)
    sem = np.asarray(cell['vertex_labels']['spiness']).reshape(-1)
    keep = ~np.isin(sem, IGNORE)
    return verts[keep], sem[keep]


def assert_stages(got, want, what):
    """got: the device tensors of one window (WindowRunner.run_batch(keep=...)), want: R.window_stages."""
    cpu = lambda t: t.cpu().numpy()
    for key in ('mask', 'filled', 'd2'):
        assert np.array_equal(cpu(got[key]), want[key]), (what, key)
    assert cpu(got['peaks']).tolist() == want['peaks'].tolist(), (what, 'peaks')
    assert cpu(got['points']).tobytes() == np.ascontiguousarray(want['points'], np.float64).tobytes(), (what, 'points')
    assert np.array_equal(cpu(got['point_labels']), want['point_labels']), (what, 'point labels')
    if not want['entry']:
        assert 'flood' not in got
        return
    assert np.array_equal(cpu(got['votes']), want['votes']), (what, 'votes')
    for key in ('markers', 'flood', 'objects'):
        assert np.array_equal(cpu(got[key]), want[key]), (what, key)


@pytest.mark.parametrize('p', CASES)
def test_golden_windows_stage_by_stage(gpu, g22, p):
    from syconn_amd.extraction import spinehead as SH
    case = R.case_from_golden(g22, p)
    n_windows = 0
    for cell in case['cells']:
        ids, rep = R.synapses_of(case, cell['id'])
        head = R.spinehead_filter(cell, rep, case['scaling'], case['k'], 1, IGNORE, R.AX_KEY)
        ids, rep = ids[head], rep[head]
        if not len(ids):
            continue
        verts, sem = cell_inputs(cell, case['scaling'])
        keep = []
        if cell['id'] in case['err_cells']:
            with pytest.raises(ValueError, match='Could not find segmentation at'):
                SH.spinehead_windows(case['seg'], cell['sv_ids'], rep, verts, sem, case['scaling'], case['ctx_vol'], case['k'], gpu, syn_ids=ids)
            continue
        res = SH.spinehead_windows(case['seg'], cell['sv_ids'], rep, verts, sem, case['scaling'], case['ctx_vol'], case['k'], gpu, batch=3, syn_ids=ids,
                                   keep=keep)
        stages = {}
        R.extract_spinehead_volume(cell, ids, rep, case['seg'], case['scaling'], case['ctx_vol'], case['k'], stages=stages)
        for i, sid in enumerate(ids.tolist()):
            want = stages[sid]
            assert_stages(keep[i], want, (p, cell['id'], sid))
            assert res[i, 0] == want['filled'].sum() and res[i, 1] == len(want['peaks']) and res[i, 5] == len(want['points'])
            if want['entry']:
                assert res[i, 2:5].tolist() == [want['n_voxels'], want['chosen'], want['nb_obj']], (p, cell['id'], sid)
            n_windows += 1
    assert n_windows >= 1


RANDOM = [((17, 33, 9), 3), ((16, 16, 16), 4), ((40, 23, 31), 5), ((33, 40, 17), 6), ((21, 19, 38), 7)]


VOXEL_SIZES = [('', np.array([10, 10, 10])), ('-9.1-float64', np.array([9.1, 9.1, 22.5], np.float64)), ('-9.1-float32', np.array([9.1, 9.1, 22.5], np.float32))]


@pytest.mark.parametrize('shape,seed,scaling', [(sh, seed, sc) for _, sc in VOXEL_SIZES for sh, seed in RANDOM],
                         ids=[f'shape{i}-{seed}{tag}' for tag, _ in VOXEL_SIZES for i, (_, seed) in enumerate(RANDOM)])
def test_random_windows_stage_by_stage(gpu, shape, seed, scaling):
    """Blobs and sticks, rows that are no multiple of a mask word; one window = the whole volume, two supervoxel ids of which the cell
    owns one or both; random vertices labelled by the side of a plane they are on, so that several head objects form.  Voxel size
    (10, 10, 10): the identity zoom; (9.1, 9.1, 22.5): ds = (2, 2, 1), so the zoom tables and ``maxima * ds`` count, and the distances of
    the head selection are no longer exact; the window then has ``shape * ds`` voxels, every blob voxel repeated ds times,
    so that the zoomed volume has `shape` and blobs as thick."""
    import torch
    from syconn_amd.extraction import spinehead as SH
    rng = np.random.default_rng(seed)
    ds = scaling[2] // scaling
    zoomed, shape = shape, tuple(int(n * d) for n, d in zip(shape, ds))
    m = R.blob_volume(zoomed, seed)
    for a in range(3):
        m = np.repeat(m, int(ds[a]), a)                                        # (the zoom samples it back with scipy's drifting step)
    ids = np.where(np.indices(shape)[1] < shape[1] // 2, 7, 9).astype(np.uint64)
    vol = np.where(m > 0, ids, np.uint64(3))                                   # a foreign id in the background
    sv = np.array([7, 9] if seed % 2 else [9, 7, 7], np.uint64)
    if seed == 4:
        sv = np.array([7], np.uint64)
    surf = np.transpose(np.nonzero(m))
    verts = surf[rng.permutation(len(surf))[:300]] + rng.uniform(0.05, 0.95, (min(300, len(surf)), 3))
    labels = np.where(verts[:, 0] + verts[:, 2] * 0.5 < (shape[0] + shape[2] * 0.5) * 0.5, 1, np.where(rng.random(len(verts)) < 0.5, 0, 2)).astype(np.int32)
    k = 7
    tabs_h = [SH.zoom_source_table(n, d) for n, d in zip(shape, ds)]
    assert [len(t) for t in tabs_h] == list(zoomed)
    runner = SH.WindowRunner([len(t) for t in tabs_h], batch=2, device=gpu)
    tabs = [torch.from_numpy(t).to(runner.dev) for t in tabs_h]
    seg_d = torch.from_numpy(vol.view(np.int64)).to(runner.dev)
    sv_d = torch.from_numpy(np.unique(sv).view(np.int64)).to(runner.dev)
    verts_d, lab_d = torch.from_numpy(verts).to(runner.dev), torch.from_numpy(labels).to(runner.dev)
    cs = np.array([[s // 2 for s in zoomed], [3, 2, 4]], np.int64)              # the slice around the first holds voxels, the second wraps
    keep = []
    res = runner.run_batch(seg_d, (0, 0, 0), np.zeros((2, 3), np.int64), tabs, sv_d, verts_d, lab_d, np.array(shape, np.int32), ds.astype(np.float64), k, cs,
                           scaling.astype(np.float64), keep)
    for w in range(2):
        want = R.window_stages(vol, sv, ds, verts, labels, np.zeros(3, np.int64), np.array(shape), cs[w], scaling, k)
        assert want['entry'] and len(want['peaks']) > 0
        assert_stages(keep[w], want, (shape, w))
        assert res[w].tolist() == [want['filled'].sum(), len(want['peaks']), want['n_voxels'], want['chosen'], want['nb_obj'], len(want['points'])]


def _table(case, skip=()):
    from syconn_amd.extraction.cs_processing_steps import CellTable
    cells = [c for c in case['cells'] if c['id'] not in skip]
    offs = lambda parts: np.concatenate(([0], np.cumsum([len(p) for p in parts])))
    t = CellTable([c['id'] for c in cells], np.concatenate([c['vertices'] for c in cells]), offs([c['vertices'] for c in cells]),
                  {'spiness': np.concatenate([c['vertex_labels']['spiness'] for c in cells])}, np.concatenate([c['nodes'] for c in cells]),
                  offs([c['nodes'] for c in cells]), {R.AX_KEY: np.concatenate([c['node_attrs'][R.AX_KEY] for c in cells])})
    return t, offs([c['sv_ids'] for c in cells]), np.concatenate([c['sv_ids'] for c in cells])


def as_dicts(table, triple):
    sb, ids, vols = triple
    return {int(cid): dict(zip(ids[sb[i]:sb[i + 1]].tolist(), vols[sb[i]:sb[i + 1]])) for i, cid in enumerate(table.ids.tolist())}


@pytest.mark.parametrize('p', CASES)
def test_calculate_spinehead_volume_matches_the_reference(gpu, g22, p):
    from syconn_amd.extraction.cs_processing_steps import calculate_spinehead_volume
    case = R.case_from_golden(g22, p)
    t, sb, sv = _table(case, skip=case['err_cells'])
    kw = dict(scaling=case['scaling'], ctx_vol=case['ctx_vol'], k=case['k'], ax_key=R.AX_KEY, device=gpu)
    triple = calculate_spinehead_volume(t, sb, sv, case['syn_ids'], case['syn_rep'], case['syn_cells'], case['seg'], **kw)
    assert triple[2].dtype == np.float64 and triple[1].dtype == np.uint64
    got = as_dicts(t, triple)
    assert sorted(got) == sorted(case['expected'])
    for cid, want in case['expected'].items():
        assert sorted(got[cid]) == sorted(want), cid
        for s in want:
            assert got[cid][s] == want[s], (cid, s, got[cid][s], want[s])
    if case['err_cells']:
        t, sb, sv = _table(case)
        with pytest.raises(ValueError, match='Could not find segmentation at'):
            calculate_spinehead_volume(t, sb, sv, case['syn_ids'], case['syn_rep'], case['syn_cells'], case['seg'], **kw)


class Kd:
    """A stand-in KnossosDataset: ``load_seg`` (z, y, x), zeros outside; counts its reads and keeps their sizes."""

    def __init__(self, vol):
        self.vol, self.reads, self.sizes = vol, 0, []

    def load_seg(self, size, offset, mag=1, **_):
        self.reads += 1
        self.sizes.append([int(v) for v in size])
        return R.load_window(self.vol, (0, 0, 0), offset, size).swapaxes(2, 0)


def test_drop_in_and_dataset_reads(gpu, g22):
    from syconn_amd.reps.super_segmentation_helper import extract_spinehead_volume_mesh
    case = R.case_from_golden(g22, 'a_')
    cell = case['cells'][0]
    ids, rep = R.synapses_of(case, cell['id'])

    class Config(dict):
        kd_seg_path = None
    cfg = Config(spines={'semseg2coords_spines': dict(k=case['k'], ds_vertices=1, ignore_labels=list(IGNORE))},
                 compartments={'view_properties_semsegax': {'semseg_key': 'axoness'}, 'dist_axoness_averaging': 10000})
    cfg.kd_seg_path = Kd(case['seg'][0])
    sso = types.SimpleNamespace(id=cell['id'], attr_dict={'x': 0}, scaling=np.array(case['scaling']), sv_ids=cell['sv_ids'], config=cfg,
                                syn_ssv=[types.SimpleNamespace(id=int(i), rep_coord=r) for i, r in zip(ids, rep)],
                                mesh=(np.zeros(0, np.uint32), cell['vertices'].reshape(-1), np.zeros(0, np.float32)),
                                skeleton={'nodes': cell['nodes'], R.AX_KEY: cell['node_attrs'][R.AX_KEY]}, label_dict=lambda kind: cell['vertex_labels'])
    extract_spinehead_volume_mesh(sso, ctx_vol=tuple(int(v) for v in case['ctx_vol']))
    want = case['expected'][cell['id']]
    assert sorted(sso.attr_dict['spinehead_vol']) == sorted(want) and len(want) >= 4
    for s in want:
        assert sso.attr_dict['spinehead_vol'][s] == want[s]
    kd = cfg.kd_seg_path
    assert 1 <= kd.reads < len(want)                               # neighbouring windows share a region
    assert all(n <= 256 + 2 * c for size in kd.sizes for n, c in zip(size, case['ctx_vol']))
    sso.label_dict = lambda kind: {}
    with pytest.raises(ValueError, match='"spiness" not available in skeleton of SSO 1'):
        extract_spinehead_volume_mesh(sso)


def test_conn_mat_columns(gpu, g22, tmp_path):
    """run_spinehead_volume_calc -> collect_properties_from_ssv_partners -> export_matrix: conn_mat.csv equals the reference form
    (tests/_syn_props_ref.py, pinned by g21) fed with the reference's own volumes of g22, byte for byte."""
    from syconn_amd.exec.exec_syns import run_spinehead_volume_calc
    from syconn_amd.extraction.cs_processing_steps import collect_properties_from_ssv_partners, export_matrix
    case = R.case_from_golden(g22, 'a_')
    t, sb, sv = _table(case, skip=case['err_cells'])
    live = np.isin(case['syn_cells'][:, 0], t.ids)
    own, rep, syn_ids = case['syn_cells'][live], case['syn_rep'][live], case['syn_ids'][live]
    n = len(syn_ids)

    class Syn:
        def __init__(self, partners):
            self.neuron_partners, self.rep_coords, self.syn_type_sym_ratio = partners, rep.astype(np.int32), np.linspace(0, 1, n)

        def __len__(self):
            return n
    run_spinehead_volume_calc(t, sb, sv, Syn(own), syn_ids, case['seg'], scaling=case['scaling'], ctx_vol=case['ctx_vol'], k=case['k'], ax_key=R.AX_KEY,
                              device=gpu)
    assert t.spinehead_vol is not None and t.spinehead_vol[2].dtype == np.float32 and len(t.spinehead_vol[2]) >= 6
    # conn_mat needs both partners in the table: the second one becomes cell 3, which holds no volume for these synapses (-1)
    partners = own.copy()
    partners[:, 1] = np.where(np.isin(partners[:, 1], t.ids), partners[:, 1], 3)
    props = collect_properties_from_ssv_partners(Syn(partners), t, case['scaling'], syn_ids=syn_ids, n_embedding=2, device=gpu)
    syn_prob, area = np.linspace(0.1, 0.9, n), np.linspace(1, 2, n)
    path = export_matrix(Syn(partners), props, syn_prob, area, str(tmp_path))
    cells = [dict(c, celltype=-1, spinehead_vol={int(k): np.float32(v) for k, v in case['expected'][c['id']].items()}) for c in case['cells']
             if c['id'] not in case['err_cells']]
    want = SP.collect_properties(partners, rep, np.linspace(0, 1, n), syn_ids, cells, case['scaling'], k=50, n_embedding=2)
    assert np.array_equal(props.partner_spineheadvol, want['partner_spineheadvol']) and (want['partner_spineheadvol'] > 0).any()
    ref_bytes = SP.conn_mat_bytes(rep, partners, want, syn_prob, area)
    got_bytes = open(path, 'rb').read()
    col = lambda b: [line.split(b'\t')[13:15] for line in b.splitlines()]
    assert col(got_bytes) == col(ref_bytes)
    assert got_bytes == ref_bytes


class BallKd:
    """A dataset without extent in memory: supervoxel 7 fills a ball of radius 5 around every centre; records the regions it is asked for."""

    def __init__(self, centres):
        self.centres, self.sizes = np.asarray(centres, np.int64), []

    def load_seg(self, size, offset, mag=1, **_):
        size, offset = np.asarray(size, np.int64), np.asarray(offset, np.int64)
        self.sizes.append(size.tolist())
        assert np.prod(size) * 8 < 2 ** 28, f'a region of {size.tolist()} voxels was requested'
        out = np.zeros(tuple(size), np.uint64)
        g = np.indices((11, 11, 11)).reshape(3, -1).T - 5
        g = g[(g ** 2).sum(1) <= 25]
        for c in self.centres:
            p = g + c - offset
            p = p[np.all((p >= 0) & (p < size), 1)]
            out[tuple(p.T)] = 7
        return out.swapaxes(2, 0)


def test_far_apart_windows_read_bounded_regions(gpu):
    """Windows of one cell thousands of voxels apart (and two close pairs): every region read from the dataset stays within one bucket
    + one window per axis, close windows share a read, and every window gives the ball's volume."""
    from syconn_amd.extraction import spinehead as SH
    centres = np.array([[40, 40, 40], [52, 44, 40], [9000, 300, 5000], [9010, 310, 5004], [300, 20000, 90], [20000, 20000, 20000]], np.int64)
    kd = BallKd(centres)
    rng = np.random.default_rng(2)
    verts = (centres[:, None, :] + rng.uniform(-4, 4, (len(centres), 30, 3))).reshape(-1, 3)
    labels = np.ones(len(verts), np.int32)
    ctx = np.array([12, 12, 12])
    res = SH.spinehead_windows(kd, [7], centres, verts, labels, (10, 10, 10), ctx, 5, gpu, batch=4)
    assert len(kd.sizes) == 4                                      # the two close pairs share a region each
    for size in kd.sizes:
        assert all(s <= SH.REGION_VOX + 2 * c for s, c in zip(size, ctx)), size
    # windows 0 / 1 and 2 / 3 see their neighbour's ball too (one or two head objects); the lone ones hold exactly one ball of 515 voxels
    assert res[4:, 2].tolist() == [515, 515] and res[4:, 4].tolist() == [1, 1] and (res[:, 2] >= 515).all() and (res[:, 5] >= 30).all()
