"""CPU: the restatement of the spine head volumes (tests/_spinehead_ref.py) against golden g22 (the reference's own
``extract_spinehead_volume_mesh`` on stand-ins, tests/golden/make_golden_spinehead.py) bit for bit, the zoom table builder of
``syconn_amd.extraction.spinehead`` against scipy, the region plan of the dataset reads, and the argument checks of the public functions, which
raise before any launch.  The head selection (``select_head``): its array form of the nearest-object distances against cKDTree's own bit for bit
on the hand-built volumes of tests/_spinehead_select_cases.py, which of those cases the reference's arithmetic decides, and the slice rule."""
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _spinehead_ref as R  # noqa: E402
import _spinehead_select_cases as K  # noqa: E402

from syconn_amd.extraction import spinehead as SH  # noqa: E402
from syconn_amd.extraction.cs_processing_steps import CellTable, calculate_spinehead_volume  # noqa: E402

CASES = ['a_', 'b_', 'c_', 'd_']


@pytest.fixture(scope='module')
def g22():
    return dict(np.load(os.path.join(HERE, 'golden', 'g22_spinehead.npz')))


@pytest.mark.parametrize('p', CASES)
def test_restatement_matches_the_reference(g22, p):
    case = R.case_from_golden(g22, p)
    n_entries = 0
    for cell in case['cells']:
        ids, rep = R.synapses_of(case, cell['id'])
        if cell['id'] in case['err_cells']:
            with pytest.raises(ValueError, match='Could not find segmentation'):
                R.extract_spinehead_volume(cell, ids, rep, case['seg'], case['scaling'], case['ctx_vol'], case['k'])
            continue
        got = R.extract_spinehead_volume(cell, ids, rep, case['seg'], case['scaling'], case['ctx_vol'], case['k'])
        want = case['expected'][cell['id']]
        assert sorted(got) == sorted(want)
        for s in want:
            assert isinstance(got[s], np.float64) and got[s] == want[s], (cell['id'], s, got[s], want[s])
        n_entries += len(want)
    assert n_entries > 0


def _select(case):
    info = {}
    objects, nb_obj, chosen, n_vox = R.select_head(case['flood'], case['c'], case['offset'], case['scaling'], info)
    return info, (chosen, n_vox, nb_obj)


@pytest.mark.parametrize('name,scaling', K.SCALINGS, ids=[n for n, _ in K.SCALINGS])
def test_nearest_array_form_is_ckdtrees_distance(name, scaling):
    """``nearest_d2`` -- both points scaled, then subtracted, ((dx dx) + dy dy) + dz dz in float64 with every operation rounded -- gives
    the distance cKDTree returns bit for bit, and, wherever one object is strictly nearest in it, cKDTree's pick; for voxel sizes as
    float64 and as float32, with window offsets and without.  Every random case is decided; the mirrored pairs around an unsymmetric c or
    with an offset are decided by the reference's rounding for the float64 non-integer sizes only (the products of a float32 or an
    integral voxel size with these integers are exact, so those pairs stay exact ties)."""
    cases = [K.random_objects(seed, off, scaling) for off in K.OFFSETS for seed in K.RANDOM_SEEDS]
    n_random = len(cases)
    for c, off in K.NEAR_TIES:
        cases += K.mirrored(c, off, scaling, K.N_NEAR, seed=2)
    decided = []
    for i, case in enumerate(cases):
        info, (chosen, n_vox, nb_obj) = _select(case)
        assert info['branch'] == 'nearest' and nb_obj >= 2
        assert np.float64(np.sqrt(info['d2'].min())).tobytes() == np.float64(info['dist']).tobytes(), (name, i)
        if info['decided']:
            assert chosen == info['ref_id'] == info['ids'][np.argmin(info['d2'])], (name, i)
        else:
            assert chosen <= info['ref_id']                          # the project's rule: the lowest of the tied ids
        assert info['decided'] or i >= n_random, (name, i)
        if i >= n_random:
            decided.append(chosen if info['decided'] else 0)
    inexact = scaling.dtype == np.float64 and name != '10-control'
    assert ({1, 2} <= set(decided)) == inexact and (0 in decided or inexact)


@pytest.mark.parametrize('name,scaling', K.SCALINGS, ids=[n for n, _ in K.SCALINGS])
def test_mirrored_pairs_tie_exactly(name, scaling):
    """c[0] == c[1], equal x and y voxel sizes, offset 0: the voxels c + (a, b, k) and c + (b, a, k) are exact ties in the reference's
    arithmetic, so the project's rule picks id 1, the first in raster order, with its single voxel."""
    cases = K.mirrored((30, 30, 4), (0, 0, 0), scaling, K.N_MIRRORED, seed=1)
    assert len(cases) >= 100
    for case in cases:
        info, got = _select(case)
        assert info['branch'] == 'nearest' and not info['decided'] and got == (1, 1, 2)
        assert len(info['d2']) == 2 and info['d2'][0].tobytes() == info['d2'][1].tobytes()


def test_slice_rule_cases():
    """The directed cases give what was worked out by hand; the random ones reach both branches, every (extent, c) pair on every axis."""
    for name, case, want in K.directed_slice_cases():
        assert _select(case)[1] == want, name
    cases = K.slice_cases()
    pairs = set(K.axis_pairs())
    assert len(pairs) == 41 and (9, 8) in pairs and (9, 9) not in pairs and (33, 21) in pairs and (20, 8) in pairs
    for a in range(3):
        assert {(c['flood'].shape[a], int(c['c'][a])) for c in cases} == pairs
    branches = [_select(c)[0]['branch'] for c in cases]
    assert branches.count('slice') >= 30 and branches.count('nearest') >= 30
    assert all(set(np.unique(c['flood']).tolist()) == {0, 1, 2, 9} for c in cases)


def test_golden_holds_its_cases(g22):
    """What the generator asserted, re-read from the file: entries of 0.0, cells that raise, synapses without entry."""
    vols = np.concatenate([g22[p + 'sh_vol'] for p in CASES])
    assert (vols == 0.0).any() and (vols > 0).any()
    assert sum(len(g22[p + 'err_cells']) for p in CASES) >= 1
    assert sum(len(g22[p + 'syn_ids']) for p in CASES) > len(vols)
    assert tuple(g22['a_scaling']) == (10, 10, 20) and tuple(g22['b_scaling']) == (10, 10, 10) and tuple(g22['c_ctx_vol']) == (15, 15, 8)


def test_zoom_table_matches_scipy():
    pairs = [(n, ds) for n in range(2, 65) for ds in (1, 2, 3, 4)] + [(400, 2), (200, 1)]
    checked = 0
    for n, ds in pairs:
        if round(n * (1 / ds)) < 1:
            with pytest.raises(ValueError):
                SH.zoom_source_table(n, ds)
            continue
        a = np.arange(1, n + 1)
        want = ndimage.zoom(a, 1 / ds, order=0)
        t = SH.zoom_source_table(n, ds)
        assert t.dtype == np.int32 and len(t) == len(want) == round(n / ds)
        assert np.array_equal(np.where(t < 0, 0, a[np.maximum(t, 0)]), want), (n, ds)
        checked += 1
    assert checked >= 250
    assert SH.zoom_source_table(30, 2)[-1] == -1                    # 14 * (29 / 14) > 29: scipy writes its constant
    for n, ds in ((400, 2), (40, 2), (41, 2), (24, 3)):
        assert (SH.zoom_source_table(n, ds) >= 0).all()
    assert len(SH.zoom_source_table(41, 2)) == 20
    assert np.array_equal(SH.zoom_source_table(200, 1), np.arange(200))
    # separable: the 3D zoom is the three tables
    rng = np.random.default_rng(5)
    v = rng.integers(1, 9, (30, 7, 12)).astype(np.uint64)
    tx, ty, tz = (SH.zoom_source_table(n, d) for n, d in zip(v.shape, (2, 1, 3)))
    got = np.where((tx[:, None, None] < 0) | (ty[None, :, None] < 0) | (tz[None, None, :] < 0), 0, v[np.ix_(np.maximum(tx, 0), np.maximum(ty, 0), np.maximum(tz, 0))])
    assert np.array_equal(got, ndimage.zoom(v, 1 / np.array([2, 1, 3]), order=0))


def test_region_plan_is_bounded():
    """Windows read from a dataset: every region stays within bucket + window per axis however far apart the windows of a cell are, no
    region holds more windows than a batch, every window is in exactly one region and inside it."""
    rng = np.random.default_rng(3)
    size = np.array([400, 400, 200])
    offsets = np.concatenate([rng.integers(0, 300, (5, 3)), rng.integers(0, 300, (4, 3)) + (9000, 0, 4000), [[255, 255, 255], [256, 256, 256]],
                              rng.integers(0, 20000, (20, 3))])
    plan = SH.plan_regions(offsets, size, 8)
    seen = np.concatenate([ix for ix, _, _ in plan])
    assert sorted(seen.tolist()) == list(range(len(offsets)))
    for ix, lo, hi in plan:
        assert 1 <= len(ix) <= 8
        assert np.all(hi - lo <= SH.REGION_VOX + size) and np.prod(hi - lo) * 8 <= SH.REGION_BYTES
        assert np.all(offsets[ix] >= lo) and np.all(offsets[ix] + size <= hi)
    assert len(plan) < len(offsets)                                # neighbours do share a region
    # a group that is too large for the byte bound is read window by window
    plan = SH.plan_regions([[0, 0, 0], [200, 200, 200]], size, 8, max_bytes=400 * 400 * 200 * 8)
    assert [(ix.tolist(), (hi - lo).tolist()) for ix, lo, hi in plan] == [([0], [400, 400, 200]), ([1], [400, 400, 200])]
    assert SH.plan_regions(np.zeros((0, 3)), size, 8) == []
    assert len(SH.plan_regions(np.zeros((20, 3)), size, 8)) == 3   # batches inside one bucket


def test_peak_rule_edges():
    m = np.zeros((7, 7, 7), np.uint8)
    m[3, 1:6, 1:6] = 1                                             # a sheet one voxel thick: a trivial image, no peaks
    d2 = np.rint(ndimage.distance_transform_edt(m) ** 2).astype(np.int64)
    assert len(R.peak_local_max(d2, m)) == 0
    m[0] = 1                                                       # only border voxels more: still none; the border is never a peak
    assert len(R.peak_local_max(np.rint(ndimage.distance_transform_edt(m) ** 2).astype(np.int64), m)) == 0
    m[:] = 0
    m[1:6, 1:6, 1:6] = 1
    p = R.peak_local_max(np.rint(ndimage.distance_transform_edt(m) ** 2).astype(np.int64), m)
    assert p.tolist() == [[3, 3, 3]]
    m[:] = 0
    m[2:5, 2:5, 1:6] = 1                                           # a bar: a plateau of equal maxima, every voxel of it a peak
    p = R.peak_local_max(np.rint(ndimage.distance_transform_edt(m) ** 2).astype(np.int64), m)
    assert p.tolist() == [[3, 3, 2], [3, 3, 3], [3, 3, 4]]


def _table(case):
    cells = case['cells']
    offs = lambda parts: np.concatenate(([0], np.cumsum([len(p) for p in parts])))
    t = CellTable([c['id'] for c in cells], np.concatenate([c['vertices'] for c in cells]), offs([c['vertices'] for c in cells]),
                  {'spiness': np.concatenate([c['vertex_labels']['spiness'] for c in cells])}, np.concatenate([c['nodes'] for c in cells]),
                  offs([c['nodes'] for c in cells]), {R.AX_KEY: np.concatenate([c['node_attrs'][R.AX_KEY] for c in cells])})
    return t, offs([c['sv_ids'] for c in cells]), np.concatenate([c['sv_ids'] for c in cells])


def test_argument_checks_raise_before_any_launch(g22):
    case = R.case_from_golden(g22, 'd_')
    t, sb, sv = _table(case)
    args = (t, sb, sv, case['syn_ids'], case['syn_rep'], case['syn_cells'], case['seg'])
    kw = dict(scaling=case['scaling'], ctx_vol=case['ctx_vol'], k=case['k'], ax_key=R.AX_KEY)
    for bad in (dict(k=0), dict(k=65), dict(k=2.5), dict(ctx_vol=(8, 8)), dict(ctx_vol=(8, 0, 8)), dict(ctx_vol=(8.5, 8, 8)), dict(scaling=(10, 10)),
                dict(scaling=(10, 10, 0)), dict(scaling=(20, 10, 10)), dict(batch=0), dict(ds_vertices=0)):
        with pytest.raises(ValueError):
            calculate_spinehead_volume(*args, **{**kw, **bad})
    with pytest.raises(TypeError):
        calculate_spinehead_volume(case['cells'], *args[1:], **kw)
    with pytest.raises(ValueError):
        calculate_spinehead_volume(t, sb[:-1], *args[2:], **kw)
    with pytest.raises(ValueError):
        calculate_spinehead_volume(*args[:4], case['syn_rep'][:0], *args[5:], **kw)
    with pytest.raises(ValueError, match='KnossosDataset'):
        calculate_spinehead_volume(*args[:6], np.zeros((4, 4, 4), np.uint64), **kw)
    with pytest.raises(ValueError, match='"nospine" not available in skeleton of SSO 1'):
        calculate_spinehead_volume(*args, semseg_key='nospine', **kw)
    # a synapse none of whose cells is in the table: nothing to do, nothing launched
    sh_begin, ids, vols = calculate_spinehead_volume(*args[:5], np.full((1, 2), 77, np.uint64), case['seg'], **kw)
    assert sh_begin.tolist() == [0, 0] and len(ids) == 0 and vols.dtype == np.float64
