"""GPU: extract_cs_syntype (csrc/sd_cs_syntype.hip) and the sj morphology bit-exact against golden g16 (the reference's own Cython
and image.py), the table-overflow retry, and the per-chunk worker end to end against the numpy restatement on a synthetic
KnossosDataset, in the three syn-type modes and with syn types unavailable."""
import os
import pickle
import sys

import numpy as np
import pytest
import scipy.ndimage
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cs_syntype_ref as R  # noqa: E402
from test_cs_syntype_cpu import case_inputs, golden_dicts  # noqa: E402

pytestmark = pytest.mark.gpu
G16 = os.path.join(HERE, 'golden', 'g16_cs_syntype.npz')


@pytest.fixture(scope='module')
def g16():
    return dict(np.load(G16))


def same(got, want, name):
    assert got == want, name
    assert list(got[4]) == sorted(got[4]) and list(got[0][0]) == sorted(got[0][0]), name      # ascending id order
    for k in want[4]:
        assert got[4][k] == want[4][k], (name, k)                                              # voxel scan order


def test_extract_cs_syntype_golden_numpy(gpu, g16):
    from syconn_amd.extraction.find_object_properties import extract_cs_syntype
    dtypes = set()
    for name in g16['cst_cases']:
        cs, s, a, y, off = case_inputs(g16, name)
        dtypes.add(cs.dtype)
        got = extract_cs_syntype(cs, s, a, y, offset=off)
        same(got, golden_dicts(g16, name), name)
        assert all(type(k) is int for k in got[0][0]) and all(type(v) is list for v in got[0][1].values())
    assert dtypes == {np.dtype(np.uint32), np.dtype(np.uint64)}


def test_extract_cs_syntype_golden_device(gpu, g16):
    import torch
    from syconn_amd.extraction.find_object_properties import cs_syntype, extract_cs_syntype
    for name in g16['cst_cases']:
        cs, s, a, y, off = case_inputs(g16, name)
        ct = torch.from_numpy(cs.view(np.int64 if cs.dtype == np.uint64 else np.int32)).to(gpu)
        m = [torch.from_numpy(v).to(gpu) for v in (s, a, y)]
        same(extract_cs_syntype(ct, *m, offset=off), golden_dicts(g16, name), name)
        res = cs_syntype(ct, *m, offset=off)
        assert res.rec.is_cuda and res.voxels.is_cuda and res.voxels.dtype == torch.int64


def test_window_and_cores(gpu, g16):
    """The pass over a window of a larger volume equals the call on the cropped arrays; the core copies are the crop and the syn
    segmentation."""
    from syconn_amd.extraction.find_object_properties import cs_syntype, cs_syntype_dicts
    cs, s, a, y, _ = case_inputs(g16, 'vor64')
    org, ext = (5, 3, 4), (50, 57, 21)
    crop = tuple(slice(o, o + e) for o, e in zip(org, ext))
    res = cs_syntype(cs, s, a, y, offset=(7, 8, 9), origin=org, extent=ext, want_cores=True)
    want = R.extract_cs_syntype(cs[crop], s[crop], a[crop], y[crop], (7, 8, 9))
    assert cs_syntype_dicts(*res.host()) == want
    assert np.array_equal(res.cs_core.cpu().numpy().view(np.uint64), cs[crop])
    assert np.array_equal(res.syn_core.cpu().numpy().view(np.uint64), np.where(s[crop] != 0, cs[crop], 0))


def test_table_overflow_retry(gpu, g16):
    from syconn_amd.extraction.find_object_properties import CsSyntypeScan, cs_syntype_dicts
    cs, s, a, y, off = case_inputs(g16, 'vor64')
    sc = CsSyntypeScan(gpu)
    sc.cap = 16                                                   # 65 sites: two overflowing passes, then 256 slots
    got = cs_syntype_dicts(*sc.run(cs, s, a, y, off).host())
    assert sc.passes == 3 and sc.cap == 256
    same(got, golden_dicts(g16, 'vor64'), 'vor64')


def test_sj_morphology_golden(gpu, g16):
    from syconn_amd.extraction.cs_extraction_steps import binary_morphology
    from syconn_amd.extraction.object_extraction_steps import get_aniso_struct
    ops = [str(o) for o in g16['mop_ops']]
    for name in g16['mop_cases']:
        st = get_aniso_struct(g16[f'mop_{name}_scaling'])
        got = binary_morphology(g16[f'mop_{name}_in'], ops, st)
        assert got.dtype == np.uint8 and np.array_equal(got, g16[f'mop_{name}_out']), name
        # the threshold form: raw > 255 * t
        raw = g16[f'mop_{name}_in'] * np.uint8(200)
        assert np.array_equal(binary_morphology(raw, ops, st, threshold=199.5), g16[f'mop_{name}_out']), name


# ---- the worker end to end ------------------------------------------------------------------------------------------------------
BOX = (128, 64, 32)                   # x, y, z: two chunks of 64 x 64 x 32
CHUNK = (64, 64, 32)


def _kd(path, data_xyz=None, raw=None):
    from syconn_amd.knossos import KnossosDataset
    kd = KnossosDataset().initialize_without_conf(path, BOX, (10, 10, 20), 'synth', mags=[1])
    if data_xyz is not None:
        kd.save_seg(offset=(0, 0, 0), mags=[1], data=np.ascontiguousarray(data_xyz.swapaxes(0, 2)), data_mag=1)
    if raw is not None:
        kd.save_raw(offset=(0, 0, 0), mags=[1], data=np.ascontiguousarray(raw.swapaxes(0, 2)), data_mag=1)
    return kd


def _sj_seg_transform(seg):
    return (seg > 2).astype(np.uint8)


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    rng = np.random.default_rng(7)
    root = tmp_path_factory.mktemp('cs_kd')
    half = tuple(s // 2 for s in BOX)
    lab = np.zeros(half, np.uint64)
    pts = tuple(rng.integers(0, s, 40) for s in half)
    lab[pts] = np.unique(rng.integers(1, 2 ** 34, 40, dtype=np.uint64))[rng.permutation(40)]     # ids >= 2^32 are truncated
    _, ind = scipy.ndimage.distance_transform_edt(lab == 0, return_indices=True)
    cells = lab[tuple(ind)].repeat(2, 0).repeat(2, 1).repeat(2, 2)
    cells[rng.random(BOX) < 0.005] = 0
    noise = scipy.ndimage.gaussian_filter(rng.random(BOX), 2.0)
    noise = (noise - noise.min()) / (noise.max() - noise.min())
    sj_raw = (255 * noise ** 3).astype(np.uint8)                 # ~10 % above the default threshold (255 * 0.19)
    sj_seg = (noise > 0.5).astype(np.uint64) * 4 + rng.integers(0, 3, BOX).astype(np.uint64)       # > 2 on the blobs
    type_raw = [(255 * scipy.ndimage.gaussian_filter(rng.random(BOX), 1.5) * 1.8).clip(0, 255).astype(np.uint8) for _ in range(2)]
    type_lab = rng.integers(0, 4, BOX).astype(np.uint64)
    p = {'cells': str(root / 'cells'), 'sj': str(root / 'sj'), 'sym_raw': str(root / 'sym_raw'), 'asym_raw': str(root / 'asym_raw'),
         'sym_lab': str(root / 'sym_lab'), 'asym_lab': str(root / 'asym_lab'), 'types': str(root / 'types')}
    _kd(p['cells'], cells)
    _kd(p['sj'], sj_seg, raw=sj_raw)
    _kd(p['sym_raw'], raw=type_raw[0])
    _kd(p['asym_raw'], raw=type_raw[1])
    _kd(p['sym_lab'], type_lab)
    _kd(p['asym_lab'], rng.integers(0, 4, BOX).astype(np.uint64))
    _kd(p['types'], type_lab)
    return p


MODES = {
    'unavailable': dict(syntype_avail=False, paths={}, labels=(None, None)),
    'two_raw': dict(syntype_avail=True, paths={'kd_sym': 'sym_raw', 'kd_asym': 'asym_raw'}, labels=(None, None)),
    'two_labels': dict(syntype_avail=True, paths={'kd_sym': 'sym_lab', 'kd_asym': 'asym_lab'}, labels=(2, 3)),
    'one_kd': dict(syntype_avail=True, paths={'kd_sym': 'types', 'kd_asym': 'types'}, labels=(1, 3)),
}


@pytest.mark.parametrize('mode', list(MODES) + ['transf_func'])
def test_worker_end_to_end(gpu, dataset, tmp_path, mode):
    from syconn_amd import global_params
    from syconn_amd.extraction.cs_extraction_steps import _contact_site_extraction_thread
    from syconn_amd.handler import basics
    from syconn_amd.knossos import Chunk
    m = MODES['unavailable' if mode == 'transf_func' else mode]
    sym_label, asym_label = m['labels']
    wd = str(tmp_path / 'wd')
    os.makedirs(wd)
    paths = {'kd_sj': dataset['sj'], **{k: dataset[v] for k, v in m['paths'].items()}}
    with open(os.path.join(wd, 'config.yml'), 'w') as f:
        yaml.safe_dump({'scaling': [10, 10, 20], 'syntype_avail': m['syntype_avail'], 'paths': paths,
                        'cell_objects': {'sym_label': sym_label, 'asym_label': asym_label}}, f)
    saved = global_params.wd, global_params.config._wd, global_params.config._entries, global_params.config.initialized
    env = os.environ.pop('syconn_wd', None)
    global_params.wd = wd
    global_params.config._load(wd)
    try:
        _kd(f'{wd}/knossosdatasets/cs_seg/')
        _kd(f'{wd}/knossosdatasets/syn_seg/')
        chunks = [Chunk(i, (x, 0, 0), CHUNK, (0, 0, 0)) for i, x in enumerate(range(0, BOX[0], CHUNK[0]))]
        transf = _sj_seg_transform if mode == 'transf_func' else None
        nr, ids = _contact_site_extraction_thread((chunks, dataset['cells'], 3, str(tmp_path / 'props'), transf))
        kd_sym = basics.kd_factory(paths['kd_sym']) if m['syntype_avail'] else None
        kd_asym = basics.kd_factory(paths['kd_asym']) if m['syntype_avail'] else None
        cfg = dict(cs_filtersize=[13, 13, 7], cs_dilation=2, sj_ops=['binary_opening', 'binary_closing', 'binary_erosion'],
                   scaling=[10, 10, 20], sj_thresh=0.19047619, syntype=m['syntype_avail'], sym_label=sym_label,
                   asym_label=asym_label, same_kd=m['paths'].get('kd_sym') == m['paths'].get('kd_asym'))
        want = R.worker(chunks, basics.kd_factory(dataset['cells']), basics.kd_factory(dataset['sj']), cfg, transf, kd_sym, kd_asym)
        w_cs, w_syn, w_vox, w_asym, w_sym, cores = want
        d = str(tmp_path / 'props' / '3')
        load = lambda n: pickle.load(open(os.path.join(d, n), 'rb'))
        assert nr == 3 and ids['cs'] == list(w_cs[0]) and sorted(ids['syn']) == sorted(w_syn[0])
        assert load('cs_props_3.pkl') == w_cs and load('syn_props_3.pkl') == w_syn
        assert load('tot_asym_cnt_3.pkl') == w_asym and load('tot_sym_cnt_3.pkl') == w_sym
        assert len(w_syn[0]) > 0 and (not m['syntype_avail'] or (len(w_asym) > 0 and len(w_sym) > 0))
        vox = np.load(os.path.join(d, 'syn_voxels_3.npz'))
        assert sorted(vox.files) == sorted(w_vox)
        for k in w_vox:
            assert vox[k].dtype == np.int64 and np.array_equal(vox[k], w_vox[k]), k
        kd_cs = basics.kd_factory(f'{wd}/knossosdatasets/cs_seg/')
        kd_syn = basics.kd_factory(f'{wd}/knossosdatasets/syn_seg/')
        for off, cs_core, syn_core in cores:
            size = cs_core.shape[::-1]
            assert np.array_equal(kd_cs.load_seg(size=size, offset=off, mag=1), cs_core)
            assert np.array_equal(kd_syn.load_seg(size=size, offset=off, mag=1), syn_core)
    finally:
        global_params.wd = saved[0]
        global_params.config._wd, global_params.config._entries, global_params.config.initialized = saved[1:]
        if env is not None:
            os.environ['syconn_wd'] = env
