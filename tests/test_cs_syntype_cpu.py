"""CPU: the numpy restatement of extract_cs_syntype and of the sj morphology against golden g16 (the reference's own Cython and
image.py functions), the new config defaults, and the worker's refusals, which come before any device work."""
import os
import sys

import numpy as np
import pytest
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cs_syntype_ref as R  # noqa: E402

G16 = os.path.join(HERE, 'golden', 'g16_cs_syntype.npz')


@pytest.fixture(scope='module')
def g16():
    return dict(np.load(G16))


def golden_dicts(g, name):
    """g16 flat arrays of one case -> the five results of extract_cs_syntype (keys ascending)."""
    p = lambda k: g[f'cst_{name}_{k}']
    def props(tag):
        ids = p(f'{tag}_ids').tolist()
        return [dict(zip(ids, p(f'{tag}_rc').tolist())), dict(zip(ids, p(f'{tag}_bb').tolist())), dict(zip(ids, p(f'{tag}_size').tolist()))]
    cnt = lambda tag: dict(zip(p(f'{tag}_ids').tolist(), p(f'{tag}_cnt').tolist()))
    vox, o = {}, 0
    for k, n in zip(p('vox_ids').tolist(), p('vox_cnt').tolist()):
        vox[k] = p('vox')[o:o + n].tolist()
        o += n
    return props('cs'), props('syn'), cnt('asym'), cnt('sym'), vox


def case_inputs(g, name):
    return tuple(g[f'cst_{name}_{k}'] for k in ('cs', 'syn', 'asym', 'sym', 'offset'))


def test_restated_cs_syntype_equals_golden(g16):
    assert len(g16['cst_cases']) >= 9
    for name in g16['cst_cases']:
        want = golden_dicts(g16, name)
        got = R.extract_cs_syntype(*case_inputs(g16, name))
        assert got == want, name
        assert [list(v) for v in got[4].values()] == [list(v) for v in want[4].values()], name   # voxel order per key


def test_restated_sj_morphology_equals_golden(g16):
    ops = [str(o) for o in g16['mop_ops']]
    assert ops == ['binary_opening', 'binary_closing', 'binary_erosion']
    for name in g16['mop_cases']:
        st = R.aniso_struct(g16[f'mop_{name}_scaling'])
        got = R.binary_morphology(g16[f'mop_{name}_in'], ops, st)
        assert np.array_equal(got, g16[f'mop_{name}_out']), name


def test_config_defaults():
    from syconn_amd.handler.config import DynConfig
    c = DynConfig()
    assert c.syntype_available is False and c['syntype_avail'] is False
    assert c.sym_label is None and c.asym_label is None
    assert c.kd_sj_path is None and c.kd_sym_path is None and c.kd_asym_path is None
    assert c['paths']['kd_seg'] is None and c['cell_objects']['cs_filtersize'] == [13, 13, 7]


@pytest.fixture
def wd(tmp_path):
    from syconn_amd import global_params
    old = global_params.wd
    saved = global_params.config._wd, global_params.config._entries, global_params.config.initialized
    env = os.environ.pop('syconn_wd', None)

    def make(entries):
        with open(tmp_path / 'config.yml', 'w') as f:
            yaml.safe_dump(entries, f)
        global_params.wd = str(tmp_path)
        global_params.config._load(str(tmp_path))
        return str(tmp_path)
    yield make
    global_params.wd = old
    global_params.config._wd, global_params.config._entries, global_params.config.initialized = saved
    if env is not None:
        os.environ['syconn_wd'] = env


def test_worker_refuses_identical_syntype_sources(wd):
    from syconn_amd.extraction.cs_extraction_steps import _contact_site_extraction_thread
    d = wd({'syntype_avail': True, 'paths': {'kd_sym': '/nonexistent/kd', 'kd_asym': '/nonexistent/kd'},
            'cell_objects': {'sym_label': 3, 'asym_label': 3}})
    with pytest.raises(ValueError, match='Both KnossosDatasets and labels for symmetric and asymmetric synapses are identical'):
        _contact_site_extraction_thread(([], '/nonexistent/cells', 0, os.path.join(d, 'props'), None))


def test_worker_refuses_zero_overlap(wd):
    from syconn_amd.extraction.cs_extraction_steps import _contact_site_extraction_thread
    d = wd({'cell_objects': {'cs_filtersize': [1, 1, 1]}})
    with pytest.raises(ValueError, match='overlap'):
        _contact_site_extraction_thread(([], '/nonexistent/cells', 0, os.path.join(d, 'props'), None))
