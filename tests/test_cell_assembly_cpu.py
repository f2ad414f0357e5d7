"""CPU: the restatement tests/_cell_assembly_ref.py against the golden of the reference's own functions (tests/golden/
g24_cell_assembly.npz) bit for bit, and the host-side argument checks, thresholds and config defaults of the cell assembly."""
import os

import numpy as np
import pytest

import _cell_assembly_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g24_cell_assembly.npz')
GRAPH_KEYS = ('node_ids', 'node_comp', 'node_size', 'ssv_ids', 'sv_begin', 'sv_ids', 'edges', 'total_size')
U = np.uint64


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('run', ['a', 'b', 'c'])
def test_components_restatement_equals_golden(gold, run):
    g = gold
    got = R.components(g['g_edges'], g['g_ids'], g['g_sizes'], g['g_box_begin'], g['g_boxes'], g[f'g_{run}_scaling'], float(g[f'g_{run}_min_cc_size']),
                       bool(g[f'g_{run}_strict']))
    for k in GRAPH_KEYS[:-1]:
        assert same_bits(got[k], g[f'g_{run}_{k}']), k
    assert got['total_size'] == int(g[f'g_{run}_total_size'])


def test_component_size_is_the_unfused_ordered_sum(gold):
    """What the device computes: max * s - min * s per axis, ((dx dx) + dy dy) + dz dz, a correctly rounded root -- against the sizes
    np.linalg.norm gave the reference, for the integral and the non-integral scaling."""
    g = gold
    mb = np.array(R.merged_boxes(g['g_box_begin'], g['g_boxes']))
    for run in 'ac':
        s = g[f'g_{run}_scaling']
        comp = g[f'g_{run}_node_comp']
        for cid in g[f'g_{run}_ssv_ids'][:50]:
            members = g[f'g_{run}_node_ids'][comp == cid]
            rows = np.flatnonzero(np.isin(g['g_ids'], members))
            lo, hi = mb[rows].reshape(-1, 3).min(0), mb[rows].reshape(-1, 3).max(0)
            d = hi * s - lo * s
            size = np.sqrt(((d[0] * d[0]) + d[1] * d[1]) + d[2] * d[2])
            assert size == g[f'g_{run}_node_size'][g[f'g_{run}_node_ids'] == cid][0]


def test_boxless_component_raises(gold):
    g = gold
    with pytest.raises(ValueError, match='Could not find a single bounding box'):
        R.components(np.concatenate([g['g_edges'], g['g_nobox_edges']]), g['g_ids'], g['g_sizes'], g['g_box_begin'], g['g_boxes'], g['g_a_scaling'], 5000)


def test_cell_props_restatement_equals_golden(gold):
    g = gold
    size, box, rep = R.cell_props(g['p_sv_begin'], g['p_sv_ids'], g['g_ids'], g['g_sizes'], g['g_rep'], g['g_box_begin'], g['g_boxes'])
    assert same_bits(size, g['p_size']) and same_bits(box, g['p_box']) and same_bits(rep, g['p_rep'])


@pytest.mark.parametrize('kind', ['mi', 'sj'])
def test_mapping_restatement_equals_golden(gold, kind):
    g = gold
    ssv_ids, sv_begin, sv_ids = R.explicit_cells(g['m_sv_begin'], g['m_sv_ids'])
    assert same_bits(ssv_ids, g['m_ssv_ids'])
    p = f'm_{kind}_'
    got = R.mapping(ssv_ids, sv_begin, sv_ids, g[p + 'sub'], g[p + 'sv'], g[p + 'count'], g[p + 'org_ids'], g[p + 'org_sizes'], *g[p + 'thresholds'])
    for k in ('cell_begin', 'ids', 'ratios', 'acc_begin', 'acc_ids'):
        assert same_bits(got[k], g[p + k]), k
    assert int(got['org_n_cells'].max()) == (2 if kind == 'sj' else 1)


def test_ratio_sums_depend_on_the_list_order(gold):
    g = gold
    ids, ratios = g['m_mi_ids'], g['m_mi_ratios']
    up, down = ratios[ids == 101][0], ratios[ids == 102][0]
    assert up == (1 / 12 + 2 / 12) + 3 / 12 and down == (3 / 12 + 2 / 12) + 1 / 12 and up != down
    assert ratios[ids == 103][0] == (9 / 56 + 18 / 56) + 1 / 56 == 0.5000000000000001


def test_synapses_restatement_equals_golden(gold):
    g = gold
    begin, out = R.cell_synapses(g['y_ssv_ids'], g['y_partners'], g['y_prob'], g['y_ids'], float(g['y_thresh']))
    assert same_bits(begin, g['y_begin']) and same_bits(out, g['y_out'])


# ---- host layer ------------------------------------------------------------------------------------------------------------------
def test_from_lists_orders_cells_and_keeps_lists(gold):
    from syconn_amd.proc.ssd_proc import CellLists, ssv_lookup
    g = gold
    cells = CellLists.from_lists(g['m_sv_begin'], g['m_sv_ids'])
    ssv_ids, sv_begin, sv_ids = R.explicit_cells(g['m_sv_begin'], g['m_sv_ids'])
    assert same_bits(cells.ssv_ids, ssv_ids) and same_bits(cells.sv_begin, sv_begin) and same_bits(cells.sv_ids, sv_ids)
    cells = CellLists.from_lists([0, 2, 5], np.array([9, 8, 3, 7, 2 ** 64 - 1], U))
    assert cells.ssv_ids.tolist() == [3, 8] and cells.sv_ids.tolist() == [3, 7, 2 ** 64 - 1, 9, 8] and cells.sv_begin.tolist() == [0, 3, 5]
    sv, ssv = ssv_lookup(cells)
    assert sv.tolist() == [3, 7, 2 ** 64 - 1, 9, 8] and ssv.tolist() == [3, 3, 3, 8, 8] and ssv.dtype == np.uint64
    assert {k: v.tolist() for k, v in cells.mapping_dict().items()} == {3: [3, 7, 2 ** 64 - 1], 8: [9, 8]}


@pytest.mark.parametrize('begin, ids, msg', [([0, 2, 4], [1, 2, 2, 3], 'two cells'), ([0, 2, 3], [1, 0, 3], 'id 0'), ([0, 2, 2, 3], [1, 2, 3], 'empty'),
                                             ([0, 2], [1, 2, 3], 'offsets'), ([0, 3], [4, 5, 4], 'two cells')])
def test_from_lists_argument_checks(begin, ids, msg):
    from syconn_amd.proc.ssd_proc import CellLists
    with pytest.raises(ValueError, match=msg):
        CellLists.from_lists(begin, np.array(ids, U))


def test_config_defaults_and_thresholds():
    from syconn_amd.handler.config import DEFAULTS
    from syconn_amd.proc.ssd_proc import mapping_thresholds
    assert DEFAULTS['min_cc_size_ssv'] == 5000
    co = DEFAULTS['cell_objects']
    assert co['lower_mapping_ratios'] == {'mi': 0.5, 'sj': 0.1, 'vc': 0.5} and co['upper_mapping_ratios'] == {'mi': 1., 'sj': 0.9, 'vc': 1.}
    assert co['sizethresholds'] == {'mi': 2786, 'sj': 498, 'vc': 1584}
    cfg = {'cell_objects': co}
    assert mapping_thresholds('sj', cfg) == (0.1, 0.9, 498.0)
    part = {'cell_objects': {'lower_mapping_ratios': {'er': 0.3}, 'upper_mapping_ratios': {}, 'sizethresholds': {'er': 7}}}
    assert mapping_thresholds('er', part) == (0.3, 1.0, 7.0)
    with pytest.raises(ValueError, match='Lower ratio undefined'):
        mapping_thresholds('golgi', part)
    with pytest.raises(ValueError, match='Size threshold undefined'):
        mapping_thresholds('er', {'cell_objects': {'lower_mapping_ratios': {'er': 0.3}, 'upper_mapping_ratios': {}, 'sizethresholds': {}}})


def test_drivers_fail_loudly_without_gpu(gold):
    import torch
    if torch.cuda.is_available():                          # the drivers themselves run in tests/test_gpu_cell_assembly.py
        return
    from syconn_amd.exec.exec_init import run_create_rag
    from syconn_amd.proc.sd_proc import PropTable
    g = gold
    with pytest.raises(RuntimeError):
        run_create_rag(g['g_edges'], PropTable(g['g_ids'], g['g_sizes'], g['g_rep'], g['g_boxes'], g['g_box_begin']), scaling=(10, 10, 20))
