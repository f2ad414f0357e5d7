"""CPU: the synapse agglomeration's numpy parts and the restatement the GPU tests compare with, against golden g19 (the reference's
own ``filter_relevant_syn``, ``connected_cluster_kdtree`` and ``_combine_and_split_syn_thread``).

1. tests/_syn_ssv_ref.py equals g19: the partitions, their order, every attribute, the aggregation in both indexing modes, the filter;
2. ``filter_relevant_syn``, ``build_syn_ssv_table`` (the host edge) and ``SynSsvTable.as_dict`` of the module equal g19 when fed the
   golden partition;
3. a gap below the two-voxel bound raises ``ValueError``; the binning cell's scaled diagonal stays below the gap;
4. a Python model of the device form (cells, reach, box classes) gives the reference's partition on g19 and the restatement's on
   random blobs."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _syn_ssv_ref as S  # noqa: E402

G19 = os.path.join(HERE, 'golden', 'g19_syn_ssv.npz')
CASES = ['a', 'b']


@pytest.fixture(scope='module')
def g19():
    return dict(np.load(G19))


def case(g, prefix):
    return {k[2:]: v for k, v in g.items() if k.startswith(prefix + '_')}


def golden_groups(c):
    """The groups as the reference's filter made them (ids looked up in the inputs)."""
    row_of = {int(i): r for r, i in enumerate(c['in_syn_ids'].tolist())}
    rows = np.array([row_of[int(i)] for i in c['f_syn_ids'].tolist()], np.int64)
    return S.groups_from_arrays(c['in_syn_ids'], c['in_vox'], c['in_vox_begin'], c['in_sym_prop'], c['in_asym_prop'], c['f_keys'],
                                c['f_group_begin'], rows), rows


def golden_rows(c, mode='r'):
    """g19's stored attributes as row dicts; `mode` 'x' takes the aggregation of the intended indexing."""
    groups, _ = golden_groups(c)
    flat = [np.concatenate([f[1] for f in frags]) for _, frags in groups]
    labels = [c['labels'][c['labels_begin'][g]:c['labels_begin'][g + 1]] for g in range(len(groups))]
    n_before = np.concatenate(([0], np.cumsum([int(lab.max()) + 1 for lab in labels])))
    rows = []
    cb = c[f'{mode}_cs_begin']
    for i, comp in enumerate(c['r_component'].tolist()):
        g = int(np.searchsorted(n_before, comp, side='right')) - 1
        rows.append(dict(neuron_partners=c['r_partners'][i], rep_coord=c['r_rep_coord'][i], bounding_box=c['r_bbox'][i], size=c['r_size'][i],
                         cs_ids=c[f'{mode}_cs_ids'][cb[i]:cb[i + 1]].tolist(), sym_prop=c[f'{mode}_sym_prop'][i],
                         asym_prop=c[f'{mode}_asym_prop'][i], syn_type_sym_ratio=c[f'{mode}_syn_type_sym_ratio'][i],
                         syn_sign=c[f'{mode}_syn_sign'][i], voxels=flat[g][labels[g] == comp - n_before[g]]))
    return rows, groups, labels


@pytest.mark.parametrize('prefix', CASES)
def test_restatement_equals_golden(g19, prefix):
    c = case(g19, prefix)
    rows_g, groups, labels_g = golden_rows(c)
    for mode, ref_ix in (('r', True), ('x', False)):
        want, _, _ = golden_rows(c, mode)
        got, labels = S.combine(groups, c['scaling'], float(c['cs_gap_nm']), int(c['min_obj_vx']), float(c['sym_thresh']), ref_ix)
        for a, b in zip(labels, labels_g):                       # the partition AND its order: label = position in the reference's list
            assert np.array_equal(a, b)
        S.assert_rows_equal(got, want, f'{prefix} {mode}')
        assert [r['component'] for r in got] == c['r_component'].tolist()
    # the reference's ids count the stored rows only: a dropped component leaves by `continue` before the id advances
    assert np.array_equal(c['r_ordinal'], np.arange(len(c['r_size']))) and c['r_component'][-1] > c['r_ordinal'][-1]


@pytest.mark.parametrize('prefix', CASES)
def test_filter_relevant_syn(g19, prefix):
    from syconn_amd.extraction.cs_processing_steps import filter_relevant_syn
    c = case(g19, prefix)
    _, rows_g = golden_groups(c)
    mapping = dict(zip(c['map_sv'].tolist(), c['map_ssv'].tolist()))
    for args in ((c['map_sv'], c['map_ssv']), (c['map_sv'][::-1], c['map_ssv'][::-1]), (mapping,)):
        keys, begin, rows = filter_relevant_syn(c['in_syn_ids'], *args)
        assert keys.dtype == np.uint64 and np.array_equal(keys, c['f_keys'])
        assert np.array_equal(begin, c['f_group_begin']) and np.array_equal(rows, rows_g)
    loop = S.filter_relevant_syn(c['in_syn_ids'], mapping)
    assert list(loop) == c['f_keys'].tolist() and [r for v in loop.values() for r in v] == rows_g.tolist()
    # nothing mapped, nothing given
    keys, begin, rows = filter_relevant_syn(c['in_syn_ids'], np.zeros(0, np.uint64), np.zeros(0, np.int64))
    assert len(keys) == 0 and begin.tolist() == [0] and len(rows) == 0
    keys, begin, rows = filter_relevant_syn(np.zeros(0, np.uint64), c['map_sv'], c['map_ssv'])
    assert len(keys) == 0 and begin.tolist() == [0] and len(rows) == 0
    with pytest.raises(ValueError):
        filter_relevant_syn(c['in_syn_ids'], np.array([5, 5], np.uint64), np.array([1, 2]))


def stats_from_labels(groups, labels):
    """What the device hands to the host edge, from a partition, in plain numpy."""
    flat = np.concatenate([f[1] for _, frags in groups for f in frags]).astype(np.int64)
    frag = np.concatenate([np.full(len(f[1]), k) for k, f in enumerate(f for _, frags in groups for f in frags)])
    n_before = np.concatenate(([0], np.cumsum([int(lab.max()) + 1 for lab in labels])))
    lab = np.concatenate([lab.astype(np.int64) + n_before[g] for g, lab in enumerate(labels)])
    group = np.concatenate([np.full(len(lab_g), g) for g, lab_g in enumerate(labels)])
    K = int(n_before[-1])
    order = np.argsort(lab, kind='stable')
    begin = np.searchsorted(lab[order], np.arange(K + 1))
    out = dict(comp_group=group[order][begin[:-1]], comp_sizes=np.diff(begin),
               comp_bbox=np.stack([np.minimum.reduceat(flat[order], begin[:-1]), np.maximum.reduceat(flat[order], begin[:-1])], 1))
    pair, cnt = np.unique(np.stack([lab, frag], 1), axis=0, return_counts=True)
    out.update(pair_comp=pair[:, 0], pair_frag=pair[:, 1], pair_cnt=cnt)
    return out, flat, lab, order, begin


@pytest.mark.parametrize('prefix', CASES)
def test_host_edge_and_as_dict(g19, prefix):
    from syconn_amd.extraction.cs_processing_steps import SynSsvTable, build_syn_ssv_table
    c = case(g19, prefix)
    min_vx = int(c['min_obj_vx'])
    for mode, ref_ix in (('r', True), ('x', False)):
        want, groups, labels = golden_rows(c, mode)
        st, flat, lab, order, begin = stats_from_labels(groups, labels)
        restated, _ = S.combine(groups, c['scaling'], float(c['cs_gap_nm']), min_vx, float(c['sym_thresh']), ref_ix, labels=labels)
        # the representative comes from the golden rows (the device finds it); dropped components get any voxel
        rep = flat[order][begin[:-1]].copy()
        rep[c['r_component']] = c['r_rep_coord']
        keep = np.repeat(st['comp_sizes'] >= min_vx, st['comp_sizes'])
        frags = [f for _, fr in groups for f in fr]
        t = build_syn_ssv_table(c['f_keys'], np.concatenate(([0], np.cumsum([len(fr) for _, fr in groups]))), [f[0] for f in frags],
                                [f[2] for f in frags], [f[3] for f in frags], st['comp_group'], st['comp_sizes'], st['comp_bbox'], rep,
                                st['pair_comp'], st['pair_frag'], st['pair_cnt'], flat[order][keep], c['scaling'], min_vx,
                                float(c['sym_thresh']), ref_ix)
        assert type(t) is SynSsvTable and len(t) == len(want) and t.n_components == len(st['comp_sizes'])
        S.assert_rows_equal(t.as_dict(), want, f'{prefix} {mode}')
        assert np.array_equal(t.ordinal, c['r_component'])
        assert t.rep_coords.dtype == np.int32 and t.voxels.dtype == np.uint32 and t.neuron_partners.dtype == np.uint64
        assert t.syn_sign.tobytes() == c[f'{mode}_syn_sign'].tobytes() and t.sym_prop.tobytes() == c[f'{mode}_sym_prop'].tobytes()
        assert t.syn_type_sym_ratio.tobytes() == c[f'{mode}_syn_type_sym_ratio'].tobytes()
        # the true contributors do not depend on the indexing mode
        fb = t.frag_begin.tolist()
        for i, r in enumerate(restated):
            assert t.frag_ids[fb[i]:fb[i + 1]].tolist() == r['frag_ids'] and t.frag_counts[fb[i]:fb[i + 1]].tolist() == r['frag_counts']
            assert t.group[i] == r['group']
        assert np.array_equal(np.diff(t.frag_begin) >= np.diff(t.cs_begin), np.ones(len(t), bool))
        first = np.concatenate(([0], np.cumsum(np.bincount(st['comp_group']))))
        assert np.array_equal(t.group_ordinal, t.ordinal - first[t.group])
        if ref_ix and prefix == 'a':                                # fragments 0 and 1 fold into one entry somewhere
            assert any(len(w['cs_ids']) < len(r['frag_ids']) for w, r in zip(want, restated))


def test_empty_table():
    from syconn_amd.extraction.cs_processing_steps import build_syn_ssv_table
    z = np.zeros(0, np.int64)
    t = build_syn_ssv_table(np.zeros(0, np.uint64), [0], z, z, z, z, z, np.zeros((0, 2, 3)), np.zeros((0, 3)), z, z, z, np.zeros((0, 3)),
                            (10, 10, 20), 100, 0.225)
    assert len(t) == 0 and t.as_dict() == [] and t.voxels.shape == (0, 3) and t.vox_begin.tolist() == [0] and t.bounding_boxes.shape == (0, 2, 3)


def test_gap_bound_and_cell():
    from syconn_amd.extraction import cs_processing_steps as P
    assert P.min_gap_nm((10, 10, 20)) == 40.0 and P.min_gap_nm((9, 9, 20)) == 40.0 and P.min_gap_nm((10, 10, 10)) == 20.0
    assert abs(P.min_gap_nm((10, 20, 5)) - 40.0) < 1e-12
    for gap, scale in ((40.0, (10, 10, 20)), (39.0, (10, 10, 20)), (20, (10, 10, 10)), (0, (1, 1, 1))):
        with pytest.raises(ValueError):
            P.choose_cell(scale, gap)
        with pytest.raises(ValueError):                                      # refused before any device is looked for
            P.connected_cluster([np.zeros((1, 3), np.uint32)], gap, scale)
    with pytest.raises(ValueError):
        P.choose_cell((10, 0, 20), 250)
    for gap, scale in ((250, (10, 10, 20)), (250, (9, 9, 20)), (40.5, (10, 10, 20)), (300, (4, 4, 40)), (1000.5, (7.5, 9.25, 33.0))):
        c = P.choose_cell(scale, gap)
        s = np.asarray(scale, np.float64)
        assert (c >= 1).all() and np.sqrt((((c - 1) * s) ** 2).sum()) < gap
    assert P.choose_cell((10, 10, 20), 250).tolist() == [15, 15, 8]


def test_defaults_in_config():
    from syconn_amd.handler.config import DynConfig
    co = DynConfig()['cell_objects']
    assert co['cs_gap_nm'] == 250 and co['sym_thresh'] == 0.225 and co['min_obj_vx']['syn_ssv'] == 100


@pytest.mark.parametrize('prefix', CASES)
def test_cell_model_equals_golden(g19, prefix):
    c = case(g19, prefix)
    groups, _ = golden_groups(c)
    for g, (_, frags) in enumerate(groups):
        got = S.cell_model_labels([f[1] for f in frags], float(c['cs_gap_nm']), c['scaling'])
        assert np.array_equal(got, c['labels'][c['labels_begin'][g]:c['labels_begin'][g + 1]]), (prefix, g)


@pytest.mark.parametrize('scale, gap, extent', [((10, 10, 20), 250, (60, 60, 30)), ((4, 4, 40), 120.5, (90, 90, 8)),
                                                ((10, 10, 10), 20.5, (12, 12, 12)), ((10, 10, 20), 1000, (200, 200, 100))])
def test_cell_model_equals_restatement(scale, gap, extent):
    rng = np.random.default_rng(7)
    n_comp = 0
    for g in range(12):
        lists = []
        for f in range(int(rng.integers(1, 7))):
            lo = np.array([int(rng.integers(0, e)) for e in extent])
            shape = rng.integers(1, 9, 3)
            box = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).reshape(-1, 3) + lo
            lists.append(box[rng.random(len(box)) < 0.7])
        lists = [v for v in lists if len(v)] or [np.zeros((1, 3), np.int64)]
        want = S.connected_cluster(lists, gap, scale)
        assert np.array_equal(S.cell_model_labels(lists, gap, scale), want), g
        n_comp += int(want.max()) + 1
    assert n_comp > 14
