"""GPU: the organelle mapping (csrc/sd_synssv_map.hip, ``extraction.cs_processing_steps.map_objects_from_synssv_partners``).

1. golden g20 (the reference's own workers over scipy's cKDTree), both cases end to end: integer columns exact, float32 columns bit
   for bit, the pair list call by call, ``pair_min_d2`` of case ``a`` bit for bit;
2. random inputs against the restatement tests/_synssv_map_ref.py (pinned to g20 on the CPU): negative and fractional vertices,
   shuffled voxel order, ``sample_fact`` 1, 2, 3, radii below and above the synapse extent; the launches once more over scratches
   with a guard band behind ``*_temp_bytes``; with a radius below the organelle length the point tests stay strictly below the
   brute-force product;
3. structure edges: organelles around the item size, synapses around the tile size, the last vertex of the last item, 65
   organelles in a cell, empty inputs;
4. the table ``combine_and_split_syn`` returns for g19's input goes into the mapping."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _synssv_map_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
G20 = os.path.join(HERE, 'golden', 'g20_synssv_map.npz')
G19 = os.path.join(HERE, 'golden', 'g19_syn_ssv.npz')
TYPES = ('mi', 'vc')
T = M.T_ITEM


@pytest.fixture(scope='module')
def g20():
    return dict(np.load(G20))


def case(g, prefix):
    return {k[2:]: v for k, v in g.items() if k.startswith(prefix + '_')}


class Syn:
    """The columns of a ``SynSsvTable`` the mapping reads."""

    def __init__(self, partners, rep, vox, vox_begin, sizes=None):
        self.neuron_partners, self.rep_coords, self.voxels, self.vox_begin = partners, rep, vox, vox_begin
        self.sizes = np.diff(vox_begin) if sizes is None else sizes

    def __len__(self):
        return len(self.sizes)


def product_table(tab):
    from syconn_amd.extraction.cs_processing_steps import OrganelleTable
    return OrganelleTable(tab['ids'], tab['cells'], tab['sizes'], tab['rep'], tab['verts'], tab['vert_begin'])


@pytest.mark.parametrize('prefix', ['a', 'b'])
def test_golden_end_to_end(gpu, g20, prefix):
    from syconn_amd.extraction.cs_processing_steps import map_objects_from_synssv_partners, synssv_o_features
    c = case(g20, prefix)
    tabs = {t: M.table(c[f'{t}_ids'], c[f'{t}_cells'], c[f'{t}_sizes'], c[f'{t}_rep'], c[f'{t}_verts'], c[f'{t}_vert_begin']) for t in TYPES}
    syn = Syn(c['syn_partners'], c['syn_rep'], c['syn_vox'], c['syn_vox_begin'], c['syn_sizes'])
    # the distances come from the config: mi 1000 / vc 500 / 4000 are the golden's
    m, stats = map_objects_from_synssv_partners(syn, {t: product_table(tabs[t]) for t in TYPES}, c['scaling'], device=gpu, return_stats=True)
    want = M.map_objects(c['syn_partners'], c['syn_rep'], c['syn_vox'], c['syn_vox_begin'], tabs, c['scaling'],
                         {t: float(c[f'R_{t}']) for t in TYPES}, float(c['D']))
    for t in TYPES:
        got = M.mapping_result(m, t)
        assert got['n_objs'].dtype == np.int32 and np.array_equal(got['n_objs'], c[f'n_{t}_objs']), t
        assert got['n_vxs'].dtype == np.int32 and np.array_equal(got['n_vxs'], c[f'n_{t}_vxs']), t
        assert got['min_dst'].dtype == np.float32 and got['min_dst'].tobytes() == c[f'min_dst_{t}_nm'].tobytes(), t
        side = np.repeat(np.arange(len(got['side_begin']) - 1), np.diff(got['side_begin']))
        assert np.array_equal(side, c[f'p_{t}_side']) and np.array_equal(got['pair_obj'], c[f'p_{t}_obj']), t
        assert np.array_equal(got['pair_close'], c[f'p_{t}_close']) and np.array_equal(got['pair_len'], c[f'p_{t}_len']), t
        assert np.sqrt(got['pair_min_d2']).tobytes() == c[f'p_{t}_min_dist'].tobytes(), t
        if prefix == 'a':                                        # exact arithmetic: one right answer for every d^2
            assert got['pair_min_d2'].tobytes() == want[t]['pair_min_d2'].tobytes(), t
        assert stats[t]['pairs'] == len(c[f'p_{t}_obj']) and stats[t]['work_items'] == stats[t]['pairs']
    assert synssv_o_features(syn, m, c['mesh_area']).tobytes() == c['features'].tobytes()
    d = m.as_dicts()
    assert d[3]['n_mi_vxs_1'] == c['n_mi_vxs'][3, 1] and d[5]['min_dst_vc_nm_0'].tobytes() == c['min_dst_vc_nm'][5, 0].tobytes()


def guarded_run(gpu, syn, tab, scaling, R, D, f):
    """Both entry points over scratches with a guard band behind what ``*_temp_bytes`` asks for.  -> PairList, counters."""
    import torch
    from syconn_amd.extraction.cs_processing_steps import _ObjectMapper
    mapper = _ObjectMapper(syn, M.scale64(scaling), f, gpu)

    def guard(need):
        g = torch.empty(need + 4096, dtype=torch.uint8, device=gpu)
        g[:need] = 0xCD
        g[need:] = 0xA5
        return g
    gp = guard(mapper.pair_tmp.numel())
    mapper.pair_tmp = gp[:mapper.pair_tmp.numel()]
    cand = mapper.candidates(product_table(tab), D)
    assert bool((gp[mapper.pair_tmp.numel():] == 0xA5).all()), 'sd_synssv_map_pairs wrote behind sd_synssv_map_pairs_temp_bytes'
    need = mapper.lib.sd_synssv_map_query_temp_bytes(mapper.n, mapper.n_sv, cand['P'])
    gq = guard(need)
    mapper.tmp, mapper.tmp_pairs, mapper.prepared = gq[:need], cand['P'], False
    pl, counters = mapper.query(cand, R)
    assert mapper.tmp.data_ptr() == gq.data_ptr() and mapper.prepared
    assert bool((gq[need:] == 0xA5).all()), 'sd_synssv_map_query wrote behind sd_synssv_map_query_temp_bytes'
    return pl, counters


def check_against_restatement(gpu, c, R, D, f, what):
    from syconn_amd.extraction.cs_processing_steps import build_synssv_mapping, map_objects_from_synssv_partners
    syn = Syn(c['partners'], c['rep'], c['vox'], c['vox_begin'])
    tabs = {t: product_table(tab) for t, tab in c['tables'].items()}
    want = M.map_objects(c['partners'], c['rep'], c['vox'], c['vox_begin'], c['tables'], c['scaling'], R, D, f)
    m, stats = map_objects_from_synssv_partners(syn, tabs, c['scaling'], max_vert_dist_nm=R, max_rep_coord_dist_nm=D, sample_fact=f, device=gpu,
                                                return_stats=True)
    for t in c['tables']:
        M.assert_result_equal(M.mapping_result(m, t), want[t], f'{what} {t}')
    return m, stats, want, tabs, syn


@pytest.mark.parametrize('seed, scaling, R, f', [
    (1, (10, 10, 20), {'mi': 1000, 'vc': 500}, 2),
    (2, (9, 9, 20), {'mi': 60, 'vc': 2500}, 3),                  # below the synapse extent / above everything
    (3, (4.5, 4, 40), {'mi': 120.5, 'vc': 800}, 1),
])
def test_random_against_restatement(gpu, seed, scaling, R, f):
    from syconn_amd.extraction.cs_processing_steps import build_synssv_mapping
    rng = np.random.default_rng(seed)
    c = M.random_case(rng, n_syn=14, scaling=scaling, extent=9, n_vert=(3, 300))
    assert c['tables']['mi']['verts'].min() < 0 and np.any(c['tables']['mi']['verts'] % 1 != 0)
    m, stats, want, tabs, syn = check_against_restatement(gpu, c, R, 4000, f, f'seed {seed}')
    for t in TYPES:
        assert want[t]['pair_close'].sum() > 0 and (want[t]['pair_close'] < want[t]['pair_len']).any() and np.isinf(want[t]['pair_min_d2']).any()
        pl, counters = guarded_run(gpu, syn, c['tables'][t], scaling, R[t], 4000, f)
        got = M.mapping_result(build_synssv_mapping(len(syn), {t: tabs[t]}, {t: pl}), t)
        M.assert_result_equal(got, want[t], f'guarded seed {seed} {t}')
        assert counters == stats[t]


def test_pruning_below_the_organelle_length(gpu):
    """A condition, not a measurement: with R well below the organelles' length the kernel must test strictly fewer point pairs than
    the product of sampled vertices and sampled voxels over all pairs, and still give the restatement's results."""
    rng = np.random.default_rng(7)
    c = M.random_case(rng, n_syn=10, scaling=(10, 10, 20), extent=9, n_vert=(200, 600), blob_nm=400, spread_nm=300, types=('mi',))
    m, stats, want, _, _ = check_against_restatement(gpu, c, 150, 4000, 2, 'pruning')
    assert want['mi']['pair_close'].sum() > 0
    assert 0 < stats['mi']['point_tests'] < want['mi']['product'], (stats['mi'], want['mi']['product'])
    assert stats['mi']['tiles_skipped'] + stats['mi']['vertices_rejected'] > 0


def line(x0, y0, z0, n, step=(0.0, 0.0, 1.0)):
    return np.array((x0, y0, z0), np.float64) + np.arange(n)[:, None] * np.asarray(step, np.float64)


def test_structure_edges(gpu):
    """f = 2.  Synapse k (cells 20 + k, 10 + k) has 63, 64, 65, 129 sampled voxels; cell 20 holds organelles of T - 1, T, T + 1 and
    2 T + 1 sampled vertices, cell 11 one of 2 T + 1 whose only close vertex is the last sampled one, cell 12 has 65 organelles."""
    rng = np.random.default_rng(11)
    scaling, f, R = (10, 10, 20), 2, 400
    partners, rep, vox = [], [], []
    for k, n_sampled in enumerate((63, 64, 65, 129)):
        n_vox = 2 * n_sampled - (k % 2)                          # odd and even voxel counts with the same ceil(n / 2)
        g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(2), indexing='ij'), -1).reshape(-1, 3)[:n_vox] + (500 * k, 40, 30)
        g = g[rng.permutation(len(g))]
        partners.append((20 + k, 10 + k))
        vox.append(g.astype(np.uint32))
        rep.append(g[0])
    centre = [v.astype(np.float64).mean(0) * np.array(scaling, np.float64) for v in vox]
    ids, cells, sizes, reps, verts = [], [], [], [], []

    def add(cell, k, v, size=1000):
        ids.append(100 + len(ids)); cells.append(cell); sizes.append(size); reps.append(rep[k]); verts.append(np.asarray(v, np.float32))
    for j, n_sampled in enumerate((T - 1, T, T + 1, 2 * T + 1)):
        add(20, 0, centre[0] + rng.normal(0, 350, (2 * n_sampled - (j % 2), 3)), size=777 + j)
    far = line(centre[1][0], centre[1][1], centre[1][2] + 5000, 2 * (2 * T + 1) - 1, (0.25, 0, 1))
    far[-1] = centre[1] + (0.5, 0.25, 300.125)                  # row 4 T: the last sampled vertex of the third item
    add(11, 1, far)
    for j in range(65):
        add(12, 2, centre[2] + rng.normal(0, 300, (3 + j % 4, 3)), size=10 + j)
    add(13, 3, centre[3] + rng.normal(0, 500, (300, 3)))
    add(23, 3, centre[3] + rng.normal(0, 500, (2 * T + 5, 3)))
    order = rng.permutation(len(ids))
    tab = M.table_from_lists(np.array(ids)[order], np.array(cells)[order], np.array(sizes)[order], np.array(reps)[order], [verts[j] for j in order])
    c = dict(partners=np.array(partners, np.uint64), rep=np.array(rep, np.int32), vox=np.concatenate(vox),
             vox_begin=np.concatenate(([0], np.cumsum([len(v) for v in vox]))), tables={'mi': tab}, scaling=np.array(scaling, np.float32))
    m, stats, want, _, _ = check_against_restatement(gpu, c, R, 4000, f, 'edges')
    w = want['mi']
    assert sorted(w['pair_len'][:4].tolist()) == [T - 1, T, T + 1, 2 * T + 1]                  # side 0 = cell 20
    k = int(np.flatnonzero(w['pair_len'] == 2 * T + 1)[-1])
    assert w['pair_close'][k] == 1 and np.sqrt(w['pair_min_d2'][k]) < R                          # the last vertex alone
    assert (np.diff(w['side_begin']) == 65).any() and m.n_mi_objs.max() > 40
    assert stats['mi']['work_items'] == int((-(-w['pair_len'] // T)).sum()) > stats['mi']['pairs']
    assert (-(-np.diff(c['vox_begin']) // 2)).tolist() == [63, 64, 65, 129]


def test_empty_inputs(gpu, g20):
    from syconn_amd.extraction.cs_processing_steps import OrganelleTable, map_objects_from_synssv_partners
    c = case(g20, 'b')
    tabs = {t: product_table(M.table(c[f'{t}_ids'], c[f'{t}_cells'], c[f'{t}_sizes'], c[f'{t}_rep'], c[f'{t}_verts'], c[f'{t}_vert_begin']))
            for t in TYPES}
    none = Syn(np.zeros((0, 2), np.uint64), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32), np.zeros(1, np.int64))
    m = map_objects_from_synssv_partners(none, tabs, c['scaling'], device=gpu)
    assert len(m) == 0 and m.n_vc_vxs.shape == (0, 2)
    syn = Syn(c['syn_partners'], c['syn_rep'], c['syn_vox'], c['syn_vox_begin'])
    n = len(syn)
    empty = OrganelleTable([], [], [], np.zeros((0, 3)), np.zeros((0, 3)), [0])
    unassigned = OrganelleTable(c['vc_ids'], np.zeros(len(c['vc_ids'])), c['vc_sizes'], c['vc_rep'], c['vc_verts'], c['vc_vert_begin'])
    foreign = OrganelleTable(c['vc_ids'], c['vc_cells'] + np.uint64(1000), c['vc_sizes'], c['vc_rep'], c['vc_verts'], c['vc_vert_begin'])
    m = map_objects_from_synssv_partners(syn, {'mi': tabs['mi'], 'er': empty, 'vc': unassigned, 'go': foreign}, c['scaling'],
                                         max_vert_dist_nm={'mi': 1000, 'er': 1, 'vc': 500, 'go': 500}, device=gpu)
    assert np.array_equal(m.n_mi_vxs, c['n_mi_vxs'])
    for t in ('er', 'vc', 'go'):
        assert not getattr(m, f'n_{t}_objs').any() and np.all(getattr(m, f'min_dst_{t}_nm') == np.float32(1e12))
        assert len(m.pairs[t].pair_obj) == 0 and len(m.pairs[t].side_begin) == 2 * n + 1
    # a candidate without a mesh is refused by name
    bare = OrganelleTable([4242], [int(c['syn_partners'][0, 0])], [5], c['syn_rep'][:1], np.zeros((0, 3)), [0, 0])
    with pytest.raises(ValueError, match='4242'):
        map_objects_from_synssv_partners(syn, {'mi': bare}, c['scaling'], device=gpu)


def test_behind_combine_and_split_syn(gpu):
    """The ``SynSsvTable`` of g19's input, with synthetic organelles around its synapses, against the restatement."""
    import _syn_ssv_ref as S
    from syconn_amd.extraction.cs_processing_steps import SynSsvTable, combine_and_split_syn
    g = {k[2:]: v for k, v in np.load(G19).items() if k.startswith('a_')}
    b = g['in_vox_begin']
    table = S.Table(g['in_syn_ids'], [g['in_vox'][b[i]:b[i + 1]] for i in range(len(g['in_syn_ids']))], g['in_sym_prop'], g['in_asym_prop'])
    t = combine_and_split_syn(table, g['map_sv'], g['map_ssv'], g['scaling'], device=gpu)
    assert type(t) is SynSsvTable and len(t) >= 5
    rng = np.random.default_rng(19)
    s = M.scale64(g['scaling'])
    lists = {k: [] for k in ('ids', 'cells', 'sizes', 'rep', 'verts')}
    for i in range(len(t)):
        v = t.voxels[t.vox_begin[i]:t.vox_begin[i + 1]].astype(np.float64) * s
        for cell in t.neuron_partners[i].tolist() + [0]:
            for _ in range(2):
                p = v.mean(0) + rng.normal(0, 500, 3) + rng.normal(0, 200, (int(rng.integers(5, 400)), 3))
                lists['ids'].append(7 * len(lists['ids']) + 1); lists['cells'].append(cell); lists['sizes'].append(int(rng.integers(0, 3000)))
                lists['rep'].append(np.maximum(np.round(p.mean(0) / s), 0)); lists['verts'].append(p.astype(np.float32))
    tab = M.table_from_lists(lists['ids'], lists['cells'], lists['sizes'], lists['rep'], lists['verts'])
    c = dict(partners=t.neuron_partners, rep=t.rep_coords, vox=t.voxels, vox_begin=t.vox_begin, tables={'mi': tab, 'vc': tab}, scaling=g['scaling'])
    from syconn_amd.extraction.cs_processing_steps import map_objects_from_synssv_partners, synssv_o_features
    want = M.map_objects(c['partners'], c['rep'], c['vox'], c['vox_begin'], c['tables'], c['scaling'], {'mi': 1000, 'vc': 500}, 4000, 2)
    m = map_objects_from_synssv_partners(t, {k: product_table(tab) for k in TYPES}, g['scaling'], device=gpu)      # the table itself
    for k in TYPES:
        M.assert_result_equal(M.mapping_result(m, k), want[k], f'g19 {k}')
    assert want['mi']['pair_close'].sum() > want['vc']['pair_close'].sum() > 0
    area = np.arange(len(t), dtype=np.float64) / 8
    assert synssv_o_features(t, m, area).tobytes() == M.features(t.sizes, area, want).tobytes()
