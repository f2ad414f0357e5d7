"""GPU: the synapse agglomeration (csrc/sd_syn_ssv.hip, ``extraction.cs_processing_steps``).

1. golden g19 (the reference's own ``connected_cluster_kdtree`` and ``_combine_and_split_syn_thread``): ``connected_cluster`` per
   group -- labels exact -- and ``combine_and_split_syn`` in both indexing modes: integer columns exact, float columns bit for bit (the
   host edge is the reference's arithmetic on exact counts);
2. randomised groups against the restatement tests/_syn_ssv_ref.py (pinned to g19 on the CPU), at several scalings and gaps, with
   negative coordinates and shuffled stored order;
3. end to end: the ``SynTable`` of ``extract_contact_sites`` on the box of the driver's test goes into ``combine_and_split_syn`` and is
   checked against the restatement fed the same table;
4. refusals and empty inputs."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _syn_ssv_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
G19 = os.path.join(HERE, 'golden', 'g19_syn_ssv.npz')


@pytest.fixture(scope='module')
def g19():
    return dict(np.load(G19))


def case(g, prefix):
    return {k[2:]: v for k, v in g.items() if k.startswith(prefix + '_')}


def golden_table(c):
    n = len(c['in_syn_ids'])
    b = c['in_vox_begin']
    return S.Table(c['in_syn_ids'], [c['in_vox'][b[i]:b[i + 1]] for i in range(n)], c['in_sym_prop'], c['in_asym_prop'])


@pytest.mark.parametrize('prefix', ['a', 'b'])
def test_connected_cluster_equals_golden(gpu, g19, prefix):
    from syconn_amd.extraction.cs_processing_steps import connected_cluster, filter_relevant_syn
    c = case(g19, prefix)
    keys, begin, rows = filter_relevant_syn(c['in_syn_ids'], c['map_sv'], c['map_ssv'])
    assert np.array_equal(keys, c['f_keys'])
    vb, lb = c['in_vox_begin'], c['labels_begin']
    n_multi = 0
    for g in range(len(keys)):
        lists = [c['in_vox'][vb[r]:vb[r + 1]] for r in rows[begin[g]:begin[g + 1]]]
        got = connected_cluster(lists, float(c['cs_gap_nm']), c['scaling'], device=gpu)
        want = c['labels'][lb[g]:lb[g + 1]]
        assert got.dtype == np.int32 and np.array_equal(got, want), (prefix, g)
        n_multi += int(want.max() > 0)
    assert n_multi >= 2


@pytest.mark.parametrize('prefix', ['a', 'b'])
def test_combine_and_split_syn_equals_golden(gpu, g19, prefix):
    from syconn_amd.extraction.cs_processing_steps import combine_and_split_syn
    c = case(g19, prefix)
    table = golden_table(c)
    for mode, ref_ix in (('r', True), ('x', False)):
        t = combine_and_split_syn(table, c['map_sv'], c['map_ssv'], c['scaling'], cs_gap_nm=float(c['cs_gap_nm']),
                                  min_obj_vx={'syn_ssv': int(c['min_obj_vx'])}, sym_thresh=float(c['sym_thresh']),
                                  reference_indexing=ref_ix, device=gpu)
        assert np.array_equal(t.neuron_partners, c['r_partners']) and np.array_equal(t.sizes, c['r_size'])
        assert np.array_equal(t.rep_coords, c['r_rep_coord']) and t.rep_coords.dtype == np.int32
        assert np.array_equal(t.bounding_boxes, c['r_bbox']) and np.array_equal(t.ordinal, c['r_component'])
        assert np.array_equal(t.cs_ids, c[f'{mode}_cs_ids']) and np.array_equal(t.cs_begin, c[f'{mode}_cs_begin'])
        assert np.array_equal(t.syn_sign, c[f'{mode}_syn_sign'])
        for k in ('sym_prop', 'asym_prop', 'syn_type_sym_ratio'):
            assert getattr(t, k).tobytes() == c[f'{mode}_{k}'].tobytes(), (mode, k)
        # the voxel runs: the golden partition in ascending flat index
        groups = S.groups_from_arrays(c['in_syn_ids'], c['in_vox'], c['in_vox_begin'], c['in_sym_prop'], c['in_asym_prop'], c['f_keys'],
                                      c['f_group_begin'], [c['in_syn_ids'].tolist().index(i) for i in c['f_syn_ids'].tolist()])
        labels = [c['labels'][c['labels_begin'][g]:c['labels_begin'][g + 1]] for g in range(len(groups))]
        want, _ = S.combine(groups, c['scaling'], float(c['cs_gap_nm']), int(c['min_obj_vx']), float(c['sym_thresh']), ref_ix, labels=labels)
        S.assert_rows_equal(t.as_dict(), want, f'{prefix} {mode}')
        fb = t.frag_begin.tolist()
        for i, r in enumerate(want):
            assert t.frag_ids[fb[i]:fb[i + 1]].tolist() == r['frag_ids'] and t.frag_counts[fb[i]:fb[i + 1]].tolist() == r['frag_counts']
    # the defaults come from the config: cs_gap_nm 250, min_obj_vx['syn_ssv'] 100, sym_thresh 0.225 are the golden's values
    d = combine_and_split_syn(table, dict(zip(c['map_sv'].tolist(), c['map_ssv'].tolist())), scaling=c['scaling'], device=gpu)
    S.assert_tables_equal(d, combine_and_split_syn(table, c['map_sv'], c['map_ssv'], c['scaling'], 250, 100, 0.225, device=gpu))
    assert np.array_equal(d.sizes, c['r_size'])


def random_groups(rng, n_groups, extent, max_frags=8, coord0=(0, 0, 0)):
    """Cell pairs with 1..max_frags fragments, each one or two random blobs (boxes with holes) inside `extent`, stored order shuffled."""
    groups = []
    for g in range(n_groups):
        frags = []
        org = np.asarray(coord0) + rng.integers(0, 2000, 3)
        for f in range(int(rng.integers(1, max_frags + 1))):
            parts = []
            for _ in range(int(rng.integers(1, 3))):
                lo = org + [int(rng.integers(0, e)) for e in extent]
                shape = rng.integers(1, 9, 3)
                box = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).reshape(-1, 3) + lo
                parts.append(box[rng.random(len(box)) < rng.choice([0.3, 0.7, 1.0])])
            vox = np.unique(np.concatenate(parts), axis=0)
            if not len(vox):
                vox = org[None] + f
            frags.append((((2 * g + 2) << 32) + 10 ** 6 + 1000 * g + f, vox[rng.permutation(len(vox))], float(rng.integers(0, 17)) / 16,
                          float(rng.integers(0, 17)) / 16))
        groups.append((((2 * g + 3) << 32) + 2 * g + 2, frags))
    return groups


def trim_to(groups, n_vox):
    """The same groups with every fragment cut to its first voxels in stored order (at least one) so that `n_vox` are left in all."""
    lens = np.array([len(f[1]) for _, fr in groups for f in fr])
    keep = np.maximum(1, lens * n_vox // lens.sum())
    i = 0
    while keep.sum() < n_vox:
        keep[i % len(keep)] += keep[i % len(keep)] < lens[i % len(keep)]
        i += 1
    assert keep.sum() == n_vox
    it = iter(keep.tolist())
    return [(k, [(f[0], f[1][:next(it)], f[2], f[3]) for f in fr]) for k, fr in groups]


def table_and_mapping(groups):
    """Every fragment of group g is the pair of supervoxels (2 g + 2, 10^6 + 1000 g + f) -> cells (2 g + 2, 2 g + 3)."""
    frags = [f for _, fr in groups for f in fr]
    mapping = {}
    for g, (_, fr) in enumerate(groups):
        mapping[2 * g + 2] = 2 * g + 2
        for f in fr:
            mapping[f[0] & 0xffffffff] = 2 * g + 3
    return S.Table([f[0] for f in frags], [f[1] for f in frags], [f[2] for f in frags], [f[3] for f in frags]), mapping


# seed -> (groups, most fragments per group, min_obj_vx, voxels in all) of the sets that are not 30 groups of up to 8 whole fragments
SMALL = {6: (4, 3, 3, 64)}


@pytest.mark.parametrize('seed, scale, gap, extent, coord0', [
    (1, (10, 10, 20), 250, (60, 60, 30), (0, 0, 0)),
    (2, (9, 9, 20), 250, (70, 70, 30), (5, 7, 11)),
    (3, (4, 4, 40), 120.5, (90, 90, 8), (100, 0, 3)),
    (4, (10, 10, 10), 20.5, (12, 12, 12), (0, 0, 0)),           # just above the two-voxel bound: cells of 2 x 2 x 2 voxels
    (5, (10, 10, 20), 1000, (200, 200, 100), (0, 0, 0)),
    (6, (10, 10, 10), 20.5, (6, 6, 6), (0, 0, 0)),              # SMALL: 64 voxels, the n + 1 cell starts cross 256 bytes of scratch
])
def test_random_groups_against_restatement(gpu, seed, scale, gap, extent, coord0):
    import torch
    from syconn_amd.extraction.cs_processing_steps import _Agglomerator, combine_and_split_syn, connected_cluster
    n_groups, max_frags, min_vx, n_vox = SMALL.get(seed, (30, 8, 40, None))
    rng = np.random.default_rng(seed)
    groups = random_groups(rng, n_groups, extent, max_frags=max_frags, coord0=coord0)
    if n_vox:
        groups = trim_to(groups, n_vox)
    table, mapping = table_and_mapping(groups)
    want, labels = S.combine(groups, scale, gap, min_vx, 0.225)
    assert sum(int(lab.max()) + 1 for lab in labels) > len(groups) + 5 and len(want) > 5       # splits and merges both happen
    got, info = combine_and_split_syn(table, mapping, scaling=scale, cs_gap_nm=gap, min_obj_vx=min_vx, sym_thresh=0.225, device=gpu,
                                      return_stats=True)
    assert got.n_components == sum(int(lab.max()) + 1 for lab in labels) == int(info['counts'][0])
    S.assert_rows_equal(got.as_dict(), want, f'seed {seed}')
    assert got.ordinal.tolist() == [r['component'] for r in want] and got.group.tolist() == [r['group'] for r in want]
    fb = got.frag_begin.tolist()
    for i, r in enumerate(want):
        assert got.frag_ids[fb[i]:fb[i + 1]].tolist() == r['frag_ids'] and got.frag_counts[fb[i]:fb[i + 1]].tolist() == r['frag_counts']
    for g in sorted({0, 7 % n_groups, n_groups - 1}):           # single groups, shifted to negative coordinates
        lists = [f[1].astype(np.int64) - 5000 for f in groups[g][1]]
        assert np.array_equal(connected_cluster(lists, gap, scale, device=gpu), labels[g]), (seed, g)
    # the launches once more over a scratch with a guard band behind it: both entry points are told sd_syn_ssv_temp_bytes(n) bytes
    frags = [f[1] for _, fr in groups for f in fr]
    agg = _Agglomerator(np.concatenate(frags), np.repeat(np.arange(len(frags)), [len(v) for v in frags]),
                        np.repeat(np.arange(n_groups), [len(fr) for _, fr in groups]), n_groups, scale, gap, gpu)
    assert n_vox in (None, agg.n)
    need = agg.tmp.numel()
    guarded = torch.empty(need + 4096, dtype=torch.uint8, device=gpu)
    guarded[:need] = 0xCD
    guarded[need:] = 0xA5
    agg.tmp = guarded[:need]
    agg.components()
    agg.read_counts()
    assert bool((guarded[need:] == 0xA5).all()), 'sd_syn_ssv_components wrote behind sd_syn_ssv_temp_bytes(n)'
    first = np.cumsum([0] + [int(lab.max()) + 1 for lab in labels])
    flat = np.concatenate([lab + o for lab, o in zip(labels, first)])
    assert np.array_equal(agg.labels(), flat)
    st = agg.stats(min_vx)
    assert bool((guarded[need:] == 0xA5).all()), 'sd_syn_ssv_stats wrote behind sd_syn_ssv_temp_bytes(n)'
    assert np.array_equal(st['comp_sizes'], np.bincount(flat)) and len(st['voxels']) == sum(len(r['voxels']) for r in want)


def test_refusals_and_empty(gpu):
    from syconn_amd.extraction.cs_processing_steps import combine_and_split_syn, connected_cluster
    assert connected_cluster([], 250, (10, 10, 20), device=gpu).shape == (0,)
    assert connected_cluster([np.zeros((0, 3), np.uint32)], 250, (10, 10, 20), device=gpu).shape == (0,)
    assert connected_cluster([np.array([[7, 7, 7]])], 250, (10, 10, 20), device=gpu).tolist() == [0]
    with pytest.raises(ValueError):
        connected_cluster([np.array([[1, 2, 3]])], 40, (10, 10, 20), device=gpu)
    empty = S.Table([], [], [], [])
    t = combine_and_split_syn(empty, {}, scaling=(10, 10, 20), device=gpu)
    assert len(t) == 0 and t.n_components == 0 and t.as_dict() == []
    one = S.Table([(5 << 32) + 6], [np.array([[1, 1, 1], [2, 2, 2]])], [0.5], [0.25])
    t = combine_and_split_syn(one, {5: 1, 6: 1}, scaling=(10, 10, 20), device=gpu)                # an intra-cell pair: nothing to do
    assert len(t) == 0
    t = combine_and_split_syn(one, {5: 1, 6: 2}, scaling=(10, 10, 20), min_obj_vx=2, device=gpu)
    assert len(t) == 1 and t.sizes.tolist() == [2] and t.neuron_partners.tolist() == [[2, 1]] and t.sym_prop.tolist() == [0.5]
    with pytest.raises(ValueError):
        combine_and_split_syn(one, {5: 1, 6: 2}, scaling=(10, 10, 20), cs_gap_nm=30, device=gpu)
    with pytest.raises(ValueError, match='Voxels not available'):
        combine_and_split_syn(S.Table([(5 << 32) + 6], [np.zeros((0, 3))], [0.5], [0.25]), {5: 1, 6: 2}, scaling=(10, 10, 20), device=gpu)


# ---- 3. end to end behind extract_contact_sites --------------------------------------------------------------------------------------
import test_gpu_cs_driver as DRV  # noqa: E402  (the synthetic working directory of the driver's test)

dataset = DRV.dataset
cached_contact_steps = DRV.cached_contact_steps


def test_end_to_end_behind_extract_contact_sites(gpu, dataset, tmp_path):
    from syconn_amd.extraction.cs_extraction_steps import SynTable
    from syconn_amd.extraction.cs_processing_steps import combine_and_split_syn, filter_relevant_syn
    with DRV.WorkDir(tmp_path, dataset, 'two_raw'):
        _, syn_t = DRV.run_driver(3, as_tables=True)
    assert type(syn_t) is SynTable and len(syn_t) > 3
    halves = np.unique(np.concatenate((syn_t.ids >> np.uint64(32), syn_t.ids & np.uint64(0xffffffff))))
    # three supervoxels per cell, every seventh supervoxel unmapped
    mapping = {int(sv): k // 3 + 1 for k, sv in enumerate(halves.tolist()) if k % 7 != 6}
    keys, begin, rows = filter_relevant_syn(syn_t.ids, mapping)
    assert 0 < len(rows) < len(syn_t) and (np.diff(begin) > 1).any()
    groups = S.groups_from_arrays(syn_t.ids, syn_t.voxels, syn_t.vox_begin, syn_t.sym_prop, syn_t.asym_prop, keys, begin, rows)
    for gap, min_vx in ((250, 5), (60, 3)):
        for ref_ix in (True, False):
            want, labels = S.combine(groups, (10, 10, 20), gap, min_vx, 0.225, ref_ix)
            got = combine_and_split_syn(syn_t, mapping, scaling=(10, 10, 20), cs_gap_nm=gap, min_obj_vx=min_vx, reference_indexing=ref_ix,
                                        device=gpu)
            S.assert_rows_equal(got.as_dict(), want, f'gap {gap}')
            assert got.ordinal.tolist() == [r['component'] for r in want] and got.n_components == sum(int(lab.max()) + 1 for lab in labels)
            assert len(want) > 0
    assert any(int(lab.max()) > 0 for lab in labels)            # the small gap splits something
