"""Golden vectors for the synapse agglomeration (``combine_and_split_syn``), produced by the REFERENCE'S OWN code:
``connected_cluster_kdtree``, ``_combine_and_split_syn_thread`` and ``filter_relevant_syn``
(/root/reference/syconn/extraction/cs_processing_steps.py:239-602), ``calc_center_of_mass`` (reps/segmentation_helper.py:650-673) and
``cs_id_to_partner_ids_vec`` (reps/connectivity_helper.py:27-31) are lifted by AST at generation time and run unchanged (networkx and
scipy's cKDTree included).  ``SegmentationDataset``, ``SuperSegmentationDataset``, ``AttributeDict``, ``VoxelStorageLazyLoading`` and
``MeshStorage`` are in-memory stand-ins that record what is stored; ``mesh_min_obj_vx`` is above every size, so the mesh branch never
runs.  Nothing compiled and no reference text is stored: inputs and outputs only, as flat arrays.

    python tests/golden/make_golden_syn_ssv.py      ->  tests/golden/g19_syn_ssv.npz

Two cases, prefixes ``a_`` (scaling 10, 10, 20) and ``b_`` (9, 9, 20); cs_gap_nm 250, min_obj_vx['syn_ssv'] 100, sym_thresh 0.225.
The inputs keep the reference deterministic: every group spans < 20000 nm (its ``dist_inter_object`` prefilter passes every pair),
every component has <= 1e5 voxels (no subsample in ``calc_center_of_mass``), the scales are integral (exact float64 products) and the
voxel nearest every centre of mass is unique by a margin (checked below).

Per case: ``in_syn_ids`` / ``in_sym_prop`` / ``in_asym_prop`` / ``in_vox`` / ``in_vox_begin`` (the syn objects in input order),
``map_sv`` / ``map_ssv`` (the supervoxel -> cell mapping), ``f_keys`` / ``f_group_begin`` / ``f_syn_ids`` (the filter's dict in its own
order), ``labels`` (the component of every voxel of every group in the flat order the worker builds, numbered by position in the list
``connected_cluster_kdtree`` returns) / ``labels_begin`` (per group), ``r_*`` the stored attributes row by row in storing order
(``r_ordinal`` = id - base id, ``r_component`` = the row's count among all components of the run) and ``x_*`` the same from the worker with ``enumerate(syn_ids[1:])`` started at 1 (the indexing the
worker intends; the one-token change is made on the AST's text at generation time)."""
import ast
import os
import sys
import tempfile
import types
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_cs import lift_function  # noqa: E402

REF = '/root/reference/syconn'
GAP, MIN_VX, SYM_THRESH = 250, 100, 0.225
MAX_MAPPED = 2 ** 32 - 10                      # the largest mapped supervoxel id; anything above it is zeroed by the filter


def blob(lo, shape, n=None, rng=None):
    """The first `n` voxels (scan order) of a box at `lo`; shuffled with `rng` (stored order need not be scan order)."""
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).reshape(-1, 3) + np.asarray(lo)
    g = g[:n] if n is not None else g
    if rng is not None:
        g = g[rng.permutation(len(g))]
    return g.astype(np.uint32)


class Maker:
    """Collects syn objects group by group and hands out supervoxel ids: cell k owns the supervoxels 100 k + t and a few large ones."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.objs = []                          # (syn id, voxels, sym_prop, asym_prop)
        self.map = {}
        self.next_sv = defaultdict(int)

    def sv(self, cell, big=False):
        t = self.next_sv[cell]
        self.next_sv[cell] += 1
        v = (2 ** 31 + 1000 * cell + t) if big else 100 * cell + t
        self.map[v] = cell
        return v

    def frag(self, cells, vox, sym=0.0, asym=0.0, big=(False, False), swap=False):
        a, b = self.sv(cells[0], big[0]), self.sv(cells[1], big[1])
        if swap:
            a, b = b, a
        self.objs.append(((a << 32) + b, np.asarray(vox, np.uint32), float(sym), float(asym)))

    def raw(self, sv_a, sv_b, vox):
        self.objs.append(((sv_a << 32) + sv_b, np.asarray(vox, np.uint32), 0.25, 0.5))


def case_a():
    m = Maker(19)
    rng = m.rng
    # G1, one fragment: a single component, sym + asym == 0 (ratio -1); supervoxel ids >= 2^31 in both halves
    m.frag((3, 4), blob((100, 100, 50), (6, 5, 5), 120, rng), 0.0, 0.0, big=(True, True))
    # G2, two fragments exactly at the gap in x (25 voxels between the nearest voxels): two components, 100 (kept) and 99 (dropped)
    m.frag((5, 6), blob((300, 100, 20), (7, 5, 3), 100), 0.5, 0.125)                  # x 300..306
    m.frag((5, 6), blob((331, 100, 20), (5, 5, 4), 99), 0.0, 0.75, swap=True)
    # G3, the same one lattice step inside the gap (24 voxels): one component of 199; fragments 0 and 1 share index 0
    m.frag((7, 8), blob((500, 100, 20), (5, 5, 4), 100, rng), 0.5, 0.125)
    m.frag((7, 8), blob((528, 100, 20), (5, 5, 4), 99, rng), 0.0625, 0.75)
    # G4, three fragments: (15, 20, 0) voxels = exactly 250 nm stays apart, (15, 19, 0) merges
    m.frag((9, 2), blob((700, 300, 30), (6, 6, 3), 101), 0.125, 0.5)             # occupies x 700..705, y 300..305
    m.frag((9, 2), blob((720, 325, 32), (6, 6, 3), 107), 0.25, 0.0)              # nearest corners (705, 305) -> (720, 325): (15, 20, 0)
    m.frag((9, 2), blob((680, 275, 30), (6, 7, 3), 110), 0.0, 0.25)              # (685, 281) -> (700, 300): (15, 19, 0)
    # G5, five fragments: fragment 0 in two pieces beyond the gap; the pieces of fragment 1 re-join through fragment 2;
    # fragment 3 merges with the second piece of fragment 0; fragment 4 stays alone and small
    m.frag((10, 11), np.concatenate((blob((900, 500, 40), (5, 5, 3), 70), blob((960, 500, 40), (5, 5, 3), 61))), 0.75, 0.0625)
    m.frag((10, 11), np.concatenate((blob((900, 560, 40), (4, 4, 4), 60), blob((934, 560, 40), (4, 4, 4), 50))), 0.0, 0.5)
    m.frag((10, 11), blob((910, 561, 41), (18, 2, 2), 72), 0.5, 0.5)
    m.frag((10, 11), blob((968, 507, 41), (4, 4, 3), 48), 0.03125, 0.875)
    m.frag((10, 11), blob((1100, 700, 60), (3, 3, 3), 27), 1.0, 0.0)
    # G6, seven fragments of random blobs; z steps of 12 (240 nm, merges) and 13 voxels (260 nm, apart) among them
    base = np.array((1300, 900, 100))
    m.frag((12, 13), blob(base, (6, 6, 3), 105, rng), 0.0, 0.9375)
    m.frag((12, 13), blob(base + (0, 0, 14), (6, 6, 2), 70, rng), 0.5, 0.25)          # z: 102 -> 114 = 12 voxels: merges
    m.frag((12, 13), blob(base + (0, 0, 28), (6, 6, 2), 66), 0.25, 0.25)              # z: 115 -> 128 = 13 voxels: apart
    for k in range(4):
        lo = base + (40, 0, 0) + rng.integers(0, 60, 3) * (1, 1, 0) + (0, 0, int(rng.integers(0, 30)))
        m.frag((12, 13), blob(lo, tuple(rng.integers(3, 7, 3)), None, rng), float(rng.integers(0, 9)) / 8, float(rng.integers(0, 9)) / 16)
    # G7, G8: one fragment each, the ratio on either side of sym_thresh
    m.frag((14, 15), blob((1600, 100, 10), (7, 5, 3), 103), 0.25, 0.75)                # 0.25 > 0.225: sign -1
    m.frag((18, 19), blob((1700, 100, 10), (7, 5, 3), 104), 0.125, 0.5)                # 0.2 <= 0.225: sign 1
    # rows the filter drops: an unmapped supervoxel, one above the largest mapped id, an intra-cell pair, supervoxel 0
    m.map[MAX_MAPPED] = 16
    m.raw(55555, m.sv(3), blob((10, 10, 10), (3, 3, 3)))
    m.raw(2 ** 32 - 3, m.sv(4), blob((20, 10, 10), (3, 3, 3)))
    m.raw(m.sv(5), m.sv(5), blob((30, 10, 10), (3, 3, 3)))
    m.raw(0, m.sv(6), blob((40, 10, 10), (3, 3, 3)))
    m.raw(MAX_MAPPED, m.sv(17), blob((50, 10, 10), (5, 5, 5)))                         # the largest mapped id itself is kept
    return m, (10, 10, 20)


def case_b():
    m = Maker(20)
    rng = m.rng
    # x: 28 voxels = 252 nm apart, 27 = 243 nm merges; (20, 0, 8): 240.8 nm merges, (20, 0, 9): 254.6 nm apart
    m.frag((2, 3), blob((100, 100, 50), (5, 5, 5), 110, rng), 0.5, 0.5)
    m.frag((2, 3), blob((132, 100, 50), (5, 5, 5), 104), 0.25, 0.0)                    # 104 -> 132: 28
    m.frag((2, 3), blob((73, 100, 50), (1, 5, 5), 21), 0.0, 0.25, swap=True)           # 73 -> 100: 27
    m.frag((4, 5), blob((300, 100, 50), (5, 5, 2), 50, rng), 0.125, 0.25)
    m.frag((4, 5), blob((324, 100, 59), (5, 5, 3), 61), 0.0, 0.0)                      # (304, ., 51) -> (324, ., 59): (20, 0, 8)
    m.frag((4, 5), blob((276, 100, 40), (5, 5, 2), 50), 0.5, 0.0)                      # (280, ., 41) -> (300, ., 50): (20, 0, 9)
    return m, (9, 9, 20)


class Store(dict):
    def __init__(self, *a, **kw):
        super().__init__()

    def push(self):
        pass

    def close(self):
        pass


def lift_patched(path, name, ns, old, new):
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            text = ast.unparse(node)
            assert text.count(old) == 1
            exec(compile(text.replace(old, new), path, 'exec'), ns)
            return ns[name]
    raise KeyError(name)


def run_case(m, scale, tmp):
    order = m.rng.permutation(len(m.objs))                     # input order: groups interleaved
    objs = [m.objs[i] for i in order]
    ids = np.array([o[0] for o in objs], np.uint64)
    assert len(np.unique(ids)) == len(ids)
    by_id = {int(o[0]): o for o in objs}
    map_sv = np.array(sorted(m.map), np.uint64)
    map_ssv = np.array([m.map[int(k)] for k in map_sv], np.int64)
    scaling = np.array(scale, dtype=np.float32)                # SegmentationDataset.scaling

    import scipy.spatial
    ns = {'np': np, 'defaultdict': defaultdict, 'os': os, 'spatial': scipy.spatial}
    exec('from typing import *', ns)
    exec('from logging import Logger', ns)
    ns.update(segmentation=types.SimpleNamespace(SegmentationDataset=object),            # the annotations of the lifted signatures
              super_segmentation=types.SimpleNamespace(SuperSegmentationDataset=object))
    for path, names in ((f'{REF}/reps/connectivity_helper.py', ['cs_id_to_partner_ids_vec']),
                        (f'{REF}/reps/segmentation_helper.py', ['calc_center_of_mass']),
                        (f'{REF}/extraction/cs_processing_steps.py', ['connected_cluster_kdtree', 'filter_relevant_syn',
                                                                       '_combine_and_split_syn_thread'])):
        for name in names:
            lift_function(path, name, ns)
    so_path = f'{tmp}/syn_ssv_0/so_storage'

    class Syn:
        def __init__(self, ix):
            _, self.voxel_list, sym, asym = by_id[int(ix)]
            self.attr_dict = dict(cs_id=ix, sym_prop=sym, asym_prop=asym)

        def load_attr_dict(self):
            pass

    class SD:
        def __init__(self, obj_type, **kw):
            self.type, self.scaling, self.n_folders_fs, self.version, self.ids = obj_type, scaling, 1000, 0, ids
            self.so_storage_path = so_path

        def get_segmentation_object(self, ix):
            if self.type == 'syn':
                return Syn(ix)
            return types.SimpleNamespace(id=ix, attr_dict_path=so_path + '/0/' + 'attr_dict.pkl')

    class Config(dict):
        use_new_subfold = True
    cfg = Config(meshes={'meshing_props_points': {'syn_ssv': {}}, 'mesh_min_obj_vx': 10 ** 9},
                 cell_objects={'min_obj_vx': {'syn_ssv': MIN_VX}, 'sym_thresh': SYM_THRESH},
                 cell_contacts={'min_path_length_partners': None})
    ssd = types.SimpleNamespace(mapping_lookup_reverse=types.SimpleNamespace(id_array=map_sv),
                                sv2ssv_ids=lambda svs, nb_cpus=1: {int(s): m.map[int(s)] for s in svs if int(s) in m.map})
    log = types.SimpleNamespace(debug=lambda *a: None, info=lambda *a: None, warning=lambda *a: None)
    stores = []

    def store(*a, **kw):
        stores.append(Store())
        return stores[-1]
    ccs_seen = []
    cck = ns['connected_cluster_kdtree']

    def recording_cck(voxel_coords, **kw):
        assert kw['dist_inter_object'] == 20000
        flat = np.concatenate(voxel_coords) * kw['scale']
        assert np.linalg.norm(flat.max(0) - flat.min(0)) < 20000           # every pair passes the prefilter
        ccs = cck(voxel_coords, **kw)
        ccs_seen.append((sum(len(v) for v in voxel_coords), ccs))
        return ccs
    ns.update(segmentation=types.SimpleNamespace(SegmentationDataset=SD), global_params=types.SimpleNamespace(config=cfg),
              ch=types.SimpleNamespace(cs_id_to_partner_ids_vec=ns['cs_id_to_partner_ids_vec']), sm=types.SimpleNamespace(cpu_count=lambda: 1),
              seghelp=types.SimpleNamespace(calc_center_of_mass=ns['calc_center_of_mass']), log_extraction=log,
              ix_from_subfold=lambda p, n: np.uint(0), VoxelStorageLazyLoading=store, AttributeDict=store, MeshStorage=store,
              connected_cluster_kdtree=recording_cck)
    lookup = ns['filter_relevant_syn'](SD('syn'), ssd, log)
    items = list(lookup.items())
    out = dict(in_syn_ids=ids, in_sym_prop=np.array([o[2] for o in objs]), in_asym_prop=np.array([o[3] for o in objs]),
               in_vox=np.concatenate([o[1] for o in objs]), in_vox_begin=np.concatenate(([0], np.cumsum([len(o[1]) for o in objs]))),
               map_sv=map_sv, map_ssv=map_ssv, scaling=scaling, cs_gap_nm=np.array(GAP), min_obj_vx=np.array(MIN_VX),
               sym_thresh=np.array(SYM_THRESH))
    out['f_keys'] = np.array([int(k) for k, _ in items], np.uint64)
    out['f_group_begin'] = np.concatenate(([0], np.cumsum([len(v) for _, v in items])))
    out['f_syn_ids'] = np.array([int(i) for _, v in items for i in v], np.uint64)

    def worker(prefix, fn):
        del stores[:], ccs_seen[:]
        fn((tmp, items, ['/0/'], 0, 0, GAP))
        voxel_dc, attr_dc, mesh_dc = stores
        assert list(voxel_dc) == list(attr_dc) and len(attr_dc) >= 3 and max(int(k) for k in attr_dc) < 1000
        A = list(attr_dc.values())
        assert all(a['mesh_area'] == 0 for a in A)
        out[f'{prefix}_ordinal'] = np.array([int(k) for k in attr_dc], np.int64)
        out[f'{prefix}_partners'] = np.array([a['neuron_partners'] for a in A]).astype(np.uint64)
        out[f'{prefix}_size'] = np.array([a['size'] for a in A], np.int64)
        out[f'{prefix}_rep_coord'] = np.array([a['rep_coord'] for a in A])
        assert out[f'{prefix}_rep_coord'].dtype == np.int32
        out[f'{prefix}_bbox'] = np.array([a['bounding_box'] for a in A])
        out[f'{prefix}_cs_ids'] = np.array([int(i) for a in A for i in a['cs_ids']], np.uint64)
        out[f'{prefix}_cs_begin'] = np.concatenate(([0], np.cumsum([len(a['cs_ids']) for a in A])))
        for k in ('sym_prop', 'asym_prop', 'syn_type_sym_ratio'):
            out[f'{prefix}_{k}'] = np.array([float(a[k]) for a in A], np.float64)
        out[f'{prefix}_syn_sign'] = np.array([a['syn_sign'] for a in A], np.int64)
        return voxel_dc, A

    voxel_dc, A = worker('r', ns['_combine_and_split_syn_thread'])
    # the partition, and what the worker stored against it
    # A dropped component leaves the loop body by ``continue`` before ``syn_ssv_id`` is advanced (:462-463, :514-515): ids count the
    # stored rows only.  ``r_component`` is the count among all components.
    labels, begin, component, row, r_component, ties = [], [0], 0, 0, [], []
    stored = {int(k): v for k, v in voxel_dc.items()}
    for (key, syn_ids), (n, ccs) in zip(items, ccs_seen):
        flat = np.concatenate([by_id[int(i)][1] for i in syn_ids])
        assert n == len(flat)
        lab = np.full(n, -1, np.int32)
        for c, cc in enumerate(ccs):
            members = np.array(sorted(cc))
            lab[members] = c
            assert len(cc) <= 100000
            if len(cc) >= MIN_VX:
                assert sorted(map(tuple, stored[row].tolist())) == sorted(map(tuple, flat[members].tolist()))
                # the voxel nearest the centre of mass must be unique by a margin, whatever the tie rule of the tree
                p = flat[members] * scaling
                d = np.sort(np.linalg.norm(p - p.mean(0), axis=1))
                if not (len(d) == 1 or d[1] - d[0] > 1e-6):
                    ties.append((int(key), c, len(cc), d[:3].tolist()))
                r_component.append(component)
                row += 1
            component += 1
        assert lab.min() == 0
        labels.append(lab)
        begin.append(begin[-1] + n)
    assert not ties, f'move a voxel: the nearest voxel to the centre of mass is not unique in {ties}'
    assert row == len(stored) < component and np.array_equal(out['r_ordinal'], np.arange(row))
    out['r_component'] = np.array(r_component, np.int64)
    out['labels'], out['labels_begin'] = np.concatenate(labels), np.array(begin)
    fixed = lift_patched(f'{REF}/extraction/cs_processing_steps.py', '_combine_and_split_syn_thread', ns, 'enumerate(syn_ids[1:])',
                         'enumerate(syn_ids[1:], 1)')
    worker('x', fixed)
    for k in ('ordinal', 'partners', 'size', 'rep_coord', 'bbox'):
        assert np.array_equal(out[f'x_{k}'], out[f'r_{k}'])
        del out[f'x_{k}']
    assert not np.array_equal(out['x_cs_ids'], out['r_cs_ids']) and not np.array_equal(out['x_sym_prop'], out['r_sym_prop'])
    return out


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for prefix, make in (('a', case_a), ('b', case_b)):
            m, scale = make()
            os.makedirs(f'{tmp}/{prefix}')
            res = run_case(m, scale, f'{tmp}/{prefix}')
            out.update({f'{prefix}_{k}': v for k, v in res.items()})
            n_groups = len(res['f_keys'])
            print(prefix, n_groups, 'groups,', len(res['in_syn_ids']), 'syn objects,', len(res['in_vox']), 'voxels,', len(res['r_size']),
                  'rows, ratios', np.round(res['r_syn_type_sym_ratio'], 3).tolist(), 'sizes', res['r_size'].tolist())
    a = {k[2:]: v for k, v in out.items() if k.startswith('a_')}
    # the inputs must exercise what they are meant to
    per_group = np.diff(a['f_group_begin']).tolist()
    assert {1, 2, 3}.issubset(per_group) and max(per_group) >= 5
    assert (a['r_size'] == MIN_VX).any() and (a['r_size'] > MIN_VX).any()
    assert (a['r_syn_type_sym_ratio'] == -1).any() and (a['r_syn_sign'] == -1).any() and (a['r_syn_sign'] == 1).any()
    r = a['r_syn_type_sym_ratio']
    assert ((r > SYM_THRESH) & (r < 0.3)).any() and ((r > 0.15) & (r <= SYM_THRESH)).any()
    assert (a['in_syn_ids'] >= 2 ** 63).any() and ((a['in_syn_ids'] & np.uint64(0xffffffff)) >= 2 ** 31).any()
    assert len(a['f_syn_ids']) < len(a['in_syn_ids'])
    path = os.path.join(HERE, 'g19_syn_ssv.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
