"""Golden vectors for the organelle mapping (``map_objects_from_synssv_partners``), produced by the REFERENCE'S OWN code:
``_map_objects_from_synssv_partners_thread``, ``_map_objects_from_synssv``, ``_objects_from_cell_to_syn_dict`` and
``synssv_o_features`` (/root/reference/syconn/extraction/cs_processing_steps.py:888-1093, :1404-1424) are lifted by AST at generation
time and run unchanged, scipy's cKDTree included.  ``SegmentationDataset``, ``SuperSegmentationDataset``, ``AttributeDict``,
``load_so_meshes_bulk`` and ``global_params.config`` are in-memory stand-ins.  Nothing compiled and no reference text is stored:
inputs and outputs only, as flat arrays.

    python tests/golden/make_golden_synssv_map.py      ->  tests/golden/g20_synssv_map.npz

Two cases, prefixes ``a_`` and ``b_``; max_vert_dist_nm mi 1000 / vc 500, max_rep_coord_dist_nm 4000 (the reference's defaults).

``a``: scaling (10, 10, 20), every vertex coordinate a multiple of 1/8 nm: every squared distance is exact in float64, so decisions at
exactly R and D are the same in every correct implementation.  It holds (checked in ``main``): a vertex at exactly R (not close)
and one lattice step inside, a representative coordinate at exactly D (candidate) and one step beyond, odd and even voxel and
vertex counts, an organelle of size 0 with close vertices, an organelle of another cell that is nearer, a cell without organelles
of one type, a side with candidates but none close, a synapse of one voxel, different results for slot 0 and slot 1, a cell
without synapses.
``b``: scaling (9, 9, 20), random float32 vertices, some negative.  No point decision lies within a relative 1e-6 of R^2 or D^2.
In both, every side's ``n_vxs`` sum either has a fractional part in [1e-6, 1 - 1e-6] or is made of terms whose sum is exact in any
order: the result does not depend on the traversal order of the tree.

Per case, inputs: ``syn_ids`` / ``syn_partners`` (n, 2) / ``syn_sizes`` / ``syn_rep`` / ``syn_vox`` / ``syn_vox_begin`` / ``mesh_area``,
``scaling`` (float32), per type t ``{t}_ids`` / ``{t}_cells`` / ``{t}_sizes`` / ``{t}_rep`` / ``{t}_verts`` / ``{t}_vert_begin``, ``R_{t}``, ``D``.
Outputs: ``n_{t}_objs`` / ``n_{t}_vxs`` int32 (n, 2), ``min_dst_{t}_nm`` float32 (n, 2) as ``_objects_from_cell_to_syn_dict`` wrote them,
``features`` float64 (n, 14), and per type the calls of ``_map_objects_from_synssv`` pair by pair, sorted by (side, organelle row):
``p_{t}_side`` / ``p_{t}_obj`` / ``p_{t}_close`` / ``p_{t}_len`` / ``p_{t}_min_dist`` (what ``cKDTree.query`` gave for the pair: the count
of finite distances, the number of queried vertices, the smallest distance or inf)."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_cs import lift_function  # noqa: E402

REF = '/root/reference/syconn'
R = {'mi': 1000, 'vc': 500}
D = 4000
TYPES = ('mi', 'vc')


def blob(lo, shape, n=None, rng=None):
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).reshape(-1, 3) + np.asarray(lo)
    g = g[:n] if n is not None else g
    if rng is not None:
        g = g[rng.permutation(len(g))]
    return g.astype(np.uint32)


class Maker:
    def __init__(self, seed, scale):
        self.rng = np.random.default_rng(seed)
        self.scale = np.array(scale, np.float32)
        self.syn = []                               # (partners, voxels, rep)
        self.org = {t: [] for t in TYPES}           # (cell, size, rep, vertices)

    def synapse(self, cells, vox, rep=None):
        vox = np.asarray(vox, np.uint32)
        self.syn.append(((max(cells), min(cells)), vox, np.asarray(vox[len(vox) // 2] if rep is None else rep, np.int32)))
        return len(self.syn) - 1

    def organelle(self, t, cell, size, rep, verts):
        self.org[t].append((cell, size, np.asarray(rep, np.int32), np.asarray(verts, np.float32).reshape(-1, 3)))

    def rep_of(self, verts):
        """A representative voxel coordinate near the vertices' centre."""
        return np.maximum(np.round(np.asarray(verts, np.float64).mean(0) / self.scale), 0).astype(np.int32)

    def cloud(self, centre_nm, radius_nm, n, lattice):
        """`n` vertices around `centre_nm`: on the 1/8 nm lattice (exact arithmetic) or plain float32."""
        p = np.asarray(centre_nm, np.float64) + self.rng.normal(0, radius_nm, (n, 3))
        return (np.round(p * 8) / 8 if lattice else p).astype(np.float32)


def case_a():
    m = Maker(201, (10, 10, 20))
    rng = m.rng
    # S0, cells (2, 1): 3 x 3 x 2 voxels in scan order: the even rows are the z = 50 layer -> sampled points x, y in {1000, 1010, 1020}, z 1000
    m.synapse((2, 1), blob((100, 100, 50), (3, 3, 2)), rep=(101, 101, 50))
    # S1, cells (3, 1): one voxel
    m.synapse((3, 1), blob((300, 100, 50), (1, 1, 1)), rep=(300, 100, 50))
    # S2, cells (3, 2): 15 voxels (odd), shuffled
    m.synapse((3, 2), blob((100, 300, 50), (5, 3, 1), None, rng), rep=(102, 301, 50))
    # S3, cells (5, 4): 32 voxels
    m.synapse((5, 4), blob((500, 500, 100), (4, 4, 2)), rep=(501, 501, 100))
    # cell 1, mi.  mA: rep at exactly D = 4000 nm from S0's (400 voxels in x); row 0 at exactly R = 1000 nm from the sampled voxel
    # (1020, 1010, 1000), row 1 (odd, never sampled) 10 nm away, row 2 one lattice step inside R, rows 3 and 4 far: close 1 of 3
    m.organelle('mi', 1, 300, (501, 101, 50), [(2020, 1010, 1000), (1030, 1010, 1000), (2019.875, 1010, 1000), (2600, 1010, 1000),
                                                 (2700, 1010, 1000)])
    # mB: rep one voxel beyond D from S0's; its vertices touch S0
    m.organelle('mi', 1, 500, (502, 101, 50), [(1000, 1000, 1000), (1010, 1010, 1000.125), (1020, 1020, 1001), (1000, 1020, 999.5)])
    # mC: size 0, every vertex close to S0
    m.organelle('mi', 1, 0, (105, 101, 50), [(1100, 1000, 1000), (1100, 1010, 1000), (1100, 1020, 1010), (1100.5, 1020, 1010)])
    # mD: belongs to cell 7 (which has no synapse) and is nearer to S0 than any organelle of cells 1 and 2
    m.organelle('mi', 7, 900, (101, 101, 51), [(1010, 1010, 1002.5), (1010, 1010, 1003), (1012, 1010, 1003)])
    # cell 2, mi: a candidate of S0 without a close vertex (2500 nm and more); cell 2 has no vc at all
    m.organelle('mi', 2, 700, (101, 300, 50), [(1010, 3500, 1000), (1010, 3600, 1000), (1010, 3700.125, 1000), (1010, 3800, 1000)])
    # cell 1, vc: one inside R = 500 of S0 (at exactly 500 in z from the z = 1000 layer: not close; the second row 0.125 inside)
    m.organelle('vc', 1, 64, (101, 101, 75), [(1010, 1010, 1500), (1010, 1010, 1499.875), (1010, 1010, 1600), (1010, 1010, 1700)])
    # further synapses on a coarse grid, and random organelles of both types around them, on the 1/8 nm lattice
    cells = [(1, 2), (1, 3), (2, 3), (4, 5), (4, 6), (5, 6), (3, 4), (2, 6)]
    for k in range(14):
        lo = np.array((150 + 330 * (k % 4), 700 + 330 * (k // 4), 40 + 7 * k))
        shape = tuple(rng.integers(1, 6, 3))
        n = int(rng.integers(1, int(np.prod(shape)) + 1))
        pair = cells[k % len(cells)]
        s = m.synapse(pair, blob(lo, shape, n, rng))
        centre = m.syn[s][1].astype(np.float64).mean(0) * m.scale
        for t in TYPES:
            for cell in pair:
                for _ in range(int(rng.integers(0, 3 if t == 'mi' else 4)) if (t, cell) != ('vc', 2) else 0):      # cell 2 stays without vc
                    off = rng.normal(0, 900 if t == 'mi' else 250, 3)
                    v = m.cloud(centre + off, 250 if t == 'mi' else 90, int(rng.integers(3, 120 if t == 'mi' else 40)), lattice=True)
                    m.organelle(t, cell, int(rng.integers(1, 5000)), m.rep_of(v), v)
    return m


def case_b():
    m = Maker(202, (9, 9, 20))
    rng = m.rng
    cells = [(1, 2), (1, 3), (2, 3), (4, 2), (4, 3)]
    for k in range(18):
        lo = np.array((5 + 300 * (k % 4), 3 + 300 * (k // 4), 1 + 9 * k))       # the first ones sit at the origin: negative vertices
        shape = tuple(rng.integers(1, 7, 3))
        n = int(rng.integers(1, int(np.prod(shape)) + 1))
        pair = cells[k % len(cells)]
        s = m.synapse(pair, blob(lo, shape, n, rng))
        centre = m.syn[s][1].astype(np.float64).mean(0) * m.scale
        for t in TYPES:
            for cell in pair:
                for _ in range(int(rng.integers(0, 3 if t == 'mi' else 4))):
                    off = rng.normal(0, 1000 if t == 'mi' else 280, 3)
                    v = m.cloud(centre + off, 300 if t == 'mi' else 100, int(rng.integers(3, 150 if t == 'mi' else 40)), lattice=False)
                    m.organelle(t, cell, int(rng.integers(1, 5000)), m.rep_of(v), v)
    return m


class Store(dict):
    def push(self):
        pass


def run_case(m):
    import scipy.spatial
    rng = m.rng
    scaling = m.scale
    n = len(m.syn)
    syn_ids = (1000 + rng.permutation(n)).astype(np.uint64)
    partners = np.array([s[0] for s in m.syn], np.uint64)
    syn_rep = np.array([s[2] for s in m.syn], np.int32)
    syn_sizes = np.array([len(s[1]) for s in m.syn], np.int64)
    mesh_area = np.round(rng.random(n) * 4, 3)
    tab = {}
    for k, t in enumerate(TYPES):
        order = rng.permutation(len(m.org[t]))                     # table order is not cell order
        o = [m.org[t][i] for i in order]
        tab[t] = dict(ids=(5000 * (k + 1) + 7 * rng.permutation(len(o))).astype(np.uint64), cells=np.array([x[0] for x in o], np.uint64),
                      sizes=np.array([x[1] for x in o], np.int64), rep=np.array([x[2] for x in o], np.int32).reshape(-1, 3),
                      verts=[x[3] for x in o])
    ssv_ids = np.arange(1, int(max(partners.max(), max(tab[t]['cells'].max() for t in TYPES))) + 1)
    stores = {}

    class Obj:
        def __init__(self, sd, ix):
            self.id, self.type, self._size, self._mesh = ix, sd.type, None, None
            if sd.type == 'syn_ssv':
                row = int(np.flatnonzero(syn_ids == ix)[0])
                self.voxel_list, self.scaling, self._size, self.mesh_area = m.syn[row][1], scaling, int(syn_sizes[row]), float(mesh_area[row])
                self.attr_dict = stores['/so/attr_dict.pkl'][ix]

        def load_attr_dict(self):
            pass

        @property
        def mesh(self):
            return self._mesh

        @property
        def size(self):
            return self._size

    class SD:
        def __init__(self, obj_type, working_dir=None, version=None, **kw):
            self.type, self.scaling = obj_type, scaling
            if obj_type == 'syn_ssv':
                self.ids, self.rep_coords, self.so_dir_paths = syn_ids, syn_rep, ['/so']
            else:
                self.ids, self.sizes, self.rep_coords = tab[obj_type]['ids'], tab[obj_type]['sizes'], tab[obj_type]['rep']

        def load_numpy_data(self, name):
            assert name == 'neuron_partners'
            return partners

        def get_segmentation_object(self, ix):
            return Obj(self, ix) if np.ndim(ix) == 0 else [Obj(self, i) for i in ix]

    def meshes(objs, use_new_subfold=True):
        out = {}
        for o in objs:
            v = tab[o.type]['verts'][int(np.flatnonzero(tab[o.type]['ids'] == o.id)[0])]
            out[o.id] = (np.zeros(0, np.uint32), v.reshape(-1).copy(), np.zeros(0, np.float32))
        return out

    class Config(dict):
        use_new_subfold = True
    cfg = Config(cell_objects={'max_vert_dist_nm': dict(R), 'max_rep_coord_dist_nm': D})

    class SSD:
        def __init__(self, working_dir=None, version=None, **kw):
            self.ssv_ids, self.config = ssv_ids, cfg

        def get_super_segmentation_object(self, ssv_id):
            return types.SimpleNamespace(ssv_dir=f'/nowhere/ssv/{int(ssv_id)}', **{f'{t}_ids': tab[t]['ids'][tab[t]['cells'] == ssv_id]
                                                                                  for t in TYPES})
    stores['/so/attr_dict.pkl'] = Store({i: dict(neuron_partners=partners[k]) for k, i in enumerate(syn_ids)})

    def attribute_dict(path, **kw):
        return stores.setdefault(path, Store())
    log = types.SimpleNamespace(debug=lambda *a: None, info=lambda *a: None, error=lambda *a: None)
    ns = {'np': np, 'os': os, 'spatial': scipy.spatial}
    exec('from typing import *', ns)
    ns.update(segmentation=types.SimpleNamespace(SegmentationDataset=SD, SegmentationObject=object),
              super_segmentation=types.SimpleNamespace(SuperSegmentationDataset=SSD), global_params=types.SimpleNamespace(config=cfg),
              seghelp=types.SimpleNamespace(load_so_meshes_bulk=meshes), AttributeDict=attribute_dict, log_extraction=log)
    path = f'{REF}/extraction/cs_processing_steps.py'
    for name in ('_map_objects_from_synssv', '_map_objects_from_synssv_partners_thread', '_objects_from_cell_to_syn_dict', 'synssv_o_features'):
        lift_function(path, name, ns)
    inner = ns['_map_objects_from_synssv']
    calls = {t: [] for t in TYPES}

    def recording(synssv_o, seg_objs, max_vert_dist_nm, sample_fact=2):
        res = inner(synssv_o, seg_objs, max_vert_dist_nm, sample_fact)
        row = int(np.flatnonzero(syn_ids == synssv_o.id)[0])
        tree = scipy.spatial.cKDTree(synssv_o.voxel_list[::sample_fact] * synssv_o.scaling)
        for o in seg_objs:
            assert R[o.type] == max_vert_dist_nm
            orow = int(np.flatnonzero(tab[o.type]['ids'] == o.id)[0])
            slot = int(np.flatnonzero(partners[row] == tab[o.type]['cells'][orow])[0])
            ds, _ = tree.query(o.mesh[1].reshape(-1, 3)[::sample_fact], distance_upper_bound=max_vert_dist_nm)
            calls[o.type].append((2 * row + slot, orow, int(np.sum(ds < np.inf)), len(ds), float(np.min(ds)), o.size))
        return res
    ns['_map_objects_from_synssv'] = recording
    ns['_map_objects_from_synssv_partners_thread'](('/nowhere', 0, 0, ssv_ids, D))
    ns['_objects_from_cell_to_syn_dict']((['/so'], '/nowhere', 0, 0))
    attr = stores['/so/attr_dict.pkl']
    out = dict(syn_ids=syn_ids, syn_partners=partners, syn_sizes=syn_sizes, syn_rep=syn_rep, syn_vox=np.concatenate([s[1] for s in m.syn]),
               syn_vox_begin=np.concatenate(([0], np.cumsum(syn_sizes))), mesh_area=mesh_area, scaling=scaling, D=np.array(D))
    for t in TYPES:
        out.update({f'{t}_ids': tab[t]['ids'], f'{t}_cells': tab[t]['cells'], f'{t}_sizes': tab[t]['sizes'], f'{t}_rep': tab[t]['rep'],
                    f'{t}_verts': np.concatenate(tab[t]['verts']), f'R_{t}': np.array(R[t]),
                    f'{t}_vert_begin': np.concatenate(([0], np.cumsum([len(v) for v in tab[t]['verts']])))})
        for name, dt in ((f'n_{t}_objs', np.int32), (f'n_{t}_vxs', np.int32), (f'min_dst_{t}_nm', np.float32)):
            col = [[attr[i][f'{name}_{p}'] for p in (0, 1)] for i in syn_ids]
            assert all(v.dtype == dt for r in col for v in r), name
            out[name] = np.array(col, dt)
        c = sorted(calls[t])
        assert len({(a[0], a[1]) for a in c}) == len(c)
        for j, (name, dt) in enumerate((('side', np.int64), ('obj', np.int64), ('close', np.int64), ('len', np.int64), ('min_dist', np.float64))):
            out[f'p_{t}_{name}'] = np.array([a[j] for a in c], dt)
        out[f'p_{t}_size'] = np.array([a[5] for a in c], np.int64)
    feats = [ns['synssv_o_features'](Obj(SD('syn_ssv'), i)) for i in syn_ids]
    out['features'] = np.array(feats, np.float64)
    assert out['features'].shape == (n, 14)
    return out


def check_case(c, exact):
    """The properties that make the reference's result independent of its traversal order and of rounding at the radii."""
    s = c['scaling'].astype(np.float64)
    n = len(c['syn_ids'])
    for t in TYPES:
        if exact:
            v8 = c[f'{t}_verts'].astype(np.float64) * 8
            assert np.array_equal(v8, np.round(v8)) and np.abs(v8).max() < 2 ** 24 and np.array_equal(s, np.round(s))
        # every (side, organelle of the side's cell): the rep decision, and for candidates every sampled vertex's decision
        cand = 0
        for side in range(2 * n):
            i, cell = side // 2, c['syn_partners'][side // 2, side % 2]
            P = c['syn_vox'][c['syn_vox_begin'][i]:c['syn_vox_begin'][i + 1]][::2].astype(np.float64) * s
            for o in np.flatnonzero(c[f'{t}_cells'] == cell).tolist():
                d2 = (((c[f'{t}_rep'][o] * s - c['syn_rep'][i] * s)) ** 2).sum()
                assert exact or abs(d2 / D ** 2 - 1) > 1e-6
                if d2 <= D ** 2:
                    cand += 1
                    V = c[f'{t}_verts'][c[f'{t}_vert_begin'][o]:c[f'{t}_vert_begin'][o + 1]][::2].astype(np.float64)
                    best = ((V[:, None, :] - P[None]) ** 2).sum(-1).min(1)
                    assert exact or np.all(np.abs(best / float(c[f'R_{t}']) ** 2 - 1) > 1e-6)
        assert cand == len(c[f'p_{t}_side']), (t, cand, len(c[f'p_{t}_side']))
        # the n_vxs sums
        x = (c[f'p_{t}_close'] / c[f'p_{t}_len']) * c[f'p_{t}_size']
        for side in np.unique(c[f'p_{t}_side']).tolist():
            terms = x[c[f'p_{t}_side'] == side]
            if len(terms) > 2:                                 # a + b == b + a: two terms have no order
                frac = np.sum(terms) % 1
                order_free = np.array_equal(terms * 2 ** 20, np.round(terms * 2 ** 20)) and terms.sum() < 2 ** 30
                assert order_free or 1e-6 <= frac <= 1 - 1e-6, (t, side, terms.tolist())


def main():
    out = {}
    for prefix, make in (('a', case_a), ('b', case_b)):
        res = run_case(make())
        check_case(res, exact=prefix == 'a')
        out.update({f'{prefix}_{k}': v for k, v in res.items()})
        print(prefix, len(res['syn_ids']), 'synapses,', {t: (len(res[f'{t}_ids']), len(res[f'{t}_verts']), len(res[f'p_{t}_side'])) for t in TYPES},
              '(organelles, vertices, pairs)')
        for t in TYPES:
            print(' ', t, 'objs', res[f'n_{t}_objs'].reshape(-1).tolist(), 'vxs', res[f'n_{t}_vxs'].reshape(-1).tolist())
    a = {k[2:]: v for k, v in out.items() if k.startswith('a_')}
    # case a must exercise what it is meant to (synapse rows 0..3 are S0..S3)
    side = lambda i, cell: 2 * i + int(np.flatnonzero(a['syn_partners'][i] == cell)[0])
    mi_of = lambda size: int(np.flatnonzero(a['mi_sizes'] == size)[0])
    pairs = set(zip(a['p_mi_side'].tolist(), a['p_mi_obj'].tolist()))
    k = [j for j in range(len(a['p_mi_side'])) if (a['p_mi_side'][j], a['p_mi_obj'][j]) == (side(0, 1), mi_of(300))]
    assert len(k) == 1 and a['p_mi_close'][k[0]] == 1 and a['p_mi_len'][k[0]] == 3 and a['p_mi_min_dist'][k[0]] == 999.875      # R, D inclusive
    assert (side(0, 1), mi_of(500)) not in pairs and (side(1, 1), mi_of(500)) in pairs                   # one step beyond D for S0 only
    k0 = [j for j in range(len(a['p_mi_side'])) if (a['p_mi_side'][j], a['p_mi_obj'][j]) == (side(0, 1), mi_of(0))]
    assert len(k0) == 1 and a['p_mi_close'][k0[0]] == a['p_mi_len'][k0[0]] == 2                         # size 0, all close
    assert a['n_mi_objs'][0, side(0, 1) % 2] == 1 and a['n_mi_vxs'][0, side(0, 1) % 2] == 100
    assert not any(o == mi_of(900) for _, o in pairs)                                                    # the other cell's organelle
    s02 = side(0, 2)
    assert a['n_mi_objs'][0, s02 % 2] == 0 and a['min_dst_mi_nm'][0, s02 % 2] == np.float32(1e12) and any(p[0] == s02 for p in pairs)
    assert not np.any(a['vc_cells'] == 2) and a['n_vc_objs'][0, s02 % 2] == 0
    kv = [j for j in range(len(a['p_vc_side'])) if a['p_vc_side'][j] == side(0, 1) and a['p_vc_size'][j] == 64]
    assert len(kv) == 1 and a['p_vc_close'][kv[0]] == 0 and a['p_vc_len'][kv[0]] == 2                    # exactly R and an unsampled row
    assert a['syn_sizes'][1] == 1 and a['syn_sizes'][2] % 2 == 1 and a['syn_sizes'][0] % 2 == 0
    assert np.any(a['n_mi_objs'][:, 0] != a['n_mi_objs'][:, 1]) and np.any(a['min_dst_vc_nm'][:, 0] != a['min_dst_vc_nm'][:, 1])
    assert not np.any(a['syn_partners'] == 7)
    b = {k[2:]: v for k, v in out.items() if k.startswith('b_')}
    assert b['mi_verts'].min() < 0 and b['vc_verts'].min() < 0
    for c in (a, b):
        for t in TYPES:
            assert len(c[f'p_{t}_side']) > 10 and (c[f'n_{t}_objs'] > 1).any() and (c[f'min_dst_{t}_nm'] == np.float32(1e12)).any()
    for k in list(out):
        if k.endswith('_size') and k[2:4] == 'p_':
            del out[k]
    path = os.path.join(HERE, 'g20_synssv_map.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
