"""Golden vectors for the dataset merge of contact sites and synapses, produced by the REFERENCE'S OWN code:
``_write_props_to_syn_thread`` and ``_write_props_collect_helper`` (/root/reference/syconn/extraction/cs_extraction_steps.py:498-673),
``merge_prop_dicts`` (proc/sd_proc.py:1248-1273), ``merge_type_dicts`` / ``merge_voxel_dicts`` (extraction/find_object_properties.py:
302-344) and ``subfold_from_ix_new`` (reps/rep_helper.py:143-163) are lifted by AST at generation time and run unchanged.  The worker
files they read (``cs_props_{w}.pkl`` ...) are written into a temporary directory by folding synthetic per-chunk results with the
lifted merge functions exactly as ``_contact_site_extraction_thread`` does (:484-495); ``AttributeDict``, ``VoxelStorageDyn``,
``CompressedStorage``, ``SegmentationDataset`` and ``start_multiprocess_imap`` are in-memory stand-ins that record what is stored.
Nothing compiled and no reference text is stored: inputs and outputs only, as flat arrays.

    python tests/golden/make_golden_cs_driver.py      ->  tests/golden/g18_cs_driver.npz

Inputs (per chunk, in worker-major processing order): ``in_rec`` int64 (N, 24) in the column layout of ``sd_cs_syntype_records`` (chunk-
local coordinates; column 23 = offset of the site's voxel rows inside its chunk), ``in_vox`` int64 (V, 3) (dataset coordinates),
``in_chunk_begin`` / ``in_vox_begin`` (chunks + 1), ``in_chunk_worker``, ``in_origin``; ``min_obj_vx`` = (cs, syn)."""
import os
import pickle
import sys
import tempfile
import types
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_cs import lift_function  # noqa: E402

REF = '/root/reference/syconn'
MIN_VX = {'cs': 20, 'syn': 5}
N_FOLDERS = 1000
CHUNK = np.array([64, 64, 32])

# ids at the edges of the number formats (packed uint32 pairs reach all of these), then the four cases of the filter
EDGE_IDS = [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 53 - 1, 2 ** 53 + 1, 2 ** 53 + 3, 2 ** 60 + 12345, 2 ** 63 - 1, 2 ** 63,
            2 ** 63 + 5, 2 ** 64 - 2, 7, 1000, 999999]
ID_CS_SMALL = (3 << 32) | 4             # cs 15 < 20 in total, syn 8 >= 5: dropped with its syn part
ID_SYN_SMALL = (5 << 32) | 6            # cs large, syn 3 < 5: only the syn object is dropped
ID_BOTH_SMALL = (7 << 32) | 8           # cs 6, syn 2
ID_SOME_CHUNKS = (9 << 32) | 10         # syn voxels in some of its chunks only


def site(rng, ident, cs_size=None, syn_size=None, mode=None):
    """One synthetic site record of a chunk (chunk-local coordinates) and its voxel rows (local)."""
    lo = np.array([rng.integers(0, s - 8) for s in CHUNK])
    ext = rng.integers(2, 8, 3)
    hi = lo + ext
    cs_size = int(rng.integers(1, 40)) if cs_size is None else cs_size
    r = np.zeros(24, np.int64)
    r[0] = np.uint64(ident).astype(np.int64)
    r[1:4], r[4], r[5:8], r[8:11] = lo + rng.integers(0, ext), cs_size, lo, hi
    if syn_size is None:
        syn_size = int(rng.integers(1, min(cs_size, 14) + 1)) if rng.random() < 0.7 else 0
    vox = np.zeros((0, 3), np.int64)
    if syn_size:
        slo = lo + rng.integers(0, ext // 2 + 1)
        shi = np.minimum(slo + rng.integers(1, 5, 3), hi)
        vox = np.stack([rng.integers(slo[a], shi[a], syn_size) for a in range(3)], 1)
        vox = vox[np.lexsort((vox[:, 2], vox[:, 1], vox[:, 0]))]                 # scan order
        r[11:14], r[14], r[15:18], r[18:21] = vox[0], syn_size, slo, shi
        mode = rng.integers(0, 4) if mode is None else mode                      # neither, asym only, sym only, both
        if mode in (1, 3):
            r[21] = rng.integers(1, syn_size + 1)
        if mode in (2, 3):
            r[22] = rng.integers(1 if mode == 2 else 0, syn_size - r[21] + 1)
    return r, vox


def make_inputs():
    rng = np.random.default_rng(18)
    pool = EDGE_IDS + np.unique(rng.integers(1, 2 ** 64 - 2, 40, dtype=np.uint64)).tolist()
    workers = [[(0, 0, 0), (1, 1, 0), (0, 1, 1), (2, 0, 1)], [(1, 0, 0), (2, 1, 0), (1, 1, 1)], [(2, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)]]
    chunks = [(w, np.array(c) * CHUNK) for w, cl in enumerate(workers) for c in cl]
    fixed = {   # chunk index -> [(id, cs size, syn size, mode)]
        0: [(ID_CS_SMALL, 9, 5, 1), (ID_SYN_SMALL, 30, 2, 0), (ID_BOTH_SMALL, 6, 2, 2), (ID_SOME_CHUNKS, 12, 0, 0)],
        2: [(ID_SOME_CHUNKS, 11, 6, 3)],
        5: [(ID_CS_SMALL, 6, 3, 2), (ID_SYN_SMALL, 25, 1, 1), (ID_SOME_CHUNKS, 9, 0, 0)],
        9: [(ID_SOME_CHUNKS, 14, 4, 1)],
    }
    recs, voxs, cb, vb = [], [], [0], [0]
    for k, (w, origin) in enumerate(chunks):
        ids = [i for i in pool if rng.random() < 0.45]
        if k in (0, 4, 7):
            ids = sorted(set(ids) | set(EDGE_IDS))                               # every edge id in three workers
        rows = [site(rng, i) for i in ids] + [site(rng, i, c, s, m) for i, c, s, m in fixed.get(k, [])]
        rows.sort(key=lambda rv: int(np.int64(rv[0][0]).astype(np.uint64)))      # ascending ids, as the scan returns them
        at = 0
        for r, v in rows:
            r[23] = at
            at += len(v)
            recs.append(r)
            voxs.append(v + origin)
        cb.append(len(recs))
        vb.append(vb[-1] + at)
    return dict(in_rec=np.array(recs), in_vox=np.concatenate(voxs), in_chunk_begin=np.array(cb), in_vox_begin=np.array(vb),
                in_chunk_worker=np.array([w for w, _ in chunks]), in_origin=np.array([o for _, o in chunks]))


def chunk_dicts(rec, vox):
    """The five results of extract_cs_syntype for one chunk, from its records (keys in record order)."""
    ids = rec[:, 0].view(np.uint64).tolist()
    cs_p, syn_p, asym, sym, vx = [{}, {}, {}], [{}, {}, {}], {}, {}, {}
    for k, r in zip(ids, rec.tolist()):
        cs_p[0][k], cs_p[1][k], cs_p[2][k] = r[1:4], [r[5:8], r[8:11]], r[4]
        if r[14]:
            syn_p[0][k], syn_p[1][k], syn_p[2][k] = r[11:14], [r[15:18], r[18:21]], r[14]
            vx[k] = vox[r[23]:r[23] + r[14]].tolist()
            if r[21]:
                asym[k] = r[21]
            if r[22]:
                sym[k] = r[22]
    return cs_p, syn_p, asym, sym, vx


class Store(defaultdict):
    """AttributeDict / VoxelStorageDyn stand-in: id -> dict of what was stored; one instance per path, kept in STORES."""

    def __init__(self):
        super().__init__(dict)

    def __setitem__(self, k, v):                       # voxel_dc[cs_id] = bbs
        if isinstance(v, dict):
            super().__setitem__(k, v)
        else:
            self[k]['boxes'] = v

    def increase_object_size(self, k, n):
        self[k]['vx_size'] = self[k].get('vx_size', 0) + n

    def set_object_repcoord(self, k, rc):
        self[k]['vx_rep_coord'] = rc

    def set_voxel_cache(self, k, vx):
        self[k]['voxels'] = vx

    def push(self):
        pass


def main():
    inp = make_inputs()
    ns = {'np': np, 'defaultdict': defaultdict, 'pkl': pickle}
    exec('from typing import *', ns)                                            # the annotations of the lifted signatures
    for path, names in ((f'{REF}/proc/sd_proc.py', ['merge_prop_dicts']),
                        (f'{REF}/extraction/find_object_properties.py', ['merge_type_dicts', 'merge_voxel_dicts']),
                        (f'{REF}/reps/rep_helper.py', ['subfold_from_ix_new']),
                        (f'{REF}/extraction/cs_extraction_steps.py', ['_write_props_collect_helper', '_write_props_to_syn_thread'])):
        for name in names:
            lift_function(path, name, ns)
    stores = {}

    def store_at(path, *a, **kw):
        return stores.setdefault(path, Store())

    with tempfile.TemporaryDirectory() as tmp:
        dir_props = f'{tmp}/tmp_props_cssyn/'
        # ---- the worker files, folded from the chunks as _contact_site_extraction_thread does (:484-495)
        worker_ids = {}
        for w in sorted(set(inp['in_chunk_worker'].tolist())):
            cs_props, syn_props = [{}, defaultdict(list), {}], [{}, defaultdict(list), {}]
            syn_voxels, tot_sym, tot_asym = {}, {}, {}
            for k in np.flatnonzero(inp['in_chunk_worker'] == w):
                rec = inp['in_rec'][inp['in_chunk_begin'][k]:inp['in_chunk_begin'][k + 1]]
                vox = inp['in_vox'][inp['in_vox_begin'][k]:inp['in_vox_begin'][k + 1]]
                cp, sp, a, s, vx = chunk_dicts(rec, vox)
                off = inp['in_origin'][k]
                ns['merge_prop_dicts']([cs_props, cp], offset=off)
                ns['merge_prop_dicts']([syn_props, sp], offset=off)
                ns['merge_voxel_dicts']([syn_voxels, vx], key_to_str=True)
                ns['merge_type_dicts']([tot_asym, a])
                ns['merge_type_dicts']([tot_sym, s])
            d = f'{dir_props}/{w}/'
            os.makedirs(d)
            for name, obj in (('cs_props', cs_props), ('syn_props', syn_props), ('tot_asym_cnt', tot_asym), ('tot_sym_cnt', tot_sym)):
                with open(f'{d}/{name}_{w}.pkl', 'wb') as f:
                    pickle.dump(obj, f)
            np.savez(f'{d}/syn_voxels_{w}.npz', **syn_voxels)
            worker_ids[w] = np.array(list(cs_props[0].keys()), dtype=np.uint64)
        with open(f'{tmp}/cs_worker_dict.pkl', 'wb') as f:
            pickle.dump(worker_ids, f, protocol=4)
        # ---- storage_targets_cs.pkl as _cache_storage_paths fills it (sd_proc.py:255-270)
        cs_ids = np.unique(np.concatenate(list(worker_ids.values()))).astype(np.uint64)
        targets = defaultdict(list)
        for obj_id in cs_ids:
            targets[ns['subfold_from_ix_new'](obj_id, N_FOLDERS)].append(obj_id)
        targets = {k: np.array(v, dtype=np.uint64) for k, v in targets.items()}

        class SD:
            def __init__(self, obj_type=None, **kw):
                self.obj_type = obj_type

            def get_segmentation_object(self, ix):
                p = f'{self.obj_type}{ns["subfold_from_ix_new"](ix, N_FOLDERS)}'
                return types.SimpleNamespace(attr_dict_path=p + 'attr_dict.pkl', voxel_path=p + 'voxel.pkl')

        class Config(dict):
            temp_path, use_new_subfold, working_dir = tmp, True, tmp
        ns.update(global_params=types.SimpleNamespace(config=Config(cell_objects={'min_obj_vx': MIN_VX})),
                  rep_helper=types.SimpleNamespace(subfold_from_ix_new=ns['subfold_from_ix_new'], subfold_from_ix_OLD=None),
                  CompressedStorage=lambda path, **kw: targets, segmentation=types.SimpleNamespace(SegmentationDataset=SD),
                  AttributeDict=store_at, VoxelStorageDyn=store_at,
                  basics=types.SimpleNamespace(load_pkl2obj=lambda p: pickle.load(open(p, 'rb'))),
                  start_multiprocess_imap=lambda func, params, **kw: [func(p) for p in params])
        storage_location_ids = [int(str(ix) + '000') for ix in np.arange(N_FOLDERS)]        # rep_helper.get_unique_subfold_ixs
        ns['_write_props_to_syn_thread']((storage_location_ids, N_FOLDERS, 'syn_seg', 'cs_seg', dir_props, 1))

    out = dict(inp)
    out['min_obj_vx'] = np.array([MIN_VX['cs'], MIN_VX['syn']], np.int64)
    out['n_folders_fs'] = np.array(N_FOLDERS)
    out['key_ids'] = cs_ids
    out['key_bucket_1000'] = np.array([ns['subfold_from_ix_new'](i, 1000) for i in cs_ids])
    out['key_bucket_100000'] = np.array([ns['subfold_from_ix_new'](i, 100000) for i in cs_ids])
    for ot in ('cs', 'syn'):
        attr, vxs = {}, {}
        for path, st in stores.items():
            if path.startswith(ot + '/'):
                (attr if path.endswith('attr_dict.pkl') else vxs).update(st)
        ids = sorted(int(k) for k in attr)
        assert ids == sorted(int(k) for k in vxs) and len(ids) > 5
        key = {int(k): k for k in attr}
        A = [attr[key[i]] for i in ids]
        V = [vxs[{int(k): k for k in vxs}[i]] for i in ids]
        out[f'{ot}_ids'] = np.array(ids, np.uint64)
        out[f'{ot}_rep_coord'] = np.array([a['rep_coord'] for a in A])
        assert all(a['rep_coord'].dtype == np.int32 for a in A)
        assert all(np.array_equal(a['rep_coord'], v['vx_rep_coord']) and a['size'] == v['vx_size'] for a, v in zip(A, V))
        out[f'{ot}_bounding_box'] = np.array([a['bounding_box'] for a in A])
        out[f'{ot}_size'] = np.array([a['size'] for a in A], np.int64)
        out[f'{ot}_boxes'] = np.concatenate([v['boxes'] for v in V])
        out[f'{ot}_box_begin'] = np.concatenate(([0], np.cumsum([len(v['boxes']) for v in V])))
        if ot == 'syn':
            out['syn_sym_prop'] = np.array([a['sym_prop'] for a in A], np.float64)
            out['syn_asym_prop'] = np.array([a['asym_prop'] for a in A], np.float64)
            out['syn_cs_id'] = np.array([int(a['cs_id']) for a in A], np.uint64)
            out['syn_cs_size'] = np.array([a['cs_size'] for a in A], np.int64)
            assert all(v['voxels'].dtype == np.uint32 for v in V)
            out['syn_voxels'] = np.concatenate([v['voxels'] for v in V])
            out['syn_vox_begin'] = np.concatenate(([0], np.cumsum([len(v['voxels']) for v in V])))
    # the inputs must exercise what they are meant to
    cs_set, syn_set = set(out['cs_ids'].tolist()), set(out['syn_ids'].tolist())
    assert ID_CS_SMALL not in cs_set and ID_CS_SMALL not in syn_set and ID_BOTH_SMALL not in cs_set
    assert ID_SYN_SMALL in cs_set and ID_SYN_SMALL not in syn_set and ID_SOME_CHUNKS in syn_set
    path = os.path.join(HERE, 'g18_cs_driver.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(cs_set), 'cs,', len(syn_set), 'syn of', len(cs_ids), 'ids')


if __name__ == '__main__':
    main()
