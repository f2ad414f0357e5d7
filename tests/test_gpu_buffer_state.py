"""GPU: the results of the dataset stages do not depend on what their outputs and scratch buffers held before the call.

The host layer allocates every output and scratch uninitialised (``_dev.empty`` / ``_dev.scratch`` / ``torch.empty``); under the caching
allocator such a buffer holds what the previous stage left.  Every row of ROWS runs one public function (or chain) four times over the
allocators of tests/_state_alloc.py:

    A  Fill(0x00)             the baseline, and a forgotten init of a min accumulator;
    B  Fill(0xFF)             max unsigned / -1 / NaN: forgotten inits of add / or / max accumulators, flags, counters, sparse outputs;
    C  Arena, first run       the row's large case;
    D  the Arena rewound      the small case over the bytes C left at the same addresses: a partial init.

A, B and D must be byte-identical in every returned array, and each run is compared with the module's reference exactly as the module's
own GPU test compares it (imported from there).  No result is exempt from the byte comparison: none comes from float atomics.  One
statistic is: ``sd_syn_ssv_components`` counts in counts[5] / counts[6] how many box-ambiguous cell pairs it found "in one set already"
and how many it "voxel-tested".  Which of the two a pair falls under depends on whether the union of another wave has landed in the
concurrent union-find when the pair is examined, so the split differs from run to run over any buffers (the labels do not: the sets
are the same in the end).  The row compares their sum; the module's own test reads counts[0] only.  The allocator
must have served the row (and a ``_dev.scratch`` name where the function takes a scratch); the last test checks that every name given to
``D.scratch`` in the package was served by some row.  Two tests at the end do the same through the C ABI helpers' FILL."""
import functools
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _state_alloc as A  # noqa: E402

pytestmark = pytest.mark.gpu
U = np.uint64
ARENA_BYTES = 1 << 28
ROWS = {}
SERVED = {}                     # row -> the scratch names served during it


def row(name, scratch=True):
    def register(cls):
        cls.name, cls.scratch = name, scratch
        ROWS[name] = cls
        return cls
    return register


def arrays_of(obj):
    """The array and number attributes of a table object."""
    return {k: v for k, v in vars(obj).items() if isinstance(v, (np.ndarray, np.generic, int, float, bool))}


def flatten(x, prefix='', out=None):
    """Nested dicts / lists / tuples of arrays and numbers -> {path: ndarray}."""
    import torch
    out = {} if out is None else out
    if isinstance(x, dict):
        for k in x:
            flatten(x[k], f'{prefix}/{k}', out)
    elif isinstance(x, (list, tuple)):
        out[prefix + '/len'] = np.asarray(len(x))
        for k, v in enumerate(x):
            flatten(v, f'{prefix}/{k}', out)
    elif isinstance(x, torch.Tensor):
        out[prefix] = x.cpu().numpy()
    elif x is not None:
        out[prefix] = np.asarray(x)
    return out


def assert_identical(a, b, what):
    assert list(a) == list(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.dtype, y.dtype, x.shape, y.shape)
        if x.dtype == object:
            assert x.tolist() == y.tolist(), (what, k)
        else:
            assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (what, k, int((x != y).sum()))


# ---- 1. label statistics and the chunk merge ------------------------------------------------------------------------------------------
@row('objprops', scratch=False)
class ObjProps:
    CHUNK = (32, 40, 24)

    @staticmethod
    @functools.lru_cache(None)
    def case(seed, nid, n_sub_ids):
        from oracle.objprops_ref import find_object_properties_np, map_subcell_extract_props_np
        from tests import _segstats_cases as SC
        shape = (64, 40, 24)                                                       # two chunks of CHUNK along x
        cell = SC.coherent_labels(seed, shape, nid)
        sub = SC.coherent_labels(seed + 1, shape, n_sub_ids, block=(4, 3, 5))
        ids = np.unique(cell[cell != 0])
        both = np.intersect1d(cell[:32], cell[32:])
        assert len(ids) >= 300 and (both != 0).sum() >= 1
        return dict(cell=cell, sub=sub, props=find_object_properties_np(cell), whole=map_subcell_extract_props_np(cell, sub[None]))

    small = staticmethod(lambda: ObjProps.case(1, 900, 60))
    large = staticmethod(lambda: ObjProps.case(5, 500, 25))

    @staticmethod
    def run(gpu, c):
        import torch
        import syconn_amd.proc.sd_proc as sp
        from syconn_amd.extraction.find_object_properties import find_object_properties, map_subcell_extract_props, segstats
        vols = {'sv': c['cell'], 'mi': c['sub']}
        dvols = {k: torch.from_numpy(v.view(np.int64)).to(gpu) for k, v in vols.items()}

        class KD:
            boundary = np.array(c['cell'].shape)

        def loader(name, off, size):
            return dvols[name][off[0]:off[0] + size[0], off[1]:off[1] + size[1], off[2]:off[2] + size[2]].contiguous()
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(sp, 'kd_factory', lambda p: KD())
            cell_t, sub_t, map_t = sp.map_subcell_extract_props('', {'mi': ''}, chunk_size=ObjProps.CHUNK, min_obj_vx={'sv': 1, 'mi': 1}, device=gpu,
                                                                as_tables=True, chunk_loader=loader)
        whole = segstats(c['cell'], [c['sub']], device=gpu)
        return dict(props=find_object_properties(c['cell']), dicts=map_subcell_extract_props(c['cell'], c['sub'][None]), cell_t=cell_t, sub_t=sub_t['mi'],
                    map_t=map_t['mi'], whole=dict(cell=whole.cell, sub=whole.sub, pairs=whole.pairs))

    @staticmethod
    def flat(o):
        as_arrays = lambda d: [np.array(sorted(d)), [np.asarray(d[k]) for k in sorted(d)]]
        return dict(props=[as_arrays(d) for d in o['props']], cell_t=arrays_of(o['cell_t']), sub_t=arrays_of(o['sub_t']), map_t=arrays_of(o['map_t']),
                    whole=o['whole'])

    @staticmethod
    def check(c, o):
        assert o['props'] == c['props']
        w_cell, w_sub, w_map = c['whole']
        assert o['dicts'][0] == w_cell and o['dicts'][1] == w_sub and o['dicts'][2] == w_map
        for tab, vol, w_bb, w_sz in ((o['cell_t'], c['cell'], w_cell[1], w_cell[2]), (o['sub_t'], c['sub'], w_sub[1][0], w_sub[2][0])):
            keys = sorted(w_sz)
            assert tab.ids.tolist() == keys and tab.sizes.tolist() == [w_sz[k] for k in keys]
            lo = np.minimum.reduceat(tab.boxes[:, 0], tab.box_begin[:-1], axis=0)
            hi = np.maximum.reduceat(tab.boxes[:, 1], tab.box_begin[:-1], axis=0)
            assert np.array_equal(np.stack((lo, hi), axis=1), np.array([w_bb[k] for k in keys]))
            rc = np.asarray(tab.rep_coords)
            assert np.array_equal(vol[rc[:, 0], rc[:, 1], rc[:, 2]], tab.ids)
            assert (np.diff(tab.box_begin) == 2).any()                             # an id with a box from each chunk
        got = {}
        for a, b, n in zip(o['map_t'].sub_ids.tolist(), o['map_t'].cell_ids.tolist(), o['map_t'].counts.tolist()):
            got.setdefault(a, {})[b] = n
        assert got == w_map[0]
        assert np.array_equal(o['cell_t'].ids, o['whole']['cell'][0]) and np.array_equal(o['cell_t'].sizes, o['whole']['cell'][2])
        s, cc, n = o['whole']['pairs'][0]
        assert np.array_equal(o['map_t'].sub_ids, s) and np.array_equal(o['map_t'].cell_ids, cc) and np.array_equal(o['map_t'].counts, n)


# ---- 2. object segmentation -------------------------------------------------------------------------------------------------------------
@row('objseg')
class ObjSeg:
    OPS = ['binary_opening', 'binary_closing']
    WS_OPS = ['binary_opening', 'binary_closing', 'binary_erosion']
    SCALING = (10, 10, 20)

    @staticmethod
    @functools.lru_cache(None)
    def case(seed, q, sigma_blobs, sigma_gauss):
        from scipy import ndimage
        from oracle.objseg_ref import gaussian_smoothing_ref, object_segmentation_ref, object_segmentation_watershed_ref, watershed_ref
        from test_objseg import _blobs, _flood_case
        prob, thr = _blobs((40, 48, 32), seed, sigma_blobs, q)
        plain = object_segmentation_ref(prob, thr, ObjSeg.OPS, ObjSeg.SCALING)
        ws = object_segmentation_watershed_ref(prob, thr, ObjSeg.WS_OPS, ObjSeg.SCALING, 2)
        comp, nc = ndimage.label(ws[2])
        multi = sum(1 for k in range(1, nc + 1) if len(np.unique(ws[3][comp == k])) > 2)
        assert plain[1] >= 24 and multi >= 1, (plain[1], nc, multi)
        d2, markers, mask = _flood_case(np.random.default_rng(seed), (24, 28, 20), 'edt', 40)
        return dict(prob=prob, thr=thr, plain=plain, ws=ws, d2=d2, markers=markers, mask=mask, flood=watershed_ref(d2.astype(np.int64), markers, mask),
                    sigma=sigma_gauss, smooth=gaussian_smoothing_ref(prob, sigma_gauss))

    small = staticmethod(lambda: ObjSeg.case(5, 0.70, 1.5, 1.0))
    large = staticmethod(lambda: ObjSeg.case(9, 0.60, 1.3, (1.5, 0.7, 2.2)))

    @staticmethod
    def run(gpu, c):
        from syconn_amd.extraction.object_extraction_steps import gaussian_threshold, marker_flood, object_segmentation_first_stage
        lab, mx, m = object_segmentation_first_stage(c['prob'], c['thr'], ObjSeg.OPS, ObjSeg.SCALING, return_mask=True, device=gpu)
        wlab, wmx, wm, wmk = object_segmentation_first_stage(c['prob'], c['thr'], ObjSeg.WS_OPS, ObjSeg.SCALING, return_mask=True, min_seed_vx=2,
                                                             return_markers=True, device=gpu)
        flood, fmx = marker_flood(c['d2'], c['markers'], c['mask'], device=gpu)
        gmask, sm = gaussian_threshold(c['prob'], c['sigma'], c['thr'], device=gpu, return_smoothed=True)
        return dict(lab=lab, mx=mx, m=m, wlab=wlab, wmx=wmx, wm=wm, wmk=wmk, flood=flood, fmx=fmx, gmask=gmask, sm=sm)

    flat = staticmethod(lambda o: o)

    @staticmethod
    def check(c, o):
        assert o['mx'] == c['plain'][1] and np.array_equal(o['lab'], c['plain'][0])
        want, want_max, tmp, markers = c['ws']
        assert np.array_equal(o['wm'], tmp) and np.array_equal(o['wmk'].astype(np.uint32), markers)
        assert o['wmx'] == want_max and np.array_equal(o['wlab'], want)
        assert np.array_equal(o['flood'], c['flood']) and o['fmx'] == c['flood'].max()
        assert float(np.abs(o['sm'] - c['smooth']).max()) <= 6.2e-5                 # (the bound of test_objseg.py: two float32 ulps at 255)
        clear = np.abs(c['smooth'] - c['thr']) > 1e-3
        assert np.array_equal(o['gmask'][clear], (c['smooth'] > c['thr']).astype(np.uint8)[clear])


# ---- 3. contact sites: partners, closing, synapse types, the dataset merge ----------------------------------------------------------------
@row('contact_sites')
class ContactSites:
    MIN_VX = dict(cs=12, syn=4)

    @staticmethod
    @functools.lru_cache(None)
    def case(seg_name, cuts):
        """The partner stencil and the closing over a Voronoi volume of golden g15; the synapse types of golden g16's contact volume chunk by
        chunk (cut along x at `cuts`) and the dataset merge of the chunks."""
        import _cs_driver_ref as DR
        import _cs_ref
        import _cs_syntype_ref as TR
        from test_cs_syntype_cpu import case_inputs
        g15, g16 = (dict(np.load(os.path.join(HERE, 'golden', f))) for f in ('g15_contact_sites.npz', 'g16_cs_syntype.npz'))
        seg, stencil = g15[f'st_{seg_name}_raw'].astype(np.uint32), tuple(int(v) for v in g15[f'st_{seg_name}_stencil'])
        edges = _cs_ref.seg_boundaries(seg)
        cs = _cs_ref.contact_partners(edges, seg, stencil)
        assert np.array_equal(cs, g15[f'st_{seg_name}_cs']) and (cs != 0).sum() > 256
        vol, syn, asym, sym, _ = case_inputs(g16, 'vor64')
        bounds = list(zip((0,) + cuts, cuts + (vol.shape[0],)))
        origins = [(a, 0, 0) for a, _ in bounds]
        crops = [tuple(np.ascontiguousarray(m[a:b]) for m in (vol, syn, asym, sym)) for a, b in bounds]
        dicts = [TR.extract_cs_syntype(*crop, o) for crop, o in zip(crops, origins)]
        per_chunk = [set(np.unique(crop[0]).tolist()) - {0} for crop in crops]
        assert len(per_chunk[0] & per_chunk[1]) >= 1 and len(set().union(*per_chunk)) > 20         # a site that spans two chunks
        return dict(seg=seg, stencil=stencil, edges=edges, cs=cs, closed=_cs_ref.close_dilate(cs, 6, 2, 'ascending'), origins=origins, crops=crops, dicts=dicts, DR=DR)

    small = staticmethod(lambda: ContactSites.case('vor7', (32,)))
    large = staticmethod(lambda: ContactSites.case('vor13', (24, 48)))

    @staticmethod
    def run(gpu, c):
        from syconn_amd.extraction.cs_extraction_steps import ContactSiteMerger, close_and_dilate_cs
        from syconn_amd.extraction.find_object_properties import cs_syntype, detect_cs, detect_seg_boundaries
        edges = detect_seg_boundaries(c['seg'], device=gpu)
        cs = detect_cs(c['seg'], c['stencil'], device=gpu)
        closed = close_and_dilate_cs(cs, 6, 2, device=gpu)
        merger = ContactSiteMerger(ContactSites.MIN_VX, gpu, capacity=64, vox_capacity=256)        # both arrays grow between the chunks
        chunks = []
        for crop, o in zip(c['crops'], c['origins']):
            res = cs_syntype(*crop, offset=o, device=gpu)
            merger.add_chunk(res, o)
            chunks.append(tuple(res.host()) + (np.asarray(o, np.int64),))
        cs_t, syn_t = merger.finish()
        return dict(edges=edges, cs=cs, closed=closed, chunks=chunks, cs_t=cs_t, syn_t=syn_t)

    @staticmethod
    def flat(o):
        return dict(edges=o['edges'], cs=o['cs'], closed=o['closed'], chunks=[list(ch) for ch in o['chunks']], cs_t=arrays_of(o['cs_t']), syn_t=arrays_of(o['syn_t']))

    @staticmethod
    def check(c, o):
        from syconn_amd.extraction.find_object_properties import cs_syntype_dicts
        assert np.array_equal(o['edges'], c['edges']) and np.array_equal(o['cs'], c['cs']) and np.array_equal(o['closed'], c['closed'])
        for (rec, vox, _), want in zip(o['chunks'], c['dicts']):
            assert cs_syntype_dicts(rec, vox) == want
        DR = c['DR']
        w_cs, w_syn = DR.merge_workers([DR.fold_chunks(o['chunks'])], ContactSites.MIN_VX['cs'], ContactSites.MIN_VX['syn'])
        assert len(w_cs) > 5 and len(w_syn) > 5 and any(len(e['boxes']) > 1 for e in w_syn.values())
        DR.assert_same(o['cs_t'].as_dict(), w_cs, 'cs')
        DR.assert_same(o['syn_t'].as_dict(), w_syn, 'syn')


# ---- 4. synapse agglomeration -------------------------------------------------------------------------------------------------------------
@row('syn_ssv')
class SynSsv:
    @staticmethod
    @functools.lru_cache(None)
    def case(seed, n_groups):
        import _syn_ssv_ref as S
        from test_gpu_syn_ssv import random_groups, table_and_mapping
        groups = random_groups(np.random.default_rng(seed), n_groups, (60, 60, 30))
        table, mapping = table_and_mapping(groups)
        want, labels = S.combine(groups, (10, 10, 20), 250, 40, 0.225)
        assert n_groups >= 50 and any(int(lab.max()) > 0 for lab in labels) and max(len(r['voxels']) for r in want) > 64
        return dict(S=S, table=table, mapping=mapping, want=want, labels=labels)

    small = staticmethod(lambda: SynSsv.case(1, 50))
    large = staticmethod(lambda: SynSsv.case(2, 64))

    @staticmethod
    def run(gpu, c):
        from syconn_amd.extraction.cs_processing_steps import combine_and_split_syn
        got, info = combine_and_split_syn(c['table'], c['mapping'], scaling=(10, 10, 20), cs_gap_nm=250, min_obj_vx=40, sym_thresh=0.225, device=gpu,
                                          return_stats=True)
        return dict(got=got, counts=np.asarray(info['counts']))

    @staticmethod
    def flat(o):
        # counts[5] ("in one set already") and counts[6] ("voxel-tested") of sd_syn_ssv_components split the box-ambiguous cell pairs by whether
        # another wave's union had landed when the pair was looked at: their sum is fixed, the split is not (see the module's docstring)
        c = o['counts']
        return dict(got=arrays_of(o['got']), rows=o['got'].as_dict(), counts=c[:5], pairs_examined=c[5] + c[6], flag=c[7])

    @staticmethod
    def check(c, o):
        got, want, labels = o['got'], c['want'], c['labels']
        assert got.n_components == sum(int(lab.max()) + 1 for lab in labels) == int(o['counts'][0])
        c['S'].assert_rows_equal(got.as_dict(), want, 'syn_ssv')
        assert got.ordinal.tolist() == [r['component'] for r in want] and got.group.tolist() == [r['group'] for r in want]
        fb = got.frag_begin.tolist()
        for i, r in enumerate(want):
            assert got.frag_ids[fb[i]:fb[i + 1]].tolist() == r['frag_ids'] and got.frag_counts[fb[i]:fb[i + 1]].tolist() == r['frag_counts']


# ---- 5. organelles of the synapses' partners ----------------------------------------------------------------------------------------------
@row('synssv_map')
class SynSsvMap:
    R, D, F = {'mi': 1000, 'vc': 500}, 4000, 2

    @staticmethod
    @functools.lru_cache(None)
    def case(seed, n_syn):
        import _synssv_map_ref as M
        c = M.random_case(np.random.default_rng(seed), n_syn=n_syn, scaling=(10, 10, 20), extent=9, n_vert=(3, 300))
        want = M.map_objects(c['partners'], c['rep'], c['vox'], c['vox_begin'], c['tables'], c['scaling'], SynSsvMap.R, SynSsvMap.D, SynSsvMap.F)
        for t in want:                                                             # pairs with and without close vertices
            assert want[t]['pair_close'].sum() > 0 and np.isinf(want[t]['pair_min_d2']).any()
        return dict(M=M, c=c, want=want)

    small = staticmethod(lambda: SynSsvMap.case(1, 30))
    large = staticmethod(lambda: SynSsvMap.case(2, 45))

    @staticmethod
    def run(gpu, case):
        from syconn_amd.extraction.cs_processing_steps import map_objects_from_synssv_partners
        from test_gpu_synssv_map import Syn, product_table
        c = case['c']
        syn = Syn(c['partners'], c['rep'], c['vox'], c['vox_begin'])
        m, stats = map_objects_from_synssv_partners(syn, {t: product_table(tab) for t, tab in c['tables'].items()}, c['scaling'], max_vert_dist_nm=SynSsvMap.R,
                                                    max_rep_coord_dist_nm=SynSsvMap.D, sample_fact=SynSsvMap.F, device=gpu, return_stats=True)
        return dict(res={t: case['M'].mapping_result(m, t) for t in c['tables']}, stats={t: dict(stats[t]) for t in c['tables']})

    flat = staticmethod(lambda o: o)

    @staticmethod
    def check(case, o):
        for t in case['c']['tables']:
            case['M'].assert_result_equal(o['res'][t], case['want'][t], t)


# ---- 6. partner kNN -----------------------------------------------------------------------------------------------------------------------
@row('segmented_knn')
class Knn:
    K = 7

    @staticmethod
    @functools.lru_cache(None)
    def case(seed, sizes):
        import _syn_props_ref as R
        from test_gpu_syn_props import random_cells
        rng = np.random.default_rng(seed)
        pts, begin, lab = random_cells(rng, list(sizes))
        q_cell = np.concatenate([np.repeat(np.arange(len(sizes)), 20), rng.integers(0, len(sizes), 200)])
        q_xyz = rng.random((len(q_cell), 3)) * 4000
        want = R.knn(pts, begin, lab, q_cell, q_xyz, Knn.K, extra=1)
        flagged = R.ambiguous(want[2][:, :Knn.K + 1])
        assert flagged.mean() <= 0.01
        return dict(pts=pts, begin=begin, lab=lab, q_cell=q_cell, q_xyz=q_xyz, want=want, keep=~flagged)

    small = staticmethod(lambda: Knn.case(11, (300, 65, 0, 1)))
    large = staticmethod(lambda: Knn.case(12, (129, 0, 64, 700, 3)))                # other cell sizes: every tile slot shifts

    @staticmethod
    def run(gpu, c):
        from syconn_amd.extraction.cs_processing_steps import segmented_knn
        vote, rows, d2, counts = segmented_knn(c['pts'], c['begin'], c['lab'], c['q_cell'], c['q_xyz'], Knn.K, gpu, return_neighbours=True, return_counts=True)
        return dict(vote=vote, rows=rows, d2=d2, counts=dict(counts))

    flat = staticmethod(lambda o: o)

    @staticmethod
    def check(c, o):
        from test_gpu_syn_props import assert_knn_equal
        assert_knn_equal((o['vote'], o['rows'], o['d2']), c['want'], c['keep'], Knn.K)
        empty = np.diff(c['begin'])[c['q_cell']] == 0
        assert empty.any() and np.all(o['vote'][empty] == -1) and np.all(o['rows'][empty] == -1) and np.all(np.isinf(o['d2'][empty]))


# ---- 7. the random forest -----------------------------------------------------------------------------------------------------------------
@row('forest', scratch=False)
class Forest:
    @staticmethod
    @functools.lru_cache(None)
    def case(prefix, n_rows, seed):
        import _syn_props_ref as R
        from syconn_amd.extraction.cs_processing_steps import PackedForest
        from test_gpu_syn_props import G21
        from test_gpu_syn_props import case as golden_case
        c = golden_case(dict(np.load(G21)), prefix)
        f = R.forest_from_case(c)
        forest = PackedForest(f['feature'], f['threshold'], f['left'], f['right'], f['proba'], f['tree_begin'], f['n_features'])
        feats = c['features']
        rng = np.random.default_rng(seed)
        x = feats[rng.integers(0, len(feats), (n_rows, feats.shape[1])), np.arange(feats.shape[1])]     # every column drawn from the golden's values
        x[:len(feats)] = feats
        return dict(forest=forest, x=x, want=R.forest_proba({k: getattr(forest, k) for k in PackedForest._FIELDS}, x), golden=c['rf_predict_proba'])

    small = staticmethod(lambda: Forest.case('a', 300, 1))
    large = staticmethod(lambda: Forest.case('b', 517, 2))

    run = staticmethod(lambda gpu, c: dict(proba=c['forest'].predict_proba(c['x'], gpu)))
    flat = staticmethod(lambda o: o)

    @staticmethod
    def check(c, o):
        assert o['proba'].dtype == np.float64 and o['proba'].tobytes() == c['want'].tobytes()
        assert o['proba'][:len(c['golden'])].tobytes() == c['golden'].tobytes()


# ---- 8. spine heads -----------------------------------------------------------------------------------------------------------------------
@row('spinehead')
class SpineHead:
    @staticmethod
    @functools.lru_cache(None)
    def case(p):
        import _spinehead_ref as R
        from test_gpu_spinehead import IGNORE, cell_inputs
        g22 = dict(np.load(os.path.join(HERE, 'golden', 'g22_spinehead.npz')))
        case = R.case_from_golden(g22, p)
        cells = []
        for cell in case['cells']:
            if cell['id'] in case['err_cells']:
                continue
            ids, rep = R.synapses_of(case, cell['id'])
            head = R.spinehead_filter(cell, rep, case['scaling'], case['k'], 1, IGNORE, R.AX_KEY)
            ids, rep = ids[head], rep[head]
            if not len(ids):
                continue
            stages = {}
            R.extract_spinehead_volume(cell, ids, rep, case['seg'], case['scaling'], case['ctx_vol'], case['k'], stages=stages)
            cells.append(dict(cell=cell, ids=ids, rep=rep, inputs=cell_inputs(cell, case['scaling']), stages=stages))
        peaks = [len(c['stages'][s]['peaks']) for c in cells for s in c['ids'].tolist()]
        assert len(peaks) >= 2
        return dict(case=case, cells=cells, peaks=peaks)

    @staticmethod
    def small():
        c = SpineHead.case('a_')
        assert any(b < a for a, b in zip(c['peaks'], c['peaks'][1:])), c['peaks']     # a window with fewer peaks than the one before it
        return c

    large = staticmethod(lambda: SpineHead.case('b_'))

    @staticmethod
    def run(gpu, c):
        from syconn_amd.extraction import spinehead as SH
        from syconn_amd.extraction.cs_processing_steps import calculate_spinehead_volume
        from _spinehead_ref import AX_KEY
        from test_gpu_spinehead import _table
        case, out = c['case'], []
        for cell in c['cells']:
            keep = []
            verts, sem = cell['inputs']
            res = SH.spinehead_windows(case['seg'], cell['cell']['sv_ids'], cell['rep'], verts, sem, case['scaling'], case['ctx_vol'], case['k'], gpu, batch=1,
                                       syn_ids=cell['ids'], keep=keep)                    # one window per batch: every window reuses the workspace
            out.append(dict(res=res, keep=[{k: None if v is None else v.cpu().numpy() for k, v in w.items()} for w in keep]))
        t, sb, sv = _table(case, skip=case['err_cells'])
        triple = calculate_spinehead_volume(t, sb, sv, case['syn_ids'], case['syn_rep'], case['syn_cells'], case['seg'], scaling=case['scaling'],
                                            ctx_vol=case['ctx_vol'], k=case['k'], ax_key=AX_KEY, device=gpu)
        return dict(windows=out, triple=list(triple), table=t)

    flat = staticmethod(lambda o: dict(windows=o['windows'], triple=o['triple']))

    @staticmethod
    def check(c, o):
        import torch
        from test_gpu_spinehead import as_dicts, assert_stages
        for cell, got in zip(c['cells'], o['windows']):
            for i, sid in enumerate(cell['ids'].tolist()):
                want = cell['stages'][sid]
                assert_stages({k: None if v is None else torch.from_numpy(v) for k, v in got['keep'][i].items()}, want, sid)
                res = got['res']
                assert res[i, 0] == want['filled'].sum() and res[i, 1] == len(want['peaks']) and res[i, 5] == len(want['points'])
                if want['entry']:
                    assert res[i, 2:5].tolist() == [want['n_voxels'], want['chosen'], want['nb_obj']], sid
        got = as_dicts(o['table'], o['triple'])
        expected = c['case']['expected']
        assert sorted(got) == sorted(expected)
        for cid, want in expected.items():
            assert sorted(got[cid]) == sorted(want) and all(got[cid][s] == want[s] for s in want), cid


# ---- 9. skeleton votes --------------------------------------------------------------------------------------------------------------------
@row('skeleton')
class Skeleton:
    SCALING, MAX_DIST = np.array([9, 9, 20], np.float32), 2700

    @staticmethod
    @functools.lru_cache(None)
    def case(seed, n_cells, cycles):
        import _skeleton_ref as R
        from syconn_amd._lib import SD_SKEL_LDS_NODES as CAP
        from test_gpu_skeleton_vote import _random_cells, chain
        rng = np.random.default_rng(seed)
        nodes, nb, edges, eb = _random_cells(rng, n_cells, cycles)
        n = CAP + 188                                                              # a chain 9 nm per edge: 601 nodes within MAX_DIST in its middle
        cn, ce = chain(n)
        nodes, edges = np.concatenate([nodes, cn.astype(np.float64)]), np.concatenate([edges, ce])
        nb, eb = np.append(nb, nb[-1] + n), np.append(eb, eb[-1] + n - 1)
        labels = rng.integers(0, 6, len(nodes)).astype(np.int16) * 3 - 4
        want, reached = R.majority_vote(nodes, nb, edges, eb, labels, Skeleton.SCALING, Skeleton.MAX_DIST)
        assert (reached[-n:] > CAP).any()
        lab = rng.choice(5, len(nodes), p=[0.3, 0.35, 0.15, 0.1, 0.1]).astype(np.uint8)
        return dict(nodes=nodes, nb=nb, edges=edges, eb=eb, labels=labels, want=want, reached=reached, lab=lab, comp=R.compartment_majority(nb, edges, eb, lab),
                    redone=int((reached > CAP).sum()))

    small = staticmethod(lambda: Skeleton.case(77, 3, False))
    large = staticmethod(lambda: Skeleton.case(78, 5, True))

    @staticmethod
    def run(gpu, c):
        from syconn_amd.reps.super_segmentation_helper import skeleton_compartment_majority, skeleton_majority_vote
        vote, reached, counts = skeleton_majority_vote(c['nodes'], c['nb'], c['edges'], c['eb'], c['labels'], Skeleton.SCALING, Skeleton.MAX_DIST, gpu, True, True)
        return dict(vote=vote, reached=reached, counts=dict(counts), comp=skeleton_compartment_majority(c['nb'], c['edges'], c['eb'], c['lab'], device=gpu))

    flat = staticmethod(lambda o: o)

    @staticmethod
    def check(c, o):
        assert np.array_equal(o['reached'], c['reached']) and np.array_equal(o['vote'], c['want']) and o['vote'].dtype == np.int16
        assert o['counts']['sources_redone'] == c['redone'] > 0                      # the global second pass ran
        assert np.array_equal(o['comp'], c['comp'])


# ---- 10. cell assembly --------------------------------------------------------------------------------------------------------------------
@row('cell_assembly')
class CellAssembly:
    SCALING, THRESHOLDS = (10, 10, 20), (0.2, 1., 20)

    @staticmethod
    @functools.lru_cache(None)
    def case(seed, n_ids, n_edges, n_cells, n_org, n_rec):
        import _cell_assembly_ref as R
        from test_gpu_cell_assembly import random_graph_case, random_mapping_case
        rng = np.random.default_rng(seed)
        edges, ids, sizes, rep, box_begin, boxes = random_graph_case(rng, n_ids, 40, n_edges)
        comp = R.components(edges, ids, sizes, box_begin, boxes, CellAssembly.SCALING, 0.0, False)
        per = np.diff(comp['sv_begin'])
        assert n_ids >= 300 and (per == 1).any() and (per == 2).any() and per.max() > 8
        in_table = np.isin(comp['sv_ids'], ids)                                    # cells over the table's supervoxels only
        keep = np.add.reduceat(~in_table, comp['sv_begin'][:-1]) == 0
        sel = np.repeat(keep, per)
        lists = (np.concatenate(([0], np.cumsum(per[keep]))), comp['sv_ids'][sel])
        props = R.cell_props(lists[0], lists[1], ids, sizes, rep, box_begin, boxes)
        m = random_mapping_case(rng, n_cells, n_org, n_rec)
        want_m = R.mapping(*m, *CellAssembly.THRESHOLDS)
        assert (want_m['org_n_cells'] >= 2).any()                                  # an organelle mapped to two cells
        ssv_ids = np.sort(rng.choice(2 ** 62, 40, replace=False).astype(U) * U(4) + U(1))
        partners = np.concatenate([ssv_ids, np.array([0, 2, 4], U)])[rng.integers(0, 43, (n_rec, 2))]
        prob, syn_ids = rng.random(n_rec).astype(np.float32), rng.permutation(n_rec).astype(U) + U(2 ** 63)
        return dict(graph=(edges, ids, sizes, rep, box_begin, boxes), comp=comp, lists=lists, cell_ids=comp['ssv_ids'][keep], props=props, m=m, want_m=want_m,
                    syn=(ssv_ids, partners, prob, syn_ids), want_syn=R.cell_synapses(ssv_ids, partners, prob, syn_ids, 0.4))

    small = staticmethod(lambda: CellAssembly.case(3, 300, 200, 30, 50, 4000))
    large = staticmethod(lambda: CellAssembly.case(4, 777, 900, 41, 90, 2500))

    @staticmethod
    def run(gpu, c):
        from syconn_amd.proc.graphs import svgraph_components
        from syconn_amd.proc.sd_proc import MapTable, PropTable
        from syconn_amd.proc.ssd_proc import CellLists, cell_properties, map_organelle, map_synssv_objects
        edges, ids, sizes, rep, box_begin, boxes = c['graph']
        tab = PropTable(ids, sizes, rep, boxes, box_begin)
        comp = svgraph_components(edges, tab, CellAssembly.SCALING, 0.0, False, gpu)
        props = cell_properties(CellLists(c['cell_ids'], *c['lists']), tab, device=gpu)
        ssv_ids, sv_begin, sv_ids, sub, rsv, cnt, org_ids, org_sizes = c['m']
        m = map_organelle(CellLists(ssv_ids, sv_begin, sv_ids), MapTable(sub, rsv, cnt), PropTable(org_ids, org_sizes, None, None, None), *CellAssembly.THRESHOLDS,
                          device=gpu)
        cells, partners, prob, syn_ids = c['syn']
        syn = map_synssv_objects(CellLists(cells, np.arange(len(cells) + 1), cells), partners, prob, syn_ids, 0.4, device=gpu)
        return dict(comp=comp, props=props, m=m, syn=syn)

    flat = staticmethod(lambda o: {k: arrays_of(v) for k, v in o.items()})

    @staticmethod
    def check(c, o):
        from test_gpu_cell_assembly import GRAPH_KEYS, MAP_KEYS, same_bits
        for k in GRAPH_KEYS:
            assert same_bits(getattr(o['comp'], k), c['comp'][k]), k
        assert o['comp'].total_size == c['comp']['total_size']
        assert same_bits(o['props'].size, c['props'][0]) and same_bits(o['props'].bounding_box, c['props'][1]) and same_bits(o['props'].rep_coord, c['props'][2])
        for k in MAP_KEYS + ('accepted', 'org_n_cells', 'org_first_cell'):
            assert same_bits(getattr(o['m'], k), c['want_m'][k]), k
        assert same_bits(o['syn'].syn_begin, c['want_syn'][0]) and same_bits(o['syn'].syn_ids, c['want_syn'][1])


# ---- 11. glia split -----------------------------------------------------------------------------------------------------------------------
def glia_case(seed, n_cells, drop):
    """(edges, ids, boxes, glia, sv_sizes) of _glia_ref.random_cells; every id is named as a node, so the node count does not depend on the
    edges; `drop` > 0 removes that share of the edges (another edge set over the same nodes)."""
    import _glia_ref as R
    rng = np.random.default_rng(seed)
    edges, ids, boxes, glia, _ = R.random_cells(rng, n_cells)
    sv_sizes = rng.integers(1, 10 ** 9, len(ids))
    if drop:
        edges = edges[rng.random(len(edges)) >= drop]
    return edges, ids, boxes, glia, sv_sizes


@row('glia_split')
class GliaSplit:
    T = 1000.0

    @staticmethod
    @functools.lru_cache(None)
    def case(seed, n_cells, drop):
        import _glia_ref as R
        edges, ids, boxes, glia, sv_sizes = glia_case(seed, n_cells, drop)
        want = R.split_table(edges, ids, boxes, glia, GliaSplit.T, ids, sv_sizes=sv_sizes)
        row_of = np.searchsorted(ids, want['node_ids'])
        mixed = want['cell_outcome'][np.searchsorted(want['cell_ids'], want['node_cell'])] == 3
        turned_back = mixed & (glia[row_of] != 0) & (want['node_class'] == 0)       # a tiny glia fragment that step 3 gives back to the neuron
        assert len(ids) > 256 and mixed.any() and turned_back.any() and want['counts'][13:16].min() > 0
        return dict(args=(edges, ids, boxes, glia), sv_sizes=sv_sizes, want=want)

    small = staticmethod(lambda: GliaSplit.case(2, 40, 0.0))
    large = staticmethod(lambda: GliaSplit.case(2, 40, 0.3))

    @staticmethod
    def run(gpu, c):
        from syconn_amd.proc.graphs import split_glia_table
        edges, ids, boxes, glia = c['args']
        s = split_glia_table(edges, ids, boxes, glia, GliaSplit.T, nodes=ids, sv_sizes=c['sv_sizes'], device=gpu)
        return dict(s=s)

    @staticmethod
    def flat(o):
        from test_gpu_glia_split import host_result
        return dict(res=host_result(o['s']), size=o['s'].astrocyte_size, outcome=list(o['s'].n_cells_by_outcome))

    @staticmethod
    def check(c, o):
        from test_gpu_glia_split import assert_same_result, host_result
        assert_same_result(host_result(o['s']), c['want'])
        assert o['s'].astrocyte_size == int(c['want']['counts'][9]) and o['s'].n_cells_by_outcome == tuple(c['want']['counts'][13:16].tolist())


# ---- 12. meshes ---------------------------------------------------------------------------------------------------------------------------
@row('meshes')
class Meshes:
    @staticmethod
    @functools.lru_cache(None)
    def case(density, r):
        import _mesh_ref as R
        from test_gpu_meshes import GOLD, SCALING
        rng = np.random.default_rng(int(density * 100))                            # the noise volume of test_noise_is_closed_and_canonical
        labels = np.array([4, 9, 2 ** 33 + 1, 2 ** 63 + 2, 77], U)
        vol = np.zeros((17, 13, 9), U)
        vol[1:-1, 1:-1, 1:-1] = np.where(rng.random((15, 11, 7)) < density, labels[rng.integers(0, 5, (15, 11, 7))], U(0))
        gold = dict(np.load(GOLD))
        merged = dict(ids=gold[f'{r}_ids'], vert_begin=(gold[f'{r}_vert_begin'] // 3).astype(U), tri_begin=(gold[f'{r}_ind_begin'] // 3).astype(U),
                      vertices=gold[f'{r}_vert'].reshape(-1, 3), indices=gold[f'{r}_ind'].reshape(-1, 3), mesh_bb=gold[f'{r}_bb'], mesh_area=gold[f'{r}_area'])
        return dict(vol=vol, want=R.find_meshes_table(vol, (3, 5, 7), pad=0, ds=None, scaling=SCALING), want_pad=R.find_meshes_table(vol, (1, 0, 2), pad=1, scaling=SCALING),
                    gold=gold, r=r, merged=merged)

    small = staticmethod(lambda: Meshes.case(0.5, 'a'))
    large = staticmethod(lambda: Meshes.case(0.2, 'b'))

    @staticmethod
    def run(gpu, c):
        from syconn_amd.proc.meshes import MeshTable, find_meshes_table
        from test_gpu_meshes import run_host
        gold, r = c['gold'], c['r']
        tables = [find_meshes_table(np.ascontiguousarray(gold['vol'][8 * k:8 * k + 8]), gold['origin'] + (8 * k, 0, 0), pad=1, ds=gold[f'{r}_ds'],
                                    scaling=gold['scaling'], device=gpu) for k in range(3)]
        return dict(noise=run_host(gpu, c['vol'], (3, 5, 7)), padded=run_host(gpu, c['vol'], (1, 0, 2), pad=1), merged=MeshTable.merge(tables, device=gpu))

    flat = staticmethod(lambda o: {k: arrays_of(v) for k, v in o.items()})

    @staticmethod
    def check(c, o):
        from test_gpu_meshes import assert_table
        assert_table(o['noise'], c['want'])                                        # (the area within n_tri 2^-52 relative, all else bit for bit)
        assert_table(o['padded'], c['want_pad'])
        assert_table(o['merged'], c['merged'])
        assert len(c['want']['indices']) > 256


# ---- 13. rendering locations --------------------------------------------------------------------------------------------------------------
@row('locations')
class Locations:
    DS, SCALING = 1500, np.array([10., 10., 20.])

    @staticmethod
    @functools.lru_cache(None)
    def case(seed, first):
        import _locations_gpu as G
        import _locations_ref as R
        begin, verts = G.base_table(seed)
        b = begin.astype(np.int64)
        verts, b = verts[b[first]:], b[first:] - b[first]                          # `first` > 0: fewer segments, every one at another offset
        n = len(b) - 1
        ids, rep = np.arange(n, dtype=U) * 3 + 5, np.arange(3 * n).reshape(n, 3) + 17
        want = {new: [R.sample_locations(verts[b[k]:b[k + 1]], rep[k], Locations.SCALING, Locations.DS, new) for k in range(n)] for new in (True, False)}
        assert len(verts) > 256
        return dict(G=G, ids=ids, begin=b.astype(U), verts=verts, rep=rep, want=want)

    small = staticmethod(lambda: Locations.case(5, 0))
    large = staticmethod(lambda: Locations.case(6, 3))

    @staticmethod
    def run(gpu, c):
        from syconn_amd.proc.locations import sample_locations_table
        return {new: sample_locations_table((c['ids'], c['begin'], c['verts']), Locations.DS, use_new_renderings_locs=new, rep_coords=c['rep'],
                                            scaling=Locations.SCALING, device=gpu) for new in (True, False)}

    flat = staticmethod(lambda o: {str(k): arrays_of(v) for k, v in o.items()})

    @staticmethod
    def check(c, o):
        for new, t in o.items():
            d = t.as_dict()
            assert t.locations.dtype == np.float32 and np.array_equal(t.ids, c['ids'])
            for k, want in enumerate(c['want'][new]):
                assert c['G'].same_bits(d[int(c['ids'][k])], want), (new, k)


# ---- 14. views and the vote over them -----------------------------------------------------------------------------------------------------
@row('views')
class Views:
    WS, NB = (32, 16), 2

    @staticmethod
    @functools.lru_cache(None)
    def case(locs):
        import _views_ref as R
        from test_gpu_views import GOLD
        g = dict(np.load(GOLD))
        n_verts = len(g['m_verts'])
        return dict(R=R, g=g, locs=list(locs), coords=g['m_coords'][list(locs)], label_of=(np.arange(n_verts) // 16 % 3).astype(np.uint8), n_verts=n_verts)

    small = staticmethod(lambda: Views.case((3, 12)))
    large = staticmethod(lambda: Views.case((3, 12, 20, 31, 5)))

    @staticmethod
    def run(gpu, c):
        from syconn_amd.proc import rendering
        from syconn_amd.reps import super_segmentation_helper as ssh
        from test_gpu_views import Cell
        g, R = c['g'], c['R']
        cell = Cell([g['m_tris'].reshape(-1), g['m_verts'].reshape(-1), np.zeros(0, np.float32)])
        views, rot = rendering.render_sso_coords(cell, c['coords'], ws=Views.WS, nb_views=Views.NB, return_rot_mat=True, device=gpu)
        ix, rot_ix = rendering.render_sso_coords_index_views(cell, c['coords'], ws=Views.WS, nb_views=Views.NB, return_rot_matrices=True, device=gpu)
        semseg = np.where(ix == R.BG_INDEX, 3, c['label_of'][np.minimum(ix, c['n_verts'] - 1)]).astype(np.uint8)
        k0 = ssh.semseg2mesh(cell, 'spiness', k=0, index_views=ix, semseg_views=semseg, device=gpu)[3]
        k1 = ssh.semseg2mesh(cell, 'spiness', k=1, index_views=ix, semseg_views=semseg, device=gpu)[3]
        return dict(views=views, rot=rot, ix=ix, rot_ix=rot_ix, semseg=semseg, k0=k0, k1=k1)

    flat = staticmethod(lambda o: o)

    @staticmethod
    def check(c, o):
        g, R = c['g'], c['R']
        E = R.edge_lengths(8000.0, g['m_max_dist'])
        cn = R.normalise(c['coords'], g['m_center'], g['m_max_dist'])
        want, _ = R.render(g['m_vn'], g['m_tris'], cn, o['rot'], E, Views.NB, Views.WS)
        assert o['views'].dtype == np.uint8 and np.array_equal(o['views'][:, 0], want) and (want != 255).any()
        want_ix, _ = R.render(g['m_vn'], g['m_tris'], cn, o['rot_ix'], E, Views.NB, Views.WS, index=True)
        assert o['ix'].dtype == np.uint32 and np.array_equal(o['ix'][:, 0], want_ix) and (want_ix != R.BG_INDEX).any()
        want0, _ = R.vote(o['ix'], o['semseg'], R.BG_INDEX, c['n_verts'], 4, 4)
        assert np.array_equal(o['k0'], want0)
        seen = np.zeros(c['n_verts'], bool)
        seen[o['ix'][o['ix'] != R.BG_INDEX]] = True
        assert np.array_equal(o['k1'][seen], c['label_of'][seen]) and o['k1'].max() <= 2 and 0 < seen.sum() < c['n_verts']


# ---- the four runs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ROWS))
def test_same_results_over_poisoned_and_stale_buffers(gpu, name):
    """Runs A, B, C and D of the module's docstring for one row.  Byte-identical across A, B and D in every returned array; the one
    exception is the split of counts[5] / counts[6] of ``sd_syn_ssv_components`` (a statistic of the concurrent union-find that differs from
    run to run over any buffers), of which the row compares the sum."""
    import torch
    r = ROWS[name]
    small, large = r.small(), r.large()
    arena = A.Arena(ARENA_BYTES, gpu)
    flats, served = {}, set()
    for tag, alloc, case in (('A', A.Fill(0x00), small), ('B', A.Fill(0xFF), small), ('C', arena, large), ('D', arena, small)):
        if tag == 'D':
            arena.rewind()
        before = alloc.calls
        with A.installed(alloc):
            out = r.run(gpu, case)
            flats[tag] = flatten(r.flat(out))
            torch.cuda.synchronize(gpu)
        names = {n for n, _ in alloc.served[before:] if n is not None}
        assert alloc.calls > before, f'run {tag}: the allocator served nothing: the row went past it'
        assert names or not r.scratch, f'run {tag}: no _dev.scratch request was served'
        served |= names
        r.check(case, out)                                                         # against the reference, as the module's own test compares
    assert_identical(flats['A'], flats['B'], 'zero fill against 0xFF fill')
    assert_identical(flats['A'], flats['D'], 'zero fill against the stale arena')
    assert arena.high > 0
    SERVED[name] = served


NOT_COVERED = ()                # only view-network / U-Net workspace names may stand here, each with a comment: none goes through D.scratch


def test_every_scratch_name_of_the_package_was_served():
    """Every name passed as ``D.scratch('<name>'`` under syconn_amd/ was served in some row above (they must have run: this is the
    module's last test)."""
    assert set(SERVED) == set(ROWS), f'rows that did not finish: {sorted(set(ROWS) - set(SERVED))}'
    names = set()
    for folder, _, files in os.walk(os.path.join(ROOT, 'syconn_amd')):
        for f in files:
            if f.endswith('.py'):
                names |= set(re.findall(r"D\.scratch\('([^']+)'", open(os.path.join(folder, f)).read()))
    assert len(names) >= 25
    served = set().union(*SERVED.values())
    assert not sorted(names - served - set(NOT_COVERED)), f'never served: {sorted(names - served - set(NOT_COVERED))}'
    assert not set(NOT_COVERED) & served


# ---- through the C ABI helpers: FILL = 0x00 against 0xFF ----------------------------------------------------------------------------------
def test_abi_glia_split_zero_against_ff(gpu, monkeypatch):
    import _glia_gpu as D
    c = GliaSplit.small()
    edges, ids, boxes, glia = c['args']
    res = {}
    for fill in (0x00, 0xFF):
        monkeypatch.setattr(D, 'FILL', fill)
        rc, counts, out = D.split(gpu, edges, ids, boxes, glia, GliaSplit.T, ids, sv_sizes=c['sv_sizes'])
        assert rc == 0 and counts.tolist() == c['want']['counts'].tolist()
        res[fill] = flatten(dict(counts=counts, out=out))
    assert_identical(res[0x00], res[0xFF], 'sd_glia_split')


def test_abi_components_and_mapping_zero_against_ff(gpu, monkeypatch):
    import _cell_assembly_gpu as D
    c = CellAssembly.small()
    edges, ids, sizes, rep, box_begin, boxes = c['graph']
    _, sv_begin, sv_ids, sub, rsv, cnt, org_ids, org_sizes = c['m']
    res = {}
    for fill in (0x00, 0xFF):
        monkeypatch.setattr(D, 'FILL', fill)
        rc, counts, comp = D.components(gpu, edges, D.table(gpu, ids, sizes, rep, box_begin, boxes), CellAssembly.SCALING, 0.0, False)
        assert rc == 0 and not counts[5:].any()
        rc, mcounts, m = D.mapping(gpu, sv_begin, sv_ids, sub, rsv, cnt, org_ids, org_sizes, *CellAssembly.THRESHOLDS)
        assert rc == 0 and not mcounts[5:].any()
        res[fill] = flatten(dict(counts=counts, comp=comp, mcounts=mcounts, m=m))
    assert_identical(res[0x00], res[0xFF], 'sd_svgraph_components / sd_cell_mapping')
