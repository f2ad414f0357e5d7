"""numpy restatement of the two-level merge behind ``extract_contact_sites`` (a test helper): chunks are folded into per-job worker
results (level 1: ``fold_chunks`` from record arrays, or ``_cs_syntype_ref.worker`` from volumes, or the files the real worker
writes), the worker results are merged in job order, joined and filtered (level 2: ``merge_workers``).  Pinned to the reference's own
functions by golden g18 (test_cs_driver_cpu.py), so the GPU tests can use it on volumes the golden does not hold."""
import os
import pickle
import sys
from collections import defaultdict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cs_syntype_ref as R  # noqa: E402


def job_major(chunk_list, max_n_jobs):
    """Chunks dealt round-robin to min(max_n_jobs, len) jobs, listed job by job."""
    n = min(int(max_n_jobs), len(chunk_list))
    return [c for i in range(n) for c in chunk_list[i::n]]


def jobs_of(chunk_list, max_n_jobs):
    n = min(int(max_n_jobs), len(chunk_list))
    return [chunk_list[i::n] for i in range(n)]


def fold_chunks(chunks):
    """Level 1 from record arrays: `chunks` = [(rec int64 (n, 24), vox int64 (v, 3) with the origin included, origin)] of one job, in
    its processing order -> (cs_props, syn_props, voxels {str(id): (v, 3)}, asym, sym) as the worker pickles them."""
    cs_props, syn_props = [{}, defaultdict(list), {}], [{}, defaultdict(list), {}]
    vox_d, tot_a, tot_s = {}, {}, {}
    for rec, vox, origin in chunks:
        ids = rec[:, 0].view(np.uint64).tolist()
        has = (rec[:, 14] > 0).tolist()
        cp = [dict(zip(ids, rec[:, 1:4].tolist())), dict(zip(ids, rec[:, 5:11].reshape(-1, 2, 3).tolist())), dict(zip(ids, rec[:, 4].tolist()))]
        sel = [k for k, h in zip(ids, has) if h]
        sr = rec[rec[:, 14] > 0]
        sp = [dict(zip(sel, sr[:, 11:14].tolist())), dict(zip(sel, sr[:, 15:21].reshape(-1, 2, 3).tolist())), dict(zip(sel, sr[:, 14].tolist()))]
        R.merge_prop_dicts(cs_props, cp, np.asarray(origin))
        R.merge_prop_dicts(syn_props, sp, np.asarray(origin))
        for k, r in zip(ids, rec.tolist()):
            if r[14]:
                vox_d.setdefault(str(k), []).extend(vox[r[23]:r[23] + r[14]].tolist())
            if r[21]:
                tot_a[k] = tot_a.get(k, 0) + r[21]
            if r[22]:
                tot_s[k] = tot_s.get(k, 0) + r[22]
    return cs_props, syn_props, {k: np.asarray(v, np.int64).reshape(-1, 3) for k, v in vox_d.items()}, tot_a, tot_s


def load_worker_files(dir_props, w):
    """What ``_contact_site_extraction_thread`` wrote for worker `w`, in the shape of ``fold_chunks``."""
    d = os.path.join(str(dir_props), str(w))
    load = lambda n: pickle.load(open(os.path.join(d, f'{n}_{w}.pkl'), 'rb'))
    vox = np.load(os.path.join(d, f'syn_voxels_{w}.npz'))
    return load('cs_props'), load('syn_props'), {k: vox[k] for k in vox.files}, load('tot_asym_cnt'), load('tot_sym_cnt')


def merge_workers(workers, min_cs, min_syn):
    """Level 2: worker results in job order -> (cs, syn): id -> stored entries, ids ascending; what ``_write_props_to_syn_thread``
    stores over all buckets (the bucket only partitions the ids)."""
    rc = [{}, {}]
    boxes = [defaultdict(list), defaultdict(list)]
    size = [defaultdict(int), defaultdict(int)]
    asym, sym, vox = defaultdict(int), defaultdict(int), defaultdict(list)
    for cs_p, syn_p, vx, a, s in workers:
        for t, p in enumerate((cs_p, syn_p)):
            for k in p[0]:
                rc[t][k] = p[0][k]                                   # the later worker's coordinate replaces the earlier one
                boxes[t][k].extend(p[1][k])
                size[t][k] += p[2][k]
        for k in syn_p[0]:
            vox[k].append(np.asarray(vx[str(k)]).reshape(-1, 3))
            asym[k] += a.get(k, 0)
            sym[k] += s.get(k, 0)
    cs, syn = {}, {}
    for k in sorted(rc[0]):
        if size[0][k] < min_cs:
            continue
        b = np.asarray(boxes[0][k], np.int32).reshape(-1, 2, 3)
        cs[k] = dict(rep_coord=np.asarray(rc[0][k], np.int32), bounding_box=np.array([b[:, 0].min(0), b[:, 1].max(0)]), size=size[0][k],
                     boxes=b)
        if k not in rc[1] or size[1][k] < min_syn:
            continue
        b = np.asarray(boxes[1][k], np.int64).reshape(-1, 2, 3)
        syn[k] = dict(rep_coord=np.asarray(rc[1][k], np.int32), bounding_box=np.array([b[:, 0].min(0), b[:, 1].max(0)]), size=size[1][k],
                      boxes=b, sym_prop=sym[k] / size[1][k], asym_prop=asym[k] / size[1][k], cs_id=k, cs_size=size[0][k],
                      voxels=np.concatenate(vox[k]).astype(np.uint32))
    return cs, syn


def golden_dicts(g):
    """The stored entries of golden g18 as (cs, syn) dictionaries."""
    out = []
    for ot in ('cs', 'syn'):
        d = {}
        bb, vb = g[f'{ot}_box_begin'], g.get('syn_vox_begin')
        for i, k in enumerate(g[f'{ot}_ids'].tolist()):
            e = dict(rep_coord=g[f'{ot}_rep_coord'][i], bounding_box=g[f'{ot}_bounding_box'][i], size=int(g[f'{ot}_size'][i]),
                     boxes=g[f'{ot}_boxes'][bb[i]:bb[i + 1]])
            if ot == 'syn':
                e.update(sym_prop=float(g['syn_sym_prop'][i]), asym_prop=float(g['syn_asym_prop'][i]), cs_id=int(g['syn_cs_id'][i]),
                         cs_size=int(g['syn_cs_size'][i]), voxels=g['syn_voxels'][vb[i]:vb[i + 1]])
            d[k] = e
        out.append(d)
    return out


def golden_jobs(g):
    """The chunks of golden g18 grouped by worker: [[(rec, vox, origin)]] in job order."""
    jobs = defaultdict(list)
    cb, vb = g['in_chunk_begin'], g['in_vox_begin']
    for k, w in enumerate(g['in_chunk_worker'].tolist()):
        jobs[w].append((g['in_rec'][cb[k]:cb[k + 1]], g['in_vox'][vb[k]:vb[k + 1]], g['in_origin'][k]))
    return [jobs[w] for w in sorted(jobs)]


def assert_same(got, want, what=''):
    """Two (cs or syn) dictionaries hold the same ids in the same order and equal entries: integers equal, float64 ratios bit-equal,
    rep_coord int32, voxels uint32."""
    assert list(got) == list(want), (what, 'ids')
    for k, w in want.items():
        g = got[k]
        assert set(g) == set(w), (what, k)
        for name, v in w.items():
            if name in ('sym_prop', 'asym_prop'):
                assert np.float64(g[name]).tobytes() == np.float64(v).tobytes(), (what, k, name, g[name], v)
            elif isinstance(v, np.ndarray):
                assert np.asarray(g[name]).shape == v.shape and np.array_equal(g[name], v), (what, k, name)
            else:
                assert int(g[name]) == int(v), (what, k, name, g[name], v)
        assert g['rep_coord'].dtype == np.int32, (what, k)
        if 'voxels' in w:
            assert g['voxels'].dtype == np.uint32 and len(g['voxels']) == g['size'], (what, k)
