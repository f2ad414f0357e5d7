"""GPU: the dataset merge of contact sites (csrc/sd_cs_merge.hip) and the driver ``extract_contact_sites``.

1. golden g18 (the reference's own ``_write_props_to_syn_thread`` on worker files) through the C ABI and through ``ContactSiteMerger``;
2. the driver end to end on a synthetic working directory whose box is no multiple of the chunk size in any axis, in the four
   syn-type modes and with ``transf_func_sj_seg``, for ``max_n_jobs`` 1 and 3 and with a ``cube_of_interest_bb``, against the numpy
   restatement (tests/_cs_driver_ref.py over tests/_cs_syntype_ref.py);
3. the driver against the merge of the files the existing per-chunk worker writes for the same jobs;
4. the kernels at their own structure against numpy: more than one grid stride of records and voxel rows, one id in every chunk, a
   long voxel run, empty inputs, arrays that grow, an overrun that is reported and not written;
5. ``overwrite``, the ``ValueError`` of the chunk size, two runs byte for byte the same."""
import logging
import os
import sys

import numpy as np
import pytest
import scipy.ndimage
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cs_driver_ref as D  # noqa: E402
import _cs_ref  # noqa: E402
import _cs_syntype_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
G18 = os.path.join(HERE, 'golden', 'g18_cs_driver.npz')


@pytest.fixture(scope='module')
def g18():
    return dict(np.load(G18))


# ---- the C ABI, driven directly ----------------------------------------------------------------------------------------------------
def abi_merge(gpu, chunks, min_cs, min_syn, cap_cs=None, cap_syn=None, cap_vox=None, pad=0):
    """Append `chunks` = [(rec int64 (n, 24), vox int64 (v, 3), origin)] and merge once.  Record arrays hold cap_* records (default:
    what is needed) followed by `pad` guard records filled with -1; the scratch of the merges is followed by a guard band of its own
    that must be intact after either merge.  -> dict of numpy arrays (merged columns, cursors, guards)."""
    import torch
    from syconn_amd import _lib as L
    lib = L.load()
    L.check(lib.sd_init(gpu.index or 0), 'sd_init')
    n_all = sum(len(c[0]) for c in chunks)
    s_all = sum(int((c[0][:, 14] > 0).sum()) for c in chunks)
    v_all = sum(len(c[1]) for c in chunks)
    cap_cs = n_all if cap_cs is None else cap_cs
    cap_syn = s_all if cap_syn is None else cap_syn
    cap_vox = v_all if cap_vox is None else cap_vox
    full = lambda n, w, dt: torch.full((max(n + pad, 1), w) if w > 1 else (max(n + pad, 1),), -1, dtype=dt, device=gpu)
    i64, i32 = torch.int64, torch.int32
    cs = [full(cap_cs, 1, i64), full(cap_cs, 3, i32), full(cap_cs, 6, i32), full(cap_cs, 1, i64)]
    syn = [full(cap_syn, 1, i64), full(cap_syn, 3, i32), full(cap_syn, 6, i32)] + [full(cap_syn, 1, i64) for _ in range(4)]
    vox_all = full(cap_vox, 3, i32)
    cursors = torch.zeros(3, dtype=i64, device=gpu)
    keep = []
    for rec, vox, origin in chunks:
        r = torch.from_numpy(np.ascontiguousarray(rec)).to(gpu)
        v = torch.from_numpy(np.ascontiguousarray(vox)).to(gpu)
        keep += [r, v]
        L.check(lib.sd_cs_merge_append(r.data_ptr() if len(rec) else None, len(rec), v.data_ptr() if len(vox) else None, len(vox),
                                       *[int(o) for o in origin], *[t.data_ptr() for t in cs], cap_cs, *[t.data_ptr() for t in syn],
                                       cap_syn, vox_all.data_ptr(), cap_vox, cursors.data_ptr(), None), 'sd_cs_merge_append')
    cur = cursors.cpu().numpy()
    out = dict(cursors=cur, guards_intact=all(bool((t[c:] == -1).all()) for t, c in
                                              [(x, cap_cs) for x in cs] + [(x, cap_syn) for x in syn] + [(vox_all, cap_vox)]))
    if cur[0] > cap_cs or cur[1] > cap_syn or cur[2] > cap_vox:
        return out
    n_cs, n_syn, n_vox = (int(x) for x in cur)
    need = lib.sd_cs_merge_temp_bytes(max(n_cs, n_syn, 1))
    guarded = torch.empty(need + 4096, dtype=torch.uint8, device=gpu)
    guarded[:need] = 0xCD
    guarded[need:] = 0xA5
    tmp = guarded[:need]                                        # the merges are told `need` bytes and may touch no more
    new = lambda n, w, dt: torch.full((max(n, 1), w) if w > 1 else (max(n, 1),), -1, dtype=dt, device=gpu)
    common = lambda n: [new(n, 1, i64), new(n, 1, i64), new(n, 3, i32), new(n, 6, i32), new(n, 1, i32), new(n, 6, i32)]
    c_out, c_cnt = common(n_cs), torch.full((4,), -1, dtype=i64, device=gpu)
    L.check(lib.sd_cs_merge_objects(cs[0].data_ptr(), cs[3].data_ptr(), cs[1].data_ptr(), cs[2].data_ptr(), n_cs, min_cs,
                                    *[t.data_ptr() for t in c_out], c_cnt.data_ptr(), tmp.data_ptr(), tmp.numel(), None),
            'sd_cs_merge_objects')
    u_cs, b_cs, _, all_cs = (int(x) for x in c_cnt.cpu().numpy())
    assert bool((guarded[need:] == 0xA5).all()), 'sd_cs_merge_objects wrote behind sd_cs_merge_temp_bytes(n)'
    s_out, s_cnt = common(n_syn), torch.full((4,), -1, dtype=i64, device=gpu)
    s_more = [new(n_syn, 1, i64), new(n_syn, 1, i64), new(n_syn, 1, i64), new(n_syn, 1, i32), new(n_vox, 3, i32)]
    L.check(lib.sd_cs_merge_synapses(syn[0].data_ptr(), syn[3].data_ptr(), syn[1].data_ptr(), syn[2].data_ptr(), syn[4].data_ptr(),
                                     syn[5].data_ptr(), syn[6].data_ptr(), n_syn, vox_all.data_ptr(), n_vox, c_out[0].data_ptr(),
                                     c_out[1].data_ptr(), u_cs, min_syn, *[t.data_ptr() for t in s_out + s_more], s_cnt.data_ptr(),
                                     tmp.data_ptr(), tmp.numel(), None), 'sd_cs_merge_synapses')
    u_syn, b_syn, v_syn, all_syn = (int(x) for x in s_cnt.cpu().numpy())
    assert bool((guarded[need:] == 0xA5).all()), 'sd_cs_merge_synapses wrote behind sd_cs_merge_temp_bytes(n)'
    for name, o, u, b in (('cs', c_out, u_cs, b_cs), ('syn', s_out, u_syn, b_syn)):
        h = [t.cpu().numpy() for t in o]
        out[f'{name}_ids'], out[f'{name}_size'], out[f'{name}_rep_coord'] = h[0][:u].view(np.uint64), h[1][:u], h[2][:u]
        out[f'{name}_bounding_box'], out[f'{name}_boxes'] = h[3][:u].reshape(u, 2, 3), h[5][:b].reshape(b, 2, 3)
        out[f'{name}_box_begin'] = np.concatenate((h[4][:u].view(np.uint32).astype(np.int64), [b]))
    m = [t.cpu().numpy() for t in s_more]
    out.update(syn_asym=m[0][:u_syn], syn_sym=m[1][:u_syn], syn_cs_size=m[2][:u_syn], syn_voxels=m[4][:v_syn].view(np.uint32),
               syn_vox_begin=np.concatenate((m[3][:u_syn].view(np.uint32).astype(np.int64), [v_syn])), n_ids=(all_cs, all_syn))
    return out


def np_merge(chunks, min_cs, min_syn):
    """The merge of `chunks` (as ``abi_merge`` takes them) in vectorised numpy: the same columns."""
    rec = np.concatenate([c[0].reshape(-1, 24) for c in chunks])
    org = np.concatenate([np.repeat(np.asarray(c[2], np.int64)[None], len(c[0]), 0) for c in chunks]).reshape(-1, 3)
    vbase = np.concatenate([np.full(len(c[0]), b, np.int64) for c, b in zip(chunks, np.cumsum([0] + [len(c[1]) for c in chunks])[:-1])])
    vox = np.concatenate([c[1].reshape(-1, 3) for c in chunks])
    out = {}

    def reduce(ids, size):
        order = np.argsort(ids, kind='stable')
        sid = ids[order]
        head = np.flatnonzero(np.concatenate(([True], sid[1:] != sid[:-1]))) if len(sid) else np.zeros(0, np.int64)
        last = np.concatenate((head[1:], [len(sid)])) - 1 if len(sid) else head
        tot = np.add.reduceat(size[order], head) if len(sid) else np.zeros(0, np.int64)
        return order, sid, head, last, tot

    ids = rec[:, 0].view(np.uint64)
    order, sid, head, last, tot = reduce(ids, rec[:, 4])
    keep_cs = tot >= min_cs
    cs_all = dict(zip(sid[head].tolist(), tot.tolist()))

    def emit(name, order, sid, head, last, tot, keep, rc, lo, hi):
        cnt = last - head + 1
        out[f'{name}_ids'], out[f'{name}_size'] = sid[head][keep], tot[keep]
        out[f'{name}_rep_coord'] = rc[order][last][keep].astype(np.int32)
        if len(head):
            mn, mx = np.minimum.reduceat(lo[order], head), np.maximum.reduceat(hi[order], head)
        else:
            mn = mx = np.zeros((0, 3), np.int64)
        out[f'{name}_bounding_box'] = np.stack([mn, mx], 1)[keep].astype(np.int32)
        rk = np.repeat(keep, cnt)
        out[f'{name}_boxes'] = np.stack([lo[order], hi[order]], 1)[rk].astype(np.int32)
        out[f'{name}_box_begin'] = np.concatenate(([0], np.cumsum(cnt[keep])))
        return rk
    emit('cs', order, sid, head, last, tot, keep_cs, rec[:, 1:4] + org, rec[:, 5:8] + org, rec[:, 8:11] + org)
    s = rec[:, 14] > 0
    srec, sorg, sbase = rec[s], org[s], vbase[s]
    order, sid, head, last, tot = reduce(srec[:, 0].view(np.uint64), srec[:, 14])
    cs_size = np.array([cs_all[k] for k in sid[head].tolist()], np.int64)
    keep = (tot >= min_syn) & (cs_size >= min_cs)
    rk = emit('syn', order, sid, head, last, tot, keep, srec[:, 11:14] + sorg, srec[:, 15:18] + sorg, srec[:, 18:21] + sorg)
    out['syn_asym'] = np.add.reduceat(srec[order, 21], head)[keep] if len(head) else np.zeros(0, np.int64)
    out['syn_sym'] = np.add.reduceat(srec[order, 22], head)[keep] if len(head) else np.zeros(0, np.int64)
    out['syn_cs_size'] = cs_size[keep]
    run_start, run_len = (sbase + srec[:, 23])[order][rk], srec[order, 14][rk]
    begin = np.concatenate(([0], np.cumsum(run_len)))
    src = np.repeat(run_start - begin[:-1], run_len) + np.arange(begin[-1])
    out['syn_voxels'] = vox[src].astype(np.uint32).reshape(-1, 3)
    out['syn_vox_begin'] = np.concatenate(([0], np.cumsum(tot[keep])))
    out['n_ids'] = (len(cs_all), len(head))
    return out


COLUMNS = [f'{t}_{c}' for t in ('cs', 'syn') for c in ('ids', 'size', 'rep_coord', 'bounding_box', 'boxes', 'box_begin')] + \
          ['syn_asym', 'syn_sym', 'syn_cs_size', 'syn_voxels', 'syn_vox_begin']


def same_columns(got, want, what=''):
    for c in COLUMNS:
        assert np.asarray(got[c]).shape == np.asarray(want[c]).shape, (what, c, np.asarray(got[c]).shape, np.asarray(want[c]).shape)
        assert np.array_equal(got[c], want[c]), (what, c)
    assert tuple(got['n_ids']) == tuple(want['n_ids']), what


def golden_chunks(g):
    return [c for job in D.golden_jobs(g) for c in job]


def test_golden_through_c_abi(gpu, g18):
    chunks = golden_chunks(g18)
    mn_cs, mn_syn = (int(v) for v in g18['min_obj_vx'])
    got = abi_merge(gpu, chunks, mn_cs, mn_syn, pad=3)
    assert got['guards_intact']
    for c in COLUMNS:
        if c in ('syn_asym', 'syn_sym'):
            continue
        assert np.array_equal(got[c], g18[c]), c
        assert np.asarray(got[c]).shape == g18[c].shape, c
    for t in ('asym', 'sym'):                                   # count / size as float64, bit for bit the reference's int / int
        assert (got[f'syn_{t}'] / got['syn_size']).tobytes() == g18[f'syn_{t}_prop'].tobytes(), t
    assert np.array_equal(got['syn_ids'], g18['syn_cs_id'])
    same_columns(got, np_merge(chunks, mn_cs, mn_syn), 'np_merge on g18')      # pins the numpy form used for the large cases below


def fake_result(gpu, rec, vox):
    import torch
    from syconn_amd.extraction.find_object_properties import CsSyntype
    return CsSyntype(torch.from_numpy(np.ascontiguousarray(rec)).to(gpu), torch.from_numpy(np.ascontiguousarray(vox)).to(gpu))


def test_golden_through_merger_and_growth(gpu, g18):
    """``ContactSiteMerger`` with record and voxel arrays that start far too small and grow between chunks; the dictionary views hold
    exactly what the reference stores."""
    from syconn_amd.extraction.cs_extraction_steps import ContactSiteMerger, CsTable, SynTable
    mn = dict(cs=int(g18['min_obj_vx'][0]), syn=int(g18['min_obj_vx'][1]))
    w_cs, w_syn = D.golden_dicts(g18)
    for caps in ((2, 3), (1 << 14, 1 << 18)):
        m = ContactSiteMerger(mn, gpu, capacity=caps[0], vox_capacity=caps[1])
        for rec, vox, origin in golden_chunks(g18):
            m.add_chunk(fake_result(gpu, rec, vox), origin)
        if caps[0] == 2:
            assert m.cs.capacity > 2 and m.vox.capacity > 3
        cs_t, syn_t = m.finish()
        assert type(cs_t) is CsTable and type(syn_t) is SynTable
        D.assert_same(cs_t.as_dict(), w_cs, 'cs')
        D.assert_same(syn_t.as_dict(), w_syn, 'syn')
        assert syn_t.sym_prop.tobytes() == g18['syn_sym_prop'].tobytes() and syn_t.asym_prop.tobytes() == g18['syn_asym_prop'].tobytes()
        assert cs_t.ids.dtype == np.uint64 and syn_t.voxels.dtype == np.uint32 and cs_t.rep_coords.dtype == np.int32
        assert cs_t.storage_keys(1000) == [b for i, b in zip(g18['key_ids'].tolist(), g18['key_bucket_1000'].tolist())
                                           if i in set(cs_t.ids.tolist())]
        assert (m.n_cs_all, m.n_syn_all) == (len(g18['key_ids']), len(np.unique(g18['in_rec'][g18['in_rec'][:, 14] > 0, 0])))


# ---- 4. the kernels at their own structure -----------------------------------------------------------------------------------------
def synth_chunk(rng, ids, origin, max_syn=2, p_syn=0.6):
    """Records for `ids` (uint64, unique) with small random sites; voxel rows in record order."""
    n = len(ids)
    ids = np.sort(ids)
    rec = np.zeros((n, 24), np.int64)
    rec[:, 0] = ids.view(np.int64)
    lo = rng.integers(0, 500, (n, 3))
    rec[:, 5:8], rec[:, 8:11] = lo, lo + rng.integers(1, 9, (n, 3))
    rec[:, 1:4] = lo + rng.integers(0, 2, (n, 3))
    rec[:, 4] = rng.integers(1, 30, n)
    ns = np.where(rng.random(n) < p_syn, rng.integers(1, max_syn + 1, n), 0)
    rec[:, 14] = ns
    has = ns > 0
    rec[has, 15:18], rec[has, 18:21], rec[has, 11:14] = lo[has], lo[has] + 2, lo[has] + 1
    rec[:, 21] = rng.integers(0, 2, n) * has
    rec[:, 22] = (ns - rec[:, 21]) * rng.integers(0, 2, n)
    rec[:, 23] = np.cumsum(ns) - ns
    vox = rng.integers(0, 2 ** 20, (int(ns.sum()), 3)) + np.asarray(origin)
    return rec, vox.astype(np.int64), np.asarray(origin, np.int64)


def test_record_counts_at_a_scratch_boundary(gpu):
    """33 + 31 + 1 = 65 cs records of which 64 carry syn voxels: 4 (n + 1) bytes of a u32 scratch array cross a 256-byte boundary
    in the cs merge and 4 n bytes end on one in the synapse merge (``abi_merge`` checks the guard band behind the scratch)."""
    rng = np.random.default_rng(40)
    ids = rng.permutation(np.arange(1, 60, dtype=np.uint64) * np.uint64(2 ** 58 + 3))
    chunks = [synth_chunk(rng, ids[:33], (0, 0, 0), p_syn=1.0), synth_chunk(rng, ids[20:51], (64, 0, 0), p_syn=1.0),
              synth_chunk(rng, ids[58:], (0, 64, 0), p_syn=0.0)]
    got, want = abi_merge(gpu, chunks, 20, 2), np_merge(chunks, 20, 2)
    assert got['cursors'].tolist()[:2] == [65, 64] and 0 < len(want['syn_ids']) < want['n_ids'][1]
    same_columns(got, want)


def test_more_than_one_grid_stride(gpu):
    """1.2 M records and 1.8 M voxel rows in one chunk: every grid-stride loop of the append and merge kernels (4096 x 256 threads)
    takes a second trip; ids from the whole uint64 range, many shared between the three chunks."""
    rng = np.random.default_rng(41)
    pool = np.unique(np.concatenate((rng.integers(1, 2 ** 64 - 1, 1_500_000, dtype=np.uint64),
                                     np.array([1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 2], np.uint64))))
    chunks = [synth_chunk(rng, rng.choice(pool, 1_200_000, replace=False), (0, 0, 0), max_syn=4),
              synth_chunk(rng, rng.choice(pool, 400_000, replace=False), (512, 0, 0), max_syn=4),
              synth_chunk(rng, rng.choice(pool, 300_000, replace=False), (0, 512, 1024), max_syn=4)]
    assert len(chunks[0][0]) > 4096 * 256 and len(chunks[0][1]) > 4096 * 256
    got = abi_merge(gpu, chunks, 8, 2)
    want = np_merge(chunks, 8, 2)
    assert len(want['syn_voxels']) > 4096 * 256 and 0 < len(want['cs_ids']) < want['n_ids'][0]
    assert (want['cs_ids'] >= 2 ** 63).any() and (np.diff(want['cs_box_begin']) == 3).any()
    same_columns(got, want)


def test_one_id_in_every_chunk_and_a_long_run(gpu):
    rng = np.random.default_rng(42)
    common, long_id = np.uint64(2 ** 63 + 17), np.uint64(99)
    chunks = []
    for k in range(37):
        ids = np.unique(np.concatenate((rng.integers(1, 50, 6, dtype=np.uint64) * np.uint64(1000), [common])))
        chunks.append(synth_chunk(rng, ids, (64 * k, 0, 0), max_syn=3, p_syn=1.0))
    rec, vox, org = synth_chunk(rng, np.array([long_id, common]), (5, 6, 7), p_syn=1.0)
    rec[:, 14], rec[:, 23] = (5000, 1), (0, 5000)                  # one run far longer than 256 rows
    rec[:, 21], rec[:, 22] = (4999, 0), (1, 1)
    chunks.append((rec, rng.integers(0, 2 ** 31, (5001, 3)).astype(np.int64), org))
    got, want = abi_merge(gpu, chunks, 1, 1), np_merge(chunks, 1, 1)
    i = want['syn_ids'].tolist().index(int(common))
    assert np.diff(want['syn_box_begin'])[i] == 38 and np.diff(want['syn_vox_begin'])[want['syn_ids'].tolist().index(99)] == 5000
    same_columns(got, want)


def test_empty_inputs(gpu):
    """No chunk at all; chunks without sites; sites without syn voxels (an empty syn table)."""
    rng = np.random.default_rng(43)
    empty = (np.zeros((0, 24), np.int64), np.zeros((0, 3), np.int64), np.zeros(3, np.int64))
    for chunks in ([], [empty], [empty, synth_chunk(rng, np.arange(1, 40, dtype=np.uint64), (0, 0, 0), p_syn=0.0), empty]):
        got, want = abi_merge(gpu, chunks, 2, 2), np_merge(chunks + [empty], 2, 2)
        same_columns(got, want)
        assert len(got['syn_ids']) == 0 and len(got['syn_voxels']) == 0 and got['cursors'][1] == 0


def test_overrun_is_reported_not_written(gpu):
    rng = np.random.default_rng(44)
    chunks = [synth_chunk(rng, np.arange(1, 3001, dtype=np.uint64), (0, 0, 0), p_syn=1.0) for _ in range(2)]
    n, v = 6000, sum(len(c[1]) for c in chunks)
    for caps in (dict(cap_cs=4000), dict(cap_syn=100), dict(cap_vox=v - 10), dict(cap_cs=0, cap_syn=0, cap_vox=0)):
        got = abi_merge(gpu, chunks, 1, 1, pad=64, **caps)
        assert got['cursors'].tolist() == [n, n, v]                # counted past the maximum
        assert got['guards_intact'] and 'cs_ids' not in got


def test_merge_limits(gpu):
    import torch
    from syconn_amd import _lib as L
    lib = L.load()
    d = torch.zeros(64, dtype=torch.int64, device=gpu)
    p = d.data_ptr()
    assert lib.sd_cs_merge_objects(p, p, p, p, 1 << 32, 1, p, p, p, p, p, p, p, p, 1 << 40, None) == L.SD_ERR_INVALID
    assert lib.sd_cs_merge_objects(p, p, p, p, 8, 1, p, p, p, p, p, p, p, p, 16, None) == L.SD_ERR_INVALID           # scratch too small
    assert lib.sd_cs_merge_synapses(*[p] * 7, 8, p, 1 << 32, p, p, 0, 1, *[p] * 13, 1 << 40, None) == L.SD_ERR_INVALID
    assert lib.sd_cs_merge_append(None, 5, None, 0, 0, 0, 0, *[p] * 4, 8, *[p] * 7, 8, p, 8, p, None) == L.SD_ERR_INVALID


# ---- 2., 3., 5. the driver on a synthetic working directory -------------------------------------------------------------------------
BOX = (100, 90, 50)                   # x, y, z: no multiple of the chunk size in any axis -> 2 x 2 x 2 chunks with overhang
CHUNK = (64, 64, 32)
CUBE = (32, 32, 16)
FILTER = [7, 7, 3]                    # a small stencil keeps the numpy restatement fast; the default is covered by the worker's test
N_CHUNKS = 8


def _kd(path, box=BOX, data_xyz=None, raw=None):
    from syconn_amd.knossos import KnossosDataset
    kd = KnossosDataset()
    kd._cube_shape = CUBE
    kd.initialize_without_conf(path, box, (10, 10, 20), 'synth', mags=[1])
    if data_xyz is not None:
        kd.save_seg(offset=(0, 0, 0), mags=[1], data=np.ascontiguousarray(data_xyz.swapaxes(0, 2)), data_mag=1)
    if raw is not None:
        kd.save_raw(offset=(0, 0, 0), mags=[1], data=np.ascontiguousarray(raw.swapaxes(0, 2)), data_mag=1)
    return kd


def _sj_seg_transform(seg):
    return (seg > 2).astype(np.uint8)


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    rng = np.random.default_rng(11)
    root = tmp_path_factory.mktemp('cs_driver_kd')
    half = tuple(s // 2 for s in BOX)
    lab = np.zeros(half, np.uint64)
    pts = tuple(rng.integers(0, s, 40) for s in half)
    lab[pts] = np.unique(rng.integers(1, 2 ** 34, 40, dtype=np.uint64))[rng.permutation(40)]
    _, ind = scipy.ndimage.distance_transform_edt(lab == 0, return_indices=True)
    cells = lab[tuple(ind)].repeat(2, 0).repeat(2, 1).repeat(2, 2)
    cells[rng.random(BOX) < 0.005] = 0
    noise = scipy.ndimage.gaussian_filter(rng.random(BOX), 2.0)
    noise = (noise - noise.min()) / (noise.max() - noise.min())
    sj_raw = (255 * noise ** 2).astype(np.uint8)
    sj_seg = (noise > 0.45).astype(np.uint64) * 4 + rng.integers(0, 3, BOX).astype(np.uint64)
    type_raw = [(255 * scipy.ndimage.gaussian_filter(rng.random(BOX), 1.5) * 1.8).clip(0, 255).astype(np.uint8) for _ in range(2)]
    type_lab = rng.integers(0, 4, BOX).astype(np.uint64)
    p = {k: str(root / k) for k in ('cells', 'sj', 'sym_raw', 'asym_raw', 'sym_lab', 'asym_lab', 'types', 'zeros')}
    _kd(p['cells'], data_xyz=cells)
    _kd(p['sj'], data_xyz=sj_seg, raw=sj_raw)
    _kd(p['sym_raw'], raw=type_raw[0])
    _kd(p['asym_raw'], raw=type_raw[1])
    _kd(p['sym_lab'], data_xyz=type_lab)
    _kd(p['asym_lab'], data_xyz=rng.integers(0, 4, BOX).astype(np.uint64))
    _kd(p['types'], data_xyz=type_lab)
    _kd(p['zeros'], data_xyz=np.zeros(BOX, np.uint64))
    return p


MODES = {
    'unavailable': dict(syntype_avail=False, paths={}, labels=(None, None)),
    'two_raw': dict(syntype_avail=True, paths={'kd_sym': 'sym_raw', 'kd_asym': 'asym_raw'}, labels=(None, None)),
    'two_labels': dict(syntype_avail=True, paths={'kd_sym': 'sym_lab', 'kd_asym': 'asym_lab'}, labels=(2, 3)),
    'one_kd': dict(syntype_avail=True, paths={'kd_sym': 'types', 'kd_asym': 'types'}, labels=(1, 3)),
}
MIN_VX = {'cs': 12, 'syn': 4}


class WorkDir:
    """A working directory with its config.yml, installed into ``global_params`` for the duration of a ``with`` block."""

    def __init__(self, tmp_path, dataset, mode, cells='cells'):
        self.m = MODES['unavailable' if mode == 'transf_func' else mode]
        self.transf = _sj_seg_transform if mode == 'transf_func' else None
        self.dataset, self.cells = dataset, dataset[cells]
        self.wd = str(tmp_path / f'wd_{mode}')
        os.makedirs(self.wd, exist_ok=True)
        self.paths = {'kd_seg': self.cells, 'kd_sj': dataset['sj'], **{k: dataset[v] for k, v in self.m['paths'].items()}}
        sym_label, asym_label = self.m['labels']
        with open(os.path.join(self.wd, 'config.yml'), 'w') as f:
            yaml.safe_dump({'scaling': [10, 10, 20], 'syntype_avail': self.m['syntype_avail'], 'paths': self.paths,
                            'cell_objects': {'sym_label': sym_label, 'asym_label': asym_label, 'cs_filtersize': FILTER,
                                             'min_obj_vx': dict(MIN_VX)}}, f)

    def __enter__(self):
        from syconn_amd import global_params
        c = global_params.config
        self.saved = global_params.wd, c._wd, c._entries, c.initialized
        self.env = os.environ.pop('syconn_wd', None)
        global_params.wd = self.wd
        c._load(self.wd)
        return self

    def __exit__(self, *exc):
        from syconn_amd import global_params
        global_params.wd = self.saved[0]
        global_params.config._wd, global_params.config._entries, global_params.config.initialized = self.saved[1:]
        if self.env is not None:
            os.environ['syconn_wd'] = self.env

    def ref_cfg(self):
        sym_label, asym_label = self.m['labels']
        return dict(cs_filtersize=FILTER, cs_dilation=2, sj_ops=['binary_opening', 'binary_closing', 'binary_erosion'],
                    scaling=[10, 10, 20], sj_thresh=0.19047619, syntype=self.m['syntype_avail'], sym_label=sym_label,
                    asym_label=asym_label, same_kd=self.m['paths'].get('kd_sym') == self.m['paths'].get('kd_asym'))

    def chunks(self):
        from syconn_amd.knossos import ChunkDataset
        from syconn_amd.handler import basics
        cset = ChunkDataset().initialize(basics.kd_factory(self.cells), BOX, CHUNK, '', box_coords=[0, 0, 0], fit_box_size=True)
        return cset

    def reference(self, chunk_numbers, max_n_jobs):
        """The numpy restatement: one ``_cs_syntype_ref.worker`` per job of ``chunkify(chunk_numbers, max_n_jobs)``, merged in job
        order.  -> (cs, syn, cores)"""
        from syconn_amd.handler import basics
        cset = self.chunks()
        kd_sym = basics.kd_factory(self.paths['kd_sym']) if self.m['syntype_avail'] else None
        kd_asym = basics.kd_factory(self.paths['kd_asym']) if self.m['syntype_avail'] else None
        workers, cores = [], []
        for job in D.jobs_of(list(chunk_numbers), max_n_jobs):
            w = R.worker([cset.chunk_dict[k] for k in job], basics.kd_factory(self.cells), basics.kd_factory(self.dataset['sj']),
                         self.ref_cfg(), self.transf, kd_sym, kd_asym)
            workers.append(w[:5])
            cores += w[5]
        cs, syn = D.merge_workers(workers, MIN_VX['cs'], MIN_VX['syn'])
        return cs, syn, cores

    def check_cores(self, cores):
        from syconn_amd.handler import basics
        kd_cs = basics.kd_factory(f'{self.wd}/knossosdatasets/cs_seg/')
        kd_syn = basics.kd_factory(f'{self.wd}/knossosdatasets/syn_seg/')
        assert tuple(kd_cs.boundary) == BOX and tuple(kd_cs._cube_shape) == CUBE and kd_cs.experiment_name == 'synth'
        # the cores over the whole box: a KnossosDataset keeps what lies inside its boundary (closing and dilation reach past it)
        want = [np.zeros(BOX[::-1], np.uint64) for _ in range(2)]
        for off, cs_core, syn_core in cores:
            hi = np.minimum(np.asarray(off) + cs_core.shape[::-1], BOX)
            dst = tuple(slice(int(off[a]), int(hi[a])) for a in (2, 1, 0))
            src = tuple(slice(0, int(hi[a] - off[a])) for a in (2, 1, 0))
            want[0][dst], want[1][dst] = cs_core[src], syn_core[src]
        assert np.array_equal(kd_cs.load_seg(size=BOX, offset=(0, 0, 0), mag=1), want[0])
        assert np.array_equal(kd_syn.load_seg(size=BOX, offset=(0, 0, 0), mag=1), want[1])
        n_site_vox = int((want[1] != 0).sum())
        return n_site_vox


@pytest.fixture(scope='module', autouse=True)
def cached_contact_steps():
    """The partner stencil and the closing of a chunk do not depend on the syn-type mode: the restatement computes them once per
    distinct input (a cache in front of the two slow numpy functions, keyed by the input bytes)."""
    import hashlib
    saved = _cs_ref.contact_partners, _cs_ref.close_dilate
    cache = {}

    def memo(fn):
        def wrapped(*args):
            key = (fn.__name__,) + tuple(hashlib.sha1(np.ascontiguousarray(a)).hexdigest() if isinstance(a, np.ndarray) else str(a)
                                         for a in args)
            if key not in cache:
                cache[key] = fn(*args)
            return cache[key].copy()
        return wrapped
    _cs_ref.contact_partners, _cs_ref.close_dilate = memo(saved[0]), memo(saved[1])
    yield
    _cs_ref.contact_partners, _cs_ref.close_dilate = saved


def run_driver(max_n_jobs, transf=None, **kw):
    from syconn_amd.extraction.cs_extraction_steps import extract_contact_sites
    return extract_contact_sites(chunk_size=CHUNK, cube_shape=CUBE, max_n_jobs=max_n_jobs, transf_func_sj_seg=transf, **kw)


@pytest.mark.parametrize('max_n_jobs', [1, 3])
@pytest.mark.parametrize('mode', list(MODES) + ['transf_func'])
def test_driver_end_to_end(gpu, dataset, tmp_path, mode, max_n_jobs):
    with WorkDir(tmp_path, dataset, mode) as w:
        cs, syn = run_driver(max_n_jobs, w.transf)
        want_cs, want_syn, cores = w.reference(range(N_CHUNKS), max_n_jobs)
        D.assert_same(cs, want_cs, 'cs')
        D.assert_same(syn, want_syn, 'syn')
        assert len(cores) == N_CHUNKS and w.check_cores(cores) > 0
        assert len(want_syn) > 3 and any(len(v['boxes']) > 1 for v in want_syn.values())            # ids shared between chunks
        assert len(want_cs) > len(want_syn)
        if w.m['syntype_avail']:
            assert any(v['sym_prop'] > 0 for v in want_syn.values()) and any(v['asym_prop'] > 0 for v in want_syn.values())
        assert not os.path.exists(f'{w.wd}/tmp/tmp_props_cssyn')                                    # no worker files


def test_driver_order_matters_and_default_jobs(gpu, dataset, tmp_path):
    """max_n_jobs = 1 and 3 differ in a representative coordinate (the test above would pass with any order otherwise); the default
    (one chunk per job) is the chunk list's order = one job."""
    with WorkDir(tmp_path, dataset, 'one_kd') as w:
        one = run_driver(1, as_tables=True)
        three = run_driver(3, as_tables=True, overwrite=True)
        default = run_driver(None, as_tables=True)
        assert np.array_equal(one[0].ids, three[0].ids) and not np.array_equal(one[0].rep_coords, three[0].rep_coords)
        for a, b in zip(one, default):
            for name, v in vars(a).items():
                assert v.tobytes() == getattr(b, name).tobytes() and v.dtype == getattr(b, name).dtype, name


def test_driver_cube_of_interest(gpu, dataset, tmp_path):
    """A box inside the upper x half selects four of the eight chunks."""
    from syconn_amd.extraction.object_extraction_wrapper import calculate_chunk_numbers_for_box
    with WorkDir(tmp_path, dataset, 'two_raw') as w:
        bb = [np.array([70, 5, 3]), np.array([95, 80, 45])]
        sel, _ = calculate_chunk_numbers_for_box(w.chunks(), bb[0], bb[1] - bb[0] + 1)
        assert len(sel) == 4
        cs, syn = run_driver(3, cube_of_interest_bb=bb)
        want_cs, want_syn, cores = w.reference(sel, 3)
        D.assert_same(cs, want_cs, 'cs')
        D.assert_same(syn, want_syn, 'syn')
        assert len(cores) == 4 and len(want_syn) > 0
        w.check_cores(cores)
        from syconn_amd.handler import basics                      # the other half of the box was not written
        kd_cs = basics.kd_factory(f'{w.wd}/knossosdatasets/cs_seg/')
        assert not kd_cs.load_seg(size=(64, 90, 50), offset=(0, 0, 0), mag=1).any()


@pytest.mark.parametrize('mode', ['one_kd', 'transf_func'])
def test_driver_equals_merged_worker_files(gpu, dataset, tmp_path, mode):
    """The new path against the existing one: the files ``_contact_site_extraction_thread`` writes for the jobs of ``max_n_jobs = 3``,
    merged by the helper, and both datasets' cubes."""
    from syconn_amd.extraction.cs_extraction_steps import _contact_site_extraction_thread
    from syconn_amd.handler import basics
    with WorkDir(tmp_path, dataset, mode) as w:
        cs, syn = run_driver(3, w.transf)
        kd_new = [basics.kd_factory(f'{w.wd}/knossosdatasets/{t}_seg/').load_seg(size=BOX, offset=(0, 0, 0), mag=1) for t in ('cs', 'syn')]
        for t in ('cs', 'syn'):
            _kd(f'{w.wd}/knossosdatasets/{t}_seg/')                # the worker writes into datasets its caller initialised
        cset = w.chunks()
        props = str(tmp_path / 'props')
        for nr, job in enumerate(D.jobs_of(list(range(N_CHUNKS)), 3)):
            _contact_site_extraction_thread(([cset.chunk_dict[k] for k in job], w.cells, nr, props, w.transf))
        want_cs, want_syn = D.merge_workers([D.load_worker_files(props, nr) for nr in range(3)], MIN_VX['cs'], MIN_VX['syn'])
        D.assert_same(cs, want_cs, 'cs')
        D.assert_same(syn, want_syn, 'syn')
        assert len(want_syn) > 3
        for t, new in zip(('cs', 'syn'), kd_new):
            old = basics.kd_factory(f'{w.wd}/knossosdatasets/{t}_seg/').load_seg(size=BOX, offset=(0, 0, 0), mag=1)
            assert np.array_equal(old, new) and new.any(), t


def test_driver_all_zero_segmentation(gpu, dataset, tmp_path, caplog):
    with WorkDir(tmp_path, dataset, 'two_labels', cells='zeros') as w:
        log = logging.getLogger('test_cs_driver_zero')
        with caplog.at_level(logging.INFO, logger=log.name):
            cs_t, syn_t = run_driver(3, as_tables=True, log=log)
        assert len(cs_t) == 0 and len(syn_t) == 0 and cs_t.boxes.shape == (0, 2, 3) and syn_t.voxels.shape == (0, 3)
        assert cs_t.as_dict() == {} and syn_t.as_dict() == {} and syn_t.sym_prop.shape == (0,)
        msgs = [(r.levelno, r.getMessage()) for r in caplog.records]
        assert (logging.CRITICAL, 'WARNING: Did not find any synapses during extraction step.') in msgs
        assert (logging.INFO, 'Finished extraction of initial contact sites (#objects: 0) and synapses (#objects: 0).') in msgs
        from syconn_amd.handler import basics
        assert not basics.kd_factory(f'{w.wd}/knossosdatasets/cs_seg/').load_seg(size=BOX, offset=(0, 0, 0), mag=1).any()


def test_driver_overwrite_valueerror_and_determinism(gpu, dataset, tmp_path, caplog):
    from syconn_amd.extraction.cs_extraction_steps import extract_contact_sites
    with WorkDir(tmp_path, dataset, 'two_raw') as w:
        with pytest.raises(ValueError, match='Chunk size must be divisible by cube shape.'):
            extract_contact_sites(chunk_size=(64, 64, 40), cube_shape=CUBE)
        assert not os.path.exists(f'{w.wd}/knossosdatasets')      # refused before anything was touched
        log = logging.getLogger('test_cs_driver_log')
        with caplog.at_level(logging.INFO, logger=log.name):
            first = run_driver(3, as_tables=True, log=log)
        n_cs = len(np.unique(np.concatenate([c[1][c[1] != 0] for c in w.reference(range(N_CHUNKS), 3)[2]])))
        assert any(r.getMessage().startswith(f'Finished extraction of initial contact sites (#objects: {n_cs}) and synapses')
                   for r in caplog.records)
        assert not any(r.levelno == logging.CRITICAL for r in caplog.records)
        for t in ('syn_0', 'cs_0'):
            os.makedirs(f'{w.wd}/{t}')
            open(f'{w.wd}/{t}/marker', 'w').close()
            with pytest.raises(FileExistsError):
                run_driver(3)
            with pytest.raises(FileExistsError):
                run_driver(3, overwrite=False)
            second = run_driver(3, as_tables=True, overwrite=True)
            assert not os.path.exists(f'{w.wd}/syn_0') and not os.path.exists(f'{w.wd}/cs_0')
            for a, b in zip(first, second):                         # two runs: byte-identical tables
                assert sorted(vars(a)) == sorted(vars(b))
                for name, v in vars(a).items():
                    assert v.dtype == getattr(b, name).dtype and v.tobytes() == getattr(b, name).tobytes(), name
        assert len(first[1]) > 0


def test_driver_refuses_bad_config_before_touching_data(gpu, dataset, tmp_path):
    from syconn_amd import global_params
    with WorkDir(tmp_path, dataset, 'one_kd') as w:
        global_params.config._entries['cell_objects']['asym_label'] = 1           # identical datasets and labels
        with pytest.raises(ValueError, match='identical'):
            run_driver(3)
        assert not os.path.exists(f'{w.wd}/knossosdatasets')
