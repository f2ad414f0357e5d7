"""Label-statistics chain on the device (`sd_segstats_scan` -> `sd_segstats_compact_*` -> `sd_chunkprops_append` / `sd_chunkpairs_append`
-> `sd_propmerge_*`) against the numpy oracle or analytic expectations, exactly (integer work): every form of the scan kernel,
misaligned volumes, saturated LDS tables, sizes past the scan's grid cap and past one grid stride of the table kernels, exactly full
tables, the 64-bit coordinate decode and the switches a process reads once.  tests/test_segstats_edges_cpu.py shows on the CPU that
the cases sit on the edges they are named after."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import _segstats_cases as SC

pytestmark = pytest.mark.gpu
ROOT = SC.ROOT
FORM_SHAPES = ((9, 10, 72), (9, 10, 71))          # rows % 4 == 0 -> four-voxel forms; else the one-voxel form
CONFIGS = [(True, n) for n in range(0, 9)] + [(False, n) for n in range(1, 9)]


def _segstats(*a, **kw):
    from syconn_amd.extraction.find_object_properties import segstats
    return segstats(*a, **kw)


def _both_forms(monkeypatch, cell, subs, want, gpu, what, want_props=True, **kw):
    """The form the library picks and, for rows of a multiple of 4, the one-voxel form as well: both equal the oracle and each other."""
    monkeypatch.delenv('SD_SEGSTATS_V1', raising=False)
    r = _segstats(cell, subs, want_props=want_props, device=gpu, **kw)
    SC.assert_equals_oracle(r, want, want_props, f'{what} (picked form)')
    shape = (cell if cell is not None else subs[0]).shape
    if shape[2] % 4 == 0:
        monkeypatch.setenv('SD_SEGSTATS_V1', '1')
        r1 = _segstats(cell, subs, want_props=want_props, device=gpu, **kw)
        monkeypatch.delenv('SD_SEGSTATS_V1', raising=False)
        SC.assert_equals_oracle(r1, want, want_props, f'{what} (one-voxel form)')
        SC.assert_same_result(r, r1, what)
    return r


# ---- 1. form matrix -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.uint32, np.uint64])
@pytest.mark.parametrize('has_cell,n_sub', CONFIGS)
def test_every_scan_form_equals_oracle(gpu, monkeypatch, has_cell, n_sub, dtype):
    """Cell present with 0-8 subcell volumes, cell absent with 1-8, rows of a multiple of 4 and not, properties on and off: the 10
    instantiations of `k_segstats_scan` per label type.  Ids include 2^32 - 1 (uint32), 2^63, 2^63 + 7 and 2^64 - 1 (uint64)."""
    for shape in FORM_SHAPES:
        cell, subs = SC.form_case(shape, has_cell, n_sub, dtype)
        want = SC.oracle(cell, subs)
        for wp in ((True, False) if has_cell else (True,)):
            _both_forms(monkeypatch, cell, subs, want, gpu, f'{shape} cell={has_cell} n_sub={n_sub} props={wp}', want_props=wp)
    # fewer than 256 voxels: one partly filled wave
    cell, subs = SC.form_case((3, 5, 12), has_cell, n_sub, dtype)
    _both_forms(monkeypatch, cell, subs, SC.oracle(cell, subs), gpu, 'tiny')


def test_too_many_volumes_and_mixed_dtypes_are_refused(gpu):
    from syconn_amd import _lib as L
    n = SC.kernel_constants()['MAX_SUB']
    cell, subs = SC.form_case((3, 5, 12), True, n + 1, np.uint64)
    with pytest.raises(ValueError, match='sd_segstats_scan'):
        _segstats(cell, subs, device=gpu)
    with pytest.raises(ValueError, match='sd_segstats_scan'):
        _segstats(None, subs, device=gpu)
    with pytest.raises(TypeError):
        _segstats(cell, [subs[0].astype(np.uint32)], device=gpu)
    r = _segstats(cell, subs[:n], device=gpu)                       # the limit itself is served, and the library is still usable
    SC.assert_equals_oracle(r, SC.oracle(cell, subs[:n]))
    assert L.load().sd_last_error() is not None


# ---- 2. misaligned pointers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.uint32, np.uint64])
@pytest.mark.parametrize('which', ['all', 'cell', 'last_sub', 'none'])
@pytest.mark.parametrize('n_sub', [2, 5])
def test_misaligned_volumes_take_the_one_voxel_form(gpu, which, n_sub, dtype):
    """Device tensors cut from a flat buffer at an offset of one element: rows are a multiple of 4, so only the pointer check keeps the
    scan away from 16-byte loads."""
    shape = FORM_SHAPES[0]
    cell, subs = SC.form_case(shape, True, n_sub, dtype, seed=7)
    mis = [which in ('all', 'cell')] + [which == 'all' or (which == 'last_sub' and k == n_sub - 1) for k in range(n_sub)]
    d = [SC.device_volume(v, gpu, m) for v, m in zip([cell] + subs, mis)]
    for t, m in zip(d, mis):
        assert (t.data_ptr() % 16 != 0) == m
        assert not m or t.data_ptr() % 16 == np.dtype(dtype).itemsize
    want = SC.oracle(cell, subs)
    SC.assert_equals_oracle(_segstats(d[0], d[1:], device=gpu), want, True, f'misaligned {which}')
    SC.assert_equals_oracle(_segstats(d[0], d[1:], want_props=False, device=gpu), want, False, f'misaligned {which}, counts only')
    if which != 'cell':
        SC.assert_equals_oracle(_segstats(None, d[1:], device=gpu), (None, want[1], []), True, f'misaligned {which}, no cell')


# ---- 3. saturated and mixed LDS tables ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(SC.SATURATED) + sorted(SC.PAIR_SATURATED))
def test_saturated_lds_tables_equal_oracle(gpu, monkeypatch, name):
    """More ids per workgroup range than the LDS object tables hold (every share: 512, 256, 128, 64, 32 slots), and -- with few ids but
    many combinations -- more pairs than the LDS pair tables hold (1024, 256, 128 slots): the rest goes to the global tables directly."""
    kw = SC.SATURATED.get(name) or SC.PAIR_SATURATED[name]
    cell, subs = SC.saturated_case(**kw)
    _both_forms(monkeypatch, cell, subs, SC.oracle(cell, subs), gpu, name)


@pytest.mark.parametrize('dtype', [np.uint32, np.uint64])
def test_ids_served_from_lds_in_some_workgroups_and_from_hbm_in_others(gpu, monkeypatch, dtype):
    cell, subs = SC.mixed_case((9, 16, 256), dtype)
    _both_forms(monkeypatch, cell, subs, SC.oracle(cell, subs), gpu, 'mixed')
    _both_forms(monkeypatch, None, [cell, subs[0]], (None, [SC._props_np(cell), SC._props_np(subs[0])], []), gpu, 'mixed, no cell')


def test_saturated_uint32_and_counts_only(gpu, monkeypatch):
    kw = dict(SC.SATURATED['lcap128_pcap256'], dtype=np.uint32)
    cell, subs = SC.saturated_case(**kw)
    want = SC.oracle(cell, subs)
    _both_forms(monkeypatch, cell, subs, want, gpu, 'uint32 saturated')
    _both_forms(monkeypatch, cell, subs, want, gpu, 'uint32 saturated, counts only', want_props=False)


# ---- 9. determinism --------------------------------------------------------------------------------------------------------------------
def test_two_passes_over_a_saturated_case_give_identical_tables(gpu):
    """The order inside the hash tables may differ from pass to pass; sums, minima and maxima, sorted by id, may not."""
    for kw in (SC.SATURATED['lcap128_pcap256'], SC.PAIR_SATURATED['pairs_pcap256']):
        cell, subs = SC.saturated_case(**kw)
        a, b = _segstats(cell, subs, device=gpu), _segstats(cell, subs, device=gpu)
        for x, y in zip([a.cell] + a.sub + a.pairs, [b.cell] + b.sub + b.pairs):
            for u, v in zip(x, y):
                assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()


# ---- 4. past the scan's grid cap ----------------------------------------------------------------------------------------------------------
def test_past_the_scan_grid_cap_full_oracle(gpu, monkeypatch):
    """(41, 500, 516): 2048 workgroups own 21 (four-voxel form) / 81 (one-voxel form) wave-chunks each -- the waves of a workgroup
    make unequal numbers of trips, the last workgroups have a short or empty range.  Every table against the full oracle."""
    t0 = time.time()
    cell, subs = SC.grid_cap_case()
    want = SC.oracle(cell, subs)
    print(f'grid-cap case: oracle {time.time() - t0:.1f} s, {len(want[0][0])} cell ids, {[len(w[0]) for w in want[1]]} organelle ids, '
          f'{[len(p[0]) for p in want[2]]} pairs')
    _both_forms(monkeypatch, cell, subs, want, gpu, 'grid cap uint64')
    r = _segstats(cell.astype(np.uint32), [s.astype(np.uint32) for s in subs], device=gpu)
    SC.assert_equals_oracle(r, want, True, 'grid cap uint32')


# ---- 5. past one grid stride of the table kernels --------------------------------------------------------------------------------------------
def test_tables_of_2_pow_21_slots_passed_explicitly(gpu, monkeypatch):
    """k_obj_init / k_zero64 / k_obj_compact / k_pair_compact make two trips of their grid-stride loops."""
    cell, subs = SC.saturated_case(**SC.SATURATED['lcap128_pcap256'])
    r = _both_forms(monkeypatch, cell, subs, SC.oracle(cell, subs), gpu, 'cap 2^21', cap_obj=1 << 21, cap_pair=1 << 21)
    assert r.cap_obj == r.cap_pair == 1 << 21


def test_every_voxel_its_own_object_at_128_cubed(gpu):
    """2,097,152 objects and pairs from the default capacity (65,536 slots): the overflow-and-repeat path at scale, then init,
    compaction of objects and pairs past one grid stride.  Expectations are arange-style."""
    n, shape = 128 ** 3, (128, 128, 128)
    cell = (np.arange(n, dtype=np.uint64) + 1).reshape(shape)
    sub = (np.uint64(n) - np.arange(n, dtype=np.uint64)).reshape(shape)                # voxel i: cell id i + 1, subcell id n - i
    r = _segstats(cell, [sub], device=gpu)
    print(f'128^3: capacities at the end {r.cap_obj} objects, {r.cap_pair} pairs')
    assert r.cap_obj >= n and r.cap_pair >= n
    idx = np.arange(n, dtype=np.int64)
    lo = np.stack(np.unravel_index(idx, shape), axis=1)
    bb = np.stack((lo, lo + 1), axis=1)
    SC._same_props(r.cell, (idx.astype(np.uint64) + 1, idx, np.ones(n, np.int64), bb), 'cell')
    SC._same_props(r.sub[0], (idx.astype(np.uint64) + 1, idx[::-1], np.ones(n, np.int64), bb[::-1]), 'sub')
    SC._same_pairs(r.pairs[0], (idx.astype(np.uint64) + 1, np.uint64(n) - idx.astype(np.uint64), np.ones(n, np.int64)), 'pairs')


def _driver(gpu, vols, names, chunk_size, **kw):
    import torch
    import syconn_amd.proc.sd_proc as sp
    boundary = np.array(vols['sv'].shape)

    class KD:
        pass
    KD.boundary = boundary
    dvols = {k: torch.from_numpy(v.view(np.int64)).to(gpu) for k, v in vols.items()}

    def loader(name, off, size):
        out = torch.zeros(tuple(int(s) for s in size), dtype=torch.int64, device=gpu)
        hi = np.minimum(off + size, boundary)
        m = hi - off
        out[:m[0], :m[1], :m[2]] = dvols[name][off[0]:hi[0], off[1]:hi[1], off[2]:hi[2]]
        return out
    orig = sp.kd_factory
    sp.kd_factory = lambda p: KD()
    try:
        return sp.map_subcell_extract_props('', {n: '' for n in names}, chunk_size=chunk_size, min_obj_vx={n: 1 for n in ['sv'] + names},
                                            device=gpu, as_tables=True, chunk_loader=loader, **kw)
    finally:
        sp.kd_factory = orig


def _table_equals_oracle(tab, want, what):
    ids, first, size, bb = want
    assert np.array_equal(tab.ids, ids.astype(np.uint64)) and np.array_equal(tab.sizes, size), what
    lo = np.minimum.reduceat(tab.boxes[:, 0], tab.box_begin[:-1], axis=0)
    hi = np.maximum.reduceat(tab.boxes[:, 1], tab.box_begin[:-1], axis=0)
    assert np.array_equal(lo, bb[:, 0]) and np.array_equal(hi, bb[:, 1]), what


def test_chunk_driver_with_tables_of_2_pow_21_slots_equals_oracle(gpu):
    """`sd_chunkprops_append` / `sd_chunkpairs_append` walk 2^21 slots per chunk (two trips); ragged last chunks."""
    shape = (40, 36, 40)
    vols = {'sv': SC.coherent_labels(1, shape, 300, special=True), 'mi': SC.coherent_labels(2, shape, 40, block=(2, 3, 5), keep=0.5),
            'vc': SC.random_labels(3, shape, 25)}
    cell_t, sub_t, map_t = _driver(gpu, vols, ['mi', 'vc'], (16, 16, 16), table_capacity=1 << 21)
    want = SC.oracle(vols['sv'], [vols['mi'], vols['vc']])
    _table_equals_oracle(cell_t, want[0], 'cell')
    for i, o in enumerate(['mi', 'vc']):
        _table_equals_oracle(sub_t[o], want[1][i], o)
        SC._same_pairs((map_t[o].sub_ids, map_t[o].cell_ids, map_t[o].counts), want[2][i], o)


def test_unique_labels_and_label_boxes_past_one_grid_stride(gpu):
    import torch
    from syconn_amd.extraction.object_extraction_steps import labels_box, make_unique_labels
    rng = np.random.default_rng(9)
    lab = rng.integers(-3, 5000, (130, 130, 90)).astype(np.int32)
    assert lab.size > SC.kernel_constants()['GRID_FOR_ITEMS']
    offset = 2 ** 40 + 17
    got = make_unique_labels(torch.from_numpy(lab).to(gpu), offset).cpu().numpy().view(np.uint64)
    want = np.where(lab > 0, lab.astype(np.int64) + offset, 0).astype(np.uint64)
    assert np.array_equal(got, want)
    vol = torch.from_numpy(np.where(lab > 0, lab, 0).astype(np.int64)).to(gpu)
    host = vol.cpu().numpy()
    lo, size = (1, 2, 3), (128, 128, 80)
    assert int(np.prod(size)) > SC.kernel_constants()['GRID_FOR_ITEMS']
    box = host[1:129, 2:130, 3:83]
    assert np.array_equal(labels_box(vol, lo, size).cpu().numpy(), box)
    lut_h = rng.permutation(5000).astype(np.int64) + 2 ** 41
    lut_h[0] = 0
    assert int(box.max()) == 4999                                   # the last entry of the table is used
    assert np.array_equal(labels_box(vol, lo, size, torch.from_numpy(lut_h).to(gpu)).cpu().numpy(), lut_h[box])
    with pytest.raises(ValueError):
        labels_box(vol, lo, size, torch.from_numpy(lut_h[:4999]).to(gpu))           # id 4999 is one past the table


# ---- 6. exactly full tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extra', [0, 1])
def test_exactly_full_object_table(gpu, monkeypatch, extra):
    """1024 distinct ids in a table of 1024 slots (every slot taken, no overflow), and 1025 (overflow, repeated with a larger table)."""
    shape, cap = (4, 16, 32), 1024
    n = int(np.prod(shape))
    cell = ((np.arange(n, dtype=np.uint64) % np.uint64(cap + extra)) + np.uint64(1)) * np.uint64(7919)
    cell = cell.reshape(shape)
    assert len(np.unique(cell)) == cap + extra
    want = SC.oracle(cell, [])
    for v1 in (False, True):
        if v1:
            monkeypatch.setenv('SD_SEGSTATS_V1', '1')
        r = _segstats(cell, [], device=gpu, cap_obj=cap, cap_pair=cap)
        monkeypatch.delenv('SD_SEGSTATS_V1', raising=False)
        print(f'{cap + extra} ids from a table of {cap} slots (one-voxel form: {v1}): ended with {r.cap_obj} object slots')
        SC.assert_equals_oracle(r, want, True, f'{cap + extra} ids')
    sub = SC.coherent_labels(4, shape, 6, special=False)
    r = _segstats(cell, [sub], device=gpu, cap_obj=cap, cap_pair=cap)
    print(f'{cap + extra} ids + one organelle volume: ended with {r.cap_obj} object slots, {r.cap_pair} pair slots')
    SC.assert_equals_oracle(r, SC.oracle(cell, [sub]), True, f'{cap + extra} ids + organelle')


# ---- 7. 64-bit coordinate decode ---------------------------------------------------------------------------------------------------------
def test_volume_of_more_than_2_pow_32_voxels(gpu, monkeypatch):
    """uint32 labels of shape (1030, 2048, 2048) built on the device: the cell label is a function of x and z, the organelle label a
    function of y, so ids, first raster indices (some beyond 2^32), sizes, boxes and overlap counts follow from 1-D index sets."""
    import torch
    X, Y, Z = 1030, 2048, 2048
    nvox = X * Y * Z
    assert nvox >= 2 ** 32 and Z % 4 == 0
    need = 2 * nvox * 4 + 6 * 2 ** 30          # two volumes; two object tables of 2^25 slots (1.6 GB each), the pair table, compaction
    free = torch.cuda.mem_get_info(gpu)[0]
    if free < need + 4 * 2 ** 30:
        pytest.skip(f'{free / 2 ** 30:.0f} GiB free on the device, the case needs {need / 2 ** 30:.0f} GiB + 4 GiB')
    xs = np.arange(X)
    A = np.where(xs < 1026, xs % 7, 7 + (xs - 1026))                       # 11 values; 7..10 only at x >= 1026: first index >= 2^32
    B = np.arange(Z) // 512
    S = np.arange(Y) % 5                                                     # 0 = background
    cell = torch.empty((X, Y, Z), dtype=torch.int32, device=gpu)
    sub = torch.empty((X, Y, Z), dtype=torch.int32, device=gpu)
    a_t = torch.from_numpy((1 + 4 * A).astype(np.int32)).to(gpu)
    b_t = torch.from_numpy(B.astype(np.int32)).to(gpu)
    s_t = torch.from_numpy(S.astype(np.int32)).to(gpu)
    for x0 in range(0, X, 64):                                               # x-slabs: no whole-volume temporary
        x1 = min(X, x0 + 64)
        cell[x0:x1] = (a_t[x0:x1].view(-1, 1, 1) + b_t.view(1, 1, -1))
        sub[x0:x1] = s_t.view(1, -1, 1)
    c_ids, c_first, c_size, c_bb, sets = [], [], [], [], {}
    for a in range(11):
        for b in range(4):
            xi, zi = np.flatnonzero(A == a), np.flatnonzero(B == b)
            c_ids.append(1 + 4 * a + b); c_first.append(int(xi[0]) * Y * Z + int(zi[0])); c_size.append(len(xi) * Y * len(zi))
            c_bb.append([[xi[0], 0, zi[0]], [xi[-1] + 1, Y, zi[-1] + 1]])
            sets[1 + 4 * a + b] = (len(xi), len(zi))
    assert max(c_first) >= 2 ** 32 and sum(c_size) == nvox
    s_ids, s_first, s_size, s_bb, p = [], [], [], [], []
    for s in range(1, 5):
        yi = np.flatnonzero(S == s)
        s_ids.append(s); s_first.append(int(yi[0]) * Z); s_size.append(X * len(yi) * Z); s_bb.append([[0, yi[0], 0], [X, yi[-1] + 1, Z]])
        p += [(s, c, nx * len(yi) * nz) for c, (nx, nz) in sorted(sets.items())]
    arr = lambda v, t=np.int64: np.asarray(v, dtype=t)
    want = ((arr(c_ids, np.uint64), arr(c_first), arr(c_size), arr(c_bb)), [(arr(s_ids, np.uint64), arr(s_first), arr(s_size), arr(s_bb))],
            [(arr([q[0] for q in p], np.uint64), arr([q[1] for q in p], np.uint64), arr([q[2] for q in p]))])
    try:
        for v1 in (False, True):
            if v1:
                monkeypatch.setenv('SD_SEGSTATS_V1', '1')
            t0 = time.time()
            r = _segstats(cell, [sub], device=gpu)
            monkeypatch.delenv('SD_SEGSTATS_V1', raising=False)
            print(f'{nvox} voxels, one-voxel form {v1}: {time.time() - t0:.2f} s with tables of {r.cap_obj} slots')
            SC.assert_equals_oracle(r, want, True, f'64-bit decode, one-voxel form {v1}')
            del r
    finally:
        del cell, sub
        torch.cuda.empty_cache()


# ---- 8. switches a process reads once ------------------------------------------------------------------------------------------------------
def _worker(env_extra, timeout=600):
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    for k in ('SD_SEGSTATS_NO_LDS', 'SD_SEGSTATS_NO_PREFETCH', 'SD_SEGSTATS_V1'):
        env.pop(k, None)
    env.update(env_extra)
    cmd = [sys.executable, os.path.join(ROOT, 'tests', '_segstats_worker.py')] + sorted(env_extra)
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert r.returncode == 0, f'{" ".join(cmd)}\nrc={r.returncode}\nSTDOUT:\n{r.stdout[-3000:]}\nSTDERR:\n{r.stderr[-3000:]}'
    assert 'segstats worker ok' in r.stdout, r.stdout[-2000:]
    return r.stdout


def test_all_global_path_and_sequential_four_voxel_form_in_fresh_processes(gpu):
    """`SD_SEGSTATS_NO_LDS` (every update and every pair goes to the global tables) and `SD_SEGSTATS_NO_PREFETCH` (the generic
    four-voxel loop for any number of volumes) are read once per process: a fresh child each, one after the other; the worker compares
    a subset of the form matrix, the misaligned and the saturated cases with the oracle itself."""
    print(_worker({'SD_SEGSTATS_NO_LDS': '1'}).strip().splitlines()[-1])
    print(_worker({'SD_SEGSTATS_NO_PREFETCH': '1'}).strip().splitlines()[-1])
