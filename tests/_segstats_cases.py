"""Helpers of tests/test_segstats_edges_cpu.py, tests/test_gpu_segstats_edges.py and tests/_segstats_worker.py (not collected):

* seeded case builders for the label-statistics pass (`sd_segstats_scan`),
* a model of the scan launch (voxels per wave, grid, wave-chunks per workgroup, LDS shares) whose constants are read from the kernel
  sources -- a retuned kernel makes the constants or the edge conditions of the CPU test fail, so the cases get looked at again,
* the oracle on arrays: `_props_np` per volume and the (subcell id, cell id) -> count table, and the comparison with a `SegStats`.
"""
import os
import re
from collections import namedtuple

import numpy as np

from oracle.objprops_ref import _props_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'syconn_amd', 'csrc')


# ---- constants of the launch, from the sources -------------------------------------------------------------------------------------
def _grab(text, pattern, what):
    m = re.search(pattern, text)
    if m is None:
        raise AssertionError(f'tests/_segstats_cases.py: {what} not found in the kernel sources (pattern {pattern!r}); the scan was '
                             f'retuned or rewritten -- revisit the edge cases of the label-statistics tests')
    return [int(g) for g in m.groups()]


def kernel_constants():
    with open(os.path.join(CSRC, 'sd_segstats.hip')) as f:
        seg = f.read()
    with open(os.path.join(CSRC, 'sd_hash.h')) as f:
        hsh = f.read()
    c = {}
    c['LDS_SLOTS'], = _grab(seg, r'constexpr int LDS_SLOTS = (\d+);', 'LDS_SLOTS')
    c['LDS_PSLOTS'], = _grab(seg, r'constexpr int LDS_PSLOTS = (\d+);', 'LDS_PSLOTS')
    c['MAX_SUB'], = _grab(seg, r'constexpr int MAX_SUB = (\d+);', 'MAX_SUB')
    c['LDS_PROBES'], = _grab(seg, r'lds_find_or_insert\(u64\* keys, int cap, u64 k\) \{[^}]*?probe < (\d+) && probe < cap', 'LDS probe limit')
    c['PAIR_PROBES'], = _grab(seg, r'lds_pair_slot\(unsigned\* keys, int cap, unsigned k\) \{[^}]*?probe < (\d+) && probe < cap',
                              'LDS pair probe limit')
    # const int grid = (int)std::max<u64>(1, std::min<u64>((nwaves + (v4 ? 15 : 63)) / (v4 ? 16 : 64), 256 * 8));
    r4, r1, w4, w1, ga, gb = _grab(seg, r'const int grid = .*?\(nwaves \+ \(v4 \? (\d+) : (\d+)\)\) / \(v4 \? (\d+) : (\d+)\), (\d+) \* (\d+)\)\);',
                                   'scan grid')
    assert r4 == w4 - 1 and r1 == w1 - 1
    c['WAVES_PER_WG_V4'], c['WAVES_PER_WG_V1'], c['GRID_CAP'] = w4, w1, ga * gb
    c['VPW_V4'], c['VPW_V1'] = _grab(seg, r'constexpr int VPW = V4 \? (\d+) : (\d+);', 'voxels per wave')
    c['LCAP_MIN'], = _grab(seg, r'int lcap = (\d+);\s*while \(lcap \* 2 \* nvol <= LDS_SLOTS\) lcap \*= 2;', 'LDS share')
    blocks, = _grab(hsh, r'inline int grid_for\(u64 n, int cap = (\d+)\)', 'grid_for cap')
    c['GRID_FOR_ITEMS'] = blocks * 256
    return c


Launch = namedtuple('Launch', 'v4 vpw nvox nwaves grid per_wg nvol lcap pcap')


def launch_model(shape, has_cell, n_sub, v4=None, want_props=True, consts=None):
    """What `sd_segstats_scan` launches for aligned volumes of `shape`: `v4` None = the form the library picks (rows % 4 == 0)."""
    c = consts or kernel_constants()
    nvox = int(shape[0]) * int(shape[1]) * int(shape[2])
    if v4 is None:
        v4 = shape[2] % 4 == 0
    assert not (v4 and shape[2] % 4)
    vpw = c['VPW_V4'] if v4 else c['VPW_V1']
    nwaves = -(-nvox // vpw)
    wpw = c['WAVES_PER_WG_V4'] if v4 else c['WAVES_PER_WG_V1']
    grid = max(1, min(-(-nwaves // wpw), c['GRID_CAP']))
    per_wg = -(-nwaves // grid)
    nvol = (1 if has_cell else 0) + n_sub
    lcap = c['LCAP_MIN']
    while lcap * 2 * nvol <= c['LDS_SLOTS']:
        lcap *= 2
    if lcap * nvol > c['LDS_SLOTS']:
        lcap = 0
    pcap = 0
    if has_cell and n_sub > 0 and want_props and lcap:
        pcap = c['LDS_PSLOTS']
        while pcap * n_sub > c['LDS_PSLOTS']:
            pcap >>= 1
    return Launch(v4, vpw, nvox, nwaves, grid, per_wg, nvol, lcap, pcap)


def range_distinct(launch, cell, subs):
    """Per workgroup range of the flattened volume: (largest number of distinct non-zero ids of any one volume, largest number of
    distinct (subcell, cell) pairs of any one subcell volume), maximised / minimised over the ranges -> (max_ids, max_pairs)."""
    span = launch.per_wg * launch.vpw
    vols = ([cell] if cell is not None else []) + list(subs)
    flats = [np.ascontiguousarray(v).reshape(-1) for v in vols]
    max_ids = max_pairs = 0
    for lo in range(0, launch.nvox, span):
        hi = min(launch.nvox, lo + span)
        for f in flats:
            u = np.unique(f[lo:hi])
            max_ids = max(max_ids, int(np.count_nonzero(u)))
        if cell is not None:
            c = flats[0][lo:hi]
            for f in flats[1:]:
                s = f[lo:hi]
                m = (s != 0) & (c != 0)
                if m.any():
                    max_pairs = max(max_pairs, len(np.unique(np.stack((s[m], c[m]), axis=1), axis=0)))
    return max_ids, max_pairs


# ---- label volumes -----------------------------------------------------------------------------------------------------------------
def _special_ids(vol, dtype):
    """ids at the ends of the type's range (key 0 is the only reserved value)."""
    if np.dtype(dtype) == np.uint32:
        vol[vol == 1] = np.uint32(2 ** 32 - 1)
    else:
        vol[vol == 1] = np.uint64(2 ** 64 - 1)
        vol[vol == 2] = np.uint64(2 ** 63 + 7)
        vol[vol == 3] = np.uint64(2 ** 63)
    return vol


def random_labels(seed, shape, nid, dtype=np.uint64, special=True):
    vol = np.random.default_rng(seed).integers(0, nid, shape).astype(dtype)
    return _special_ids(vol, dtype) if special else vol


def coherent_labels(seed, shape, nid, dtype=np.uint64, block=(3, 4, 6), special=True, keep=1.0):
    """Blocky supervoxel-like labels (blocks of `block` voxels, so runs start at every in-lane position); `keep` < 1 zeroes ids."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, nid, [s // b + 1 for s, b in zip(shape, block)])
    if keep < 1.0:
        small[rng.random(small.shape) > keep] = 0
    vol = np.kron(small, np.ones(block, dtype=np.int64))[:shape[0], :shape[1], :shape[2]]
    vol = np.ascontiguousarray(vol).astype(dtype)
    return _special_ids(vol, dtype) if special else vol


def form_case(shape, has_cell, n_sub, dtype, seed=0):
    """Form matrix: a few ids per workgroup range -- coherent volumes, every third subcell volume random with 8 ids."""
    cell = coherent_labels(seed + 1, shape, 9, dtype) if has_cell else None
    subs = [random_labels(seed + 10 + k, shape, 8, dtype) if k % 3 == 1 else
            coherent_labels(seed + 10 + k, shape, 6 + k, dtype, block=(2, 3, 5 + k), keep=0.7) for k in range(n_sub)]
    return cell, subs


def saturated_case(shape, nid, has_cell, n_sub, dtype=np.uint64, seed=100):
    """Every voxel a random id of `nid`: far more ids and pairs per workgroup range than the LDS tables hold."""
    cell = random_labels(seed, shape, nid, dtype) if has_cell else None
    subs = [random_labels(seed + 1 + k, shape, nid, dtype) for k in range(n_sub)]
    return cell, subs


def mixed_case(shape, dtype=np.uint64, seed=200, n_far=5, local_run=6):
    """Thousands of ids that live in one place each (a new one every `local_run` voxels, more per workgroup range than the LDS share)
    and `n_far` ids sprinkled over the whole volume: a far id meets a full LDS table in some workgroups and a free slot in others."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    base = 100 + np.arange(n, dtype=np.int64) // local_run
    far = rng.random(n) < 0.06
    base[far] = 10 + rng.integers(0, n_far, int(far.sum()))
    cell = base.reshape(shape).astype(dtype)
    sub = 100 + (np.arange(n, dtype=np.int64) + 3) // (local_run + 1)
    far2 = rng.random(n) < 0.05
    sub[far2] = 20 + rng.integers(0, n_far, int(far2.sum()))
    sub[rng.random(n) < 0.1] = 0
    return cell, [sub.reshape(shape).astype(dtype)]


GRID_CAP_SHAPE = (41, 500, 516)


def grid_cap_case(shape=GRID_CAP_SHAPE, dtype=np.uint64, n_sub=3, seed=300):
    """Past the scan's grid cap: a supervoxel-like cell volume and sparse organelle volumes (ids < 2^32, so the uint32 run uses
    the same labels)."""
    cell = coherent_labels(seed, shape, 3000, dtype, block=(7, 9, 11), special=False)
    subs = [coherent_labels(seed + 1 + k, shape, 50, dtype, block=(4, 5, 6), special=False, keep=0.3) * np.dtype(dtype).type(k + 1)
            for k in range(n_sub)]
    return cell, subs


# name -> (builder, full-size arguments, cut-down shape for the literal loops)
SATURATED = {
    'lcap512_lone':      dict(shape=(9, 16, 256), nid=5000, has_cell=True, n_sub=0),
    'lcap512_lone_sub':  dict(shape=(9, 16, 256), nid=5000, has_cell=False, n_sub=1),
    'lcap256_pcap1024':  dict(shape=(9, 16, 256), nid=5000, has_cell=True, n_sub=1),
    'lcap128_pcap256':   dict(shape=(9, 16, 256), nid=5000, has_cell=True, n_sub=3),
    'lcap64_pcap128':    dict(shape=(12, 20, 128), nid=4000, has_cell=True, n_sub=7),
    'lcap32_pcap128':    dict(shape=(12, 20, 128), nid=4000, has_cell=True, n_sub=8),
    'lcap64_cellless':   dict(shape=(12, 20, 128), nid=4000, has_cell=False, n_sub=5),
}
# few ids per volume (every one finds an LDS slot) but more distinct (subcell, cell) pairs per workgroup range than the LDS pair table
# holds: the pair table itself saturates.  (In SATURATED most ids miss the LDS object tables, and a pair is only counted in LDS when both
# of its ids sit there, so those cases fill the object tables and leave the pair table sparse.)
PAIR_SATURATED = {
    'pairs_pcap1024': dict(shape=(9, 16, 256), nid=60, has_cell=True, n_sub=1),
    'pairs_pcap256':  dict(shape=(9, 16, 256), nid=40, has_cell=True, n_sub=3),
    'pairs_pcap128':  dict(shape=(12, 20, 128), nid=30, has_cell=True, n_sub=7),
}
EXPECTED_SHARES = {'pairs_pcap1024': (256, 1024), 'pairs_pcap256': (128, 256), 'pairs_pcap128': (64, 128),
                   'lcap512_lone': (512, 0), 'lcap512_lone_sub': (512, 0), 'lcap256_pcap1024': (256, 1024), 'lcap128_pcap256': (128, 256),
                   'lcap64_pcap128': (64, 128), 'lcap32_pcap128': (32, 128), 'lcap64_cellless': (64, 0)}


# ---- oracle on arrays ---------------------------------------------------------------------------------------------------------------
def pairs_np(cell, sub):
    """(subcell ids, cell ids, counts) over the voxels where both are non-zero, sorted by (subcell id, cell id)."""
    s, c = np.ascontiguousarray(sub).reshape(-1), np.ascontiguousarray(cell).reshape(-1)
    both = np.flatnonzero((s != 0) & (c != 0))
    if both.size == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int64)
    pr, cnt = np.unique(np.stack((s[both], c[both]), axis=1).astype(np.uint64), axis=0, return_counts=True)
    return pr[:, 0], pr[:, 1], cnt.astype(np.int64)


def oracle(cell, subs):
    """-> (cell props or None, [sub props], [pairs]) with props = `_props_np` (ids ascending, first raster index, count, bbox)."""
    return (_props_np(cell) if cell is not None else None, [_props_np(s) for s in subs],
            [pairs_np(cell, s) for s in subs] if cell is not None else [])


def props_cellless_np(subs):
    """`map_subcell_extract_props` without a cell volume: the properties of every subcell volume, no overlap counts."""
    return [_props_np(s) for s in subs]


def _same_props(got, want, what):
    ids, first, size, bb = got
    w_ids, w_first, w_size, w_bb = want
    assert np.array_equal(np.asarray(ids).astype(np.uint64), np.asarray(w_ids).astype(np.uint64)), f'{what}: ids differ'
    assert np.array_equal(np.asarray(first).astype(np.int64), w_first), f'{what}: first voxels differ'
    assert np.array_equal(np.asarray(size).astype(np.int64), w_size), f'{what}: sizes differ'
    assert np.array_equal(np.asarray(bb).astype(np.int64).reshape(-1, 2, 3), w_bb), f'{what}: bounding boxes differ'


def _same_pairs(got, want, what):
    for g, w, n in zip(got, want, ('subcell ids', 'cell ids', 'counts')):
        assert np.array_equal(np.asarray(g).astype(np.uint64), np.asarray(w).astype(np.uint64)), f'{what}: pair {n} differ'


def assert_equals_oracle(res, want, want_props=True, what=''):
    """`res`: a SegStats; `want`: `oracle(cell, subs)`."""
    w_cell, w_subs, w_pairs = want
    if want_props:
        if w_cell is not None:
            _same_props(res.cell, w_cell, f'{what} cell')
        else:
            assert res.cell is None
        assert len(res.sub) == len(w_subs)
        for k, (g, w) in enumerate(zip(res.sub, w_subs)):
            _same_props(g, w, f'{what} sub[{k}]')
    else:
        assert res.cell is None and res.sub == []
    assert len(res.pairs) == len(w_pairs)
    for k, (g, w) in enumerate(zip(res.pairs, w_pairs)):
        _same_pairs(g, w, f'{what} pairs[{k}]')


def assert_same_result(a, b, what=''):
    """Two SegStats (for example the four-voxel and the one-voxel form) hold the same arrays."""
    if a.cell is not None or b.cell is not None:
        _same_props(a.cell, (b.cell[0], b.cell[1].astype(np.int64), b.cell[2].astype(np.int64), b.cell[3].astype(np.int64)), f'{what} cell')
    assert len(a.sub) == len(b.sub) and len(a.pairs) == len(b.pairs)
    for k, (g, w) in enumerate(zip(a.sub, b.sub)):
        _same_props(g, (w[0], w[1].astype(np.int64), w[2].astype(np.int64), w[3].astype(np.int64)), f'{what} sub[{k}]')
    for k, (g, w) in enumerate(zip(a.pairs, b.pairs)):
        _same_pairs(g, w, f'{what} pairs[{k}]')


# ---- device tensors at chosen alignments ----------------------------------------------------------------------------------------------
def device_volume(vol, device, misaligned=False):
    """numpy uint32 / uint64 (X, Y, Z) -> contiguous device tensor with the same bits; `misaligned`: cut from a flat buffer at an
    offset of one element, so its pointer is not 16-byte aligned."""
    import torch
    signed = np.int32 if vol.dtype == np.uint32 else np.int64
    flat = torch.from_numpy(np.ascontiguousarray(vol).view(signed).reshape(-1))
    if not misaligned:
        t = flat.to(device).view(*vol.shape)
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(flat.numel() + 1, dtype=flat.dtype, device=device)
    buf[1:] = flat.to(device)
    t = buf[1:].view(*vol.shape)
    assert t.data_ptr() % 16 != 0 and t.is_contiguous()
    return t
