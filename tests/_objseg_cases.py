"""Helpers of tests/test_objseg_edges_cpu.py and tests/test_gpu_objseg_edges.py (not collected):

* the constants of `syconn_amd/csrc/sd_objseg.hip` the cases are placed on, read from the sources -- a retuned kernel makes the
  constants or the edge conditions of the CPU test fail, so the cases get looked at again,
* a model of the word-indexed passes: which mask words (32 z-voxels of the volume padded by P, raster order over (x, y, word)) one
  workgroup visits,
* seeded / periodic case builders (pure numpy, deterministic, small) and the oracle composed from its pieces for a custom element.
"""
import os
import re

import numpy as np
from scipy import ndimage

from oracle.objseg_ref import (apply_morphological_operations_ref, distance_transform_ref, seed_markers_ref, watershed_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'syconn_amd', 'csrc')

Z_ELEMENT = np.ones((1, 1, 3), np.uint8)          # erosion along z only: a z-run of n voxels keeps n - 2


# ---- constants of the kernels, from the sources ------------------------------------------------------------------------------------
def _grab(text, pattern, what, flags=0):
    m = re.search(pattern, text, flags)
    if m is None:
        raise AssertionError(f'tests/_objseg_cases.py: {what} not found in the kernel sources (pattern {pattern!r}); the kernels were '
                             f'retuned or rewritten -- revisit the edge cases of the object-segmentation tests')
    return [int(g, 0) for g in m.groups()]


# the word-indexed passes of the watershed branch (run_cc's passes stand for "run_cc with cnt")
WORD_PASSES = ('k_apply_map', 'k_seed_bits_sync', 'k_edt_z', 'k_comp_markers', 'k_cc_init_heads', 'k_cc_merge_runs', 'k_cc_head_labels',
               'k_cc_fill_runs', 'k_morph_bits', 'k_threshold_bits')


def kernel_constants():
    with open(os.path.join(CSRC, 'sd_objseg.hip')) as f:
        src = f.read()
    with open(os.path.join(CSRC, 'sd_host_util.h')) as f:
        util = f.read()
    c = {}
    for name in ('SCAN_PER_THREAD', 'WI_WORDS', 'WSP_CAP', 'WS_LDS_CAP', 'MAX_OFFS', 'EDT_INF', 'GAUSS_MAX_R', 'WSP_THREADS'):
        c[name], = _grab(src, r'constexpr int %s = (0x[0-9a-fA-F]+|\d+)[,;]' % name, name)
    body = r'\([^{]*\{[^}]*?'      # parameter list, opening brace, then the first statements of the body
    c['HEAD_SLOTS'], = _grab(src, r'void k_cc_head_labels' + body + r'constexpr int SLOTS = (\d+);', 'SLOTS of k_cc_head_labels')
    c['HEAD_PROBES'], = _grab(src, r'void k_cc_head_labels\(.*?for \(; tries < (\d+); \+\+tries', 'probes of k_cc_head_labels', re.S)
    c['COMP_SLOTS'], = _grab(src, r'void k_comp_markers' + body + r'constexpr int SLOTS = (\d+);', 'SLOTS of k_comp_markers')
    c['INIT_SLOTS'], c['INIT_LIST'] = _grab(src, r'void k_ws_init' + body + r'constexpr int SLOTS = (\d+), LIST = (\d+);',
                                            'SLOTS / LIST of k_ws_init')
    c['LDS_PROBES'], = _grab(src, r'int lds_slot\(int\* skey, int k\) \{[^}]*?tries < (\d+);', 'probes of lds_slot')
    lb, c['SCAN_ROUND'] = _grab(src, r'__launch_bounds__\((\d+)\) void k_scan_excl\(.*?for \(int base = 0; base < n; base \+= (\d+)\)',
                                'round of k_scan_excl', re.S)
    assert lb == c['SCAN_ROUND']
    c['FLOOD_GRID'], = _grab(src, r'hipLaunchKernelGGL\(k_ws_flood<WSP_THREADS>, dim3\((\d+)\)', 'grid of k_ws_flood')
    c['FLOOD_SEQ_GRID'], = _grab(src, r'hipLaunchKernelGGL\(k_ws_flood_seq, dim3\((\d+)\)', 'grid of k_ws_flood_seq')
    caps = set()
    for k in WORD_PASSES:
        found = re.findall(r'hipLaunchKernelGGL\(%s, dim3\(grid_for\([^;]*?, (\d+)\)\), dim3\((\d+)\)' % k, src)
        if not found:
            raise AssertionError(f'tests/_objseg_cases.py: launch of {k} through grid_for(n, cap) not found -- revisit the launch-cap cases')
        caps |= {(int(a), int(b)) for a, b in found}
    assert len(caps) == 1, f'the word passes no longer share one launch cap: {sorted(caps)}'
    (c['WORD_GRID_CAP'], blk), = caps
    rnd, c['GRID_BLOCK'] = _grab(util, r'inline int grid_for\(unsigned long long n, int cap\) \{ const unsigned long long g = \(n \+ (\d+)\) / (\d+);',
                                 'block of grid_for')
    assert rnd == c['GRID_BLOCK'] - 1 and blk == c['GRID_BLOCK']
    # k_ws_init: one workgroup per GRID_BLOCK * WI_WORDS words, no grid stride
    _grab(src, r'hipLaunchKernelGGL\(k_ws_init, dim3\(\(unsigned\)\(\(\(size_t\)d\.X \* d\.Y \* d\.PZW \+ 256 \* WI_WORDS - 1\) / \(256 \* WI_WORDS\)\)\)',
          'grid of k_ws_init')
    c['MAX_ITER'], = _grab(src, r'iterations\[i\] < 1 \|\| iterations\[i\] > (\d+)', 'iteration limit')
    c['MAX_EXTENT'], = _grab(src, r'sx > (\d+) \|\| sy > \1 \|\| sz > \1', 'element extent limit')
    c['MAX_PITCH_EXTENT'], = _grab(src, r'\(a == 0 \? X : a == 1 \? Y : Z\) > (\d+)\.0', 'pitch x extent limit')
    return c


# ---- launch model ------------------------------------------------------------------------------------------------------------------
def words_per_row(Z, P):
    return (Z + 2 * P + 31) // 32


def word_of_voxels(shape, P=0):
    """int64 (X, Y, Z): index of the mask word that holds each voxel, in the order the word-indexed passes walk
    ((x * Y + y) * PZW + (z + P) // 32)."""
    X, Y, Z = shape
    pzw = words_per_row(Z, P)
    row = (np.arange(X)[:, None] * Y + np.arange(Y)[None, :])[:, :, None]
    return row * pzw + ((np.arange(Z) + P) // 32)[None, None, :]


def n_words(shape, P=0):
    return int(shape[0]) * int(shape[1]) * words_per_row(shape[2], P)


def span_words(kind, consts=None):
    """consecutive words one workgroup owns at a time: 'stride' = a grid-stride pass (256 per stride), 'init' = k_ws_init"""
    c = consts or kernel_constants()
    return c['GRID_BLOCK'] * (c['WI_WORDS'] if kind == 'init' else 1)


def strides_of_word_pass(shape, P=0, consts=None):
    """how many strides of WORD_GRID_CAP * GRID_BLOCK words a grid-stride pass over the volume's words takes (shapes only)"""
    c = consts or kernel_constants()
    per = c['WORD_GRID_CAP'] * c['GRID_BLOCK']
    return -(-n_words(shape, P) // per)


def run_heads(mask):
    """bool: first voxel of every z-run of `mask`"""
    m = mask != 0
    h = m.copy()
    h[:, :, 1:] &= ~m[:, :, :-1]
    return h


def head_word_of_voxels(mask, P=0):
    """per foreground voxel the word of its z-run's head (the passes handle a run in the thread of the word it STARTS in); -1 in
    the background"""
    m = mask != 0
    w = word_of_voxels(mask.shape, P)
    hw = np.where(run_heads(m), w, -1)
    hw = np.maximum.accumulate(hw, axis=2)      # words ascend along z: the last head at or below the voxel
    return np.where(m, hw, -1)


def max_distinct_per_span(words, ids, span):
    """largest number of distinct `ids` among the entries whose word falls into one span of `span` consecutive words, and the
    largest number of entries in one span"""
    words, ids = np.asarray(words).reshape(-1), np.asarray(ids).reshape(-1)
    if words.size == 0:
        return 0, 0
    s = words // span
    pairs = np.unique(np.stack((s, ids.astype(np.int64)), axis=1), axis=0)
    return int(np.bincount(pairs[:, 0]).max()), int(np.bincount(s).max())


def queued_markers(mask, markers, comp):
    """bool: what k_ws_init queues -- marker voxels of a component with several markers that have a 6-neighbour inside the mask
    without a marker -- and the bool vector (index = component id) of the components with several markers"""
    m = mask != 0
    mk = np.where(m, markers, 0)
    nc = int(comp.max())
    sel = mk > 0
    lo = np.full(nc + 1, np.iinfo(np.int64).max)
    hi = np.zeros(nc + 1, np.int64)
    np.minimum.at(lo, comp[sel], mk[sel])
    np.maximum.at(hi, comp[sel], mk[sel])
    multi = hi > lo
    free = m & (mk == 0)
    nb = np.zeros(m.shape, bool)
    for ax in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[ax], b[ax] = slice(1, None), slice(None, -1)
        nb[tuple(a)] |= free[tuple(b)]
        nb[tuple(b)] |= free[tuple(a)]
    return sel & nb & multi[comp], multi


# ---- the oracle for a custom element -----------------------------------------------------------------------------------------------
def watershed_oracle(vol, ops, struct, min_seed_vx, pitch):
    """object_extraction_steps.py:316-352 composed from the oracle's pieces for an explicit element (threshold 0: `vol` is a 0/1
    mask) -> dict(mask, markers, d2, dist, labels, max_label)"""
    tmp, markers = seed_markers_ref(vol, ops, np.asarray(struct).astype(bool), min_seed_vx)
    dist, d2 = distance_transform_ref(tmp, np.asarray(pitch).astype(np.uint32))
    labels = watershed_ref(d2, markers, tmp)
    return dict(mask=tmp, markers=markers, d2=d2, dist=dist, labels=labels, max_label=int(labels.max()) if labels.size else 0)


def seed_handover(markers0, min_seed_vx):
    """the id lists of the min_seed_vx filter (:330-347) from the unfiltered seed labels: (deleted ids, kept ids, J = number of
    freed ids handed to the largest kept ids)"""
    cnt = np.bincount(markers0.reshape(-1).astype(np.int64))
    ids = np.arange(1, len(cnt))
    dele, keep = ids[cnt[1:] < min_seed_vx], ids[cnt[1:] >= min_seed_vx]
    j = 0
    while j < min(len(dele), len(keep)) and dele[j] < keep[len(keep) - 1 - j]:
        j += 1
    return dele, keep, j


# ---- A: table and id-count lattice -------------------------------------------------------------------------------------------------
LATTICE_SLABS = (6, 28, 4)
LATTICE_YZ = (48, 160)


def table_lattice(slabs=LATTICE_SLABS, yz=LATTICE_YZ):
    """0/1 volume of three x-slabs with an empty plane between them -- A: isolated z-runs `111` (one single-voxel seed each under
    the z-only erosion), B: on every second plane pairs of runs `1111` joined at one voxel (two two-voxel seeds, not adjacent: the
    flood decides the rest), C: one component of interlocking runs with thousands of seeds of one and two voxels."""
    a, b, c = slabs
    Y, Z = yz
    X = a + 1 + b + 1 + c
    x, y, z = np.indices((X, Y, Z))
    vol = np.zeros((X, Y, Z), bool)
    ina = x < a
    vol |= ina & (((z % 6) // 3) == ((x + y) % 2))
    xb = x - (a + 1)
    inb = (xb >= 0) & (xb < b) & (xb % 2 == 0)
    vol |= inb & (((y % 3 == 0) & (z % 8 < 4)) | ((y % 3 == 1) & (z % 8 >= 3) & (z % 8 < 7)))
    inc = x >= a + 1 + b + 1
    even = (x + y) % 2 == 0
    vol |= inc & ((even & (z % 5 < 4)) | (~even & np.isin(z % 5, (3, 4, 0))))
    return vol.astype(np.uint8)


# ---- B: flood lattice for sd_marker_flood ------------------------------------------------------------------------------------------
def flood_lattice(shape, variant):
    """components `m o m` along z, one background voxel between them, on the rows with even x + y (the others are empty: nothing
    touches across rows); marker ids are a permutation of 1..n.  variant 'differ': the two markers of a component have different
    levels (the higher one wins the middle voxel; which of the two alternates), the middle voxel's level varies around them;
    'equal': one level everywhere, the raster order of the markers decides.  -> (d2 int32, markers int32, mask uint8)"""
    X, Y, Z = shape
    x, y, z = np.indices(shape)
    mask = ((x + y) % 2 == 0) & (z % 4 < 3)
    is_mk = mask & (z % 4 != 1)
    n = int(is_mk.sum())
    perm = (np.arange(n, dtype=np.int64) * 7919 + 13) % n      # 7919 is prime and n < 7919 ** 2 is not a multiple of it
    assert len(np.unique(perm)) == n
    markers = np.zeros(shape, np.int32)
    markers[is_mk] = (perm + 1).astype(np.int32)
    if variant == 'equal':
        d2 = np.where(mask, 5, 0)
    else:
        cell = x * 31 + y * 17 + z // 4
        first_high = cell % 2 == 0
        lvl = np.where((z % 4 == 0) == first_high, 9, 4)      # the marker that wins has level 9, the other 4
        mid = np.choose(cell % 3, [1, 6, 12])                 # below both, between them, above both (a cascade seed)
        d2 = np.where(z % 4 == 1, mid, lvl) * mask
    return d2.astype(np.int32), markers, mask.astype(np.uint8)


# ---- C: thin volume past the launch caps -------------------------------------------------------------------------------------------
THIN_SHAPE = (1460, 1460, 8)
THIN_PERIOD = (8, 10)


def thin_lattice(shape=THIN_SHAPE, period=THIN_PERIOD):
    """Z = 8 (one mask word per row), one object per cell of `period` rows in x and y, the cell's kind cycling through
    pair 3 + 3 (row y [a, a+3), row y+1 [a+2, a+5): two single-voxel seeds), pair 3 + 3, pair 4 + 4 ([a, a+4) and [a+3, a+7): two
    two-voxel seeds), isolated run of 3, isolated run of 4; a varies with the cell.  Cells cut off by the volume's end are left out."""
    X, Y, Z = shape
    assert Z == 8
    px, py = period
    vol = np.zeros(shape, np.uint8)
    cx, cy = np.meshgrid(np.arange(X // px), np.arange((Y - 1) // py), indexing='ij')
    cx, cy = cx.reshape(-1), cy.reshape(-1)
    kind = (cx * 3 + cy) % 5
    x0, y0 = cx * px + (cy % 3), cy * py + (cx % 4)      # jitter inside the cell (px >= 4, py >= 6 keep the objects apart)
    a = (cx + 2 * cy) % 12
    for k, (l0, l1, shift, amax) in enumerate(((3, 3, 2, 4), (3, 3, 2, 4), (4, 4, 3, 2), (3, 0, 0, 6), (4, 0, 0, 5))):
        s = kind == k
        aa = a[s] % amax
        for dz in range(l0):
            vol[x0[s], y0[s], aa + dz] = 1
        for dz in range(l1):
            vol[x0[s], y0[s] + 1, aa + shift + dz] = 1
    return vol


# ---- D: words, pads and wide elements ----------------------------------------------------------------------------------------------
def _asym_element():
    e = np.ones((3, 3, 5), np.uint8)
    e[0, 0, :2] = 0
    e[2, 1, 4] = 0
    return e


ELEMENTS = {'3x3x7': np.ones((3, 3, 7), np.uint8), '1x1x15': np.ones((1, 1, 15), np.uint8), '5x3x5': np.ones((5, 3, 5), np.uint8),
            'asym3x3x5': _asym_element()}
# (operation list, largest `iterations`, pad P = largest count of a closing / dilation)
OP_LISTS = ((['binary_opening'], 1, 0), (['binary_closing'], 1, 1), (['binary_dilation'] * 2, 2, 2), (['binary_closing'] * 3, 3, 3),
            (['binary_dilation'] * 5, 5, 5), (['binary_closing'] * 5, 5, 5), (['binary_opening'] * 2 + ['binary_closing'], 2, 1),
            (['binary_opening'] * 3 + ['binary_dilation'], 3, 1), (['binary_closing'] * 2 + ['binary_opening'] * 2, 2, 2))
PADDED_Z = (31, 32, 33, 64, 65)
MASK_KINDS = ('blobs', 'full', 'full_rows', 'word_runs', 'six_faces')
MORPH_XY = (16, 14)


def morph_mask(kind, shape, P, seed=0):
    """structured 0/1 masks for the bit-packed morphology; `P` places the runs of 'word_runs' on the words of the padded volume"""
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    if kind == 'blobs':
        v = ndimage.gaussian_filter(rng.random(shape), (2.0, 2.0, 3.0))
        return (v > np.quantile(v, 0.45)).astype(np.uint8)
    if kind == 'full':
        return np.ones(shape, np.uint8)
    m = np.zeros(shape, np.uint8)
    if kind == 'full_rows':                    # full rows between empty ones: one run over every word of the row
        m[::2, ::3, :] = 1
        m[1::2, 1::3, :] = 1
        return m
    if kind == 'word_runs':                    # padded z = z + P; per row one pattern over the words of the padded row
        def put(x, y, a, b):
            m[x, y, max(a, 0):max(min(b, Z), 0)] = 1
        for r, (x, y) in enumerate((x, y) for x in range(X) for y in range(Y)):
            for w in range(words_per_row(Z, P)):
                lo, hi, n = 32 * w - P, 32 * w + 32 - P, 1 + (r // 4 + w) % 5
                if r % 4 == 0:
                    put(x, y, lo, lo + n)                      # runs that start at bit 0
                elif r % 4 == 1:
                    put(x, y, hi - n, hi)                      # runs that end at bit 31
                elif r % 4 == 2 and (w + r // 4) % 2 == 0:
                    put(x, y, lo, hi)                          # whole words
                elif r % 4 == 3:
                    put(x, y, hi - n, hi + n)                  # runs across the word boundary
        return m
    if kind == 'six_faces':                    # a sparse body whose bounding box is the whole volume: the closing quirk at its faces
        v = ndimage.gaussian_filter(rng.random(shape), (1.0, 1.0, 1.5))
        m = (v > np.quantile(v, 0.7)).astype(np.uint8)
        m[0, Y // 2, Z // 2] = m[X - 1, Y // 3, Z // 3] = m[X // 2, 0, Z // 2] = m[X // 3, Y - 1, Z - 1] = 1
        m[X // 2, Y // 2, 0] = m[X // 3, Y // 3, Z - 1] = 1
        return m
    raise ValueError(kind)


def morph_oracle(mask, ops, struct):
    """mask after the operations, its scipy labels and their count"""
    out = apply_morphological_operations_ref(mask, ops, np.asarray(struct).astype(bool))
    lab, n = ndimage.label(out)
    return out, lab, int(n)


# ---- E: masks for the distance output ----------------------------------------------------------------------------------------------
def distance_mask(kind, seed=0):
    rng = np.random.default_rng(seed)
    if kind == 'blobs':
        v = ndimage.gaussian_filter(rng.random((37, 30, 41)), 2.0)
        return (v > np.quantile(v, 0.45)).astype(np.uint8)
    if kind == 'full_z_rows':                  # rows without background along z: the z pass leaves "infinity", y / x decide
        m = np.zeros((19, 23, 34), np.uint8)
        m[2:17, 3:20, :] = 1
        m[5, 7, 11] = 0
        m[8:11, 12, :] = 0
        return m
    if kind == 'full':
        return np.ones((9, 11, 33), np.uint8)
    if kind == 'x_slab':                       # the nearest background of the far end is 40+ voxels away along x only; the outward
        m = np.ones((47, 6, 5), np.uint8)      # search runs in rounds of four candidates up to the array edge
        m[0, :, :] = 0
        return m
    if kind == 'faces':                        # a foreground voxel on each face of the array (the border is not background)
        m = np.zeros((13, 12, 35), np.uint8)
        m[4:9, 4:9, 10:25] = 1
        m[0, 5, 17] = m[12, 6, 3] = m[6, 0, 20] = m[7, 11, 30] = m[5, 5, 0] = m[8, 7, 34] = 1
        m[0:3, 2, 2] = 1
        return m
    raise ValueError(kind)


DISTANCE_MASKS = ('blobs', 'full_z_rows', 'full', 'x_slab', 'faces')
PITCHES = ((10, 10, 20), (4, 4, 35), (1, 1, 1), (9, 9, 20))

# ---- F / G: shapes of the Gaussian and error-return cases ---------------------------------------------------------------------------
GAUSS_BIG_SHAPE = (130, 128, 127)                  # more voxels than one grid stride of the voxel passes
THINNER_THAN_PAD = (((7, 6, 1), 5), ((7, 6, 1), 16))
PITCH_REJECTED = ((47, 3, 8), (383, 1, 1))         # pitch x extent = 18001
PITCH_ACCEPTED = ((48, 3, 8), (375, 1, 1))         # ... = 18000
TOO_MANY_VOXELS = (2048, 1024, 1024)
