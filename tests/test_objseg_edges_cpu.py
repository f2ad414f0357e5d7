"""CPU: the cases of tests/test_gpu_objseg_edges.py sit where they claim -- proven with the oracle (oracle/objseg_ref.py) and a model
of the word-indexed passes of `syconn_amd/csrc/sd_objseg.hip` whose constants are read from the sources (tests/_objseg_cases.py).
"More than the slot count" distinct keys in one workgroup's span is the only order-independent guarantee that a probe sequence of
an LDS table fails, so the counts are asserted to EXCEED the tables, not merely to load them."""
import functools

import numpy as np
import pytest
from scipy import ndimage

import _objseg_cases as K
from oracle.objseg_ref import apply_morphological_operations_ref, seed_markers_ref, watershed_ref

C = K.kernel_constants()


def test_kernel_constants_are_the_ones_the_cases_were_built_for():
    """a retuned kernel lands here first: look at every case of this file again before changing a number"""
    assert C == dict(SCAN_PER_THREAD=8, HEAD_SLOTS=512, HEAD_PROBES=8, COMP_SLOTS=512, INIT_SLOTS=256, INIT_LIST=3072, LDS_PROBES=8,
                     WI_WORDS=4, WSP_CAP=8192, WS_LDS_CAP=4608, WSP_THREADS=1024, MAX_OFFS=128, EDT_INF=0x3f000000, GAUSS_MAX_R=64,
                     SCAN_ROUND=1024, FLOOD_GRID=2048, FLOOD_SEQ_GRID=4096, WORD_GRID_CAP=8192, GRID_BLOCK=256, MAX_ITER=64,
                     MAX_EXTENT=15, MAX_PITCH_EXTENT=18000)
    assert K.span_words('stride', C) == 256 and K.span_words('init', C) == 1024


def test_launch_model_words():
    w = K.word_of_voxels((2, 3, 40), P=3)                      # padded rows of 46 bits: 2 words
    assert K.words_per_row(40, 3) == 2 and K.n_words((2, 3, 40), 3) == 12
    assert w[0, 0, 28] == 0 and w[0, 0, 29] == 1 and w[0, 1, 0] == 2 and w[1, 2, 39] == 11
    m = np.zeros((1, 1, 70), np.uint8)
    m[0, 0, 30:67] = 1                                         # one run over three words: handled where it starts
    assert set(np.unique(K.head_word_of_voxels(m))) == {-1, 0}
    assert K.max_distinct_per_span([0, 1, 255, 256, 257], [5, 5, 6, 7, 7], 256) == (2, 3)


# ---- A ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lattice():
    vol = K.table_lattice()
    tmp, mk0 = seed_markers_ref(vol, ['binary_erosion'], K.Z_ELEMENT.astype(bool), 0)
    _, mk2 = seed_markers_ref(vol, ['binary_erosion'], K.Z_ELEMENT.astype(bool), 2)
    comp, nc = ndimage.label(tmp)
    return vol, tmp, mk0, mk2, comp, nc


def test_table_lattice_id_counts_pass_the_scan_round_and_the_flood_grids():
    vol, tmp, mk0, mk2, comp, nc = _lattice()
    assert np.array_equal(tmp, vol) and vol.size < 400000
    n_seeds = int(mk0.max())
    print(f'{vol.shape}: {n_seeds} seeds, {int(mk2.max())} after min_seed_vx = 2, {nc} mask components')
    assert n_seeds > 2 * C['SCAN_ROUND'] and nc > 2 * C['SCAN_ROUND']      # k_scan_excl carries twice (rd[] and off[])
    for mk in (mk0, mk2):
        _, multi = K.queued_markers(tmp, mk, comp)
        print('multi-marker components:', int(multi.sum()))
        assert int(multi.sum()) > max(C['FLOOD_GRID'], C['FLOOD_SEQ_GRID'])
    # components without any marker, with one and with several all occur
    per_comp = np.bincount(np.unique(np.stack((comp[mk0 > 0], mk0[mk0 > 0].astype(np.int64)), 1), axis=0)[:, 0], minlength=nc + 1)[1:]
    assert (per_comp == 0).any() and (per_comp == 1).sum() > 1000 and (per_comp == 2).sum() > 4000 and per_comp.max() > 5000
    # the giant component's generation never outgrows the LDS sort (generations beyond WSP_CAP: test_gpu_marker_flood_large_generations)
    assert int(np.bincount(comp.reshape(-1))[1:].max()) > C['WS_LDS_CAP']


def test_table_lattice_saturates_the_lds_tables():
    vol, tmp, mk0, mk2, comp, nc = _lattice()
    span, ispan = K.span_words('stride', C), K.span_words('init', C)
    words = K.word_of_voxels(vol.shape, 0)
    # k_cc_head_labels with cnt (min_seed_vx > 1): labels of the seed runs that start in a span, before the filter
    sh = K.run_heads(mk0 > 0)
    seeds_per_span, _ = K.max_distinct_per_span(words[sh], mk0[sh], span)
    # run_cc(cnt = off) of the mask: component ids of the mask runs that start in a span
    mh = K.run_heads(tmp)
    comps_per_span, _ = K.max_distinct_per_span(words[mh], comp[mh], span)
    # k_comp_markers (S given): components among the seed runs of a span
    seedcomps_per_span, _ = K.max_distinct_per_span(words[sh], comp[sh], span)
    print(f'per 256-word span: {seeds_per_span} seed ids, {comps_per_span} mask components, {seedcomps_per_span} components of seed runs')
    assert seeds_per_span > C['HEAD_SLOTS'] and comps_per_span > C['HEAD_SLOTS'] and seedcomps_per_span > C['COMP_SLOTS']
    # (after the min_seed_vx = 2 filter the single-voxel seeds are gone: k_comp_markers' table overflows at min_seed_vx <= 1 only)
    for mk in (mk0, mk2):      # k_ws_init (S given: queued markers sit in the word of the marker voxel itself)
        q, multi = K.queued_markers(tmp, mk, comp)
        comps_q, n_q = K.max_distinct_per_span(words[q], comp[q], ispan)
        print(f'per 1024-word span: {comps_q} multi-marker components with a queued marker, {n_q} queued markers; '
              f'{int(q[comp == np.argmax(np.bincount(comp.reshape(-1))[1:]) + 1].sum())} in the giant component')
        assert comps_q > C['INIT_SLOTS'] and n_q > C['INIT_LIST']


def test_table_lattice_seed_filter_lists():
    vol, tmp, mk0, mk2, comp, nc = _lattice()
    dele, keep, j = K.seed_handover(mk0, 2)
    print(f'min_seed_vx = 2: {len(dele)} deleted, {len(keep)} kept, J = {j}')
    assert len(dele) > C['SCAN_ROUND'] and len(keep) > C['SCAN_ROUND'] and 0 < j < min(len(dele), len(keep))
    # the holes are filled from the top: dense ids 1..kept, J ids changed hands
    assert np.array_equal(np.unique(mk2), np.arange(len(keep) + 1))
    moved = np.unique(mk0[(mk2 != mk0) & (mk2 > 0)])
    assert len(moved) == j and np.array_equal(moved, keep[len(keep) - j:])


# ---- B ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(12, 32, 96), (12, 32, 97)])
def test_flood_lattice(shape):
    ispan = K.span_words('init', C)
    for variant in ('differ', 'equal'):
        d2, markers, mask = K.flood_lattice(shape, variant)
        assert mask.size < 40000 and not markers[mask == 0].any() and not d2[mask == 0].any()
        comp, nc = ndimage.label(mask)
        q, multi = K.queued_markers(mask, markers, comp)
        n_multi = 6 * 32 * (shape[2] // 4)
        assert int(multi.sum()) == n_multi > C['FLOOD_SEQ_GRID'] and nc == n_multi + (6 * 32 if shape[2] % 4 == 1 else 0)
        assert np.array_equal(np.unique(markers), np.arange(2 * n_multi + nc - n_multi + 1))      # a permutation of 1..n
        # S == nullptr: k_ws_init walks the voxels of the runs that start in a word
        hw = K.head_word_of_voxels(mask, 0)
        comps_q, n_q = K.max_distinct_per_span(hw[q], comp[q], ispan)
        print(f'{shape} {variant}: {nc} components, per 1024-word span {comps_q} components / {n_q} queued markers')
        assert comps_q > C['INIT_SLOTS'] and n_q > C['INIT_LIST'] and int(q.sum()) == 2 * n_multi
        want = watershed_ref(d2.astype(np.int64), markers, mask)
        mid = mask.astype(bool) & (markers == 0)
        lower = np.roll(markers, 1, axis=2)[mid]                  # the marker below the middle voxel, the one above
        upper = np.roll(markers, -1, axis=2)[mid]
        if variant == 'equal':                                    # ties: the marker voxel that comes first in raster order
            assert np.array_equal(want[mid], lower)
        else:                                                     # the higher level wins, which is the upper marker half of the time
            up = np.roll(d2, -1, axis=2)[mid] > np.roll(d2, 1, axis=2)[mid]
            assert np.array_equal(want[mid], np.where(up, upper, lower)) and 0.4 < up.mean() < 0.6
            assert set(np.unique(d2[mid])) == {1, 6, 12}


# ---- C ---------------------------------------------------------------------------------------------------------------------------
def test_thin_lattice_passes_the_launch_caps():
    per = C['WORD_GRID_CAP'] * C['GRID_BLOCK']
    X, Y, Z = K.THIN_SHAPE
    assert K.words_per_row(Z, 0) == 1 and K.n_words(K.THIN_SHAPE, 0) > per and K.strides_of_word_pass(K.THIN_SHAPE, 0, C) == 2
    px, py = K.THIN_PERIOD
    # objects start in rows past the first stride (x * Y + y >= per), of every kind
    first_x = -(-per // Y)
    cells_past = [(cx, cy) for cx in range(X // px) for cy in range((Y - 1) // py) if cx * px >= first_x]
    assert len(cells_past) > 100 and {(cx * 3 + cy) % 5 for cx, cy in cells_past} == {0, 1, 2, 3, 4}
    # the lattice on a cut-down copy of a few periods
    shape = (5 * px, 6 * py + 1, 8)
    vol = K.thin_lattice(shape)
    full = K.thin_lattice()
    assert np.array_equal(vol[:, :6 * py], full[:shape[0], :6 * py])      # ... is the corner of the full one
    assert int(full.reshape(X * Y, Z).any(axis=1)[per:].sum()) > 300      # occupied rows (= words) of the second stride
    comp, nc = ndimage.label(vol)
    assert nc == 5 * 6                                            # one object per cell, none touching
    sizes = np.bincount(comp.reshape(-1))[1:]
    assert sorted(set(sizes.tolist())) == [3, 4, 6, 8]
    o0 = K.watershed_oracle(vol, ['binary_erosion'], K.Z_ELEMENT, 0, (10, 10, 20))
    o2 = K.watershed_oracle(vol, ['binary_erosion'], K.Z_ELEMENT, 2, (10, 10, 20))
    per_comp = [len(np.unique(o0['markers'][(comp == c) & (o0['markers'] > 0)])) for c in range(1, nc + 1)]
    assert [per_comp[c] for c in range(nc) if sizes[c] in (6, 8)] == [2] * int(np.isin(sizes, (6, 8)).sum())
    assert all(per_comp[c] == 1 for c in range(nc) if sizes[c] in (3, 4))
    # seeds of one voxel (runs of 3) and of two (runs of 4): min_seed_vx = 2 deletes the former, keeps the latter, and the 4 + 4
    # pairs still hold two markers each
    cnt = np.bincount(o0['markers'].reshape(-1))[1:]
    assert set(cnt.tolist()) == {1, 2} and 0 < o2['max_label'] == int((cnt == 2).sum()) < o0['max_label']
    assert int(((o2['labels'] > 0) & (o2['markers'] == 0)).sum()) > 0
    # the whole volume stays cheap for the oracle's Python flood
    assert int(full.sum()) < 500000


# ---- D ---------------------------------------------------------------------------------------------------------------------------
def test_morphology_cases_reach_every_shift_pad_and_word_edge():
    offs = {n: np.argwhere(e) - np.array(e.shape) // 2 for n, e in K.ELEMENTS.items()}
    dz = set()
    for n, o in offs.items():
        assert len(o) <= C['MAX_OFFS'] and max(K.ELEMENTS[n].shape) <= C['MAX_EXTENT']
        dz |= set(o[:, 2].tolist()) | set((-o[:, 2]).tolist())                  # erosion reads +dz, dilation -dz
    assert dz == set(range(-7, 8)) and len(offs['5x3x5']) == 75
    a = offs['asym3x3x5']
    assert {tuple(v) for v in a} != {tuple(-v) for v in a}                      # not symmetric: reflection matters
    assert {it for _, it, _ in K.OP_LISTS} == {1, 2, 3, 5} and {p for _, _, p in K.OP_LISTS} == {0, 1, 2, 3, 5}
    for ops, it, p in K.OP_LISTS:
        names, cnt = [], []
        for o in ops:
            if names and names[-1] == o:
                cnt[-1] += 1
            else:
                names.append(o)
                cnt.append(1)
        assert max(cnt) == it and max([c for n, c in zip(names, cnt) if n in ('binary_closing', 'binary_dilation')], default=0) == p
        for pz in K.PADDED_Z:
            Z = pz - 2 * p
            assert Z >= 21 and K.words_per_row(Z, p) == (pz + 31) // 32
    assert K.words_per_row(31, 0) == 1 and K.words_per_row(33, 0) == 2 and K.words_per_row(65, 0) == 3      # one bit into a new word
    # word_runs: runs from bit 0 of a word and runs up to bit 31, in padded coordinates, and whole words
    for p in (0, 3, 5):
        Z = 65 - 2 * p
        m = K.morph_mask('word_runs', (4, 5, Z), p)
        pad = np.pad(m, ((0, 0), (0, 0), (p, p)))
        head = K.run_heads(pad)
        tail = K.run_heads(pad[:, :, ::-1])[:, :, ::-1]
        hz, tz = np.nonzero(head)[2], np.nonzero(tail)[2]
        assert (hz % 32 == 0).sum() > 5 and (tz % 32 == 31).sum() > 5 and (hz % 32 != 0).any() and (tz % 32 != 31).any()
    rows = K.morph_mask('full_rows', (4, 6, 64), 0)
    assert set(rows.sum(axis=2).reshape(-1).tolist()) == {0, 64}               # a run over every word: run_start_pz walks to word 0
    # six_faces: the bounding box is the volume; the closing REMOVES voxels on its faces (the reference's quirk)
    six = K.morph_mask('six_faces', K.MORPH_XY + (27,), 3)
    fg = np.argwhere(six)
    assert fg.min(0).tolist() == [0, 0, 0] and (fg.max(0) + 1).tolist() == list(K.MORPH_XY) + [27]
    closed = apply_morphological_operations_ref(six, ['binary_closing'], K.ELEMENTS['3x3x7'].astype(bool))
    assert int((six & ~closed.astype(bool)).sum()) > 0
    # thinner than the pad: Z = 1 with P = 5 has more PADDED words than voxels; more words than voxels inside the volume's own rows
    # (the branch in ws_layout that sizes the scan by words) needs Z + 2 P > 32 Z: Z = 1 with P = 16
    (sh5, p5), (sh16, p16) = K.THINNER_THAN_PAD
    assert sh5[2] == 1 and p5 == 5 and (sh5[0] + 2 * p5) * (sh5[1] + 2 * p5) * K.words_per_row(1, p5) > int(np.prod(sh5)) == K.n_words(sh5, p5)
    assert sh16[2] == 1 and K.n_words(sh16, p16) == 2 * int(np.prod(sh16))
    assert p16 <= C['MAX_ITER']


# ---- E ---------------------------------------------------------------------------------------------------------------------------
def test_distance_masks():
    from oracle.objseg_ref import distance_transform_ref
    m = {k: K.distance_mask(k) for k in K.DISTANCE_MASKS}
    assert m['full'].all()
    assert distance_transform_ref(m['full'], (10, 10, 20))[1].min() == C['EDT_INF']
    rows = m['full_z_rows']
    assert int((rows.all(axis=2)).sum()) > 100 and not rows.all()
    slab = m['x_slab']
    _, d2 = distance_transform_ref(slab, (1, 1, 1))
    assert d2.max() == (slab.shape[0] - 1) ** 2 >= 40 ** 2 and slab[1:].all()
    f = m['faces']
    assert f[0].any() and f[-1].any() and f[:, 0].any() and f[:, -1].any() and f[:, :, 0].any() and f[:, :, -1].any()
    for k, v in m.items():
        for pitch in K.PITCHES:
            assert max(p * n for p, n in zip(pitch, v.shape)) <= C['MAX_PITCH_EXTENT']
            if not v.all():      # (the squared-distance check reads the float32 output where it is exact)
                d2 = distance_transform_ref(v, pitch)[1]
                assert int(((d2 > 0) & (d2 < 2 ** 22)).sum()) > 50


# ---- F / G -----------------------------------------------------------------------------------------------------------------------
def test_gauss_and_error_cases():
    from oracle.objseg_ref import gaussian_kernel_ref
    assert int(np.prod(K.GAUSS_BIG_SHAPE)) > C['WORD_GRID_CAP'] * C['GRID_BLOCK']
    assert len(gaussian_kernel_ref(21.2)) == 2 * C['GAUSS_MAX_R'] + 1 and len(gaussian_kernel_ref(21.5)) == 2 * C['GAUSS_MAX_R'] + 3
    assert int(np.ones((15, 15, 1)).sum()) == 225 > C['MAX_OFFS']
    (s1, p1), (s0, p0) = K.PITCH_REJECTED, K.PITCH_ACCEPTED
    assert max(a * b for a, b in zip(s1, p1)) == C['MAX_PITCH_EXTENT'] + 1
    assert max(a * b for a, b in zip(s0, p0)) == C['MAX_PITCH_EXTENT']
    assert 3 * (C['MAX_PITCH_EXTENT'] ** 2) < C['EDT_INF']      # what the limit is for: squared distances stay below "infinity"
    assert int(np.prod(K.TOO_MANY_VOXELS)) == 2 ** 31
