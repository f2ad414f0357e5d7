"""GPU: the synapse agglomeration past its launch caps, on an analytic input (run once, under its own time limit like the other scale
tests).  Four cell pairs:

A  a lattice of solid blocks of 3 x 2 x 2 voxels whose spacings alternate, per axis, between one lattice step inside the gap and
   exactly the gap (x: 24 / 25 voxels at 10 nm, y: 25 / 24, z: 12 / 13 at 20 nm; a z step of 12.5 does not exist, so 13 = 260 nm stands
   for "at the gap or beyond" there): ~1.1 M voxels, more cells than one trip of the wave-per-cell kernel, three fragments;
B  a lattice of single voxels exactly at the gap in x and y and beyond it in z: every voxel is a component of its own -- more than
   2^20 + 2^16 voxels, cells and components, so every grid-stride loop (4096 x 256 threads) takes a second trip; all of them fall to
   the size filter and still count for ``ordinal``;
C  chains of single voxels 24 voxels apart that cross hundreds of cells, a parallel chain exactly at the gap, and one with a break;
D  one solid block of 61 x 59 x 31 voxels: more than 10^5 voxels in a single component.

The expected partition comes from a graph over the blocks: the smallest distance between two solid boxes is analytic.  The expected
statistics are numpy reductions over that partition, the expected table is the host edge (pinned to golden g19 on the CPU) on them.
A second call with the groups permuted must give the same rows per group."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.csgraph

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _syn_ssv_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
SCALE, GAP, MIN_VX = (10, 10, 20), 250, 50


def lattice_positions(n, size, steps):
    """Start coordinates of n blocks of `size` voxels along one axis; the coordinate difference between the facing voxels of two
    neighbours alternates through `steps`."""
    gaps = np.resize(np.asarray(steps), n - 1) if n > 1 else np.zeros(0, np.int64)
    return np.concatenate(([0], np.cumsum(size - 1 + gaps))).astype(np.int64)


def block_components(lo, hi):
    """Components of solid boxes [lo, hi] (inclusive voxel boxes, (n, 3)): an edge where the smallest scaled distance between two
    boxes is strictly below the gap.  Candidates through a KD-tree on the box centres with a radius that cannot miss an edge."""
    import scipy.spatial
    s = np.asarray(SCALE, np.float64)
    centre, half = (lo + hi) * 0.5 * s, ((hi - lo) * 0.5 * s)
    reach = GAP + 2 * np.linalg.norm(half.max(0)) + 1
    pairs = scipy.spatial.cKDTree(centre).query_pairs(r=reach, output_type='ndarray')
    i, j = pairs[:, 0], pairs[:, 1]
    free = np.maximum(0, np.maximum(lo[j] - hi[i], lo[i] - hi[j]))
    d2 = ((free * np.asarray(SCALE, np.int64)) ** 2).sum(1)                 # exact integers
    e = d2 < GAP * GAP
    g = scipy.sparse.coo_matrix((np.ones(int(e.sum()), bool), (i[e], j[e])), shape=(len(lo), len(lo)))
    return scipy.sparse.csgraph.connected_components(g, directed=False)[1]


def fill_blocks(lo, shape):
    """All voxels of the boxes at `lo` (n, 3) with common `shape`, block-major, scan order inside a block.  -> (voxels, block index)"""
    cell = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).reshape(-1, 3)
    vox = (lo[:, None, :] + cell[None]).reshape(-1, 3)
    return vox, np.repeat(np.arange(len(lo)), len(cell))


def build_input():
    """-> list of groups: (key, [(syn id, voxels, sym, asym)], block label per voxel (equal labels <=> one component))."""
    groups = []
    # A: 56 x 52 x 32 blocks of 12 voxels
    px, py, pz = lattice_positions(56, 3, [24, 25]), lattice_positions(52, 2, [25, 24]), lattice_positions(32, 2, [12, 13])
    lo = np.stack(np.meshgrid(px, py, pz, indexing='ij'), -1).reshape(-1, 3)
    comp = block_components(lo, lo + (2, 1, 1))
    vox, blk = fill_blocks(lo, (3, 2, 2))
    third = (np.arange(len(lo)) * 3) // len(lo)                             # three fragments: thirds of the block list
    frags = [((2 << 32) + 100 + f, vox[third[blk] == f], 0.25 * f, 0.125) for f in range(3)]
    groups.append([(3 << 32) + 2, frags, np.concatenate([comp[blk][third[blk] == f] for f in range(3)])])
    # B: 105 x 105 x 102 single voxels, 25 / 25 / 13 apart: no edges at all
    q = np.stack(np.meshgrid(np.arange(105) * 25, np.arange(105) * 25, np.arange(102) * 13, indexing='ij'), -1).reshape(-1, 3) + (7, 3, 5)
    groups.append([(5 << 32) + 4, [((4 << 32) + 200, q[:600000], 0.5, 0.5), ((4 << 32) + 201, q[600000:], 0.0, 1.0)], np.arange(len(q))])
    # C: chains; voxel k of a chain at x = 24 k, y wiggling by +-1 (sqrt(240^2 + 10^2) < 250)
    k = np.arange(420)
    main = np.stack([24 * k, 50 + (k % 2), np.full_like(k, 9)], 1)
    side = np.stack([24 * k[:200], np.full(200, 50 + 26), np.full(200, 9)], 1)          # 25 voxels from the nearest main voxel: apart
    broken = np.stack([24 * k[:300] + (k[:300] >= 150), np.full(300, 200), np.full(300, 9)], 1)    # one step of 25 voxels in the middle
    frags = [((6 << 32) + 300, main[::2], 1.0, 0.0), ((6 << 32) + 301, main[1::2], 0.0, 1.0), ((6 << 32) + 302, side, 0.5, 0.0),
             ((6 << 32) + 303, broken, 0.25, 0.25)]
    lab = np.concatenate([np.zeros(210), np.zeros(210), np.ones(200), 2 + (k[:300] >= 150)]).astype(np.int64)
    groups.append([(7 << 32) + 6, frags, lab])
    # D: one block above 10^5 voxels, two fragments
    vox, _ = fill_blocks(np.array([[1000, 2000, 300]]), (61, 59, 31))
    assert len(vox) > 100000
    groups.append([(9 << 32) + 8, [((8 << 32) + 400, vox[:70000], 0.125, 0.0), ((8 << 32) + 401, vox[70000:], 0.0, 0.75)], np.zeros(len(vox), np.int64)])
    return groups


def expected_table(groups, reference_indexing=True):
    from syconn_amd.extraction.cs_processing_steps import build_syn_ssv_table
    vox = np.concatenate([f[1] for _, fr, _ in groups for f in fr])
    frags = [f for _, fr, _ in groups for f in fr]
    vox_frag = np.repeat(np.arange(len(frags)), [len(f[1]) for f in frags])
    frag_group = np.repeat(np.arange(len(groups)), [len(fr) for _, fr, _ in groups])
    # component numbers over the whole input, ascending in the smallest flat index
    raw = np.concatenate([lab.astype(np.int64) + off for (_, _, lab), off in
                          zip(groups, np.concatenate(([0], np.cumsum([int(lab.max()) + 1 for _, _, lab in groups])))[:-1])])
    _, first, inv = np.unique(raw, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    labels = rank[inv.reshape(-1)]
    st = S.stats_from_labels(vox, vox_frag, frag_group, labels, SCALE, MIN_VX)
    return build_syn_ssv_table([k for k, _, _ in groups], np.concatenate(([0], np.cumsum([len(fr) for _, fr, _ in groups]))),
                               [f[0] for f in frags], [f[2] for f in frags], [f[3] for f in frags], scaling=SCALE, min_obj_vx=MIN_VX,
                               sym_thresh=0.225, reference_indexing=reference_indexing, **st), labels


def run(groups, gpu):
    from syconn_amd.extraction.cs_processing_steps import combine_and_split_syn
    frags = [f for _, fr, _ in groups for f in fr]
    table = S.Table([f[0] for f in frags], [f[1] for f in frags], [f[2] for f in frags], [f[3] for f in frags])
    mapping = {sv: sv for sv in (2, 4, 6, 8)}
    mapping.update({f[0] & 0xffffffff: (f[0] >> 32) + 1 for f in frags})
    return combine_and_split_syn(table, mapping, scaling=SCALE, cs_gap_nm=GAP, min_obj_vx=MIN_VX, sym_thresh=0.225, device=gpu,
                                 return_stats=True)


def test_past_the_launch_caps(gpu):
    groups = build_input()
    want, labels = expected_table(groups)
    n_vox = len(labels)
    assert n_vox > 2 ** 20 + 2 ** 16 and want.n_components > 2 ** 20 + 2 ** 16
    got, info = run(groups, gpu)
    counts = [int(v) for v in info['counts']]
    print('cell', info['cell'].tolist(), 'voxels', n_vox, 'counts', counts)
    assert counts[0] == want.n_components and counts[1] > 2 ** 20 + 2 ** 16 and counts[7] == 0
    S.assert_tables_equal(got, want)
    # what the input is meant to hold
    sizes_a = want.sizes[want.group == 0]
    # A: blocks pair up along x (28 pairs) and z (16 pairs); along y the first step is AT the gap, so blocks 0 and 51 stay single between
    # 25 pairs: 28 x 27 x 16 components, of which the 28 x 2 x 16 = 896 with a single y block hold 4 blocks (48 voxels) and are dropped
    assert len(sizes_a) == 28 * 25 * 16 and (sizes_a == 8 * 12).all()
    assert int((np.bincount(labels[:12 * 56 * 52 * 32]) == 48).sum()) == 28 * 2 * 16
    assert not (want.group == 1).any()                                              # B: every single voxel dropped, and counted:
    assert want.ordinal[want.group == 2].min() > 105 * 105 * 102
    assert want.sizes[want.group == 2].tolist() == [420, 200, 150, 150] and want.sizes[want.group == 3].tolist() == [61 * 59 * 31]
    assert counts[6] > 0 and counts[4] > 0 and counts[3] > 0                        # voxel-tested, joined by boxes, skipped by boxes
    # the groups permuted: the same rows per group
    perm = [2, 0, 3, 1]
    got_p, _ = run([groups[p] for p in perm], gpu)
    assert len(got_p) == len(got)
    for new_g, old_g in enumerate(perm):
        a, b = np.flatnonzero(got_p.group == new_g), np.flatnonzero(got.group == old_g)
        assert len(a) == len(b)
        for name in ('neuron_partners', 'sizes', 'rep_coords', 'bounding_boxes', 'sym_prop', 'asym_prop', 'syn_type_sym_ratio', 'syn_sign',
                     'group_ordinal'):
            assert getattr(got_p, name)[a].tobytes() == getattr(got, name)[b].tobytes(), (old_g, name)
        for begin, col in (('vox_begin', 'voxels'), ('cs_begin', 'cs_ids'), ('frag_begin', 'frag_counts')):
            if len(a):
                pa, pb = getattr(got_p, begin), getattr(got, begin)
                assert np.array_equal(getattr(got_p, col)[pa[a[0]]:pa[a[-1] + 1]], getattr(got, col)[pb[b[0]]:pb[b[-1] + 1]]), (old_g, col)
