"""CPU: golden g17 (the reference's own Cython stencil and closing loop at the edges of the device kernels' structure: 8 / 9 / more
partners per window, output extents around the 8 x 8 x 16 tile, degenerate stencils, closings with n or k = 0 and n = 12) is
reproduced by the numpy / scipy restatement the GPU tests compare with, the golden covers its claims, and an independent brute-force
count per window agrees with the restatement."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cs_ref  # noqa: E402

G17 = os.path.join(HERE, 'golden', 'g17_cs_edges.npz')
CP_SLOTS = 8                                     # register slots of k_contact_partners (csrc/sd_contacts.hip)


@pytest.fixture(scope='module')
def g17():
    return dict(np.load(G17))


def stencil_case(g, name):
    """-> (uint32 segmentation, edge mask, stencil, expected contacts) of one g17 stencil case."""
    return (g[f'st_{name}_raw'].astype(np.uint32), g[f'st_{name}_edges'], tuple(int(s) for s in g[f'st_{name}_stencil']),
            g[f'st_{name}_cs'])


def brute_partners(edges, seg, st):
    """Per flagged centre, from the window alone: np.unique with counts, 0 and the centre id dropped, first maximum (the smallest id
    of the highest count).  -> (packed result, number of distinct partners, True where the highest count is shared)."""
    out_shape = tuple(n - s + 1 for n, s in zip(seg.shape, st))
    res = np.zeros(out_shape, np.uint64)
    n_part = np.zeros(out_shape, np.int32)
    tie = np.zeros(out_shape, bool)
    h = [s // 2 for s in st]
    for x, y, z in np.ndindex(*out_shape):
        if not edges[x + h[0], y + h[1], z + h[2]]:
            continue
        c = int(seg[x + h[0], y + h[1], z + h[2]])
        ids, cnt = np.unique(seg[x:x + st[0], y:y + st[1], z:z + st[2]], return_counts=True)
        keep = (ids != 0) & (ids != c)
        ids, cnt = ids[keep], cnt[keep]
        n_part[x, y, z] = len(ids)
        if len(ids):
            k = int(ids[np.argmax(cnt)])
            tie[x, y, z] = (cnt == cnt.max()).sum() > 1
            res[x, y, z] = (min(c, k) << 32) | max(c, k)
    return res, n_part, tie


def test_restatement_reproduces_stencil_golden(g17):
    assert len(g17['stencil_cases']) == 15
    for name in g17['stencil_cases']:
        seg, g_edges, st, want = stencil_case(g17, name)
        edges = _cs_ref.seg_boundaries(seg)
        assert np.array_equal(edges, g_edges != 0), name
        cs = _cs_ref.contact_partners(edges, seg, st)
        assert cs.dtype == np.uint64 and cs.shape == want.shape and np.array_equal(cs, want), name


def test_restatement_reproduces_closing_golden(g17):
    assert [tuple(v) for v in g17['close_nk'].tolist()] == [(0, 2), (1, 1), (12, 3), (6, 0)]
    for n, k in g17['close_nk'].tolist():
        assert np.array_equal(_cs_ref.close_dilate(g17['cl_in'], n, k), g17[f'cl_{n}_{k}_out']), (n, k)


def test_brute_force_agrees_and_golden_covers_its_claims(g17):
    extents, stencils = set(), set()
    for name in g17['stencil_cases']:
        seg, edges, st, want = stencil_case(g17, name)
        stencils.add(st)
        extents.update(want.shape)
        res, n_part, tie = brute_partners(edges, seg, st)
        assert np.array_equal(res, want), name
        flagged = edges[tuple(slice(s // 2, s // 2 + o) for s, o in zip(st, want.shape))] != 0
        pool = int(name[1:name.index('_')])
        assert n_part.max() <= pool - 1, name
        if name in ('p9_s333', 'p9_s531', 'p9_s3d7', 'p9_sdd7'):                   # a full table, never more
            assert (n_part == CP_SLOTS).sum() > 0 and n_part.max() == CP_SLOTS, name
        if name in ('p10_s333', 'p10_s531', 'p10_s3d7', 'p10_sdd7'):               # the first overflow, next to windows that fit
            assert (n_part == CP_SLOTS + 1).sum() > 0, name
        if name in ('p10_s333', 'p10_s531'):                                       # ... and a tie for the highest count there
            assert (n_part == CP_SLOTS).sum() > 0 and (tie & (n_part == CP_SLOTS + 1)).any(), name
        if name.startswith('p12') and name != 'p12_s531':
            assert (n_part > CP_SLOTS + 1).sum() > 0, name
        if name in ('p9_sdd7', 'p10_sdd7', 'p12_sdd7'):                            # large windows hold the whole pool
            assert flagged.sum() > 500 and (n_part[flagged] == pool - 1).all(), name
        if name == 'p10_s111':
            assert flagged.any() and not want.any()
        if name.startswith('p10_eq'):
            assert want.shape == (1, 1, 1) and want.any(), name
    assert extents >= {1, 7, 8, 9, 15, 16, 17}
    assert stencils >= {(3, 3, 3), (5, 3, 1), (3, 13, 7), (13, 13, 7), (1, 1, 1)}
    # ids: 2^32 - 1 as centre and as partner, pairs >= 2^63
    cs = g17['st_p10_s333_cs']
    assert ((cs & np.uint64(0xFFFFFFFF)) == np.uint64(2 ** 32 - 1)).any() and (cs >= np.uint64(2 ** 63)).any()


def test_closing_golden_covers_its_claims(g17):
    c0 = g17['cl_in']
    for ax in range(3):
        first, last = np.take(c0, 0, ax), np.take(c0, -1, ax)
        assert (first[first != 77] != 0).any() and (last[last != 77] != 0).any(), ax       # a compact site on each of the six faces
    assert (c0 == 13).sum() == 1                                                            # one voxel
    w = np.argwhere(c0 == 77)
    assert np.array_equal(w.min(0), [0, 0, 0]) and np.array_equal(w.max(0) + 1, c0.shape)  # box = the whole volume
    assert (c0 >= np.uint64(2 ** 63)).any() and (c0 == np.uint64(2 ** 64 - 2)).any()
    # competing sites: the order of the sites matters somewhere, and ascending order is the one the golden holds
    asc, desc = _cs_ref.close_dilate(c0, 1, 1, 'ascending'), _cs_ref.close_dilate(c0, 1, 1, 'descending')
    assert (asc != desc).any() and np.array_equal(asc, g17['cl_1_1_out'])
    # every case changes the volume; n = 12 closes what n = 1 leaves open (the gap of three in site 12, the hole of site 15)
    for n, k in g17['close_nk'].tolist():
        assert (g17[f'cl_{n}_{k}_out'] != c0).any(), (n, k)
    gap = (slice(18, 21), slice(21, 24), 17)
    assert not c0[gap].any() and (g17['cl_12_3_out'][gap] == 12).all() and not (g17['cl_1_1_out'][gap] == 12).all()
    assert (g17['cl_6_0_out'][21:23, 15:17, 17] == 15).all()                # the tube is open along z: its middle closes
    # a face site loses its closing to the clipped box (erosion with border 0): it stays as it is at (6, 0)
    assert np.array_equal(g17['cl_6_0_out'] == 21, c0 == 21)
