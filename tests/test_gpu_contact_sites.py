"""GPU: the contact-site kernels (csrc/sd_contacts.hip) bit-exact against golden g15 (the reference's own Cython stencil and
closing loop) and against the numpy / scipy restatement on a larger random cell volume."""
import os
import sys

import numpy as np
import pytest
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cs_ref  # noqa: E402

pytestmark = pytest.mark.gpu
G15 = os.path.join(HERE, 'golden', 'g15_contact_sites.npz')


@pytest.fixture(scope='module')
def g15():
    return dict(np.load(G15))


def _cells(shape, n, seed):
    """Voronoi-like cells (random uint32 ids) at half resolution, upsampled, with 1 % background speckle."""
    rng = np.random.default_rng(seed)
    half = tuple(s // 2 for s in shape)
    lab = np.zeros(half, np.uint32)
    pts = tuple(rng.integers(0, s, n) for s in half)
    lab[pts] = rng.choice(np.arange(1, 2 ** 32 - 1, dtype=np.uint64), n, replace=False).astype(np.uint32)
    _, ind = scipy.ndimage.distance_transform_edt(lab == 0, return_indices=True)
    seg = lab[tuple(ind)].repeat(2, 0).repeat(2, 1).repeat(2, 2)
    seg[rng.random(shape) < 0.01] = 0
    return seg


def test_seg_boundaries_golden(gpu, g15):
    from syconn_amd.extraction.find_object_properties import detect_seg_boundaries
    for name in g15['stencil_cases']:
        seg = g15[f'st_{name}_raw'].astype(np.uint32)
        b = detect_seg_boundaries(seg)
        assert b.dtype == np.bool_ and np.array_equal(b, g15[f'st_{name}_edges'] != 0), name


def test_contact_partners_golden(gpu, g15):
    from syconn_amd.extraction.find_object_properties import detect_cs, process_block_nonzero
    for name in g15['stencil_cases']:
        seg = g15[f'st_{name}_raw'].astype(np.uint32)
        st = tuple(int(s) for s in g15[f'st_{name}_stencil'])
        want = g15[f'st_{name}_cs']
        got = process_block_nonzero(g15[f'st_{name}_edges'].astype(np.uint32), seg, st)
        assert got.dtype == np.uint64 and np.array_equal(got, want), name
        assert np.array_equal(detect_cs(seg, st), want), name


def test_detect_cs_default_stencil_and_device_io(gpu, g15):
    import torch
    from syconn_amd.extraction.find_object_properties import detect_cs
    seg = g15['st_vor13_raw'].astype(np.uint32)
    out = detect_cs(torch.from_numpy(seg.view(np.int32)).to(gpu), return_device=True)   # config default (13, 13, 7)
    assert out.is_cuda and out.dtype == torch.int64
    assert np.array_equal(out.cpu().numpy().view(np.uint64), g15['st_vor13_cs'])


def test_close_dilate_golden(gpu, g15):
    from syconn_amd.extraction.cs_extraction_steps import close_and_dilate_cs
    for name in g15['close_cases']:
        n, k = (int(v) for v in g15[f'cl_{name}_nk'])
        c0, want = g15[f'cl_{name}_in'], g15[f'cl_{name}_out']
        assert np.array_equal(close_and_dilate_cs(c0, n, k), want), name
        # one site per batch: the batching must not change the result
        assert np.array_equal(close_and_dilate_cs(c0, n, k, ws_budget=1), want), name


def test_close_dilate_trivial_cases(gpu):
    from syconn_amd.extraction.cs_extraction_steps import close_and_dilate_cs
    z = np.zeros((5, 6, 7), np.uint64)
    assert np.array_equal(close_and_dilate_cs(z, 6, 2), z)
    c = z.copy()
    c[2, 3, 3] = 2 ** 64 - 2
    assert np.array_equal(close_and_dilate_cs(c, 0, 0), c)
    assert np.array_equal(close_and_dilate_cs(c, 0, 1), _cs_ref.close_dilate(c, 0, 1))
    c[0, 0, 0] = 2 ** 64 - 1                                               # the reserved unclaimed marker is refused
    with pytest.raises(ValueError):
        close_and_dilate_cs(c, 6, 2)


def test_random_cells_against_restatement(gpu):
    from syconn_amd.extraction.cs_extraction_steps import close_and_dilate_cs
    from syconn_amd.extraction.find_object_properties import detect_cs, detect_seg_boundaries
    seg = _cells((160, 160, 80), 200, 1)
    edges = _cs_ref.seg_boundaries(seg)
    assert np.array_equal(detect_seg_boundaries(seg), edges)
    want = _cs_ref.contact_partners(edges, seg, (13, 13, 7))
    cs = detect_cs(seg, (13, 13, 7))
    assert np.array_equal(cs, want)
    asc = _cs_ref.close_dilate(want, 6, 2, 'ascending')
    desc = _cs_ref.close_dilate(want, 6, 2, 'descending')
    got = close_and_dilate_cs(cs, 6, 2)
    assert np.array_equal(got, asc)
    # the set of claimed voxels does not depend on the order; where orders disagree the smallest id holds the voxel
    assert np.array_equal(got != 0, desc != 0)
    diff = asc != desc
    assert diff.any() and np.array_equal(got[diff], np.minimum(asc[diff], desc[diff]))


def test_bad_stencil_rejected(gpu):
    from syconn_amd.extraction.find_object_properties import process_block_nonzero
    seg = np.ones((8, 8, 8), np.uint32)
    with pytest.raises(AssertionError):
        process_block_nonzero(seg, seg, (4, 3, 3))
    big = np.ones((40, 40, 40), np.uint32)
    with pytest.raises(ValueError):
        process_block_nonzero(big, big, (31, 31, 31))
