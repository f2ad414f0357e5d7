"""GPU: the contact-site kernels (csrc/sd_contacts.hip, csrc/sd_cs_syntype.hip) at the edges of their own structure, bit-exact
against golden g17 (the reference's own code) and the numpy restatement: a partner table that is exactly full (8 ids) or one
past it (9), outputs around the 8 x 8 x 16 tile, a stencil axis of 1, the largest stencils the entry point admits, batches of
sites that split between overlapping boxes, runs of the syn scan at lane 0, at z == 0 and across waves, and a table beyond one
grid stride of its init / compact kernels."""
import os
import sys

import numpy as np
import pytest
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cs_ref  # noqa: E402
import _cs_syntype_ref as R  # noqa: E402
from test_cs_edges_cpu import G17, brute_partners, stencil_case  # noqa: E402
from test_gpu_cs_syntype import same  # noqa: E402

pytestmark = pytest.mark.gpu

CP_TILE = (8, 8, 16)                  # CP_TX, CP_TY, CP_TZ of csrc/sd_contacts.hip


@pytest.fixture(scope='module')
def g17():
    return dict(np.load(G17))


def assert_same_volume(got, want, what, tile=None):
    """np.array_equal with the first differing raster index (and its tile / 524 288-output trip of the exact kernel) in the message."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if np.array_equal(got, want):
        return
    i = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
    pos = tuple(int(v) for v in np.unravel_index(i, want.shape))
    msg = (f'{what}: {int((got != want).sum())} of {want.size} differ; first at raster index {i} = {pos}: got {int(got[pos]):#x}, '
           f'want {int(want[pos]):#x}; trip {i // (2048 * 256)} of the exact kernel')
    if tile:
        msg += f'; tile {tuple(p // t for p, t in zip(pos, tile))}, in-tile {tuple(p % t for p, t in zip(pos, tile))}'
    raise AssertionError(msg)


def pool_volume(rng, shape, p):
    """Every voxel one of `p` ids (2^32 - 1 and an id >= 2^31 among them), 10 % background."""
    ids = np.concatenate([[2 ** 32 - 1, 2 ** 31 + 3], rng.choice(np.arange(1, 5000), p - 2, replace=False)]).astype(np.uint32)
    vol = ids[rng.integers(0, p, shape)]
    vol[rng.random(shape) < 0.1] = 0
    return vol


# ---- golden g17 -----------------------------------------------------------------------------------------------------------------
def test_g17_boundaries_and_partners(gpu, g17):
    import torch
    from syconn_amd.extraction.find_object_properties import detect_cs, detect_seg_boundaries, process_block_nonzero
    for name in g17['stencil_cases']:
        seg, edges, st, want = stencil_case(g17, name)
        b = detect_seg_boundaries(seg)
        assert b.dtype == np.bool_
        assert_same_volume(b, edges != 0, f'{name} boundaries')
        assert_same_volume(process_block_nonzero(edges.astype(np.uint32), seg, st), want, f'{name} process_block_nonzero', CP_TILE)
        assert_same_volume(detect_cs(seg, st), want, f'{name} detect_cs', CP_TILE)
        out = detect_cs(torch.from_numpy(seg.view(np.int32)).to(gpu), st, return_device=True)
        assert out.is_cuda and out.dtype == torch.int64
        assert_same_volume(out.cpu().numpy().view(np.uint64), want, f'{name} detect_cs (device in / out)', CP_TILE)


def test_g17_closing(gpu, g17):
    from syconn_amd.extraction.cs_extraction_steps import close_and_dilate_cs
    c0 = g17['cl_in']
    for n, k in g17['close_nk'].tolist():
        want = g17[f'cl_{n}_{k}_out']
        assert_same_volume(close_and_dilate_cs(c0, n, k), want, f'closing n={n} k={k}')
        assert_same_volume(close_and_dilate_cs(c0, n, k, ws_budget=1), want, f'closing n={n} k={k}, smallest budget')


# ---- tile edges -----------------------------------------------------------------------------------------------------------------
# output extents from {1, 7, 8, 9, 16, 17}: one short of, equal to and one past the tile along every axis, and a single output
TILE_SWEEP = [
    ((3, 3, 3), (8, 8, 16)), ((3, 3, 3), (9, 7, 17)), ((3, 3, 3), (7, 9, 1)), ((3, 3, 3), (17, 16, 7)),
    ((13, 13, 7), (1, 1, 1)), ((13, 13, 7), (9, 8, 17)), ((13, 13, 7), (7, 17, 16)), ((13, 13, 7), (16, 1, 9)),
    ((13, 3, 1), (8, 9, 16)), ((13, 3, 1), (17, 7, 17)), ((13, 3, 1), (1, 16, 8)),
    ((1, 13, 7), (9, 9, 9)), ((1, 13, 7), (16, 8, 1)), ((1, 13, 7), (7, 16, 17)),
]


@pytest.mark.parametrize('st,ext', TILE_SWEEP, ids=lambda v: 'x'.join(str(i) for i in v))
def test_tile_edges_against_restatement(gpu, st, ext):
    """A pool of 10 ids: windows of 8 partners (answered from the registers) and of 9 (marked, answered by the exact kernel) lie in
    the same workgroup's tile."""
    from syconn_amd.extraction.find_object_properties import detect_cs
    rng = np.random.default_rng(sum(st) * 1000 + sum(e * 31 ** i for i, e in enumerate(ext)))
    want = np.zeros(ext, np.uint64)
    while not want.any():                                          # (a single output may fall on background: draw again)
        seg = pool_volume(rng, tuple(e + s - 1 for e, s in zip(ext, st)), 10)
        edges = _cs_ref.seg_boundaries(seg)
        want = _cs_ref.contact_partners(edges, seg, st)
    assert want.shape == ext
    if np.prod(ext) * np.prod(st) <= 2_000_000:                    # the restatement itself against the count per window
        res, n_part, _ = brute_partners(edges, seg, st)
        assert np.array_equal(res, want) and n_part.max() == 9
    assert_same_volume(detect_cs(seg, st), want, f'stencil {st} outputs {ext}', CP_TILE)


def _small_voronoi(shape, n, seed):
    rng = np.random.default_rng(seed)
    lab = np.zeros(shape, np.uint32)
    lab[tuple(rng.integers(0, s, n) for s in shape)] = rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    _, ind = scipy.ndimage.distance_transform_edt(lab == 0, return_indices=True)
    seg = lab[tuple(ind)]
    seg[rng.random(shape) < 0.02] = 0
    return seg


@pytest.mark.parametrize('st', [(15, 15, 15), (19, 19, 9)], ids=lambda v: 'x'.join(str(i) for i in v))
def test_largest_admitted_stencils(gpu, st):
    """(15, 15, 15): a 3 375-voxel window, near CP_WIN_MAX = 4 096.  (19, 19, 9): 26 x 26 x 24 x 4 = 64 896 B of dynamic LDS, just
    under CP_LDS_MAX = 65 536, on top of the kernel's 2 056 B of static LDS (the compiler's resource report); the exact kernel
    declares 19 460 B.  A gfx950 workgroup may declare 163 840 B, so every stencil the entry point admits fits."""
    from syconn_amd.extraction.find_object_properties import detect_cs, process_block_nonzero
    lds = np.prod([t + s - 1 for t, s in zip(CP_TILE, st)]) * 4
    assert lds <= 65536 and np.prod(st) <= 4096 and lds + 2056 <= 163840
    rng = np.random.default_rng(st[0])
    shape = tuple(s + e - 1 for s, e in zip(st, (9, 10, 17)))
    salt = rng.choice(np.arange(1, 2 ** 32, 2 ** 22, dtype=np.uint64), 400).astype(np.uint32)[rng.integers(0, 400, shape)]
    salt[rng.random(shape) < 0.1] = 0
    for name, seg in (('salt', salt), ('voronoi', _small_voronoi(shape, 40, st[1]))):
        edges = _cs_ref.seg_boundaries(seg)
        want = _cs_ref.contact_partners(edges, seg, st)
        assert (want != 0).sum() > 50, name
        assert_same_volume(detect_cs(seg, st), want, f'{name} {st}', CP_TILE)
    # one step further along an axis is refused, not launched
    for big in ((21, 19, 9), (17, 17, 15)):
        v = np.ones(tuple(s + 2 for s in big), np.uint32)
        with pytest.raises(ValueError):
            process_block_nonzero(v, v, big)


# ---- batches of sites -----------------------------------------------------------------------------------------------------------
def test_closing_batches_do_not_change_the_result(gpu):
    import torch
    from syconn_amd.extraction.cs_extraction_steps import close_and_dilate_cs, plan_sites
    from test_gpu_contact_sites import _cells
    seg = _cells((72, 64, 40), 70, 5)
    c0 = _cs_ref.contact_partners(_cs_ref.seg_boundaries(seg), seg, (7, 7, 3))
    n, k = 4, 2
    want = _cs_ref.close_dilate(c0, n, k)
    c0_d = torch.from_numpy(c0.view(np.int64)).to(gpu)
    full = plan_sites(c0_d, n, gpu)
    assert len(full.batches) == 1 and 200 < len(full.ids) < 2000
    tab = full.batches[0][0].cpu().numpy()
    vol = np.prod(tab[:, 4:7], axis=1)
    # plan_sites raises a budget below the largest box to that box (one box is never split), so 1 and the median box volume
    # give the same plan: the finest there is.  Twice the largest box lies between it and the third of the sum.
    budgets = [1, int(np.median(vol)), 2 * int(vol.max()), int(vol.sum() // 3), None]
    counts, split_between_overlapping = [], False
    for b in budgets:
        plan = plan_sites(c0_d, n, gpu) if b is None else plan_sites(c0_d, n, gpu, ws_budget=b)
        counts.append(len(plan.batches))
        assert sum(nb for _, nb, _ in plan.batches) == len(full.ids) and plan.box_voxels == full.box_voxels
        assert max(tot for _, _, tot in plan.batches) <= max(b or 1 << 28, int(vol.max()))
        ends = np.cumsum([nb for _, nb, _ in plan.batches])[:-1]
        for e in ends:                                             # the last site of a batch and the first of the next
            lo_a, hi_a, lo_b, hi_b = tab[e - 1, 1:4], tab[e - 1, 1:4] + tab[e - 1, 4:7], tab[e, 1:4], tab[e, 1:4] + tab[e, 4:7]
            split_between_overlapping |= bool(np.all(lo_a < hi_b) and np.all(lo_b < hi_a))
        got = close_and_dilate_cs(c0, n, k) if b is None else close_and_dilate_cs(c0, n, k, ws_budget=b)
        assert_same_volume(got, want, f'ws_budget={b} ({len(plan.batches)} batches)')
    assert counts[0] == counts[1] > counts[2] > counts[3] > counts[4] == 1 and counts[3] in (3, 4), counts
    assert split_between_overlapping


# ---- syn statistics -------------------------------------------------------------------------------------------------------------
def _syntype_volume(nz, dtype, seed):
    """A volume with a (9, 8, nz) window at origin (2, 1, 3): runs of ~5 voxels along z, some z-rows of one id (a run as long as
    the row: it crosses waves for nz > 64 and, for nz != 64, starts away from lane 0), masks drawn from {0, 1, 2, 255}."""
    rng = np.random.default_rng(seed)
    shape = (12, 10, nz + 4)
    top = 2 ** 64 if dtype == np.uint64 else 2 ** 32
    ids = np.array([0, 0, 3, 4, 5, 900, 2 ** 31 + 1, top // 2 + 7, top - 2, top - 1], dtype)
    cs = ids[rng.integers(0, len(ids), (shape[0], shape[1], -(-shape[2] // 5)))].repeat(5, 2)[:, :, :shape[2]].copy()
    cs[3, 2:6, :] = ids[3:7, None]                                # whole z-rows of one id
    cs[4, 2, :] = ids[4]
    cs[4, 3, :] = ids[4]                                           # the same id in consecutive rows: the run ends at z == 0
    vals = np.array([0, 1, 2, 255], np.uint8)
    syn, asym, sym = (vals[rng.integers(0, 4, shape)] for _ in range(3))
    syn[cs == ids[5]] = 0                                          # a site without syn voxels between two with many
    return cs, syn, asym, sym, int(ids[4]), int(ids[5]), int(ids[6])


@pytest.mark.parametrize('dtype', [np.uint32, np.uint64], ids=['u32', 'u64'])
@pytest.mark.parametrize('nz', [1, 63, 64, 65, 130])
def test_syntype_window_depths(gpu, nz, dtype):
    from syconn_amd.extraction.find_object_properties import cs_syntype, cs_syntype_dicts
    cs, syn, asym, sym, lo_id, mid_id, hi_id = _syntype_volume(nz, dtype, 100 + nz)
    org, ext = (2, 1, 3), (9, 8, nz)
    crop = tuple(slice(o, o + e) for o, e in zip(org, ext))
    want = R.extract_cs_syntype(cs[crop], syn[crop], asym[crop], sym[crop], (11, 22, 33))
    assert mid_id in want[0][0] and mid_id not in want[1][0] and lo_id in want[1][0] and hi_id in want[1][0]
    assert lo_id < mid_id < hi_id and max(want[0][0]) >= (2 ** 63 if dtype == np.uint64 else 2 ** 31)
    assert {int(v) for v in np.unique(asym[crop])} == {0, 1, 2, 255} or nz == 1
    # only "== 1" counts: fewer typed voxels than syn voxels with a non-zero type
    n_one = int(((syn[crop] != 0) & (cs[crop] != 0) & (asym[crop] == 1)).sum())
    assert sum(want[2].values()) == n_one and n_one < int(((syn[crop] != 0) & (cs[crop] != 0) & (asym[crop] != 0)).sum())
    res = cs_syntype(cs, syn, asym, sym, offset=(11, 22, 33), origin=org, extent=ext, want_cores=True)
    same(cs_syntype_dicts(*res.host()), want, f'nz={nz} {np.dtype(dtype).name}')
    assert_same_volume(res.cs_core.cpu().numpy().view(dtype), cs[crop], f'cs core nz={nz}')
    assert_same_volume(res.syn_core.cpu().numpy().view(dtype), np.where(syn[crop] != 0, cs[crop], 0).astype(dtype), f'syn core nz={nz}')


def test_syntype_large_table(gpu):
    """cap = 2^21 slots (218 MB): k_cst_init and k_cst_compact go round their 4 096 x 256 grid stride twice."""
    from syconn_amd.extraction.find_object_properties import CsSyntypeScan, cs_syntype_dicts
    cs, syn, asym, sym, *_ = _syntype_volume(65, np.uint64, 7)
    sc = CsSyntypeScan(gpu, cap=2 ** 21)
    assert sc.cap == 2 ** 21 > 4096 * 256
    want = R.extract_cs_syntype(cs, syn, asym, sym, (0, 0, 0))
    for _ in range(2):                                             # the table is reused: it must be cleared in full
        same(cs_syntype_dicts(*sc.run(cs, syn, asym, sym).host()), want, 'cap 2^21')
    assert sc.passes == 1 and sc.cap == 2 ** 21
