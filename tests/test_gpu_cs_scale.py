"""GPU: one production-shaped cell volume past every launch cap of the contact-site kernels, through the device steps of the
per-chunk worker on arrays (boundaries -> partner stencil (13, 13, 7) -> closing n = 6, dilation k = 2 -> syn statistics of the core),
bit-exact against the numpy restatement.  Every grid-stride loop of csrc/sd_contacts.hip and csrc/sd_cs_syntype.hip takes a second
trip here, the exact-count kernel finds overflow markers in its first and in a later trip, and the prefix sum of k_cst_offsets
carries across blocks of 256 sites.  The fixture asserts these conditions on the input, so the test cannot shrink below its purpose."""
import os
import sys

import numpy as np
import pytest
import scipy.ndimage
import scipy.spatial

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cs_ref  # noqa: E402
import _cs_syntype_ref as R  # noqa: E402
from test_gpu_cs_edges import assert_same_volume  # noqa: E402
from test_gpu_cs_syntype import same  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE, SEEDS, STENCIL, N_CLOSE, K_DILATE = (300, 280, 110), 900, (13, 13, 7), 6, 2
PATCH = (24, 24, 14)                                   # "salt": every voxel its own id
PATCH_AT = ((0, 100, 40), (276, 256, 96))              # within the first 18 output x-planes; the high corner
OFFSET = (1000, 2000, 300)
# launch caps of the two .hip files
GRID_STRIDE = 256 * 64 * 256                           # grid_of(): k_seg_boundaries, k_claim_init / _finish, k_box_dt_pass, k_box_claim
EXACT_TRIP = 2048 * 256                                # k_contact_partners_exact: outputs per trip
SCAN_STRIDE = 8192 * 4 * 64                            # k_cst_scan: window voxels per trip
OFFSETS_BLOCK = 256                                    # k_cst_offsets: sites per block of its running carry
CP_SLOTS = 8


def _volume():
    rng = np.random.default_rng(2024)
    half = tuple(s // 2 for s in SHAPE)
    pts = np.stack([rng.integers(0, s, SEEDS) for s in half], 1)
    ids = rng.choice(np.arange(2 ** 20, 2 ** 32 - 1, dtype=np.uint64), SEEDS, replace=False).astype(np.uint32)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in half], indexing='ij'), -1).reshape(-1, 3)
    near = scipy.spatial.cKDTree(pts).query(grid)[1]
    seg = ids[near].reshape(half).repeat(2, 0).repeat(2, 1).repeat(2, 2)
    n = int(np.prod(PATCH))
    for q, (x, y, z) in enumerate(PATCH_AT):
        seg[x:x + PATCH[0], y:y + PATCH[1], z:z + PATCH[2]] = (1 + q * n + rng.permutation(n)).reshape(PATCH).astype(np.uint32)
    seg[rng.random(SHAPE) < 0.01] = 0
    return seg


def _masks(shape):
    """syn: blobs covering about a fifth of the volume; type masks: blocks of 0, 1, 2, 255."""
    rng = np.random.default_rng(7)
    half = tuple(-(-s // 2) for s in shape)
    up = lambda a: a.repeat(2, 0).repeat(2, 1).repeat(2, 2)[:shape[0], :shape[1], :shape[2]]
    noise = scipy.ndimage.gaussian_filter(rng.random(half), 2.0)
    syn = up((noise > np.quantile(noise, 0.8)).astype(np.uint8)) * rng.choice(np.array([1, 3, 255], np.uint8), shape)
    vals = np.array([0, 1, 2, 255], np.uint8)
    asym, sym = (np.ascontiguousarray(up(vals[rng.integers(0, 4, half)])) for _ in range(2))
    return np.ascontiguousarray(syn), asym, sym


def _overflow_rasters(seg, edges, out_shape):
    """Raster indices of flagged outputs inside the salt patches whose window holds more than CP_SLOTS distinct partners."""
    h = [s // 2 for s in STENCIL]
    found = []
    for x0, y0, z0 in PATCH_AT:
        for dx, dy, dz in ((2, 3, 1), (7, 9, 5), (10, 10, 6)):
            x, y, z = x0 + dx, y0 + dy, z0 + dz                   # output index = window origin; the window lies in the patch
            if x + STENCIL[0] > SHAPE[0] or y + STENCIL[1] > SHAPE[1] or z + STENCIL[2] > SHAPE[2]:
                continue
            c = seg[x + h[0], y + h[1], z + h[2]]
            w = np.unique(seg[x:x + STENCIL[0], y:y + STENCIL[1], z:z + STENCIL[2]])
            if edges[x + h[0], y + h[1], z + h[2]] and len(w[(w != 0) & (w != c)]) > CP_SLOTS:
                found.append(int(np.ravel_multi_index((x, y, z), out_shape)))
    return found


@pytest.fixture(scope='module')
def ref():
    seg = _volume()
    edges = _cs_ref.seg_boundaries(seg)
    c0 = _cs_ref.contact_partners(edges, seg, STENCIL)
    closed = _cs_ref.close_dilate(c0, N_CLOSE, K_DILATE)
    syn, asym, sym = _masks(c0.shape)
    core = tuple(s - 2 * N_CLOSE for s in c0.shape)
    c = (slice(N_CLOSE, -N_CLOSE),) * 3
    dicts = R.extract_cs_syntype(closed[c], syn[c], asym[c], sym[c], OFFSET)
    # ---- conditions on the input (from the reference, not from the device): every loop of the table takes a second trip
    assert seg.size > GRID_STRIDE and c0.size > GRID_STRIDE
    ovf = _overflow_rasters(seg, edges, c0.shape)
    assert any(i < EXACT_TRIP for i in ovf) and any(i >= EXACT_TRIP for i in ovf), ovf
    n_sites = len(dicts[0][0])
    assert n_sites > OFFSETS_BLOCK and n_sites % OFFSETS_BLOCK != 0, n_sites
    assert len(dicts[1][0]) > OFFSETS_BLOCK and 0 < len(dicts[1][0]) < n_sites           # sites without syn voxels among them
    lab, inv = np.unique(c0.reshape(-1), return_inverse=True)
    box_voxels = 0
    for k, sl in enumerate(scipy.ndimage.find_objects(inv.reshape(c0.shape) + 1)):
        if lab[k]:
            box_voxels += int(np.prod([min(s.stop + N_CLOSE, n) - max(s.start - N_CLOSE, 0) for s, n in zip(sl, c0.shape)]))
    assert box_voxels > GRID_STRIDE                                                         # one batch under the default budget
    assert int(np.prod(core)) > SCAN_STRIDE
    return dict(seg=seg, edges=edges, c0=c0, closed=closed, syn=syn, asym=asym, sym=sym, core=core, crop=c, dicts=dicts,
                n_c0_sites=len(lab) - 1, box_voxels=box_voxels)


def _chain(gpu, ref, ws_budget=None):
    """Steps 2-5 of the worker on device tensors -> host copies."""
    import torch
    from syconn_amd.extraction.cs_extraction_steps import plan_sites, run_sites
    from syconn_amd.extraction.find_object_properties import CsSyntypeScan, cs_syntype_dicts, detect_cs, detect_seg_boundaries
    seg_d = torch.from_numpy(ref['seg'].view(np.int32)).to(gpu)
    edges = detect_seg_boundaries(seg_d, return_device=True).cpu().numpy()
    c0_d = detect_cs(seg_d, STENCIL, return_device=True, device=gpu)
    plan = plan_sites(c0_d, N_CLOSE, gpu) if ws_budget is None else plan_sites(c0_d, N_CLOSE, gpu, ws_budget)
    closed_d = torch.empty_like(c0_d)
    ws = torch.empty(max(plan.ws_bytes, 1), dtype=torch.uint8, device=gpu)
    run_sites(c0_d, plan, N_CLOSE, K_DILATE, closed_d, ws)
    del ws
    res = CsSyntypeScan(gpu).run(closed_d, ref['syn'], ref['asym'], ref['sym'], offset=OFFSET, origin=(N_CLOSE,) * 3,
                                 extent=ref['core'], want_cores=True)
    rec, vox = res.host()
    return dict(edges=edges, c0=c0_d.cpu().numpy().view(np.uint64), closed=closed_d.cpu().numpy().view(np.uint64),
                cs_core=res.cs_core.cpu().numpy().view(np.uint64), syn_core=res.syn_core.cpu().numpy().view(np.uint64),
                rec=rec, vox=vox, dicts=cs_syntype_dicts(rec, vox), n_batches=len(plan.batches), box_voxels=plan.box_voxels,
                n_sites=len(plan.ids))


@pytest.fixture(scope='module')
def dev(gpu, ref):
    return _chain(gpu, ref)


def test_scale_boundaries_and_contacts(ref, dev):
    assert_same_volume(dev['edges'] != 0, ref['edges'], 'boundaries')
    assert_same_volume(dev['c0'], ref['c0'], 'contacts (13, 13, 7)', (8, 8, 16))


def test_scale_closing(ref, dev):
    # one batch of more box voxels than one grid stride of k_box_dt_pass / k_box_claim
    assert dev['n_batches'] == 1 and dev['box_voxels'] == ref['box_voxels'] > GRID_STRIDE and dev['n_sites'] == ref['n_c0_sites']
    assert_same_volume(dev['closed'], ref['closed'], f'closing n={N_CLOSE} k={K_DILATE}')


def test_scale_cores_and_statistics(ref, dev):
    c = ref['crop']
    assert_same_volume(dev['cs_core'], ref['closed'][c], 'cs core')
    assert_same_volume(dev['syn_core'], np.where(ref['syn'][c] != 0, ref['closed'][c], 0).astype(np.uint64), 'syn core')
    got, want = dev['dicts'], ref['dicts']
    assert list(got[0][0]) == list(want[0][0])
    for part, name in ((0, 'cs'), (1, 'syn')):                     # name the first site and block of 256 that differ
        for q, what in enumerate(('rep_coord', 'bounding box', 'size')):
            for i, k in enumerate(want[part][q]):
                assert got[part][q].get(k) == want[part][q][k], (name, what, k, f'site {i}, block {i // OFFSETS_BLOCK} of k_cst_offsets')
    for i, k in enumerate(want[4]):
        assert got[4].get(k) == want[4][k], ('syn voxels', k, f'syn site {i}')
    same(got, want, 'scale')


def test_scale_second_run_is_bit_identical(gpu, ref, dev):
    again = _chain(gpu, ref)
    for k in ('edges', 'c0', 'closed', 'cs_core', 'syn_core', 'rec', 'vox'):
        assert_same_volume(again[k], dev[k], f'second run: {k}')


def test_scale_closing_in_batches(gpu, ref, dev):
    import torch
    from syconn_amd.extraction.cs_extraction_steps import close_and_dilate_cs, plan_sites
    budget = ref['box_voxels'] // 5
    assert budget > GRID_STRIDE                                    # every batch still goes round the grid stride
    plan = plan_sites(torch.from_numpy(ref['c0'].view(np.int64)).to(gpu), N_CLOSE, gpu, budget)
    assert len(plan.batches) >= 4
    got = close_and_dilate_cs(ref['c0'], N_CLOSE, K_DILATE, ws_budget=budget)
    assert_same_volume(got, ref['closed'], f'closing in {len(plan.batches)} batches')
