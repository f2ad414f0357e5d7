"""GPU: `syconn_amd/csrc/sd_objseg.hip` at the edges of its own structure -- id counts past the single-workgroup scan's round and
the floods' grids, LDS aggregation tables that overflow into global atomics, word passes past their launch cap, every z-shift
and pad of the bit-packed morphology, the distance output, the Gaussian at its largest window, and the argument checks --
everything compared bit for bit with oracle/objseg_ref.py.  tests/test_objseg_edges_cpu.py proves with the oracle and a model of
the launches (tests/_objseg_cases.py) that every case sits where it claims."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import _objseg_cases as K

pytestmark = pytest.mark.gpu

PITCH = (10, 10, 20)
EROSION = ['binary_erosion']


def _first_stage(vol, min_seed, **kw):
    from syconn_amd.extraction.object_extraction_steps import object_segmentation_first_stage
    return object_segmentation_first_stage(vol, 0.0, EROSION, kw.pop('scaling', PITCH), structure=K.Z_ELEMENT, return_mask=True,
                                           min_seed_vx=min_seed, return_markers=True, **kw)


def _assert_branch_equals(got, want):
    lab, mx, mask, mk = got[:4]
    assert np.array_equal(mask, want['mask']), 'tmp_data (the mask the flood is confined to) differs'
    assert np.array_equal(mk.astype(np.uint32), want['markers']), f"markers differ at {int((mk != want['markers']).sum())} voxels"
    assert lab.dtype == np.int32 and np.array_equal(lab, want['labels']), f"labels differ at {int((lab != want['labels']).sum())} voxels"
    assert mx == want['max_label']


# ---- A: table and id-count lattice -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lattice_oracle(min_seed):
    return K.watershed_oracle(K.table_lattice(), EROSION, K.Z_ELEMENT, min_seed, PITCH)


@pytest.mark.parametrize('sequential', [False, True], ids=['levelsync', 'sequential'])
@pytest.mark.parametrize('min_seed', [0, 2])
def test_gpu_table_lattice_equals_oracle(gpu, monkeypatch, min_seed, sequential):
    """22 640 seeds / 12 257 mask components / 4481 multi-marker components (one of them with thousands of markers): the scans carry
    across rounds, the seed filter relabels thousands of ids, the LDS tables of k_cc_head_labels / k_comp_markers / k_ws_init
    overflow, both floods loop over their grid -- in both forms of the flood"""
    if sequential:
        monkeypatch.setenv('SD_WS_SEQUENTIAL', '1')
    else:
        monkeypatch.delenv('SD_WS_SEQUENTIAL', raising=False)
    _assert_branch_equals(_first_stage(K.table_lattice(), min_seed), _lattice_oracle(min_seed))


@pytest.mark.parametrize('min_seed', [0, 2])
def test_gpu_table_lattice_with_distance_output(gpu, monkeypatch, min_seed):
    """asking for the distances switches the transform from the multi-marker components to the whole volume: the labels are the
    same, and the distances are the oracle's"""
    monkeypatch.delenv('SD_WS_SEQUENTIAL', raising=False)
    want = _lattice_oracle(min_seed)
    plain = _first_stage(K.table_lattice(), min_seed)
    withd = _first_stage(K.table_lattice(), min_seed, return_distance=True)
    assert len(withd) == 5 and np.array_equal(withd[0], plain[0]) and withd[1] == plain[1]
    _assert_branch_equals(withd, want)
    _assert_distance(withd[4], want)


# ---- B: flood lattice through marker_flood -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('sequential', [False, True], ids=['levelsync', 'sequential'])
@pytest.mark.parametrize('variant', ['differ', 'equal'])
@pytest.mark.parametrize('shape', [(12, 32, 96), (12, 32, 97)])
def test_gpu_flood_lattice_equals_oracle(gpu, monkeypatch, shape, variant, sequential):
    """more than 4096 three-voxel components `m o m` with arbitrary marker ids (the per-voxel queue path of k_ws_init with its table
    and list overflowing, more components than either flood has workgroups); the middle voxel goes to the higher marker, or on a tie
    to the first in raster order"""
    from oracle.objseg_ref import watershed_ref
    from syconn_amd.extraction.object_extraction_steps import marker_flood
    if sequential:
        monkeypatch.setenv('SD_WS_SEQUENTIAL', '1')
    else:
        monkeypatch.delenv('SD_WS_SEQUENTIAL', raising=False)
    d2, markers, mask = K.flood_lattice(shape, variant)
    want = watershed_ref(d2.astype(np.int64), markers, mask)
    got, mx = marker_flood(d2, markers, mask)
    assert np.array_equal(got, want), int((got != want).sum())
    assert mx == int(want.max()) == int(markers.max())


# ---- C: past the launch caps of the watershed branch --------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def thin_case():
    """the thin lattice and what the two runs share of its expectation (mask, squared distances), computed once"""
    from oracle.objseg_ref import distance_transform_ref
    vol = K.thin_lattice()
    _, d2 = distance_transform_ref(vol, np.asarray(PITCH, np.uint32))
    return vol, d2


@pytest.mark.parametrize('min_seed', [0, 2])
def test_gpu_thin_volume_past_the_word_launch_cap(gpu, thin_case, min_seed):
    """1460 x 1460 x 8: one mask word per row and more rows than one stride of 8192 x 256 words, so k_apply_map, k_seed_bits_sync,
    k_edt_z, k_comp_markers, k_ws_init and the labelling passes (with the voxel counts: min_seed_vx = 2) take a second stride;
    26 390 components keep both scans and the flood's grid loop busy"""
    from oracle.objseg_ref import seed_markers_ref, watershed_ref
    from syconn_amd import _lib as L
    vol, d2 = thin_case
    X, Y, Z = vol.shape
    need = L.load().sd_objseg_watershed_workspace_bytes(X, Y, Z, 0) + vol.size * (1 + 4 + 4 + 1) + (256 << 20)
    free = torch.cuda.mem_get_info(gpu)[0]
    if free < need:
        pytest.skip(f'{free >> 20} MiB of device memory free, the thin-volume case needs {need >> 20} MiB')
    tmp, markers = seed_markers_ref(vol, EROSION, K.Z_ELEMENT.astype(bool), min_seed)
    labels = watershed_ref(d2, markers, tmp)
    want = dict(mask=tmp, markers=markers, labels=labels, max_label=int(labels.max()))
    # (a fifth of the 26 390 cells are 4 + 4 pairs, whose four unmarked voxels the flood decides whatever min_seed_vx is)
    assert want['max_label'] > 10000 and int(((labels > 0) & (markers == 0)).sum()) > 20000
    _assert_branch_equals(_first_stage(vol, min_seed), want)


# ---- D: words, pads and wide elements in the morphology ------------------------------------------------------------------------------
def _morph_both_ways(mask, ops, struct):
    from syconn_amd.extraction.cs_extraction_steps import binary_morphology
    from syconn_amd.extraction.object_extraction_steps import object_segmentation_first_stage
    want, want_lab, want_n = K.morph_oracle(mask, ops, struct)
    got = binary_morphology(mask, ops, struct)
    assert np.array_equal(got, want), ('sd_binary_morphology', mask.shape, ops, int((got != want).sum()))
    lab, n, m = object_segmentation_first_stage(mask, 0.0, ops, structure=struct, return_mask=True)
    assert np.array_equal(m, want), ('sd_object_segmentation: mask', mask.shape, ops, int((m != want).sum()))
    assert n == want_n and np.array_equal(lab, want_lab), ('sd_object_segmentation: labels', mask.shape, ops)
    return int(want.sum()) != int(mask.sum())


@pytest.mark.parametrize('ops,iters,pad', K.OP_LISTS, ids=['-'.join(f'{o[7:9]}' for o in ops) for ops, _, _ in K.OP_LISTS])
@pytest.mark.parametrize('element', sorted(K.ELEMENTS))
def test_gpu_morphology_words_pads_and_wide_elements(gpu, element, ops, iters, pad):
    """elements with z-extents 5, 7 and 15 (every funnel shift from -7 to +7), an asymmetric one, 75 offsets; iterations 1, 2, 3, 5
    and pads 0, 1, 2, 3, 5; padded rows of 31, 32, 33, 64 and 65 bits; masks that fill words, rows and the whole volume"""
    struct = K.ELEMENTS[element]
    changed = 0
    for pz in K.PADDED_Z:
        shape = K.MORPH_XY + (pz - 2 * pad,)
        for kind in K.MASK_KINDS:
            changed += _morph_both_ways(K.morph_mask(kind, shape, pad, seed=pz), ops, struct)
    assert changed >= len(K.PADDED_Z)                             # (the operations did something)
    shape, p = K.THINNER_THAN_PAD[0]
    if pad == p:                                                  # a volume thinner than the pad: Z = 1 with P = 5
        for kind in ('blobs', 'full', 'six_faces'):
            _morph_both_ways(K.morph_mask(kind, shape, p, seed=1), ops, struct)


@pytest.mark.parametrize('element', ['1x1x15', 'asym3x3x5'])
def test_gpu_morphology_more_words_than_voxels(gpu, element):
    """Z = 1 under 16 dilations: rows of 33 padded bits = two mask words per voxel, the scan of the labelling is sized by words"""
    (shape, p), struct = K.THINNER_THAN_PAD[1], K.ELEMENTS[element]
    for kind in ('blobs', 'six_faces', 'full'):
        for ops in (['binary_dilation'] * p, ['binary_closing'] * p):
            _morph_both_ways(K.morph_mask(kind, shape, p, seed=2), ops, struct)


def test_gpu_erosion_lists_through_binary_morphology(gpu):
    """binary_erosion outside the watershed branch (sd_binary_morphology only), with the wide elements"""
    from oracle.objseg_ref import apply_morphological_operations_ref
    from syconn_amd.extraction.cs_extraction_steps import binary_morphology
    for element, struct in sorted(K.ELEMENTS.items()):
        for ops in (['binary_erosion'], ['binary_dilation'] * 3 + ['binary_erosion'] * 2):
            for pz in K.PADDED_Z:
                for kind in ('blobs', 'word_runs', 'full'):
                    mask = K.morph_mask(kind, K.MORPH_XY + (pz - 6,), 3, seed=pz)
                    want = apply_morphological_operations_ref(mask, ops, struct.astype(bool))
                    assert np.array_equal(binary_morphology(mask, ops, struct), want), (element, ops, pz, kind)


# ---- E: the distance output --------------------------------------------------------------------------------------------------------
def _assert_distance(dist, want):
    """float32 distances against the exact squared ones: the square rounds back to d2 where float32 resolves it, and the value is
    within one float32 ulp of the correctly rounded root (0 for a correctly rounded sqrtf, 1 ulp for any conforming one)"""
    d2 = want['d2']
    assert dist.dtype == np.float32 and dist.shape == d2.shape
    small = d2 < 2 ** 22
    assert np.array_equal(np.rint(dist.astype(np.float64) ** 2)[small], d2[small].astype(np.float64)), 'squared distances differ'
    ref = np.sqrt(d2.astype(np.float32))
    ulps = np.abs(dist.astype(np.float64) - ref.astype(np.float64)) / np.spacing(ref).astype(np.float64)
    print(f'distance output: max |dist - sqrt(d2)| = {float(ulps.max())} ulp over {int((d2 > 0).sum())} foreground voxels')
    assert float(ulps.max()) <= 1.0
    return float(ulps.max())


@pytest.mark.parametrize('pitch', K.PITCHES, ids=lambda p: 'x'.join(str(v) for v in p))
def test_gpu_distance_output_equals_oracle(gpu, pitch):
    """`return_distance` against distance_transform_ref: blobs, rows without background along z, a volume without any background
    (every voxel EDT_INF), a slab whose far end is 46 voxels from the only background plane, foreground on each face"""
    worst = 0.0
    for kind in K.DISTANCE_MASKS:
        mask = K.distance_mask(kind)
        want = K.watershed_oracle(mask, EROSION, K.Z_ELEMENT, 0, pitch)
        got = _first_stage(mask, 0, scaling=pitch, return_distance=True)
        _assert_branch_equals(got, want)
        worst = max(worst, _assert_distance(got[4], want))
        if kind == 'full':
            assert np.all(got[4] == np.sqrt(np.float32(K.kernel_constants()['EDT_INF'])))
    print(f'pitch {pitch}: worst {worst} ulp')


def test_gpu_distance_output_needs_the_watershed_branch(gpu):
    from syconn_amd.extraction.object_extraction_steps import object_segmentation_first_stage
    mask = K.distance_mask('blobs')
    with pytest.raises(ValueError):
        object_segmentation_first_stage(mask, 0.0, ['binary_opening'], return_distance=True)
    with pytest.raises(ValueError):
        object_segmentation_first_stage(mask, 0.0, [], return_distance=True)
    lab, mx, dist = object_segmentation_first_stage(mask, 0.0, EROSION, return_device=True, return_distance=True)
    assert dist.is_cuda and dist.dtype == torch.float32 and tuple(dist.shape) == mask.shape


# ---- F: Gaussian smoothing ---------------------------------------------------------------------------------------------------------
def _assert_gauss(vol, sigma, gpu):
    from oracle.objseg_ref import gaussian_smoothing_ref
    from syconn_amd.extraction.object_extraction_steps import gaussian_threshold
    thr = float(np.median(vol))
    mask, sm = gaussian_threshold(vol, sigma, thr, device=gpu, return_smoothed=True)
    ref = gaussian_smoothing_ref(vol, sigma)
    err = float(np.abs(sm - ref).max())
    print(f'{vol.shape} sigma {sigma}: max |smoothed - ref| = {err}')
    assert sm.dtype == np.float32 and err <= 6.2e-5                # (the bound tests/test_objseg.py states: two float32 ulps at 255)
    clear = np.abs(ref - thr) > 1e-3
    assert np.array_equal(mask[clear], (ref > thr).astype(np.uint8)[clear]) and set(np.unique(mask)) <= {0, 1}
    return mask


def test_gpu_gaussian_past_one_grid_stride(gpu):
    rng = np.random.default_rng(4)
    small = ndimage.gaussian_filter(rng.random(tuple(-(-v // 2) for v in K.GAUSS_BIG_SHAPE)), 1.0)
    vol = np.kron(small, np.ones((2, 2, 2)))[:K.GAUSS_BIG_SHAPE[0], :K.GAUSS_BIG_SHAPE[1], :K.GAUSS_BIG_SHAPE[2]]
    vol = np.ascontiguousarray(((vol - vol.min()) / (vol.max() - vol.min()) * 255).astype(np.uint8))
    vol[-1, -1, -5:] = (255, 0, 255, 0, 255)                       # the last voxels of the last stride
    mask = _assert_gauss(vol, (0.8, 1.1, 0.6), gpu)
    assert 0.05 < mask.mean() < 0.95


def test_gpu_gaussian_largest_window_and_beyond(gpu):
    """sigma = 21.2: radius 64 = GAUSS_MAX_R on an axis of 9 voxels (mirrored many times); sigma = 21.5: radius 65 is refused"""
    from syconn_amd.extraction.object_extraction_steps import gaussian_threshold
    rng = np.random.default_rng(6)
    vol = rng.integers(0, 256, (9, 14, 21), dtype=np.uint8)
    _assert_gauss(vol, (21.2, 0.0, 0.0), gpu)
    _assert_gauss(np.ascontiguousarray(vol.transpose(1, 2, 0)), (0.0, 1.0, 21.2), gpu)
    with pytest.raises(ValueError, match='sigma too large'):
        gaussian_threshold(vol, (21.5, 0.0, 0.0), 100.0, device=gpu)
    _assert_gauss(vol, (1.0, 21.2, 0.5), gpu)                      # (a valid call after the refused one)


# ---- G: error returns --------------------------------------------------------------------------------------------------------------
class _Calls:
    """small valid device buffers and the three entry points with keyword overrides; every call returns the library's code"""

    def __init__(self, gpu, shape=(6, 5, 40)):
        from syconn_amd import _lib as L
        self.L, self.lib = L, L.load()
        L.check(self.lib.sd_init(gpu.index or 0), 'sd_init')
        self.shape = shape
        self.vol = K.morph_mask('blobs', shape, 0, seed=3)
        n = int(np.prod(shape))
        self.prob = torch.from_numpy(self.vol).to(gpu)
        self.labels = torch.zeros(n, dtype=torch.int32, device=gpu)
        self.maxl = torch.zeros(1, dtype=torch.int32, device=gpu)
        self.mask = torch.zeros(n, dtype=torch.uint8, device=gpu)
        self.ws_bytes = 4 * int(self.lib.sd_objseg_watershed_workspace_bytes(*shape, 1))      # (room for the other small shapes)
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=gpu)
        self.stream = torch.cuda.current_stream(gpu).cuda_stream

    @staticmethod
    def _ints(v):
        return (C.c_int32 * max(len(v), 1))(*v)

    def _common(self, kw):
        L = self.L
        shape = kw.get('shape', self.shape)
        st = np.ascontiguousarray(kw.get('struct', np.ones((3, 3, 3), np.uint8))).astype(np.uint8)
        ops, its = kw.get('ops', [L.SD_MOP_CLOSING]), kw.get('iterations', [1])
        return shape, st, ops, its

    def plain(self, **kw):
        shape, st, ops, its = self._common(kw)
        ws_bytes = kw.get('ws_bytes', self.ws_bytes)
        return self.lib.sd_object_segmentation(self.prob.data_ptr(), *shape, kw.get('threshold', 0.0), self._ints(ops), self._ints(its), len(ops),
                                               st.ctypes.data_as(C.c_void_p), *st.shape, self.labels.data_ptr(), self.maxl.data_ptr(),
                                               self.mask.data_ptr(), self.ws.data_ptr(), ws_bytes, self.stream)

    def morph(self, **kw):
        shape, st, ops, its = self._common(kw)
        ws_bytes = kw.get('ws_bytes', self.ws_bytes)
        return self.lib.sd_binary_morphology(self.prob.data_ptr(), *shape, kw.get('threshold', 0.0), self._ints(ops), self._ints(its), len(ops),
                                             st.ctypes.data_as(C.c_void_p), *st.shape, self.mask.data_ptr(), self.ws.data_ptr(), ws_bytes,
                                             self.stream)

    def watershed(self, **kw):
        L = self.L
        shape, st, ops, its = self._common(kw)
        sops, sits = kw.get('seed_ops', [L.SD_MOP_EROSION]), kw.get('seed_iterations', [1])
        pitch = (C.c_int32 * 3)(*kw.get('pitch', PITCH))
        return self.lib.sd_object_segmentation_watershed(
            self.prob.data_ptr(), *shape, kw.get('threshold', 0.0), self._ints(ops), self._ints(its), len(ops), self._ints(sops),
            self._ints(sits), len(sops), st.ctypes.data_as(C.c_void_p), *st.shape, kw.get('min_seed_vx', 0), pitch, self.labels.data_ptr(),
            self.maxl.data_ptr(), None, None, self.mask.data_ptr(), self.ws.data_ptr(), kw.get('ws_bytes', self.ws_bytes), self.stream)

    def refused(self, fn, **kw):
        """the call returns a negative code and leaves a message; the same entry point then accepts a valid call"""
        rc = fn(**kw)
        msg = self.lib.sd_last_error()
        assert rc < 0 and msg and len(msg.strip()) > 0, (fn.__name__, kw, rc, msg)
        assert fn() == 0, (fn.__name__, 'valid call after', kw, self.lib.sd_last_error())
        torch.cuda.synchronize()
        return rc, msg.decode(errors='replace')


def test_gpu_error_returns_before_any_launch(gpu):
    c = _Calls(gpu)
    L = c.L
    entry = (c.plain, c.morph, c.watershed)
    for fn in entry:
        for it in (0, 65):
            c.refused(fn, iterations=[it])
        for ext in (2, 17):
            for ax in range(3):
                sh = [3, 3, 3]
                sh[ax] = ext
                c.refused(fn, struct=np.ones(sh, np.uint8))
        c.refused(fn, struct=np.zeros((3, 3, 3), np.uint8))
        assert 'empty' in c.refused(fn, struct=np.zeros((5, 5, 3), np.uint8))[1]
        assert 'too large' in c.refused(fn, struct=np.ones((15, 15, 1), np.uint8))[1]
        assert 'NaN' in c.refused(fn, threshold=float('nan'))[1]
        assert c.refused(fn, shape=K.TOO_MANY_VOXELS)[0] == L.SD_ERR_INVALID           # (returns before it touches memory)
        assert fn(struct=np.ones((15, 1, 1), np.uint8)) == 0                            # the largest extent is accepted
    for it in (0, 65):
        c.refused(c.watershed, seed_iterations=[it])
    for fn, exact in ((c.plain, c.lib.sd_objseg_workspace_bytes), (c.morph, c.lib.sd_objseg_workspace_bytes),
                      (c.watershed, c.lib.sd_objseg_watershed_workspace_bytes)):
        need = int(exact(*c.shape, 1))
        assert c.refused(fn, ws_bytes=need - 1)[0] == L.SD_ERR_NOMEM
        assert fn(ws_bytes=need) == 0
    for bad in ([L.SD_MOP_OPENING], [L.SD_MOP_CLOSING, L.SD_MOP_EROSION], [L.SD_MOP_DILATION]):
        assert 'erosion' in c.refused(c.watershed, seed_ops=bad, seed_iterations=[1] * len(bad))[1]
    assert 'watershed' in c.refused(c.plain, ops=[L.SD_MOP_EROSION])[1]                 # the plain entry point refuses erosions
    c.refused(c.plain, ops=[7])
    # pitch x extent: 18001 refused, exactly 18000 accepted (on every axis)
    (sh1, p1), (sh0, p0) = K.PITCH_REJECTED, K.PITCH_ACCEPTED
    assert int(np.prod(sh1)) <= int(np.prod(c.shape)) and int(np.prod(sh0)) <= int(np.prod(c.shape))
    for ax in range(3):
        bad_shape, ok_shape = tuple(np.roll(sh1, ax).tolist()), tuple(np.roll(sh0, ax).tolist())
        assert int(c.lib.sd_objseg_watershed_workspace_bytes(*ok_shape, 1)) <= c.ws_bytes
        assert 'pitch' in c.refused(c.watershed, shape=bad_shape, pitch=tuple(np.roll(p1, ax).tolist()))[1]
        assert c.watershed(shape=ok_shape, pitch=tuple(np.roll(p0, ax).tolist())) == 0
    c.refused(c.watershed, pitch=(10, 0, 20))
    # sd_marker_flood and sd_gaussian_threshold: 2^31 voxels with dummy non-null pointers, short workspaces
    p = c.prob.data_ptr()
    assert c.lib.sd_marker_flood(p, p, p, *K.TOO_MANY_VOXELS, p, p, p, 1 << 40, c.stream) == L.SD_ERR_INVALID and c.lib.sd_last_error()
    need = int(c.lib.sd_objseg_watershed_workspace_bytes(*c.shape, 0))
    assert c.lib.sd_marker_flood(c.labels.data_ptr(), c.labels.data_ptr(), p, *c.shape, c.labels.data_ptr(), c.maxl.data_ptr(),
                                 c.ws.data_ptr(), need - 1, c.stream) == L.SD_ERR_NOMEM
    sg = (C.c_double * 3)(1.0, 1.0, 1.0)
    assert c.lib.sd_gaussian_threshold(p, *K.TOO_MANY_VOXELS, sg, 1.0, p, None, p, 1 << 40, c.stream) == L.SD_ERR_INVALID
    assert c.lib.sd_gaussian_threshold(p, *c.shape, sg, 1.0, c.mask.data_ptr(), None, c.ws.data_ptr(),
                                       int(c.lib.sd_gauss_workspace_bytes(*c.shape)) - 1, c.stream) == L.SD_ERR_NOMEM
    # after all of it the buffers still compute the right thing
    assert c.plain() == 0
    torch.cuda.synchronize()
    out, lab, n = K.morph_oracle(c.vol, ['binary_closing'], np.ones((3, 3, 3), np.uint8))
    assert int(c.maxl.item()) == n and np.array_equal(c.labels.cpu().numpy().reshape(c.shape), lab)
    assert np.array_equal(c.mask.cpu().numpy().reshape(c.shape), out)
