"""Glia probabilities from supervoxel views on the device: the centre component (``sd_views_center_component``) against the
``scipy.ndimage.label`` restatement bit for bit, the float64 softmax (``sd_glia_view_probas``), ``GliaViewModel`` against a plain
``ViewModel`` and the float32 restatement, ``predict_views`` / ``predict_sos_views`` against the golden of the reference's own
functions, and the chain locations -> views -> probabilities -> classes -> astrocyte splitting on a small synthetic dataset."""
import os

import numpy as np
import pytest
import torch

import _glia_views_ref as G
import _viewnet_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORES = ('f16', 'bf16')
GUARD = 4096


# -- the centre component -------------------------------------------------------------------------------------------------------------
def _center(gpu, planes, bg, in_place, offset=0):
    """The entry on `planes` (n, H, W) with a guard band behind the output (and, with `offset`, a misaligned start)."""
    from syconn_amd import _dev as dv
    planes = np.ascontiguousarray(planes, np.uint8)
    n, H, W = planes.shape
    src = torch.full((offset + planes.size + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    src[offset:offset + planes.size] = torch.from_numpy(planes.reshape(-1)).to(gpu)
    dst = src if in_place else torch.full_like(src, 0x5A)
    dv.call('sd_views_center_component', gpu, src[offset:], n, H, W, int(bg), dst[offset:])
    torch.cuda.synchronize(gpu)
    out = dst.cpu().numpy()
    assert (out[:offset] == (0xA5 if in_place else 0x5A)).all() and (out[offset + planes.size:] == (0xA5 if in_place else 0x5A)).all()
    if not in_place:
        assert np.array_equal(src[offset:offset + planes.size].cpu().numpy(), planes.reshape(-1))      # the input is left alone
    return out[offset:offset + planes.size].reshape(planes.shape)


@pytest.mark.parametrize('in_place', (False, True))
@pytest.mark.parametrize('bg', (1, 255))
def test_center_component_small_sizes(gpu, bg, in_place):
    """W in {1, 31, 32, 33, 64, 65} x H in {1, 2, 3, 17}: no foreground, all foreground, the centre on background, random planes; W = 32
    and 64 take the 16-byte path when the buffers are aligned and the byte path when they are not."""
    for H in (1, 2, 3, 17):
        for W in (1, 31, 32, 33, 64, 65):
            planes = G.small_planes(H, W, bg)
            want = G.center_component_planes(planes, bg)
            assert (want[0] == bg).all() and np.array_equal(want[1], planes[1]) and (want[2] == bg).all()
            for offset in ((0, 3) if W % 32 == 0 else (0,)):
                assert np.array_equal(_center(gpu, planes, bg, in_place, offset), want), (H, W, bg, in_place, offset)


@pytest.mark.parametrize('in_place', (False, True))
def test_center_component_shapes(gpu, in_place):
    """Two components that touch only diagonally at the centre; a run that ends at bit W - 1 of a row while another starts at bit 0 of
    the next (W = 32, 33); a one-pixel spiral and two serpentines over 64 x 96 that cross word seams in both directions and take
    hundreds of rounds."""
    p = G.diagonal_pair()
    got = _center(gpu, p[None], 255, in_place)[0]
    assert np.array_equal(got, G.center_component(p, 255)) and (got == 30).sum() == 0 and (got == 20).sum() == (p == 20).sum()
    for W in (32, 33):
        p = G.row_end_pair(W)
        got = _center(gpu, p[None], 255, in_place)[0]
        assert np.array_equal(got, G.center_component(p, 255)) and (got[3] == 255).all() and (got[2, W // 2:] == 50).all()
    long = np.stack([G.spiral(64, 96), G.serpentine(64, 96), G.serpentine(64, 96, vertical=True), G.spiral(64, 96)[::-1, ::-1]])
    got = _center(gpu, long, 255, in_place)
    assert np.array_equal(got, G.center_component_planes(long, 255)) and np.array_equal(got[:3], long[:3])
    # ... and cut: the part behind the cut is another component
    cut = long.copy()
    cut[0, 0, 40] = cut[1, 10, 50] = cut[2, 30, 20] = 255
    want = G.center_component_planes(cut, 255)
    assert all(0 < (want[k] != 255).sum() < (cut[k] != 255).sum() for k in range(3))
    assert np.array_equal(_center(gpu, cut, 255, in_place), want)


@pytest.mark.parametrize('bg', (1, 255))
def test_center_component_view_planes(gpu, bg):
    """64 random planes of 128 x 256, foreground densities 0.3 and 0.6, in place and out of place."""
    planes = G.random_planes(64, 128, 256, bg, 11)
    want = G.center_component_planes(planes, bg)
    kept = (want != bg).reshape(64, -1).sum(1)
    assert kept.min() >= 1 and kept[1::2].max() > 1000 and (kept < (planes != bg).reshape(64, -1).sum(1)).all()
    for in_place in (False, True):
        assert np.array_equal(_center(gpu, planes, bg, in_place), want)


def test_center_component_lds_bound_and_grid(gpu):
    """One 512 x 1024 plane (two masks of 64 KiB); the largest planes the bound admits (8 H ceil(W / 32) + 16 = 163840 bytes); the first
    sizes past it, which are an argument error before anything is launched; one batch of planes past the grid cap."""
    from syconn_amd import _dev as dv
    from syconn_amd import _lib as L
    rng = np.random.default_rng(5)
    big = np.full((1, 512, 1024), 255, np.uint8)
    big[0][rng.random((512, 1024)) < 0.62] = 9
    big[0, 200:320, 400:640] = 17
    want = G.center_component_planes(big, 255)
    assert 10 ** 5 < (want != 255).sum() < (big != 255).sum()
    for in_place in (False, True):
        assert np.array_equal(_center(gpu, big, 255, in_place), want)
    words = (L.SD_GLIA_VIEWS_LDS_BYTES - 16) // 8
    assert words == 20478
    for H, W in ((words, 32), (1, 32 * words - 31)):
        p = np.full((1, H, W), 255, np.uint8)
        p[0, :, :1] = 4
        p[0, H // 2, :] = 5
        assert np.array_equal(_center(gpu, p, 255, False), p)
    buf = torch.full((32 * (words + 1) + GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    for H, W in ((words + 1, 32), (words + 1, 1), (1, 32 * words + 1), (512, 1280)):
        with pytest.raises(ValueError, match='do not fit the LDS'):
            dv.call('sd_views_center_component', gpu, buf, 1, H, W, 255, buf)
        with pytest.raises(ValueError, match='do not fit the LDS'):      # ... also without planes: the check comes first
            dv.call('sd_views_center_component', gpu, None, 0, H, W, 255, None)
    torch.cuda.synchronize(gpu)
    assert (buf == 0xA5).all()
    dv.call('sd_views_center_component', gpu, None, 0, 4, 4, 255, None)      # n = 0 is legal
    for args, msg in (((buf, 1, 0, 4, 255, buf), 'positive'), ((buf, 1, 4, 4, 256, buf), 'uint8'), ((None, 1, 4, 4, 1, buf), 'bad argument'),
                      ((buf, 1, 4, 4, 1, None), 'bad argument')):
        with pytest.raises(ValueError, match=msg):
            dv.call('sd_views_center_component', gpu, *args)
    n = L.SD_GLIA_VIEWS_GRID + 3
    many = np.tile(G.small_planes(3, 33, 255), (n // 9 + 1, 1, 1))[:n]
    many[-1, 1, 16] = 201
    assert np.array_equal(_center(gpu, many, 255, True), G.center_component_planes(many, 255))


def test_single_conn_comp_img(gpu):
    """The drop-in on one image: the golden planes of the reference's own function, any shape that squeezes to 2-D, uint8-valued float32."""
    from syconn_amd.proc.image import center_component_planes, single_conn_comp_img
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'g32_glia_views.npz'))
    for k, (p, bg) in enumerate(G.golden_planes()):
        got = single_conn_comp_img(p, background=bg, device=gpu) if bg != 1 else single_conn_comp_img(p, device=gpu)
        assert got.dtype == np.uint8 and np.array_equal(got, gold[f'plane{k}']), k
    p, bg = G.golden_planes()[6]
    want = gold['plane6']
    assert np.array_equal(single_conn_comp_img(p[None, :, :, None], 255., device=gpu), want[None, :, :, None])
    f = single_conn_comp_img(p.astype(np.float32), 255, device=gpu)
    assert f.dtype == np.float32 and np.array_equal(f, want.astype(np.float32))
    stack = torch.from_numpy(np.stack([p, p[::-1].copy()])).to(gpu)
    out = center_component_planes(stack.view(1, 2, *p.shape), 255)
    assert out.shape == (1, 2, *p.shape) and np.array_equal(out[0, 0].cpu().numpy(), want) and np.array_equal(stack[0].cpu().numpy(), p)
    assert center_component_planes(stack, 255, out=stack) is stack and np.array_equal(stack[0].cpu().numpy(), want)


# -- the softmax --------------------------------------------------------------------------------------------------------------------------
def test_softmax(gpu):
    """Within 1 float32 ulp of the float64 restatement (the device's float64 exp and the host's each err below one float64 ulp, which
    moves the single rounding to float32 by at most one step); rows sum to 1 within 2 ulp; +-80, equal logits, n = 0, one sample past a
    grid stride; a NaN or infinite logit raises."""
    from syconn_amd import _lib as L
    from syconn_amd.handler.prediction import glia_view_probas
    rng = np.random.default_rng(2)
    n = 256 * L.SD_GLIA_VIEWS_GRID + 1
    x = (rng.standard_normal((n, 2)) * rng.choice([0.01, 1.0, 10.0, 40.0], (n, 1))).astype(np.float32)
    x[:6] = [[80, -80], [-80, 80], [0, 0], [3.25, 3.25], [-80, -80], [1e30, -1e30]]
    got = glia_view_probas(torch.from_numpy(x).to(gpu)).cpu().numpy()
    want = G.softmax64(x)
    assert got.dtype == np.float32 and got.shape == (n, 2) and (got >= 0).all() and (got <= 1).all()
    d = G.ulp_distance(got, want)
    print(f'softmax: {n} rows, max ulp distance {d.max()}, rows that differ {(d.max(1) > 0).sum()}')
    assert d.max() <= 1
    assert got[:6].tolist() == [[1, 0], [0, 1], [.5, .5], [.5, .5], [.5, .5], [1, 0]]
    s = got.astype(np.float64).sum(1)
    assert np.abs(s - 1).max() <= 2 * 2.0 ** -24      # one ulp below 1 is 2^-24
    assert np.array_equal(glia_view_probas(torch.from_numpy(x[:1]).to(gpu)).cpu().numpy(), got[:1])
    assert glia_view_probas(torch.zeros((0, 2), device=gpu)).shape == (0, 2)
    for bad in (np.nan, np.inf, -np.inf):
        y = x[:300].copy()
        y[257, 1] = bad
        with pytest.raises(ValueError, match='NaN or infinite'):
            glia_view_probas(torch.from_numpy(y).to(gpu))
    assert np.array_equal(glia_view_probas(torch.from_numpy(x[:300]).to(gpu)).cpu().numpy(), got[:300])      # ... and the flag is cleared


# -- the model --------------------------------------------------------------------------------------------------------------------------
def _weights(seed=321):
    from syconn_amd.cnn.viewnet_spec import GLIA_CMN
    spec = GLIA_CMN()
    return spec, R.make_weights(spec, seed, 2, 128, 256)


def _glia_model(gpu, store='f16', seed=321, bs=400):
    from syconn_amd.handler.prediction import GliaViewModel
    spec, arrs = _weights(seed)
    return GliaViewModel(spec, R.state_dict_of(spec, arrs), act_dtype=store, bs=bs, device=gpu)


@pytest.mark.parametrize('store', STORES)
def test_glia_view_model(gpu, store):
    """The logits are the bits of a plain ``ViewModel`` with the same spec and weights through the same head entry; the probabilities are
    the softmax of the device's own logits within 1 ulp; the logits are within T of the float32 restatement on the stored weights, T = 4
    x |emulation - restatement| on these very views, both on the CPU (the rule of tests/test_gpu_viewnet.py::test_cmn_geometry and
    tests/test_gpu_embedding.py for a whole network)."""
    from syconn_amd.handler.prediction import ViewModel, ViewSamples, naive_view_normalization_new
    spec, arrs = _weights()
    m = _glia_model(gpu, store)
    assert m._entry == 'sd_viewnet_embed' and m.bs == 400

    class Plain(ViewModel):
        _entry = 'sd_viewnet_embed'

    plain = Plain(spec, R.state_dict_of(spec, arrs), act_dtype=store, device=gpu)
    views = R.synthetic_views(50, 11, 1, 2, 128, 256)
    logits = m.predict_proba(views, apply_softmax=False)
    assert logits.shape == (11, 2) and logits.dtype == np.float32 and len(np.unique(logits, axis=0)) == 11
    assert np.array_equal(logits, plain.predict_proba(views))
    probas = m.predict_proba(views)
    assert probas.shape == (11, 2) and probas.dtype == np.float32 and G.ulp_distance(probas, G.softmax64(logits)).max() <= 1
    vd = torch.from_numpy(views).to(gpu)
    table = np.arange(22, dtype=np.int32).reshape(11, 2)
    for form in (vd, naive_view_normalization_new(views), ViewSamples(vd, table)):
        assert np.array_equal(m.predict_proba(form), probas)
    for bs in (1, 4, 11):
        assert np.array_equal(m.predict_proba(vd, bs=bs), probas), bs
    assert m.predict_device(vd).is_cuda and m.predict_proba(views[:0]).shape == (0, 2)
    l32 = R.forward32_stored(spec, arrs, views, None, store)
    T = 4 * np.abs(R.forward_emul(spec, arrs, views, None, store) - l32).max()
    d = np.abs(logits - l32).max()
    print(f'glia_cmn {store}: |logits - float32| {d:.5f} of T = {T:.5f}')
    assert d <= T
    four = R.synthetic_views(51, 2, 4, 2, 128, 256)
    with pytest.raises(ValueError, match='views have 4 channels'):
        m.predict_proba(four)
    with pytest.raises(ValueError, match='flattens to 279'):      # three views
        m.predict_proba(R.synthetic_views(52, 2, 1, 3, 128, 256))
    with pytest.raises(ValueError, match='flattens to 1860'):      # the 20 views of a cell type sample
        m.predict_proba(ViewSamples(torch.from_numpy(R.synthetic_views(53, 20, 1, 2, 128, 256)).to(gpu), np.arange(40, dtype=np.int32).reshape(2, 20)))
    with pytest.raises(NotImplementedError):
        m.predict_proba(views.astype(np.float32))


# -- predict_views / predict_sos_views -------------------------------------------------------------------------------------------------------
class _Fake:
    """The model of the partition golden on the device path: the views come as one device tensor."""

    def __init__(self, gpu):
        self.dev, self.calls = gpu, []

    def predict_proba(self, views, verbose=False):
        assert isinstance(views, torch.Tensor) and views.is_cuda
        self.calls.append(tuple(views.shape))
        return G.fake_proba(views.cpu().numpy())


class _So:
    def __init__(self, i, views=None):
        self.id, self.attr_dict, self._views, self.asked = i, {}, views, None

    def load_views(self, woglia=True, raw_only=False):
        self.asked = (woglia, raw_only)
        return self._views


@pytest.mark.parametrize('cc', (False, True))
def test_predict_views_golden(gpu, cc):
    """Three supervoxels with 3, 0 and 5 locations: the partition, ``single_cc_only`` (background 1, the reference's call) and the
    stored key are those of the reference's own ``predict_views``; host arrays and device tensors; ``raw_only`` on a 4-channel array."""
    from syconn_amd.proc.sd_proc import predict_sos_views, predict_views
    from syconn_amd.reps.super_segmentation_object import predict_views_gliaSV
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'g32_glia_views.npz'))
    for C in (1, 4):
        tag = f'pv_c{C}_cc{int(cc)}'
        views = G.golden_views(C)
        keep = [v.copy() for v in views]
        for form in (views, [torch.from_numpy(v).to(gpu) for v in views]):
            m = _Fake(gpu)
            probas = predict_views(m, form, None, 'k', single_cc_only=cc, return_proba=True)
            assert m.calls == [(8, C, 2, 12, 20)] and [len(p) for p in probas] == [3, 0, 5]
            assert np.array_equal(np.concatenate(probas), gold[f'{tag}_probas'])
        assert all(np.array_equal(a, b) for a, b in zip(views, keep))      # the caller's arrays are left alone
        sos = [_So(10 + i) for i in range(3)]
        assert predict_views(_Fake(gpu), views, sos, 'glia_probas_x', single_cc_only=cc) is None
        assert all(list(so.attr_dict) == [str(gold['pv_key'])] for so in sos)
        assert np.array_equal(np.concatenate([so.attr_dict['glia_probas_x'] for so in sos]), gold[f'{tag}_probas'])
    # the filter with the renderer's background is another one
    v255 = [np.where(v == 1, 255, v).astype(np.uint8) for v in G.golden_views(1)]
    a = predict_views(_Fake(gpu), v255, None, 'k', single_cc_only=True, return_proba=True, background=255)
    want, _ = G.predict_views(G.fake_proba, v255, single_cc_only=True, background=255)
    plain, _ = G.predict_views(G.fake_proba, v255)
    assert np.array_equal(np.concatenate(a), np.concatenate(want)) and not np.array_equal(np.concatenate(want), np.concatenate(plain))
    # predict_sos_views: raw_only keeps channel 0 of the four
    four = G.golden_views(4)
    sos = [_So(20 + i, v) for i, v in enumerate(four)]
    m = _Fake(gpu)
    got = predict_sos_views(m, sos, 'glia_probas', woglia=False, raw_only=True, single_cc_only=cc, return_proba=True)
    want, _ = G.predict_views(G.fake_proba, [v[:, :1] for v in four], single_cc_only=cc, background=1)
    assert m.calls == [(8, 1, 2, 12, 20)] and np.array_equal(got, np.concatenate(want)) and all(so.asked == (False, True) and not so.attr_dict for so in sos)
    assert predict_sos_views(_Fake(gpu), sos, 'glia_probas', raw_only=True, single_cc_only=cc) is None
    assert all(np.array_equal(so.attr_dict['glia_probas'], w) for so, w in zip(sos, want))
    cell = type('Cell', (), {'svs': [_So(30 + i, v) for i, v in enumerate(four)], 'version': 'tmp'})()
    assert np.array_equal(predict_views_gliaSV(cell, _Fake(gpu), single_cc_only=cc), got) and not any(sv.attr_dict for sv in cell.svs)
    cell.version = 0
    assert predict_views_gliaSV(cell, _Fake(gpu), pred_key_appendix='_v2', single_cc_only=cc) is None
    assert all(np.array_equal(sv.attr_dict['glia_probas_v2'], w) for sv, w in zip(cell.svs, want))


def test_predict_views_with_the_model(gpu):
    """The same three supervoxels through the glia network: one call over all locations equals the network on every supervoxel alone."""
    from syconn_amd.proc.sd_proc import predict_views
    m = _glia_model(gpu)
    views = [R.synthetic_views(60 + k, n, 1, 2, 128, 256) for k, n in enumerate(G.GOLDEN_COUNTS)]
    for cc in (False, True):
        probas = predict_views(m, views, None, 'k', single_cc_only=cc, return_proba=True, background=255)
        filt = [G.center_component_planes(v, 255) for v in views] if cc else views
        assert [p.shape for p in probas] == [(3, 2), (0, 2), (5, 2)]
        for p, v in zip(probas, filt):
            assert np.array_equal(p, m.predict_proba(v))
    assert not np.array_equal(m.predict_proba(views[2]), m.predict_proba(G.center_component_planes(views[2], 255)))


# -- the synthetic dataset ----------------------------------------------------------------------------------------------------------------
SCALING = (100., 100., 100.)


class _Sv:
    def __init__(self, i, mesh, rep):
        self.id, self.mesh, self.rep_coord, self.scaling, self.attr_dict = int(i), mesh, rep, SCALING, {}

    def load_attr_dict(self):
        pass


class _Cell:
    """A connected component of the supervoxel graph: its supervoxels and the mesh they make together."""

    def __init__(self, svs):
        self.svs = svs
        ind, vert, n = [], [], 0
        for sv in svs:
            ind.append(np.asarray(sv.mesh[0], np.uint32) + np.uint32(n))
            vert.append(np.asarray(sv.mesh[1], np.float32))
            n += len(sv.mesh[1]) // 3
        self.mesh = [np.concatenate(ind), np.concatenate(vert), np.zeros(0, np.float32)]

    def load_mesh(self, name):
        return [np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.float32)]


@pytest.fixture(scope='module')
def dataset(gpu):
    """A label volume of 100 nm voxels: a tube of three supervoxels (1, 2, 3), a ball (7), a bar (5); 9 has voxels in the table of
    properties but no mesh.  -> (supervoxels by id, PropTable, edges)."""
    from syconn_amd.proc.meshes import find_meshes_table
    from syconn_amd.proc.sd_proc import PropTable
    shape = (100, 56, 40)
    x, y, z = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
    vol = np.zeros(shape, np.uint64)
    tube = ((y - 14 - 4 * np.sin(x / 9.)) ** 2 + (z - 14) ** 2 < (5 + 2 * np.sin(x / 5.) ** 2) ** 2) & (x >= 3) & (x < 97)
    vol[tube & (x < 45)] = 1
    vol[tube & (x >= 45) & (x < 60)] = 2
    vol[tube & (x >= 60)] = 3
    vol[(x - 20) ** 2 + (y - 42) ** 2 + (z - 26) ** 2 < 81] = 7
    vol[(abs(x - 70) < 24) & (abs(y - 42) < 5) & (abs(z - 28) < 4)] = 5
    meshes = find_meshes_table(vol, (0, 0, 0), pad=1, scaling=SCALING, meshing_props={'normals': False}, device=gpu)
    assert meshes.ids.tolist() == [1, 2, 3, 5, 7]
    ids = np.array([1, 2, 3, 5, 7, 9], np.uint64)
    boxes, sizes, rep = [], [], []
    for i in ids[:-1]:
        w = np.argwhere(vol == i)
        boxes.append([w.min(0), w.max(0) + 1])
        sizes.append(len(w))
        rep.append(w[len(w) // 2])
    boxes.append([[60, 30, 20], [66, 36, 24]])
    sizes.append(100)
    rep.append([62, 33, 22])
    props = PropTable(ids, np.array(sizes), np.array(rep), np.array(boxes, np.int64), np.arange(len(ids) + 1))
    svs = {int(i): _Sv(i, meshes.mesh_of(i), tuple(int(v) for v in r)) for i, r in zip(ids, rep)}
    assert len(svs[9].mesh[1]) == 0
    edges = np.array([[1, 2], [2, 3], [5, 9]], np.uint64)
    return svs, props, edges


def test_gliapred_sso_nocache(gpu, dataset):
    """A cell of three supervoxels: the stored ``glia_probas`` are the hand-made chain of locations, ``render_sso_coords``, model and
    slices, bit for bit."""
    from syconn_amd.proc.rendering import render_sso_coords
    from syconn_amd.reps.super_segmentation_helper import glia_pred_exists, gliapred_sso_nocache, sample_locations_sso
    svs, _, _ = dataset
    m = _glia_model(gpu)
    cell = _Cell([svs[1], svs[2], svs[3]])
    for sv in cell.svs:
        sv.attr_dict.clear()
    assert not glia_pred_exists(cell.svs[0])
    gliapred_sso_nocache(cell, m, verbose=False, device=gpu)
    locs = sample_locations_sso(cell, device=gpu)
    counts = [len(l) for l in locs]
    assert min(counts) >= 1 and max(counts) >= 3 and sum(counts) <= 40
    views = render_sso_coords(cell, np.concatenate(locs), add_cellobjects=False, device=gpu)
    assert views.shape == (sum(counts), 1, 2, 128, 256) and (views != 255).any()
    probas = m.predict_proba(views)
    assert len(np.unique(probas, axis=0)) > 1
    b = np.cumsum([0] + counts)
    for k, sv in enumerate(cell.svs):
        assert glia_pred_exists(sv) and sv.attr_dict['glia_probas'].dtype == np.float32
        assert np.array_equal(sv.attr_dict['glia_probas'], probas[b[k]:b[k + 1]]), k


def _cells(dataset):
    svs, _, _ = dataset
    for sv in svs.values():
        sv.attr_dict.clear()
    return [_Cell([svs[7]]), _Cell([svs[3], svs[1], svs[2]]), _Cell([svs[9], svs[5]])]


def test_predict_glia_table(gpu, dataset):
    """Three cells -- a single supervoxel; three supervoxels in another order than their ids; one holding a supervoxel without vertices --
    at max_locs_per_batch = 2 (a supervoxel straddles batches), 1 and the default: the same bits, equal to ``gliapred_sso_nocache``
    per cell, rows ascending by id, consistent offsets; the supervoxel without vertices has no locations, a NaN mean and class 0."""
    from syconn_amd.proc import graphs
    from syconn_amd.reps.super_segmentation_helper import gliapred_sso_nocache, predict_glia_table
    m = _glia_model(gpu)
    cells = _cells(dataset)
    tables = [predict_glia_table(cells, m, thresh=0.4, max_locs_per_batch=b, device=gpu) for b in (2, 1, None)]
    t = tables[0]
    assert t.sv_ids.tolist() == [1, 2, 3, 5, 7, 9] and t.sv_ids.dtype == np.uint64 and t.view_begin.dtype == np.int64
    counts = np.diff(t.view_begin)
    assert t.view_begin[0] == 0 and t.view_begin[-1] == len(t.glia_probas) and counts[-1] == 0 and counts[:-1].min() >= 1 and counts.max() > 2
    assert t.glia_probas.dtype == np.float32 and t.glia_probas.shape == (counts.sum(), 2) and t.glia_proba.dtype == np.float64 and t.glia.dtype == np.uint8
    for o in tables[1:]:
        for name in ('sv_ids', 'view_begin', 'glia_probas', 'glia'):
            assert np.array_equal(getattr(o, name), getattr(t, name)), name
        assert np.array_equal(o.glia_proba, t.glia_proba, equal_nan=True)
    assert np.isnan(t.glia_proba[-1]) and t.glia[-1] == 0 and np.isfinite(t.glia_proba[:-1]).all()
    glia, mean = graphs.glia_pred(t.glia_probas[:, 1], t.view_begin, 0.4, False, gpu)
    assert np.array_equal(glia, t.glia) and np.array_equal(mean, t.glia_proba, equal_nan=True)
    d = t.as_dict()
    for cell in cells[:2]:
        gliapred_sso_nocache(cell, m, verbose=False, device=gpu)
        for sv in cell.svs:
            assert np.array_equal(sv.attr_dict['glia_probas'], d[sv.id]) and np.array_equal(t.probas_of(sv.id), d[sv.id]), sv.id
    # the last cell: gliapred_sso_nocache looks at the supervoxel without vertices from its representative coordinate, the table does not
    gliapred_sso_nocache(cells[2], m, verbose=False, device=gpu)
    assert cells[2].svs[0].attr_dict['glia_probas'].shape == (1, 2) and np.array_equal(cells[2].svs[1].attr_dict['glia_probas'], d[5]) and d[9].shape == (0, 2)
    filtered = predict_glia_table(cells, m, thresh=0.4, single_cc_only=True, background=255, max_locs_per_batch=3, device=gpu)
    # (a rendered view of these cells is one blob around its centre, so the filter may well change nothing here: what is checked is
    # that the table's filter is the hand-made chain's; that the filter changes probabilities: test_predict_views_with_the_model)
    from syconn_amd.proc.rendering import render_sso_coords
    from syconn_amd.reps.super_segmentation_helper import sample_locations_sso
    assert np.array_equal(filtered.view_begin, t.view_begin)
    locs = sample_locations_sso(cells[1], device=gpu)
    views = render_sso_coords(cells[1], np.concatenate(locs), add_cellobjects=False, device=gpu)
    want = m.predict_proba(G.center_component_planes(views, 255))
    b = np.cumsum([0] + [len(l) for l in locs])
    for k, sv in enumerate(cells[1].svs):
        assert np.array_equal(filtered.probas_of(sv.id), want[b[k]:b[k + 1]]), sv.id
    empty = _Cell([dataset[0][9]])
    with pytest.raises(ValueError, match='empty mesh'):
        predict_glia_table([empty], m, device=gpu)
    with pytest.raises(ValueError, match='occurs twice'):
        predict_glia_table([cells[0], cells[0]], m, device=gpu)
    with pytest.raises(ValueError, match='max_locs_per_batch'):
        predict_glia_table(cells, m, max_locs_per_batch=0, device=gpu)
    none = predict_glia_table([], m, device=gpu)
    assert len(none) == 0 and none.view_begin.tolist() == [0] and none.glia_probas.shape == (0, 2)


def test_rag_to_prediction_to_splitting(gpu, dataset):
    """``run_create_rag -> run_astrocyte_prediction -> run_astrocyte_splitting(glia_probas=..., view_begin=...)``: the cells are the
    components of the pruned graph, the splitting's classes are the table's.  `thresh` is the median of the means, so that both classes
    occur with seeded weights.  The weight seed is one for which the float32 restatement on the CPU, over these cells' rendered views,
    gives both classes with room to spare: supervoxels 3 and 7 are glia with 9 of 12 and 6 of 8 views above the threshold, no view's
    probability within 0.009 of it and no other mean within 0.028 (the network's own error is a tenth of that)."""
    from syconn_amd.exec.exec_inference import run_astrocyte_prediction, run_astrocyte_splitting
    from syconn_amd.exec.exec_init import run_create_rag
    svs, props, edges = dataset
    m = _glia_model(gpu, seed=329)
    rag = run_create_rag(edges, props, scaling=SCALING, min_cc_size=0.0, device=gpu)
    sv_begin, sv_ids = np.asarray(rag.sv_begin, np.int64), np.asarray(rag.sv_ids)
    assert len(rag.ssv_ids) == 3 and sorted(sv_ids.tolist()) == [1, 2, 3, 5, 7, 9]
    for sv in svs.values():
        sv.attr_dict.clear()
    cells = [_Cell([svs[int(i)] for i in sv_ids[sv_begin[k]:sv_begin[k + 1]]]) for k in range(len(rag.ssv_ids))]
    first = run_astrocyte_prediction(cells, m, thresh=0.5, device=gpu)
    thresh = float(np.nanmedian(first.glia_proba))
    table = run_astrocyte_prediction(cells, m, thresh=thresh, device=gpu)
    print(f'means {table.glia_proba.tolist()}, thresh {thresh}, classes {table.glia.tolist()}')
    assert np.array_equal(table.sv_ids, props.ids) and np.array_equal(table.glia_probas, first.glia_probas)
    assert table.glia.tolist() == [0, 0, 1, 0, 1, 0]
    res = run_astrocyte_splitting(rag, props, glia_probas=table.glia_probas[:, 1], view_begin=table.view_begin, thresh=thresh, use_point_models=False,
                                  scaling=SCALING, min_cc_size=0.0, device=gpu)
    assert np.array_equal(res.glia, table.glia) and np.array_equal(res.glia_proba, table.glia_proba, equal_nan=True)
    got = {int(i): int(c) for i, c in zip(res.split.node_ids, res.split.node_class)}
    assert sorted(got) == [1, 2, 3, 5, 7, 9]
    assert len(res.svs['astrocyte_svs']) + len(res.svs['neuron_svs']) == 6 and len(res.svs['pruned_svs']) == 0
