"""The view network on the device (syconn_amd/csrc/sd_viewnet.hip): every layer's stored output and every Linear's output against the
float64 one-op reference on the device's own inputs (tests/_viewnet_ref.py), the CMN geometry against the float32 restatement, the
sample table, batching, guard bands, argument checks, the fp16 range flag and the cell type step end to end."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import _viewnet_cases as K
import _viewnet_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(spec, arrs, store, gpu, bs=40):
    from syconn_amd.handler.prediction import ViewModel
    return ViewModel(spec, R.state_dict_of(spec, arrs), act_dtype=store, bs=bs, device=gpu)


def _planes(views):
    """(n, C, D, H, W) -> (n D, H, W, C): the planes in sample order, channels last."""
    n, Cc, D, H, W = views.shape
    return np.ascontiguousarray(views.transpose(0, 2, 3, 4, 1)).reshape(n * D, H, W, Cc)


def _step_checks(model, spec, arrs, store, views, scal, D, logits):
    """Every op of the last forward against StepRef on the device's own stored input.  -> the largest |dev - ref| / bound."""
    sr = R.StepRef(spec, arrs, store)
    assert model.num_ops == sr.n_ops()
    x, share = _planes(views), 0.0
    for i in range(sr.nl):
        dev = torch.from_numpy(model.read_buffer(i)).double()
        ref, S = sr.layer(i, x)
        assert dev.shape == ref.shape, (i, dev.shape, ref.shape)
        assert torch.isfinite(dev).all()
        ratio = ((dev - ref).abs() / R.bound_stored(ref, S, K.C[store], store)).max().item()
        assert ratio <= 1, f'layer {i}: |dev - ref| is {ratio:.3f} of the bound'
        share, x = max(share, ratio), dev.numpy()
    v = sr.head_input(x, scal, D).float()
    for j in range(sr.n_fc):
        dev = torch.from_numpy(model.read_buffer(sr.nl + j)).double()
        ref, S = sr.linear(j, v)
        assert dev.shape == ref.shape
        ratio = ((dev - ref).abs() / R.bound_f32(ref, S, K.C[store])).max().item()
        assert ratio <= 1, f'Linear {j}: |dev - ref| is {ratio:.3f} of the bound'
        share, v = max(share, ratio), dev.float()
    assert np.array_equal(v.numpy(), logits)      # the last Linear's buffer is the logits
    return share


SMALL_CASES = [('a', 'shapes'), ('a', 'zeros'), ('a', 'ones'), ('a', 'checker'), ('b', 'shapes'), ('c', 'shapes'), ('d', 'shapes')]


@pytest.mark.parametrize('store', K.STORES)
@pytest.mark.parametrize('name, mode', SMALL_CASES)
def test_steps_small(gpu, name, mode, store):
    spec, D, H, W, arrs, views, scal = K.inputs(name, mode)
    m = _model(spec, arrs, store, gpu)
    logits = m.predict_proba((views, scal) if spec.n_scalar else views)
    assert logits.shape == (views.shape[0], spec.n_classes) and logits.dtype == np.float32
    share = _step_checks(m, spec, arrs, store, views, scal, D, logits)
    print(f'{name}:{mode} {store}: largest share of the bound {share:.3f}')


@pytest.mark.parametrize('store', K.STORES)
def test_cmn_geometry(gpu, store):
    """Two samples of 20 x 128 x 256 through the in-tree net: all seven layers and the head as single ops, the logits within T of the
    float32 restatement, the same argmax (both samples are safe: tests/test_viewnet_cpu.py::test_cmn_tolerance_and_safety)."""
    spec, D, H, W, arrs, views, scal = K.inputs('cmn')
    m = _model(spec, arrs, store, gpu)
    logits = m.predict_proba((views, scal))
    share = _step_checks(m, spec, arrs, store, views, scal, D, logits)
    l32 = R.forward32_stored(spec, arrs, views, scal, store)      # float32 on the weights the plan stores: T is activation rounding only
    d = np.abs(logits - l32).max()
    print(f'cmn {store}: largest share of the bound {share:.3f}; |logits - float32| {d:.5f} of T = {K.T[store]:.5f}')
    assert d <= K.T[store]
    assert np.array_equal(logits.argmax(1), l32.argmax(1))


@pytest.mark.parametrize('store', K.STORES)
def test_sample_table(gpu, store):
    """Repeated planes, a permutation, planes of several cells interleaved: bit for bit the same samples materialised in order.  An
    index outside the planes is an IndexError -- the device flags it and reads nothing."""
    from syconn_amd.handler.prediction import ViewSamples
    spec, D, H, W, arrs, _, _ = K.inputs('a')
    m = _model(spec, arrs, store, gpu)
    n_loc, vpl = 6, 2
    views = R.synthetic_views(5, n_loc, spec.in_channels, vpl, H, W)      # (n_loc, C, vpl, H, W): 12 planes
    planes = views.swapaxes(1, 0).reshape(spec.in_channels, n_loc * vpl, H, W)
    rng = np.random.default_rng(2)
    table = np.array([[3, 3, 3], [11, 0, 5], [0, 6, 1], [7, 2, 8], [5, 0, 11], *rng.permutation(12).reshape(4, 3)], np.int32)
    scal = rng.uniform(-1, 1, (len(table), 2)).astype(np.float32)
    got = m.predict_proba((ViewSamples(torch.from_numpy(views).to(gpu), table), scal))
    mat = planes[:, table.reshape(-1)].reshape(spec.in_channels, len(table), D, H, W).swapaxes(1, 0)
    want = m.predict_proba((np.ascontiguousarray(mat), scal))
    assert np.array_equal(got, want)
    assert np.array_equal(got[1, :], m.predict_proba((np.ascontiguousarray(mat[1:2]), scal[1:2]))[0])
    _step_checks(m, spec, arrs, store, np.ascontiguousarray(mat[1:2]), scal[1:2], D, got[1:2])
    for bad in (12, -1, 2 ** 31 - 1):
        t = table.copy()
        t[4, 1] = bad
        with pytest.raises(IndexError, match=r'outside \[0, 12\)'):
            m.predict_proba((ViewSamples(views, t), scal))
    assert np.array_equal(m.predict_proba((ViewSamples(views, table), scal)), want)      # ... and the model still works


@pytest.mark.parametrize('store', K.STORES)
def test_batching(gpu, store):
    """1 sample; bs and bs + 1; more samples than one launch set; more workgroups than one grid stride of the layer kernel (one tile per
    plane here) and of the head kernel: a sample has the same bits in every batch position."""
    from syconn_amd import _lib as L
    from syconn_amd.handler.prediction import ViewSamples
    spec, D, H, W, arrs, views, scal = K.inputs('b')
    n = views.shape[0]
    m = _model(spec, arrs, store, gpu, bs=4)
    one = np.concatenate([m.predict_proba((views[i:i + 1], scal[i:i + 1])) for i in range(n)])
    assert len(np.unique(one, axis=0)) == n
    for count, bs in ((4, 4), (5, 4), (5, 1), (11, 4), (L.SD_VIEWNET_GRID + 37, 4096)):
        idx = (np.arange(count) * 3 + 1) % n
        sm = ViewSamples(views, idx.astype(np.int32).reshape(count, 1) * D + np.arange(D, dtype=np.int32)[None])
        got = m.predict_proba((sm, scal[idx]), bs=bs)
        assert np.array_equal(got, one[idx]), (count, bs)
    assert L.SD_VIEWNET_GRID + 37 > L.SD_VIEWNET_HEAD_GRID


def _layout(spec, n, D, H, W):
    """The workspace layout of syconn_amd/csrc/sd_viewnet_plan.cpp: layer buffers n D Ho Wo cout_p fp16 / bf16, then the hidden vectors
    float32, each rounded up to 256 bytes.  -> [(offset, used bytes)], total."""
    out, off = [], 0
    for (cout, _, _), (h, w) in zip(spec.layers, spec.check_geometry(D, H, W)):
        used = n * D * h * w * (-(-cout // 8) * 8) * 2
        out.append((off, used))
        off += -(-used // 256) * 256
    for nout in spec.linear_sizes[1:-1]:
        out.append((off, n * nout * 4))
        off += -(-(n * nout * 4) // 256) * 256
    return out, off


@pytest.mark.parametrize('store', K.STORES)
def test_guard_bands(gpu, store):
    """Nothing is written behind the workspace, the logits, a layer's buffer or a hidden vector."""
    from syconn_amd import _dev as dv
    from syconn_amd import _lib as L
    spec, D, H, W, arrs, views, scal = K.inputs('a')
    m = _model(spec, arrs, store, gpu)
    want = m.predict_proba((views, scal))
    n = views.shape[0]
    ranges, total = _layout(spec, n, D, H, W)
    assert L.load().sd_viewnet_workspace_bytes(m._h, n, D, H, W) == total
    guard = 4096
    ws = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    logits = torch.full((n * spec.n_classes + 64,), -7.0, dtype=torch.float32, device=gpu)
    flags = torch.full((6,), 9, dtype=torch.int32, device=gpu)
    table = torch.arange(n * D, dtype=torch.int32, device=gpu)
    dv.call('sd_viewnet_forward', gpu, m._h, torch.from_numpy(views).to(gpu), n * D, D, H, W, table, n, D, torch.from_numpy(scal).to(gpu), logits, ws,
            total, flags)
    torch.cuda.synchronize(gpu)
    assert np.array_equal(logits[:n * spec.n_classes].cpu().numpy().reshape(n, -1), want)
    assert (logits[n * spec.n_classes:] == -7.0).all() and (ws[total:] == 0xA5).all()
    assert flags.cpu().tolist() == [0, 0, 9, 9, 9, 9]
    ends = [o for o, _ in ranges[1:]] + [total]
    for (off, used), end in zip(ranges, ends):
        assert (ws[off + used:end] == 0xA5).all(), (off, used, end)


def test_argument_checks(gpu):
    from syconn_amd import _dev as dv
    from syconn_amd import _lib as L
    from syconn_amd.handler.prediction import ViewModel, ViewSamples
    spec, D, H, W, arrs, views, scal = K.inputs('a')
    sd = R.state_dict_of(spec, arrs)
    with pytest.raises(ValueError, match='act_dtype'):
        ViewModel(spec, sd, act_dtype='f32', device=gpu)
    with pytest.raises(ValueError, match='bs must be positive'):
        ViewModel(spec, sd, bs=0, device=gpu)
    with pytest.raises(ValueError, match='has shape'):
        ViewModel(spec, {k: (v[:-1] if k == 'fc.0.bias' else v) for k, v in sd.items()}, device=gpu)
    m = ViewModel(spec, sd, device=gpu)
    calls = {
        'views have 3 channels': lambda: m.predict_proba((views[:, :3], scal)),
        'views must be': lambda: m.predict_proba((views[0], scal)),
        'uint8 array': lambda: m.predict_proba((views.astype(np.int16), scal)),
        'flattens to': lambda: m.predict_proba((views[:, :, :2], scal)),
        'has an empty output': lambda: m.predict_proba((views[:, :, :, :8], scal)),
        'takes 2 scalars': lambda: m.predict_proba(views),
        r'scalars must be \(3, 2\)': lambda: m.predict_proba((views, scal[:, :1])),
        'bs must be positive': lambda: m.predict_proba((views, scal), bs=0),
        'sample table must be int32': lambda: m.predict_proba((ViewSamples(views, np.zeros((1, D), np.int64)), scal[:1])),
        'at least one sample': lambda: m.predict_proba((ViewSamples(views, np.zeros((0, D), np.int32)), scal[:0])),
    }
    for msg, call in calls.items():
        with pytest.raises(ValueError, match=msg):
            call()
    with pytest.raises(NotImplementedError):
        m.predict_proba((views.astype(np.float32) / 255 - 0.4, scal))
    # float32 views that ARE the normalised uint8 views are taken, with the same bits
    assert np.array_equal(m.predict_proba((views.astype(np.float32) / 255. - 0.5, scal)), m.predict_proba((views, scal)))
    # the C entry itself
    n = views.shape[0]
    vd, sc, tb = torch.from_numpy(views).to(gpu), torch.from_numpy(scal).to(gpu), torch.arange(n * D, dtype=torch.int32, device=gpu)
    ws = dv.scratch('sd_viewnet_workspace_bytes', gpu, m._h, n, D, H, W)
    lg, fl = torch.zeros((n, spec.n_classes), device=gpu), torch.zeros(2, dtype=torch.int32, device=gpu)
    good = [m._h, vd, n * D, D, H, W, tb, n, D, sc, lg, ws, ws.numel(), fl]
    dv.call('sd_viewnet_forward', gpu, *good)
    for pos, val, msg in ((0, None, 'null'), (1, None, 'null'), (6, None, 'null'), (10, None, 'null'), (11, None, 'null'), (13, None, 'null'),
                          (9, None, 'scalars_dev is null'), (12, ws.numel() - 1, 'workspace smaller'), (3, 0, 'multiple of nb_views'),
                          (3, 2, 'multiple of nb_views'), (2, 0, 'multiple of nb_views'), (4, 8, 'empty output'), (8, 2, 'features'),
                          (7, 0, 'n_samples out of range'), (11, ws[1:], '16-byte aligned')):
        args = list(good)
        args[pos] = val
        with pytest.raises(ValueError, match=msg):
            dv.call('sd_viewnet_forward', gpu, *args)
    lib = L.load()
    assert lib.sd_viewnet_workspace_bytes(m._h, n, D, 4, W) == 0 and lib.sd_viewnet_workspace_bytes(None, n, D, H, W) == 0
    assert lib.sd_viewnet_num_ops(None) == 0 and lib.sd_viewnet_num_ops(m._h) == 4
    dims = (C.c_int32 * 4)()
    for idx in (-1, 4):
        assert lib.sd_viewnet_read_buffer(m._h, idx, ws.data_ptr(), lg.data_ptr(), n, D, H, W, None, dims, None) == L.SD_ERR_INVALID
    assert lib.sd_viewnet_read_buffer(m._h, 1, ws.data_ptr(), lg.data_ptr(), n, D, H, W, None, dims, None) == 0 and list(dims) == [n * D, 2, 6, 30]


def test_f16_overflow_flag(gpu):
    """First-layer weights scaled so that every STORED weight stays finite and the largest stored activation of layer 0 passes 65504
    (about 75,000): fp16 storage raises and names bf16; bf16 storage runs.  Scaled a little less, so that the largest one is about
    64,700 -- 1.3 % below the 65520 at which the kernel flags --, nothing is flagged and everything stored is finite."""
    from syconn_amd import _lib as L
    spec, D, H, W, _, views, scal = K.inputs('a')
    x = _planes(views)

    def weights(gain):
        arrs = R.make_weights(spec, 31, D, H, W, gain=gain)
        assert np.abs(arrs[0]).max() < 30000      # far inside fp16: the plan would refuse a weight that rounds to infinity
        ref, _ = R.StepRef(spec, arrs, 'f16').layer(0, x)
        return arrs, float(ref.max())

    over, top = weights(14000.0)
    assert 70000 < top < 80000
    with pytest.raises(L.ActivationOverflowError, match="act_dtype='bf16'"):
        _model(spec, over, 'f16', gpu).predict_proba((views, scal))
    assert np.isfinite(_model(spec, over, 'bf16', gpu).predict_proba((views, scal))).all()
    under, top = weights(12000.0)
    assert 64000 < top < 65400
    m = _model(spec, under, 'f16', gpu)
    assert np.isfinite(m.predict_proba((views, scal))).all()
    stored = m.read_buffer(0)
    assert np.isfinite(stored).all() and 64000 < stored.max() <= 65504


# -- end to end -------------------------------------------------------------------------------------------------------------------
class _Cell:
    view_caching = True

    def __init__(self, tris, verts, syn_props):
        self.mesh = (tris, verts)
        self.attr_dict = {}
        self.syn_props = syn_props
        self.saved = None

    def load_mesh(self, name):
        # 'mi': a part of the cell's own surface stands in for an organelle; the others are empty (a channel of 255)
        if name == 'mi':
            return (self.mesh[0][:len(self.mesh[0]) // 3], self.mesh[1])
        return (np.zeros(0, np.uint32), np.zeros((0, 3), np.float32))

    def save_attributes(self, keys, values):
        self.saved = dict(zip(keys, values))


@pytest.fixture(scope='module')
def cells(gpu):
    spec_ = importlib.util.spec_from_file_location('views_probe', os.path.join(ROOT, 'tools', 'views_probe.py'))
    probe = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(probe)
    from syconn_amd.proc import meshes
    out = []
    for seed, shape in ((0, (256, 192, 128)), (1, (160, 128, 96))):
        t = meshes.find_meshes_table(probe.make_cell(shape, seed), (0, 0, 0), scaling=(50.,) * 3, meshing_props={'normals': False}, device=gpu)
        rng = np.random.default_rng(seed)
        k = 12
        props = (rng.choice([-1, 1], k), rng.uniform(0.1, 2, k), rng.integers(0, 5, k))
        out.append(_Cell(np.asarray(t.indices), np.asarray(t.vertices, np.float32), props))
    return out


def _cmn_model(gpu, store):
    spec, D, H, W, arrs, _, _ = K.inputs('cmn')
    return spec, arrs, _model(spec, arrs, store, gpu)


def _reference_flow(cell, spec, arrs, views, nb_views_model, store):
    """celltype_of_sso_nocache :1723-1753 on the downloaded views, float32 on torch-CPU / numpy, the network on the weights the plan
    stores (as in test_cmn_geometry).  The subsets come from the literal restatement of the reference's text; the ratios, the
    certainty and the vote are this package's host functions, which is sound only because tests/test_viewnet_cpu.py pins them bit for
    bit (the certainty to float32 rounding) to the reference's own functions (golden g29): what this comparison is independent of is
    the device code."""
    from syconn_amd.handler.prediction import certainty_estimate
    from syconn_amd.reps.super_segmentation_helper import syn_sign_ratio_celltype
    inp = R.modelinput_literal(views, nb_views_model)
    ratio = np.array([[syn_sign_ratio_celltype(*cell.syn_props, comp_types=[1, ]), syn_sign_ratio_celltype(*cell.syn_props, comp_types=[0, ])]] * len(inp))
    res = R.forward32_stored(spec, arrs, np.ascontiguousarray(inp), ratio, store)
    raw = res.copy()
    res[:, 1] += res[:, 6]
    res = np.delete(res, [6], axis=1)
    clf = np.argmax(res, axis=1)
    major_dec = np.zeros(7)
    for ii in range(len(major_dec)):
        major_dec[ii] = np.sum(clf == ii)
    major_dec /= np.sum(major_dec)
    return np.argmax(major_dec), res, certainty_estimate(res, is_logit=True), raw


def _certainty_bound(res, T):
    """What a change of every merged logit by at most 2 T (two raw logits of error T each are added) can do to the certainty
    1 - H(mean softmax) / ln C: a softmax moves by at most a factor e^(+-2 d) per class (numerator e^(+-d), denominator e^(-+d)), so
    every mean probability p moves to within [p e^(-2 d), p e^(2 d)], d = 2 T; H changes by at most sum over classes of the largest
    change of -p ln p over that interval, found by evaluating the three candidates (both ends and the stationary point 1 / e)."""
    d = 2 * T
    z = res.astype(np.float64) - res.max(1, keepdims=True)
    p = (np.exp(z) / np.exp(z).sum(1, keepdims=True)).mean(0)
    lo, hi = p * np.exp(-2 * d), np.minimum(p * np.exp(2 * d), 1.0)
    ent = lambda q: np.where(q > 0, -q * np.log(np.maximum(q, 1e-300)), 0.0)
    cand = [ent(lo), ent(hi), np.where((lo <= np.exp(-1)) & (np.exp(-1) <= hi), np.exp(-1), ent(p))]
    dev = np.max([np.abs(c - ent(p)) for c in cand], axis=0)
    return dev.sum() / np.log(len(p))


def _compare_with_flow(cell, spec, arrs, views, got, store, tag):
    pred, res, cert = got
    rpred, rres, rcert, _ = _reference_flow(cell, spec, arrs, views, 20, store)
    assert res.shape == rres.shape and res.shape[1] == 6 and res.dtype == np.float32
    d = np.abs(res - rres).max()
    print(f'{tag} {store}: {len(views)} locations, {len(res)} samples, |probas - float32| {d:.5f} (2 T = {2 * K.T[store]:.5f}), '
          f'certainty {cert:.6f} vs {rcert:.6f}')
    assert d <= 2 * K.T[store]      # column 1 is the sum of two logits
    s = np.sort(rres, axis=1)
    safe = (s[:, -1] - s[:, -2]) > 4 * K.T[store]
    assert np.array_equal(res.argmax(1)[safe], rres.argmax(1)[safe])
    # the vote: the safe samples' classes are fixed; if the lead of their winner exceeds the number of unsafe samples, those cannot
    # change the majority (nor tie it) and the prediction must be the reference's
    votes = np.sort(np.bincount(rres.argmax(1)[safe], minlength=6))
    decided = votes[-1] - votes[-2] > (~safe).sum()
    print(f'{tag} {store}: {int(safe.sum())} of {len(safe)} samples safe, prediction {"" if decided else "not "}decided by them')
    assert safe.sum() >= 1
    if decided:
        assert pred == rpred
    assert abs(cert - rcert) <= _certainty_bound(rres, K.T[store]) + 1e-6
    assert cell.attr_dict['celltype_cnn_e3'] == pred and cell.saved['celltype_cnn_e3_certainty'] == cert
    assert np.array_equal(cell.attr_dict['celltype_cnn_e3_probas'], res)


@pytest.mark.parametrize('store', K.STORES)
def test_celltype_end_to_end(gpu, cells, store):
    """celltype_of_sso_nocache (locations, render on the device, sample table, view net, vote) against the reference's flow restated on
    the downloaded views: logits within T, the same class wherever the float32 margin allows, the certainty within what T allows."""
    from syconn_amd.proc.rendering import render_sso_coords
    from syconn_amd.reps.super_segmentation_helper import celltype_of_sso_nocache
    spec, arrs, model = _cmn_model(gpu, store)
    ws, nb_views, cw = (256, 128), 2, 4000.0      # locations every 1333 nm: a few dozen on this cell
    cell = cells[0]
    got = celltype_of_sso_nocache(cell, model, ws, nb_views, cw, device=gpu)
    views = render_sso_coords(cell, cell._sample_locations, ws=ws, comp_window=cw, nb_views=nb_views, add_cellobjects=True, device=gpu)
    assert views.shape[1:] == (4, nb_views, 128, 256) and 20 <= len(views) <= 200
    _compare_with_flow(cell, spec, arrs, views, got, store, 'cell 0')
    # the method form: the window from the config, updated by view_props
    from syconn_amd.reps.super_segmentation_object import certainty_celltype, predict_celltype_multiview
    again = predict_celltype_multiview(cell, model, onthefly_views=True, view_props=dict(comp_window=cw), device=gpu)
    assert again[0] == got[0] and np.array_equal(again[1], got[1]) and again[2] == got[2] == certainty_celltype(cell)
    with pytest.raises(NotImplementedError):
        predict_celltype_multiview(cell, model, model_tnet=object())


@pytest.mark.parametrize('store', K.STORES)
def test_celltype_padding_draw(gpu, cells, store, monkeypatch):
    """Fewer than 20 views (7 locations x 2): the reference pads with a random draw; views passed in as a device tensor."""
    from syconn_amd import global_params
    from syconn_amd.handler.multiviews import generate_rendering_locs
    from syconn_amd.proc.rendering import render_sso_coords
    from syconn_amd.reps.super_segmentation_helper import predict_sso_celltype
    monkeypatch.setitem(global_params.config._entries, 'syntype_avail', True)
    spec, arrs, model = _cmn_model(gpu, store)
    cell = cells[1]
    locs = generate_rendering_locs(np.asarray(cell.mesh[1]).reshape(-1, 3), 4000.0 / 3, device=gpu)[:7]
    assert len(locs) == 7
    kw = dict(ws=(256, 128), comp_window=4000.0, nb_views=2, add_cellobjects=True, device=gpu)
    views_d = render_sso_coords(cell, locs, return_device=True, **kw)
    assert isinstance(views_d, torch.Tensor) and views_d.is_cuda
    got = predict_sso_celltype(cell, model, overwrite=True, views=views_d)
    assert got[1].shape == (1, 6)
    assert predict_sso_celltype(cell, model, views=views_d) is None      # overwrite=False: the key exists
    _compare_with_flow(cell, spec, arrs, render_sso_coords(cell, locs, **kw), got, store, 'cell 1 (7 locations)')


@pytest.mark.parametrize('store', K.STORES)
def test_celltypes_table_equals_single_calls(gpu, cells, store, monkeypatch):
    """Three cells through one pass (launch sets of 2 samples cut across the cells) = three single calls, bit for bit."""
    from syconn_amd import global_params
    from syconn_amd.handler.multiviews import generate_rendering_locs
    from syconn_amd.proc.rendering import render_sso_coords
    from syconn_amd.reps.super_segmentation_helper import predict_celltypes_table, predict_sso_celltype
    monkeypatch.setitem(global_params.config._entries, 'syntype_avail', True)
    spec, arrs, model = _cmn_model(gpu, store)
    kw = dict(ws=(256, 128), comp_window=4000.0, nb_views=2, add_cellobjects=True, device=gpu, return_device=True)
    trio = [cells[0], cells[1], _Cell(cells[1].mesh[0], cells[1].mesh[1], ([], [], []))]
    views = []
    for k, (c, take) in enumerate(zip(trio, (slice(0, 23), slice(0, 11), slice(3, 8)))):
        locs = generate_rendering_locs(np.asarray(c.mesh[1]).reshape(-1, 3), 4000.0 / 3, device=gpu)[take]
        views.append(render_sso_coords(c, locs, **kw))
    assert [len(v) for v in views] == [23, 11, 5]      # 2 + 1 + 1 samples; the last one padded
    table = predict_celltypes_table(trio, model, views=views, bs=2, ids=[7, 8, 9])
    assert table.sample_begin.tolist() == [0, 2, 3, 4] and table.probas.shape == (4, 6) and len(table) == 3
    for k, (c, v) in enumerate(zip(trio, views)):
        pred, res, cert = predict_sso_celltype(c, model, overwrite=True, views=v)
        assert table.pred[k] == pred and table.certainty[k] == cert and np.array_equal(table.probas_of(k), res)
    from syconn_amd.exec.exec_inference import run_celltype_prediction
    same = run_celltype_prediction(trio, model, views=views, ids=[7, 8, 9], bs=3)      # config: 20 views per sample, syntype_avail (patched)
    assert np.array_equal(same.probas, table.probas) and np.array_equal(same.pred, table.pred) and np.array_equal(same.certainty, table.certainty)
    d = table.as_dict()
    assert sorted(d) == [7, 8, 9] and np.array_equal(d[9]['celltype_cnn_e3_probas'], table.probas_of(2))


def test_forward_timed(gpu):
    """sd_viewnet_forward_timed: the same logits, bit for bit, and one time per layer kernel and one for the head."""
    from syconn_amd import _dev as dv
    from syconn_amd import _lib as L
    spec, D, H, W, arrs, views, scal = K.inputs('a')
    m = _model(spec, arrs, 'f16', gpu)
    want = m.predict_proba((views, scal))
    n = views.shape[0]
    vd, sc, tb = torch.from_numpy(views).to(gpu), torch.from_numpy(scal).to(gpu), torch.arange(n * D, dtype=torch.int32, device=gpu)
    ws = dv.scratch('sd_viewnet_workspace_bytes', gpu, m._h, n, D, H, W)
    lg, fl = torch.zeros((n, spec.n_classes), device=gpu), torch.zeros(2, dtype=torch.int32, device=gpu)
    ms = (C.c_float * (len(spec.layers) + 2))(*([-1.0] * (len(spec.layers) + 2)))
    args = dv.pointers((m._h, vd, n * D, D, H, W, tb, n, D, sc, lg, ws, ws.numel(), fl))
    L.check(L.load().sd_viewnet_forward_timed(*args, dv.stream(gpu), ms), 'sd_viewnet_forward_timed')
    assert np.array_equal(lg.cpu().numpy(), want) and fl.cpu().tolist() == [0, 0]
    assert all(0 <= t < 1000 for t in list(ms)[:-1]) and ms[len(spec.layers) + 1] == -1.0      # n_layers + 1 values, nothing behind them
    assert L.load().sd_viewnet_forward_timed(*args, dv.stream(gpu), None) == L.SD_ERR_INVALID
