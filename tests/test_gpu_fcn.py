"""The FCN semantic-segmentation network on the device (syconn_amd/csrc/sd_fcn.hip): every stored tensor against the float64 one-op
reference on the device's own stored inputs (tests/_fcn_ref.py), the labels as one op, ties, logits and labels end to end against the
float32 restatement, the label layout, launch sets, guard bands, argument checks, the fp16 range flag and the compartment chain."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import _fcn_cases as K
import _fcn_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(spec, arrs, store, gpu, bs=64):
    from syconn_amd.handler.prediction import SemsegViewModel
    return SemsegViewModel(spec, R.state_dict_of(spec, arrs), act_dtype=store, bs=bs, device=gpu)


def _step_checks(m, spec, arrs, store, planes, logits, tag):
    """Every op of the last forward against StepRef on the device's own stored input; the labels against the float64 classifier on the
    stored last tensor.  -> (largest |dev - ref| / bound, labels the one-op check expects, mask of the pixels it covers)."""
    sr = R.StepRef(spec, arrs, store)
    assert m.num_ops == sr.n_ops() == spec.n_ops
    dev = [m.read_buffer(i) for i in range(sr.n_ops())]
    shapes = spec.shapes(planes.shape[2], planes.shape[3])
    share, c = 0.0, K.C[store]

    def check(i, ref, S, bound):
        nonlocal share
        d = torch.from_numpy(dev[i]).double()
        assert d.shape == ref.shape, (i, d.shape, ref.shape)
        assert torch.isfinite(d).all()
        ratio = ((d - ref).abs() / bound(ref, S)).max().item()
        print(f'{tag} {store}: op {i} |dev - ref| is {ratio:.3f} of the bound')
        assert ratio <= 1, f'op {i}: |dev - ref| is {ratio:.3f} of the bound'
        share = max(share, ratio)

    stored_bound = lambda ref, S: R.bound_stored(ref, S, c, store)
    x = np.ascontiguousarray(planes.transpose(0, 2, 3, 1))
    for i in range(sr.nc):
        assert dev[i].shape[1:] == (shapes[i][1], shapes[i][2], shapes[i][0])
        check(i, *sr.conv(i, x), stored_bound)
        x = dev[i]
    for d in range(5):
        k = sr.skip_of(d)
        check(sr.nc + d, *sr.deconv(d, x, dev[k] if k is not None else None), stored_bound)
        x = dev[sr.nc + d]
    ref, S = sr.classify(x)
    check(sr.nc + 5, ref, S, lambda r, s: R.bound_f32(r, s, c))
    assert np.array_equal(dev[-1], logits)      # the last op's buffer is the logits
    # the labels as one op: pixels whose float64 top-2 margin is below twice the fp32 one-op bound are left out
    b = R.bound_f32(ref, S, c).max(1).values.numpy()
    covered = R.top2_margin(ref.numpy()) >= 2 * b
    return share, ref.numpy().argmax(1), covered


ONE_OP = [('v', 'shapes'), ('s', 'shapes'), ('s', 'zeros'), ('s', 'ones'), ('s', 'checker'), ('o1', 'shapes'), ('o2', 'shapes'), ('w', 'shapes'),
          ('g', 'shapes')]


@pytest.mark.parametrize('store', K.STORES)
@pytest.mark.parametrize('name, mode', ONE_OP)
def test_steps_and_labels(gpu, name, mode, store):
    """Stored tensors one op at a time, the labels as one op, and (v, s, g) the logits -- fp16: and the labels -- end to end."""
    spec, arrs, views = K.inputs(name, mode)
    planes = R.planes_of(views)
    m = _model(spec, arrs, store, gpu)
    logits = m.predict_proba(planes)
    assert logits.shape == (len(planes), spec.n_class) + planes.shape[2:] and logits.dtype == np.float32
    share, want, covered = _step_checks(m, spec, arrs, store, planes, logits, f'{name}:{mode}')
    labels = m.predict_labels(views)
    assert labels.shape == (views.shape[0], 1, views.shape[2]) + views.shape[3:] and labels.dtype == np.uint8
    lab = labels[:, 0].reshape(want.shape)      # (n_loc, nb_views, H, W) -> planes
    assert np.array_equal(lab, logits.argmax(1))      # the device's argmax is numpy's on its own logits, first maximum included
    left = 1 - covered.mean()
    print(f'{name}:{mode} {store}: largest share of the bound {share:.3f}; one-op label check leaves out {100 * left:.4f} % of the pixels')
    assert left <= 1e-3
    assert np.array_equal(lab[covered], want[covered])
    if mode == 'shapes' and name in K.E2E:
        l32 = K.restatement(name, store)
        T = K.T[store][name]
        d = np.abs(logits - l32).max()
        print(f'{name} {store}: |logits - float32 restatement| {d:.5f} of T = {T:.5f}')
        assert d <= T
        if store == 'f16':
            safe = R.top2_margin(l32) >= 2 * T
            print(f'{name} f16: end-to-end labels compared on {100 * safe.mean():.2f} % of the pixels')
            assert np.array_equal(lab[safe], l32.argmax(1)[safe])


@pytest.mark.parametrize('store', K.STORES)
def test_ties(gpu, store):
    """Zero classifier weights: every pixel is a tie of the biases; the lowest index among the maximal biases is the label everywhere."""
    spec, arrs, views = K.inputs('s')
    arrs = list(arrs)
    arrs[-2] = np.zeros_like(arrs[-2])
    arrs[-1] = np.array([0.25, 1.5, -3.0, 1.5, 1.5], np.float32)
    m = _model(spec, arrs, store, gpu)
    labels = m.predict_labels(views)
    assert (labels == 1).all()
    logits = m.predict_proba(R.planes_of(views))
    assert np.array_equal(logits, np.broadcast_to(arrs[-1].reshape(1, -1, 1, 1), logits.shape))


@pytest.mark.parametrize('store', K.STORES)
def test_layout_and_launch_sets(gpu, store):
    """(n_loc, C, nb_views, H, W) in, (n_loc, 1, nb_views, H, W) out through the drop-in, host and device; planes in several launch sets
    equal one launch set bit for bit; a plane has the same bits wherever it stands."""
    from syconn_amd.reps.super_segmentation_helper import predict_views_semseg
    spec, arrs, _ = K.inputs('o2')
    views = R.synthetic_views(11, 3, 1, 2, 32, 32)
    m = _model(spec, arrs, store, gpu)
    one = predict_views_semseg(views, m, batch_size=64)
    assert one.shape == (3, 1, 2, 32, 32) and one.dtype == np.uint8 and len(np.unique(one)) == 2
    planes = R.planes_of(views)
    logits = m.predict_proba(planes, bs=64)
    assert np.array_equal(one, logits.argmax(1).reshape(3, 2, 32, 32)[:, None])
    for bs in (1, 4, 5):
        assert np.array_equal(predict_views_semseg(views, m, batch_size=bs), one), bs
        assert np.array_equal(m.predict_proba(planes, bs=bs), logits), bs
    dev = predict_views_semseg(torch.from_numpy(views).to(gpu), m)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), one)
    # location 2, view 1 alone
    assert np.array_equal(m.predict_labels(np.ascontiguousarray(views[2:3, :, 1:2]))[0, 0, 0], one[2, 0, 1])
    # float32 views that ARE uint8 / 255 are taken, with the same bits; others are refused
    assert np.array_equal(m.predict_proba(planes.astype(np.float32) / 255.), logits)
    with pytest.raises(NotImplementedError):
        m.predict_proba(planes.astype(np.float32) / 254.)


@pytest.mark.parametrize('name', [g[0] for g in K.GOLDEN])
def test_golden_labels(gpu, name):
    """``predict_labels`` / the drop-in ``predict_views_semseg`` against the reference's own function (golden g30), layout included:
    equal wherever the float32 restatement's top-2 margin is at least 2 T (fp16; tests/test_fcn_cpu.py::test_golden_semseg: the golden
    model's weights are exact in the storage type and at most 10 % are left out).  bf16: the layout only -- its labels are covered
    by the logit bound and the one-op check."""
    from syconn_amd.reps.super_segmentation_helper import predict_views_semseg
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g30_semseg.npz'))
    spec, arrs, views = K.golden_inputs(name)
    want = g[f'{name}_labels']
    n_loc, _, nb_views, H, W = views.shape
    l32 = R.forward32(spec, arrs, R.planes_of(views))
    safe = (R.top2_margin(l32) >= 2 * K.GOLDEN_T['f16'][name]).reshape(n_loc, nb_views, H, W)[:, None]
    got = predict_views_semseg(views, _model(spec, arrs, 'f16', gpu), batch_size=4)
    assert got.shape == want.shape == (n_loc, 1, nb_views, H, W) and got.dtype == np.uint8
    print(f'golden {name}: compared on {100 * safe.mean():.2f} % of the pixels, {int((got != want).sum())} of all differ')
    assert safe.mean() >= 0.9 and np.array_equal(got[safe], want[safe])
    assert predict_views_semseg(views, _model(spec, arrs, 'bf16', gpu)).shape == want.shape


def _layout(spec, n, H, W):
    """The workspace layout of syconn_amd/csrc/sd_fcn_plan.cpp: every stored tensor but the logits, n h w cp fp16 / bf16, each rounded up
    to 256 bytes.  -> [(offset, used bytes)], total."""
    out, off = [], 0
    for c, h, w in spec.shapes(H, W)[:-1]:
        used = n * h * w * (-(-c // 8) * 8) * 2
        out.append((off, used))
        off += -(-used // 256) * 256
    return out, off


@pytest.mark.parametrize('store', K.STORES)
def test_guard_bands(gpu, store):
    """Nothing is written behind the workspace, the labels, the logits or a stored tensor."""
    from syconn_amd import _dev as dv
    from syconn_amd import _lib as L
    spec, arrs, views = K.inputs('s')
    n, H, W = 3, 64, 96
    m = _model(spec, arrs, store, gpu)
    want = m.predict_proba(R.planes_of(views))
    ranges, total = _layout(spec, n, H, W)
    assert L.load().sd_fcn_workspace_bytes(m._h, n, H, W) == total
    guard = 4096
    ws = torch.full((total + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    logits = torch.full((n * spec.n_class * H * W + 64,), -7.0, dtype=torch.float32, device=gpu)
    labels = torch.full((n * H * W + 64,), 99, dtype=torch.uint8, device=gpu)
    flags = torch.full((4,), 9, dtype=torch.int32, device=gpu)
    dv.call('sd_fcn_forward', gpu, m._h, torch.from_numpy(views).to(gpu), n, 1, H, W, 0, n, labels, logits, ws, total, flags)
    torch.cuda.synchronize(gpu)
    assert np.array_equal(logits[:want.size].cpu().numpy().reshape(want.shape), want)
    assert np.array_equal(labels[:n * H * W].cpu().numpy().reshape(n, H, W), want.argmax(1))
    assert (logits[want.size:] == -7.0).all() and (labels[n * H * W:] == 99).all() and (ws[total:] == 0xA5).all()
    assert flags.cpu().tolist() == [0, 9, 9, 9]
    ends = [o for o, _ in ranges[1:]] + [total]
    for (off, used), end in zip(ranges, ends):
        assert (ws[off + used:end] == 0xA5).all(), (off, used, end)


def test_argument_checks(gpu):
    from syconn_amd import _dev as dv
    from syconn_amd import _lib as L
    from syconn_amd.cnn.fcn_spec import FcnSpec
    from syconn_amd.handler.prediction import SemsegViewModel
    spec, arrs, views = K.inputs('s')
    sd = R.state_dict_of(spec, arrs)
    with pytest.raises(ValueError, match='act_dtype'):
        SemsegViewModel(spec, sd, act_dtype='f32', device=gpu)
    with pytest.raises(ValueError, match='bs must be positive'):
        SemsegViewModel(spec, sd, bs=0, device=gpu)
    with pytest.raises(ValueError, match='has shape'):
        SemsegViewModel(spec, {k: (v[:-1] if k == 'bn2.bias' else v) for k, v in sd.items()}, device=gpu)
    for bad in (dict(in_channels=5), dict(blocks=((8,),) * 4), dict(blocks=((8,),) * 4 + ((8, 8, 8, 8),)), dict(blocks=((8,),) * 4 + ((513,),)),
                dict(n_class=17), dict(n_class=0), dict(dec_last=0)):
        kw = dict(in_channels=3, blocks=((8,),) * 5, dec_last=8, n_class=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            FcnSpec(**kw)
    m = SemsegViewModel(spec, sd, device=gpu)
    planes = R.planes_of(views)
    calls = {
        'views have 2 channels': lambda: m.predict_proba(planes[:, :2]),
        r'uint8 array / tensor \(N, C, H, W\)': lambda: m.predict_proba(views),
        r'uint8 array / tensor \(n_loc': lambda: m.predict_labels(planes),
        'uint8 array': lambda: m.predict_proba(planes.astype(np.int16)),
        'multiples of 32': lambda: m.predict_proba(planes[:, :, :48]),
        'multiples of 32.*64 x 80': lambda: m.predict_proba(planes[:, :, :, :80]),
        'bs must be positive': lambda: m.predict_proba(planes, bs=0),
    }
    for msg, call in calls.items():
        with pytest.raises(ValueError, match=msg):
            call()
    # the C entries themselves
    lib = L.load()
    w = np.concatenate([a.ravel() for a in arrs]).astype(np.float32)
    wp = w.ctypes.data_as(C.POINTER(C.c_float))
    flat = [c for b in spec.blocks for c in b]
    i32 = lambda v: (C.c_int32 * len(v))(*v)
    good = [3, i32(flat), i32([len(b) for b in spec.blocks]), spec.dec_last, spec.n_class, wp, w.size, L.SD_F16]
    h = C.c_void_p()
    for pos, val, msg in ((0, 0, 'in_channels'), (0, 5, 'in_channels'), (1, None, 'null'), (2, None, 'null'), (5, None, 'null'),
                          (2, i32([2, 1, 3, 2, 0]), 'block 4: 1 to 3'), (2, i32([2, 1, 4, 2, 1]), 'block 2: 1 to 3'),
                          (1, i32([12, 20, 24, 40, 40, 513, 72, 72, 72]), 'convolution 5: channels'), (1, i32([0] + flat[1:]), 'convolution 0: channels'),
                          (3, 0, 'dec_last'), (3, 513, 'dec_last'), (4, 0, 'n_class'), (4, 17, 'n_class'), (6, w.size - 1, 'weights hold'),
                          (7, L.SD_F32, 'act_dtype')):
        args = list(good)
        args[pos] = val
        assert lib.sd_fcn_create(*args, C.byref(h)) == L.SD_ERR_INVALID and not h.value
        assert msg in lib.sd_last_error().decode(), (msg, lib.sd_last_error())
    assert lib.sd_fcn_create(*good, None) == L.SD_ERR_INVALID
    big = w.copy()
    big[5] = 65520.0      # the first value that rounds to an fp16 infinity
    assert lib.sd_fcn_create(*good[:5], big.ctypes.data_as(C.POINTER(C.c_float)), w.size, L.SD_F16, C.byref(h)) == L.SD_ERR_INVALID
    assert 'overflows the storage type' in lib.sd_last_error().decode()
    n, H, W = 3, 64, 96
    vd = torch.from_numpy(views).to(gpu)
    ws = dv.scratch('sd_fcn_workspace_bytes', gpu, m._h, n, H, W)
    lb, lg, fl = torch.zeros((n, H, W), dtype=torch.uint8, device=gpu), torch.zeros((n, spec.n_class, H, W), device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu)
    good = [m._h, vd, n, 1, H, W, 0, n, lb, lg, ws, ws.numel(), fl]
    dv.call('sd_fcn_forward', gpu, *good)
    want = lb.cpu().numpy()
    args = list(good)
    args[9] = None      # the logits are optional
    lb.zero_()
    dv.call('sd_fcn_forward', gpu, *args)
    assert np.array_equal(lb.cpu().numpy(), want)
    for pos, val, msg in ((0, None, 'null'), (1, None, 'null'), (8, None, 'null'), (10, None, 'null'), (12, None, 'null'),
                          (11, ws.numel() - 1, 'workspace smaller'), (3, 0, 'multiple of nb_views'), (3, 2, 'multiple of nb_views'),
                          (2, 0, 'multiple of nb_views'), (4, 48, 'multiples of 32'), (5, 100, 'multiples of 32'), (4, 0, 'multiples of 32'),
                          (7, 0, 'n_planes out of range'), (6, 1, 'outside the views'), (6, 3, 'outside the views'), (10, ws[1:], '16-byte aligned')):
        args = list(good)
        args[pos] = val
        with pytest.raises(ValueError, match=msg):
            dv.call('sd_fcn_forward', gpu, *args)
    assert lib.sd_fcn_workspace_bytes(m._h, n, 48, W) == 0 and lib.sd_fcn_workspace_bytes(None, n, H, W) == 0
    assert lib.sd_fcn_num_ops(None) == 0 and lib.sd_fcn_num_ops(m._h) == 15
    dims = (C.c_int32 * 4)()
    for idx in (-1, 15):
        assert lib.sd_fcn_read_buffer(m._h, idx, ws.data_ptr(), lg.data_ptr(), n, H, W, None, dims, None) == L.SD_ERR_INVALID
    assert lib.sd_fcn_read_buffer(m._h, 1, ws.data_ptr(), None, n, H, W, None, dims, None) == 0 and list(dims) == [n, 32, 48, 20]
    assert lib.sd_fcn_read_buffer(m._h, 14, ws.data_ptr(), None, n, H, W, None, dims, None) == 0 and list(dims) == [n, 5, 64, 96]
    out = np.empty(1, np.float32)
    assert lib.sd_fcn_read_buffer(m._h, 14, ws.data_ptr(), None, n, H, W, out.ctypes.data_as(C.POINTER(C.c_float)), dims, None) == L.SD_ERR_INVALID
    flags_out = (C.c_int32 * 1)(7)
    assert lib.sd_fcn_overflow(m._h, fl.data_ptr(), None, flags_out) == 0 and flags_out[0] == 0
    assert lib.sd_fcn_overflow(m._h, None, None, flags_out) == L.SD_ERR_INVALID


def test_f16_overflow_flag(gpu):
    """First-layer weights scaled so that every STORED weight stays finite and the largest stored activation of layer 0 passes 65504:
    fp16 storage raises and names bf16; bf16 storage runs (its labels are finite arithmetic)."""
    from syconn_amd import _lib as L
    spec, _, views = K.inputs('s')
    planes = R.planes_of(views)
    arrs = R.make_weights(spec, 31, 64, 96, gain=30000.0)
    assert np.abs(arrs[0]).max() < 40000      # inside fp16: the plan would refuse a weight that rounds to infinity
    top = float(R.StepRef(spec, arrs, 'f16').conv(0, planes.transpose(0, 2, 3, 1))[0].max())
    assert 70000 < top < 400000, top
    with pytest.raises(L.ActivationOverflowError, match="act_dtype='bf16'"):
        _model(spec, arrs, 'f16', gpu).predict_labels(views)
    m = _model(spec, arrs, 'bf16', gpu)
    assert np.isfinite(m.predict_proba(planes)).all()
    assert np.isfinite(m.read_buffer(0)).all() and m.read_buffer(0).max() > 65520


def test_forward_timed(gpu):
    """sd_fcn_forward_timed: the same labels and logits, bit for bit, and one time per op."""
    from syconn_amd import _dev as dv
    from syconn_amd import _lib as L
    spec, arrs, views = K.inputs('o2')
    m = _model(spec, arrs, 'f16', gpu)
    want = m.predict_proba(R.planes_of(views))
    vd = torch.from_numpy(views).to(gpu)
    ws = dv.scratch('sd_fcn_workspace_bytes', gpu, m._h, 1, 32, 32)
    lb, lg, fl = torch.zeros((1, 32, 32), dtype=torch.uint8, device=gpu), torch.zeros((1, 2, 32, 32), device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu)
    n_ops = spec.n_ops
    ms = (C.c_float * (n_ops + 1))(*([-1.0] * (n_ops + 1)))
    args = dv.pointers((m._h, vd, 1, 1, 32, 32, 0, 1, lb, lg, ws, ws.numel(), fl))
    L.check(L.load().sd_fcn_forward_timed(*args, dv.stream(gpu), ms), 'sd_fcn_forward_timed')
    assert np.array_equal(lg.cpu().numpy(), want) and np.array_equal(lb.cpu().numpy(), want.argmax(1)) and fl.cpu().tolist() == [0]
    assert all(0 <= t < 1000 for t in list(ms)[:-1]) and ms[n_ops] == -1.0      # n_ops values, nothing behind them
    assert L.load().sd_fcn_forward_timed(*args, dv.stream(gpu), None) == L.SD_ERR_INVALID


# -- the chain ------------------------------------------------------------------------------------------------------------------------
class _Labels(dict):
    pushed = 0

    def push(self):
        self.pushed += 1


class _Cell:
    view_caching = True
    _sample_locations = None

    def __init__(self, tris, verts):
        self.mesh = (tris, verts)
        self.view_dict = {}
        self._labels = _Labels()

    def label_dict(self, kind):
        assert kind == 'vertex'
        return self._labels

    def load_mesh(self, name):
        # 'mi': a part of the cell's own surface stands in for an organelle; the others are empty (a channel of 255)
        if name == 'mi':
            return (self.mesh[0][:len(self.mesh[0]) // 3], self.mesh[1])
        return (np.zeros(0, np.uint32), np.zeros((0, 3), np.float32))


@pytest.fixture(scope='module')
def cell(gpu):
    spec_ = importlib.util.spec_from_file_location('views_probe', os.path.join(ROOT, 'tools', 'views_probe.py'))
    probe = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(probe)
    from syconn_amd.proc import meshes
    t = meshes.find_meshes_table(probe.make_cell((160, 128, 96), 1), (0, 0, 0), scaling=(50.,) * 3, meshing_props={'normals': False}, device=gpu)
    return _Cell(np.asarray(t.indices), np.asarray(t.vertices, np.float32))


def test_semseg_of_sso_nocache(gpu, cell):
    """Locations, raw views, labels, index views and the vertex vote on a synthetic cell, against the same chain with the float32
    restatement's labels fed into semseg2mesh (k = 0: every vertex keeps its own vote): equal vertex labels except at vertices that see
    a pixel the restatement leaves out (top-2 margin below 2 T of the spiness geometry)."""
    from syconn_amd.proc.rendering import render_sso_coords, render_sso_coords_index_views
    from syconn_amd.reps.super_segmentation_helper import semseg2mesh, semseg_of_sso_nocache
    from syconn_amd.reps.super_segmentation_object import predict_semseg
    spec, arrs, _ = K.inputs('g')
    m = _model(spec, arrs, 'f16', gpu, bs=10)
    ws, nb_views, cw = (256, 128), 2, 8000.0
    from syconn_amd.handler.multiviews import generate_rendering_locs
    locs = generate_rendering_locs(np.asarray(cell.mesh[1]).reshape(-1, 3), cw / 3, device=gpu)[:3]
    cell._sample_locations = [locs]
    got = semseg_of_sso_nocache(cell, m, 'spiness', ws, nb_views, cw, k=0, bs=4, device=gpu)
    assert cell.label_dict('vertex')['spiness'] is got and cell._labels.pushed == 1 and len(got) == len(cell.mesh[1].reshape(-1, 3))
    views = render_sso_coords(cell, locs, ws=ws, comp_window=cw, nb_views=nb_views, add_cellobjects=True, device=gpu)
    assert views.shape == (3, 4, 2, 128, 256)
    index_views = render_sso_coords_index_views(cell, locs, ws=ws, comp_window=cw, nb_views=nb_views, device=gpu)
    l32 = R.forward32_stored(spec, arrs, R.planes_of(views), 'f16')
    ref_labels = l32.argmax(1).astype(np.uint8).reshape(3, 2, 128, 256)[:, None]
    left_out = (R.top2_margin(l32) < 2 * K.T['f16']['g']).reshape(3, 2, 128, 256)[:, None]
    # the labels themselves, through the method form
    lab = predict_semseg(cell, m, 'spiness', nb_views=nb_views, views=views)
    assert cell.view_dict['spiness'] is lab and np.array_equal(lab[~left_out], ref_labels[~left_out])
    want = semseg2mesh(cell, 'spiness', k=0, index_views=index_views, semseg_views=ref_labels, device=gpu)[3]
    # background and unpredicted labels depend on max(labels): the same in both runs if every class occurs among the safe pixels
    assert lab.max() == ref_labels.max()
    touched = np.unique(index_views[left_out])
    touched = touched[touched < len(got)]
    same = np.ones(len(got), bool)
    same[touched] = False
    print(f'chain: {len(got)} vertices, {len(touched)} see a left-out pixel, {100 * left_out.mean():.2f} % of the pixels left out')
    assert same.sum() > 0.5 * len(got)
    assert np.array_equal(np.asarray(got)[same], np.asarray(want)[same])
    with pytest.raises(NotImplementedError):
        predict_semseg(cell, m, 'spiness')


class _SkelCell(_Cell):
    """A cell with a skeleton: every 400th mesh vertex (in voxels) as a chain of nodes."""
    scaling = np.array([50., 50., 50.])

    def __init__(self, ident, tris, verts, broken=False):
        super().__init__(tris, verts)
        self.id, self.broken, self.skeleton, self.saved = ident, broken, None, 0

    def load_mesh(self, name):
        if self.broken:
            raise RuntimeError('mesh storage not readable')
        return super().load_mesh(name)

    def load_skeleton(self):
        nodes = np.asarray(self.mesh[1]).reshape(-1, 3)[::400] / self.scaling
        self.skeleton = {'nodes': nodes, 'edges': np.stack([np.arange(len(nodes) - 1), np.arange(1, len(nodes))], 1), 'diameters': np.ones(len(nodes))}

    def save_skeleton(self):
        self.saved += 1


def test_exec_table_forms(gpu, cell):
    """run_semsegspiness_prediction and run_semsegaxoness_prediction over cells in memory: the vertex labels are those of
    semseg_of_sso_nocache, the skeleton gets the node labels (spiness) / the three axoness keys, a cell that raises a RuntimeError is
    listed as missing and the others are still done."""
    from syconn_amd.exec.exec_inference import run_semsegaxoness_prediction, run_semsegspiness_prediction
    from syconn_amd.reps.super_segmentation_helper import semseg_of_sso_nocache
    from syconn_amd.reps.super_segmentation_object import semseg_for_coords
    tris, verts = cell.mesh
    mk = lambda: [_SkelCell(7, tris, verts), _SkelCell(8, tris, verts, broken=True), _SkelCell(9, tris, verts)]
    # spiness: the view properties of the config (256 x 128, 2 views, 8000 nm), FCN_VGG13(5)
    spec, arrs, _ = K.inputs('g')
    m = _model(spec, arrs, 'f16', gpu, bs=10)
    cells = mk()
    assert run_semsegspiness_prediction(cells, m, device=gpu) == [8]
    direct = _SkelCell(1, tris, verts)
    want = semseg_of_sso_nocache(direct, m, 'spiness', (256, 128), 2, 8000, k=0, device=gpu)
    for c in (cells[0], cells[2]):
        assert np.array_equal(c.label_dict('vertex')['spiness'], want) and c.saved == 1
        nodes = c.skeleton['nodes']
        assert c.skeleton['spiness'].shape == (len(nodes),) and c.skeleton['spiness'].dtype == np.int32
        assert np.array_equal(c.skeleton['spiness'], semseg_for_coords(c, nodes, 'spiness', k=50, ds_vertices=1, ignore_labels=[4, 5], device=gpu))
        assert set(np.unique(c.skeleton['spiness'])) <= {0, 1, 2, 3}
    assert cells[1].skeleton is None and 'spiness' not in cells[1].label_dict('vertex')
    # axoness: small views in place of the config's 1024 x 512 x 3, FCN_VGG13(6)
    spec6, arrs6, _ = K.inputs('v')
    m6 = _model(spec6, arrs6, 'f16', gpu, bs=5)
    cells = mk()
    props = dict(ws=(64, 32), nb_views=2, comp_window=8000)
    assert run_semsegaxoness_prediction(cells, m6, view_props=props, device=gpu) == [8]
    want = semseg_of_sso_nocache(_SkelCell(2, tris, verts), m6, 'axoness', (64, 32), 2, 8000, k=0, bs=5, device=gpu)
    for c in (cells[0], cells[2]):
        assert np.array_equal(c.label_dict('vertex')['axoness'], want) and c.saved == 1
        n = len(c.skeleton['nodes'])
        assert all(len(c.skeleton[k]) == n for k in ('axoness', 'axoness_avg10000', 'axoness_avg10000_comp_maj'))
        assert set(np.unique(c.skeleton['axoness'])) <= {0, 1, 2}      # boutons (3, 4) are merged into the axon class
