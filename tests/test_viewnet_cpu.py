"""The view network without a GPU: the spec's shape inference and refusals, the host-only plan builder (syconn_amd/csrc/
sd_viewnet_plan.cpp) through tools/viewnet_plan_dump, the numpy side of the cell type step against literal restatements of the reference's
text, the state-dict loader, and the constants the GPU test relies on (tests/_viewnet_cases.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import _viewnet_cases as K
import _viewnet_ref as R
from _unet_step_ref import to_storage
from syconn_amd.cnn.viewnet_spec import CELLTYPE_CMN, VIEWNET_SMALL, ViewNetSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD_ERR_INVALID = -1


# -- spec -------------------------------------------------------------------------------------------------------------------------
def test_named_specs_shapes_and_flops():
    cmn = CELLTYPE_CMN()
    assert cmn.check_geometry(20, 128, 256) == [(62, 126), (29, 61), (13, 29), (5, 13), (2, 6), (1, 3), (1, 3)]
    assert cmn.linear_sizes == (4202, 100, 50, 7) and CELLTYPE_CMN(11, 2).linear_sizes[-1] == 11
    assert VIEWNET_SMALL(2, 0).check_geometry(20, 128, 256)[-1] == (1, 3) and VIEWNET_SMALL(2, 1).linear_sizes == (1861, 50, 30, 2)
    # the count the layer shapes give, written out: computed convolution outputs x taps x cin x cout, + the head
    conv = 20 * (124 * 252 * 25 * 4 * 20 + 58 * 122 * 25 * 20 * 30 + 26 * 58 * 16 * 30 * 40 + 10 * 26 * 16 * 40 * 50 + 4 * 12 * 4 * 50 * 60 +
                 2 * 6 * 60 * 70 + 1 * 3 * 70 * 70)
    assert cmn.macs_per_sample(20, 128, 256) == conv + 4202 * 100 + 100 * 50 + 50 * 7
    assert round(cmn.flops_per_sample(20, 128, 256) / 1e9, 1) == 8.3


@pytest.mark.parametrize('kw, msg', [
    (dict(layers=((20, 3, 2),)), 'k = 3'), (dict(layers=((20, 5, 3),)), 'pool = 3'), (dict(layers=((81, 5, 2),)), 'cout = 81'),
    (dict(layers=()), 'at least one layer'), (dict(in_channels=5), 'in_channels'), (dict(act='gelu'), 'act'), (dict(n_scalar=-1), 'bad head'),
    (dict(fc=(1, 2, 3, 4)), 'bad head')])
def test_spec_refusals(kw, msg):
    base = dict(in_channels=4, layers=((20, 5, 2),), fc_in=10, fc=(8,), n_classes=3)
    base.update(kw)
    with pytest.raises(ValueError, match=msg):
        ViewNetSpec(**base)


def test_shape_refusals():
    cmn = CELLTYPE_CMN()
    with pytest.raises(ValueError, match='layer 5 has an empty output'):
        cmn.check_geometry(20, 127, 256)      # 127 -> 61 -> 28 -> 12 -> 4 -> 1 -> 0
    with pytest.raises(ValueError, match='layer 0 has an empty output'):
        cmn.check_geometry(20, 4, 256)
    with pytest.raises(ValueError, match='flattens to 3990 features, the first Linear takes 4200'):
        cmn.check_geometry(19, 128, 256)
    with pytest.raises(ValueError, match='flattens to 7000'):
        cmn.check_geometry(20, 128, 384)      # 384 -> 190 -> 93 -> 45 -> 21 -> 10 -> 5 -> 5
    with pytest.raises(ValueError):
        cmn.check_geometry(0, 128, 256)


def test_weights_from_state_dict_checks_shapes():
    spec, D, H, W, arrs, _, _ = K.inputs('a')
    sd = R.state_dict_of(spec, arrs)
    got = spec.weights_from_state_dict({'x%d' % i: v for i, v in enumerate(sd.values())})      # the names do not matter, the order does
    assert all(np.array_equal(a, b) for a, b in zip(got, arrs))
    bad = dict(sd)
    bad['seq.1.conv.weight'] = bad['seq.1.conv.weight'][:, :-1]
    with pytest.raises(ValueError, match='seq.1.conv.weight has shape'):
        spec.weights_from_state_dict(bad)
    with pytest.raises(ValueError, match='has 7 tensors'):
        spec.weights_from_state_dict(dict(list(sd.items())[:-1]))
    nan = dict(sd)
    nan['fc.0.bias'] = nan['fc.0.bias'] * float('nan')
    with pytest.raises(ValueError, match='non-finite'):
        spec.weights_from_state_dict(nan)


def test_loader_through_traced_standin(tmp_path):
    """A torch.jit file knows nothing of elektronn3's attribute names: the registration order carries the weights."""
    spec, D, H, W, arrs, views, scal = K.inputs('a')

    class Layer(torch.nn.Module):      # the stated stand-in of Conv3DLayer
        def __init__(self, cin, cout, k, p):
            super().__init__()
            self.conv = torch.nn.Conv3d(cin, cout, (1, k, k))
            self.pool = torch.nn.MaxPool3d((1, p, p))

        def forward(self, x):
            return torch.relu(self.pool(self.conv(x)))

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            cins = [spec.in_channels] + [l[0] for l in spec.layers[:-1]]
            self.seq = torch.nn.Sequential(*[Layer(ci, co, k, p) for ci, (co, k, p) in zip(cins, spec.layers)])
            s = spec.linear_sizes
            self.fc = torch.nn.Sequential(torch.nn.Linear(s[0], s[1]), torch.nn.ReLU(), torch.nn.Linear(s[1], s[2]))

        def forward(self, x, scal):
            x = self.seq(x)
            x = x.view(x.size()[0], -1)
            return self.fc(torch.cat((x, scal), 1))

    net = Net()
    with torch.no_grad():
        for p, a in zip(net.parameters(), arrs):
            p.copy_(torch.from_numpy(a))
    x = torch.from_numpy(views).float() / 255 - 0.5
    path = str(tmp_path / 'model.pts')
    torch.jit.trace(net, (x, torch.from_numpy(scal))).save(path)
    loaded = torch.jit.load(path, map_location='cpu')
    got = spec.weights_from_state_dict(loaded.state_dict())
    assert all(np.array_equal(a, b) for a, b in zip(got, arrs))
    # ... and the restatement is that module
    with torch.no_grad():
        want = loaded(x, torch.from_numpy(scal)).numpy()
    assert np.allclose(R.forward32(spec, arrs, views, scal), want, rtol=0, atol=1e-5)


# -- the host-only plan -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def plan_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('viewnet_plan_dump') / 'viewnet_plan_dump')
    hipcc = '/opt/rocm/bin/hipcc'
    assert os.path.isfile(hipcc), 'hipcc is needed to build tools/viewnet_plan_dump.cpp'
    subprocess.run([hipcc, '-O2', '-std=c++17', os.path.join(ROOT, 'syconn_amd', 'csrc', 'sd_viewnet_plan.cpp'),
                    os.path.join(ROOT, 'tools', 'viewnet_plan_dump.cpp'), '-o', exe], check=True, timeout=600)
    return exe


def _write_net(path, layers, sizes, in_channels, n_scalar, act, floats):
    floats = np.asarray(floats, np.float32)
    with open(path, 'wb') as f:
        f.write(b'SDVNET1\0' + struct.pack('<5iq', len(layers), len(sizes) - 1, in_channels, n_scalar, act, floats.size))
        f.write(np.asarray(layers, np.int32).tobytes() + np.asarray(sizes, np.int32).tobytes() + floats.tobytes())


def _spec_net(path, spec, arrs):
    _write_net(path, spec.layers, spec.linear_sizes, spec.in_channels, spec.n_scalar, 0 if spec.act == 'relu' else 1,
               np.concatenate([a.ravel() for a in arrs]))


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd', 'cmn'])
@pytest.mark.parametrize('store', K.STORES)
def test_packing_round_trip(plan_dump, tmp_path, name, store):
    """Fragment order, channel and K padding, the first layer's fold: read back by the lane map, the blob is the input with the
    convolution weights rounded to the storage type and nothing else; every padding element is zero."""
    spec, D, H, W, arrs, _, _ = K.inputs(name)
    _spec_net(tmp_path / 'n.bin', spec, arrs)
    out = _run(plan_dump, tmp_path / 'n.bin', '--dtypes', store, '--unpack', tmp_path / 'u.bin')
    assert out[0].startswith(f'dtype {store} rc 0')
    pads = [l for l in out if l.startswith('unpack layer')]
    assert len(pads) == len(spec.layers) and all(l.endswith('pad_nonzero 0') for l in pads)
    got = np.fromfile(tmp_path / 'u.bin', np.float32)
    nl = len(spec.layers)
    want = []
    for i, a in enumerate(arrs):
        conv_w = i < 2 * nl and i % 2 == 0
        want.append(to_storage(torch.from_numpy(a), store).float().numpy().ravel() if conv_w else a.ravel())
    want = np.concatenate(want)
    assert got.shape == want.shape
    first_bias = slice(arrs[0].size, arrs[0].size + arrs[1].size)      # b - 0.5 sum(w) is rounded to float32 once: half an ulp of it
    tol = np.zeros_like(want)
    tol[first_bias] = 2.0 ** -23 * (np.abs(arrs[1]) + 0.5 * np.abs(arrs[0]).reshape(len(arrs[1]), -1).sum(1))
    assert (np.abs(got - want) <= tol).all()
    assert np.array_equal(np.delete(got, np.r_[first_bias]), np.delete(want, np.r_[first_bias]))


def test_plan_fields_and_workspace(plan_dump, tmp_path):
    spec, D, H, W, arrs, _, _ = K.inputs('cmn')
    _spec_net(tmp_path / 'n.bin', spec, arrs)
    out = _run(plan_dump, tmp_path / 'n.bin', '--dtypes', 'f16', '--geom', '20,128,256:40', '--geom', '20,127,256', '--geom', '19,128,256')
    f = {l.split()[1]: dict(zip(l.split()[2::2], l.split()[3::2])) for l in out if l.startswith('layer ')}
    assert [(f[str(i)]['cin_p'], f[str(i)]['cout_p'], f[str(i)]['NT'], f[str(i)]['nks']) for i in range(7)] == [
        ('4', '24', '2', '4'), ('24', '32', '2', '19'), ('32', '40', '3', '16'), ('40', '56', '4', '20'), ('56', '64', '4', '7'),
        ('64', '72', '5', '2'), ('72', '72', '5', '3')]
    assert all(int(v['lds']) <= 65536 for v in f.values())
    geom = [l for l in out if l.startswith('geom ')]
    assert geom[0].startswith('geom 20 128 256 n 40 workspace ') and geom[0].endswith(f'macs {spec.macs_per_sample(20, 128, 256)}')
    # the buffers lie behind one another, 256-byte aligned, each n D Ho Wo cout_p 2 bytes
    offs = [int(l.split()[-1]) for l in out if l.startswith('out ')]
    shapes = spec.check_geometry(20, 128, 256)
    exp, o = [], 0
    for (h, w), i in zip(shapes, range(7)):
        exp.append(o)
        o += -(-(40 * 20 * h * w * int(f[str(i)]['cout_p']) * 2) // 256) * 256
    assert offs == exp
    hid = [int(l.split()[-1]) for l in out if l.startswith('hidden ')]
    assert hid == [o, o + -(-(40 * 100 * 4) // 256) * 256]
    assert int(geom[0].split()[7]) == hid[1] + -(-(40 * 50 * 4) // 256) * 256
    assert geom[1] == 'geom 20 127 256 n 1 error: viewnet: layer 5 has an empty output for a 127 x 256 view'
    assert geom[2] == 'geom 19 128 256 n 1 error: viewnet: the layers give 3990 features + 2 scalars, the first Linear takes 4202'


@pytest.mark.parametrize('change, msg', [
    (dict(layers=[(20, 3, 2)]), 'viewnet: layer 0: k must be 1, 2, 4 or 5'), (dict(layers=[(20, 5, 4)]), 'viewnet: layer 0: pool must be 1 or 2'),
    (dict(layers=[(96, 5, 2)]), 'viewnet: layer 0: cout must be 1 to 80'), (dict(in_channels=5), 'viewnet: in_channels must be 1 to 4'),
    (dict(act=2), 'viewnet: act must be 0 (relu) or 1 (leaky_relu)'), (dict(n_scalar=10), 'viewnet: the first Linear takes no features'),
    (dict(sizes=[10, 8, 7, 6, 5, 3]), 'viewnet: 1 to 4 Linear layers'), (dict(sizes=[10, 9000, 3]), 'viewnet: a Linear vector exceeds 8192 values'),
    (dict(drop=1), None), (dict(nan=True), 'viewnet: layer 0: non-finite weight'),
    (dict(big=65520.0), 'viewnet: layer 0: a weight overflows the storage type (use bf16, or rescale)'), (dict(dtype='f32'), 'viewnet: act_dtype must be SD_F16 or SD_BF16')])
def test_refused_plan(plan_dump, tmp_path, change, msg):
    kw = dict(layers=[(20, 5, 2)], sizes=[10, 8, 3], in_channels=4, n_scalar=2, act=0)
    kw.update({k: v for k, v in change.items() if k in kw})
    cin, n = kw['in_channels'], 0
    for cout, k, _ in kw['layers']:
        n += cout * cin * k * k + cout
        cin = cout
    n += sum(a * b + b for a, b in zip(kw['sizes'][:-1], kw['sizes'][1:]))
    floats = np.full(n - change.get('drop', 0), 0.25, np.float32)
    if change.get('nan'):
        floats[3] = np.nan
    if change.get('big'):
        floats[3] = change['big']      # the first value that rounds to an fp16 infinity
    if msg is None:
        msg = f'viewnet: weights hold {n - 1} floats, the description needs {n}'
    _write_net(tmp_path / 'n.bin', **kw, floats=floats)
    dt = change.get('dtype', 'f16')
    assert _run(plan_dump, tmp_path / 'n.bin', '--dtypes', dt) == [f'dtype {dt} rc {SD_ERR_INVALID} error: {msg}']


# -- numpy side of the cell type step -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_loc, vpl, nb', [(7, 2, 5), (3, 2, 20), (1, 2, 20), (1, 1, 20), (31, 2, 20), (10, 3, 4), (10, 2, 20)])
def test_views_to_modelinput_bit_for_bit(n_loc, vpl, nb):
    """The padding branch (< nb views), the dropped remainder, one location, an exact fit: array form and table form."""
    from syconn_amd.reps.super_segmentation_helper import sso_views_to_modelinput, view_sample_table
    v = np.random.default_rng(n_loc).integers(0, 256, (n_loc, 4, vpl, 6, 5), dtype=np.uint8)
    want = R.modelinput_literal(v, nb)
    got = sso_views_to_modelinput(v, nb)
    assert got.shape == want.shape and np.array_equal(got, want)
    sm = sso_views_to_modelinput(v, nb, return_table=True)
    assert sm.views is v and sm.table.dtype == np.int32 and np.array_equal(sm.table, view_sample_table(n_loc, vpl, nb))
    planes = v.swapaxes(1, 0).reshape(4, n_loc * vpl, 6, 5)
    assert np.array_equal(planes[:, sm.table.reshape(-1)].reshape(4, -1, nb, 6, 5).swapaxes(1, 0), want)
    assert sm.table.min() >= 0 and sm.table.max() < n_loc * vpl


def test_normalisation_and_uint8_mapping():
    from syconn_amd.handler.prediction import naive_view_normalization_new, views_to_uint8
    u = np.arange(256, dtype=np.uint8).reshape(1, 1, 1, 16, 16)
    x = naive_view_normalization_new(u)
    assert x.dtype == np.float32 and np.array_equal(x, u.astype(np.float32) / 255. - 0.5)
    assert np.array_equal(views_to_uint8(x), u)
    for bad in (x + np.float32(1e-4), np.nextafter(x, np.float32(1)), x.astype(np.float64), np.where(u == 3, np.float32('nan'), x),
                x * 2):
        with pytest.raises(NotImplementedError):
            views_to_uint8(bad)


def test_certainty_estimate():
    from syconn_amd.handler.prediction import certainty_estimate
    rng = np.random.default_rng(3)
    logits = rng.normal(0, 2, (9, 7)).astype(np.float32)
    p = np.exp(logits.astype(np.float64))
    p /= p.sum(1, keepdims=True)
    m = p.mean(0)
    want = 1 - (-(m * np.log(m)).sum()) / np.log(7)
    assert abs(certainty_estimate(logits, is_logit=True) - want) < 1e-6
    assert abs(certainty_estimate(p) - want) < 1e-12
    assert certainty_estimate(np.full((4, 5), 0.2)) == pytest.approx(0, abs=1e-12)
    assert certainty_estimate(np.eye(3)[[1, 1]]) == 1      # 0 ln 0 = 0
    with pytest.raises(ValueError):
        certainty_estimate(np.zeros(3))
    try:
        from scipy.special import softmax
        from scipy.stats import entropy
    except ImportError:
        return
    pr = np.mean(softmax(logits, axis=1), axis=0)
    assert abs(certainty_estimate(logits, is_logit=True) - (1 - entropy(pr) / np.log(len(pr)))) < 1e-6      # float32 there and here


def test_syn_sign_ratio_edges():
    from syconn_amd.reps.super_segmentation_helper import syn_sign_ratio_celltype as ratio
    sign = np.array([-1, 1, -1, 1, -1])
    area = np.array([2.0, 4.0, 6.0, 8.0, 10.0])
    ax = np.array([1, 3, 4, 0, 2])                                   # boutons 3, 4 count as axon
    assert ratio(sign, area, ax) == (1.0 + 3.0) / (1.0 + 2.0 + 3.0)      # sizes are mesh_area / 2
    assert ratio(sign, area, ax, weighted=False) == 2 / 3
    assert ratio(sign, area, ax, comp_types=[0]) == 0.0
    assert ratio(sign, area, ax, comp_types=[2]) == 1.0
    assert ratio(sign, area, ax, comp_types=[0, 2]) == 5.0 / 9.0
    assert ratio([], [], []) == -1                                   # no synapses
    assert ratio(sign, area, np.full(5, 2), comp_types=[1]) == -1    # none on the compartment
    assert ratio(sign, np.zeros(5), ax) == -1                        # zero area
    assert np.array_equal(ax, [1, 3, 4, 0, 2])                       # the caller's labels are not rewritten
    with pytest.raises(ValueError):
        ratio(sign, area[:-1], ax)


def test_vote_and_da_tan_merge():
    from syconn_amd.handler.prediction import certainty_estimate
    from syconn_amd.reps.super_segmentation_helper import celltype_vote
    res = np.array([[0.1, 1.0, 0.0, 1.2, 0.0, 0.0, 0.9],      # argmax 3 alone; logit 6 onto logit 1 makes it 1
                    [0.0, 2.0, 0.0, 0.0, 0.0, 0.0, -1.5],     # 1 either way
                    [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 3.0]], np.float32)     # 6 alone, 1 merged
    pred, out, cert = celltype_vote(res, True, 7)
    lit = res.copy()
    lit[:, 1] += lit[:, 6]
    lit = np.delete(lit, [6], axis=1)
    assert pred == 1 and out.dtype == np.float32 and np.array_equal(out, lit) and cert == certainty_estimate(lit, is_logit=True)
    assert np.array_equal(res[0], np.array([0.1, 1.0, 0.0, 1.2, 0.0, 0.0, 0.9], np.float32))      # the caller's logits are not touched
    pred2, out2, _ = celltype_vote(res, False, 7)
    assert pred2 == 1 and np.array_equal(np.argmax(out2, 1), [3, 1, 6]) and out2.shape == (3, 7)
    assert celltype_vote(res[[0, 2, 2]], False, 7)[0] == 6
    with pytest.raises(ValueError, match='Unknown cell type'):
        celltype_vote(res, False, 5)
    # certainty_celltype: the stored value if there is one, else from the stored logits
    import types
    from syconn_amd.reps.super_segmentation_object import certainty_celltype
    cell = types.SimpleNamespace(attr_dict={'celltype_cnn_e3_probas': out, 'x_probas': out2, 'x_certainty': 0.25})
    assert certainty_celltype(cell) == cert and certainty_celltype(cell, 'x') == 0.25
    from syconn_amd import global_params
    assert global_params.config['celltypes']['nb_views_model'] == 20
    from syconn_amd.handler.config import DynConfig
    assert DynConfig('/nowhere/wd').mpath_celltype_e3 == '/nowhere/wd/models//celltype_e3/model.pts'


# -- the constants of the GPU test -----------------------------------------------------------------------------------------------
def _chain_cref(name, mode, store):
    spec, D, H, W, arrs, views, scal = K.inputs(name, mode)
    sr = R.StepRef(spec, arrs, store)
    x = np.ascontiguousarray(views.transpose(0, 2, 3, 4, 1)).reshape(-1, H, W, spec.in_channels)
    worst = 0.0
    for i in range(sr.nl):
        r64, S = sr.layer(i, x)
        r32, _ = sr.layer(i, x, torch.float32)
        worst = max(worst, float(((r32.double() - r64).abs() / (2.0 ** -24 * S)).max()))
        x = to_storage(r64.float(), store)
    v = sr.head_input(x, scal, D).float()
    for j in range(sr.n_fc):
        r64, S = sr.linear(j, v)
        r32, _ = sr.linear(j, v, torch.float32)
        worst = max(worst, float(((r32.double() - r64).abs() / (2.0 ** -24 * S)).max()))
        v = r64.float()
    return worst


@pytest.mark.parametrize('store', K.STORES)
def test_accumulation_constant(store):
    """c_ref = the largest |ref32 - ref64| / (2^-24 S) over every op of every case; printed, and within what the cases file records."""
    worst = {}
    for name in ('a', 'b', 'c', 'd', 'cmn'):
        for mode in (('shapes', 'zeros', 'ones', 'checker') if name == 'a' else ('shapes',)):
            worst[f'{name}:{mode}'] = _chain_cref(name, mode, store)
    print(store, {k: round(v, 3) for k, v in worst.items()})
    # the recorded constant is the measured one (torch's float32 summation order may move the last digits)
    assert 0.9 * K.C_REF[store] <= max(worst.values()) <= 1.02 * K.C_REF[store]
    assert K.C[store] == 4 * K.C_REF[store]


@pytest.mark.parametrize('store', K.STORES)
def test_cmn_tolerance_and_safety(store):
    """T = 4 x the largest |emulation - float32 restatement| on the CMN samples, both on the stored weights (activation rounding only),
    recomputed; every sample is safe (float32 top-2 margin > 2 T)."""
    spec, D, H, W, arrs, views, scal = K.inputs('cmn')
    l32 = R.forward32_stored(spec, arrs, views, scal, store)
    d = float(np.abs(R.forward_emul(spec, arrs, views, scal, store) - l32).max())
    s = np.sort(l32, axis=1)
    print(store, 'emulation diff', d, 'T', K.T[store], 'margins', s[:, -1] - s[:, -2])
    assert 0.95 * K.EMUL_DIFF[store] <= d <= 1.05 * K.EMUL_DIFF[store]      # (torch's float32 summation order moves the last digits)
    assert K.T[store] == 4 * K.EMUL_DIFF[store]
    assert ((s[:, -1] - s[:, -2]) > 2 * K.T[store]).all()
    # the samples differ by far more than the tolerance
    assert np.abs(l32[0] - l32[1]).max() > 10 * K.T['bf16']


def test_restatement_chain_is_the_net():
    """StepRef's ops chained without rounding restate forward32 (float64 vs float32: 1e-4)."""
    for name in ('a', 'b', 'c', 'd'):
        spec, D, H, W, arrs, views, scal = K.inputs(name)
        sr = R.StepRef(spec, arrs, 'f16')
        stored = [to_storage(torch.from_numpy(a), 'f16').float().numpy() if i < 2 * sr.nl and i % 2 == 0 else a for i, a in enumerate(arrs)]
        x = np.ascontiguousarray(views.transpose(0, 2, 3, 4, 1)).reshape(-1, H, W, spec.in_channels)
        for i in range(sr.nl):
            x, _ = sr.layer(i, x)
        v = sr.head_input(x, scal, D)
        for j in range(sr.n_fc):
            v, _ = sr.linear(j, v)
        want = R.forward32(spec, stored, views, scal, dtype=torch.float64)
        assert np.abs(v.numpy() - want).max() < 1e-9


# -- the reference's own functions (golden g29) -------------------------------------------------------------------------------------
# The certainty goes through float32 exp, division, mean, log and a sum of C <= 7 terms -p ln p <= 1 / e, in scipy there (its own entr
# and softmax) and in numpy here: a few float32 roundings per term, 7 terms, divided by ln C >= 1.79 -- below 8 x 2^-24 x 7 / e / 1.79.
# The vote, the merge and the stored logits are bit for bit.
CERT_TOL = 8 * 2.0 ** -24 * 7 / np.e / 1.79


@pytest.fixture(scope='module')
def g29():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g29_celltype.npz'))


def test_golden_generators_did_not_drift(g29):
    arrs = K.golden_weights()
    assert K.crc(*arrs) == g29['weights_crc'], 'make_weights changed: regenerate the golden, the kernels are not at fault'
    for cell in K.GOLDEN_CELLS:
        views, syn = K.golden_cell_inputs(*cell)
        assert K.crc(views, *syn) == g29[f'{cell[0]}_crc'], 'the input generators changed: regenerate the golden'
    assert list(g29['names']) == [c[0] for c in K.GOLDEN_CELLS]


@pytest.mark.parametrize('cell', K.GOLDEN_CELLS, ids=[c[0] for c in K.GOLDEN_CELLS])
def test_golden_cell(g29, cell):
    """The restatement and the host side of this package against the reference's own flow: the sample table, the ratios and the vote bit
    for bit (numpy), the certainty to float32 rounding (CERT_TOL); layer-7 features and logits of the float32 restatement to 1e-5 (torch's float32 summation order)."""
    from syconn_amd.handler.prediction import naive_view_normalization_new
    from syconn_amd.reps.super_segmentation_helper import celltype_vote, sso_views_to_modelinput, syn_sign_ratio_celltype, view_sample_table
    name, n_loc, vpl, _ = cell
    views, syn = K.golden_cell_inputs(*cell)
    table = view_sample_table(n_loc, vpl, 20)
    assert table.dtype == np.int32 and np.array_equal(table, g29[f'{name}_table'])
    ratios = [syn_sign_ratio_celltype(*syn, comp_types=[1]), syn_sign_ratio_celltype(*syn, comp_types=[0]),
              syn_sign_ratio_celltype(*syn, weighted=False, comp_types=[1]), syn_sign_ratio_celltype(*syn, comp_types=[0, 2])]
    assert np.array_equal(np.array(ratios, np.float64), g29[f'{name}_ratios'])
    # the vote and the certainty on the reference's logits: bit for bit
    pred, res, cert = celltype_vote(g29[f'{name}_logits'], True, 7)
    assert pred == g29[f'{name}_pred'] and np.array_equal(res, g29[f'{name}_probas']) and res.dtype == g29[f'{name}_probas'].dtype
    assert abs(cert - g29[f'{name}_cert']) <= CERT_TOL
    # the network restated
    spec = CELLTYPE_CMN(7, 2)
    arrs = K.golden_weights()
    inp = sso_views_to_modelinput(views, 20)
    logits, feat = R.forward32(spec, arrs, inp, np.array([ratios[:2]] * len(inp)), return_features=True)
    assert feat.shape == g29[f'{name}_feat'].shape == (len(table), 70, 20, 1, 3)
    assert np.abs(feat - g29[f'{name}_feat']).max() <= 1e-5 and np.abs(logits - g29[f'{name}_logits']).max() <= 1e-5
    assert np.array_equal(naive_view_normalization_new(inp[:1, :, :2]), inp[:1, :, :2].astype(np.float32) / 255. - 0.5)


def test_golden_vote_block(g29):
    """celltype_of_sso_nocache :1733-1749 alone, on logits where adding logit 6 onto logit 1 changes an argmax."""
    from syconn_amd.reps.super_segmentation_helper import celltype_vote
    pred, res, cert = celltype_vote(g29['vote_in'], True, 7)
    assert pred == g29['vote_pred_merged'] and np.array_equal(res, g29['vote_merged']) and abs(cert - g29['vote_cert']) <= CERT_TOL
    pred0, res0, _ = celltype_vote(g29['vote_in'], False, 7)
    assert pred0 == g29['vote_pred_plain'] and np.array_equal(res0, g29['vote_in'])
    assert not np.array_equal(res.argmax(1), res0.argmax(1))
