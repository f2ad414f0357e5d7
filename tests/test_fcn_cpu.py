"""The FCN semantic-segmentation network without a GPU: the spec against torch (shapes, multiply-adds, the state-dict loader), the
host-only plan builder (syconn_amd/csrc/sd_fcn_plan.cpp) through tools/fcn_plan_dump -- also built with the address and undefined
behaviour sanitizers --, and the constants the GPU test relies on (tests/_fcn_cases.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

import _fcn_cases as K
import _fcn_ref as R
from _unet_step_ref import to_storage
from syconn_amd.cnn.fcn_spec import FCN_VGG13, FcnSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD_ERR_INVALID = -1
NETS = ['v', 's', 'o1', 'o2', 'g']


# -- the spec -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['s', 'o2', 'v'])
def test_spec_is_the_torch_module(name, tmp_path):
    """param_shapes() is the module's state dict (names, shapes, order, without num_batches_tracked); the loader takes the state dict of
    the module and of its torch.jit trace; forward32 is the module in eval mode; shapes() and macs_per_view() agree with torch."""
    spec, arrs, views = K.inputs(name)
    net = R.Fcns(spec).eval()
    sd = net.state_dict()
    named = [(k, tuple(v.shape)) for k, v in sd.items() if v.dim() > 0]
    assert named == [(k, tuple(s)) for k, s in spec.param_shapes().items()]
    assert any(k.endswith('num_batches_tracked') for k in sd)
    net.load_state_dict({**sd, **R.state_dict_of(spec, arrs)})
    got = spec.weights_from_state_dict(net.state_dict())
    assert len(got) == len(arrs) and all(np.array_equal(a, b) for a, b in zip(got, arrs))
    planes = R.planes_of(views)
    x = torch.from_numpy(planes).float() / 255.
    with torch.no_grad():
        want = net(x).numpy()
        traced = torch.jit.trace(net, x)
    assert np.allclose(R.forward32(spec, arrs, planes), want, rtol=0, atol=1e-5)
    path = str(tmp_path / 'm.pts')
    traced.save(path)
    got = spec.weights_from_state_dict(torch.jit.load(path, map_location='cpu').state_dict())
    assert all(np.array_equal(a, b) for a, b in zip(got, arrs))
    # shapes: hooks on every module whose output the device stores
    H, W = planes.shape[2:]
    seen = []
    feats = net.pretrained_net.features
    hooks = []
    for i, l in enumerate(feats):
        last_of_block = isinstance(l, nn.MaxPool2d)
        inner = isinstance(l, nn.ReLU) and not isinstance(feats[i + 1], nn.MaxPool2d)
        if last_of_block or inner:
            hooks.append(l.register_forward_hook(lambda m, a, o: seen.append(tuple(o.shape[1:]))))
    for i in range(1, 6):
        hooks.append(getattr(net, f'bn{i}').register_forward_hook(lambda m, a, o: seen.append(tuple(o.shape[1:]))))
    hooks.append(net.classifier.register_forward_hook(lambda m, a, o: seen.append(tuple(o.shape[1:]))))
    with torch.no_grad():
        net(x[:1])
    for h in hooks:
        h.remove()
    assert seen == spec.shapes(H, W) and len(seen) == spec.n_ops
    # multiply-adds: weights x output pixels of every convolution; a transposed convolution's weights x INPUT pixels
    macs = 0
    for (c, h, w), ((_, cin, cout, pooled)) in zip(spec.shapes(H, W), spec.convs):
        macs += 9 * cin * cout * h * w * (4 if pooled else 1)
    for (c, h, w), (cin, cout) in zip(spec.shapes(H, W)[len(spec.convs):], spec.deconvs):
        macs += 9 * cin * cout * (h // 2) * (w // 2)
    assert spec.macs_per_view(H, W) == macs + H * W * spec.dec_last * spec.n_class


def test_spec_refusals_and_vgg13():
    spec = FCN_VGG13(5)
    assert spec.blocks == ((64, 64), (128, 128), (256, 256), (512, 512), (512, 512)) and spec.deconvs == [(512, 512), (512, 256), (256, 128), (128, 64), (64, 32)]
    assert 7.9e9 < spec.macs_per_view(128, 256) < 8.1e9 and spec.macs_per_view(512, 1024) == 16 * spec.macs_per_view(128, 256)
    for H, W in ((128, 250), (100, 256), (0, 32), (16, 32)):
        with pytest.raises(ValueError, match='multiples of 32'):
            spec.shapes(H, W)
    kw = dict(in_channels=3, blocks=((8,),) * 5, dec_last=8, n_class=2)
    for bad in (dict(in_channels=0), dict(in_channels=5), dict(blocks=((8,),) * 4), dict(blocks=((8,),) * 6), dict(blocks=((8,),) * 4 + ((),)),
                dict(blocks=((8,),) * 4 + ((8,) * 4,)), dict(blocks=((8,),) * 4 + ((0,),)), dict(blocks=((8,),) * 4 + ((513,),)), dict(dec_last=0),
                dict(dec_last=513), dict(n_class=0), dict(n_class=17)):
        with pytest.raises(ValueError):
            FcnSpec(**{**kw, **bad})
    s, arrs, _ = K.inputs('s')
    sd = R.state_dict_of(s, arrs)
    with pytest.raises(ValueError, match='has shape'):
        s.weights_from_state_dict({k: (v.transpose(0, 1).contiguous() if k == 'deconv2.weight' else v) for k, v in sd.items()})
    with pytest.raises(ValueError, match='tensors'):
        s.weights_from_state_dict({**sd, 'extra': torch.zeros(3)})
    with pytest.raises(ValueError, match='non-finite'):
        s.weights_from_state_dict({k: (v * float('nan') if k == 'bn3.running_var' else v) for k, v in sd.items()})
    assert len(s.weights_from_state_dict({**sd, 'bn1.num_batches_tracked': torch.tensor(7)})) == len(arrs)


# -- the host-only plan -----------------------------------------------------------------------------------------------------------
def _build_dump(tmp, flags):
    exe = str(tmp / 'fcn_plan_dump')
    hipcc = '/opt/rocm/bin/hipcc'
    assert os.path.isfile(hipcc), 'hipcc is needed to build tools/fcn_plan_dump.cpp'
    csrc = os.path.join(ROOT, 'syconn_amd', 'csrc')
    subprocess.run([hipcc, *flags, '-std=c++17', os.path.join(csrc, 'sd_fcn_plan.cpp'), os.path.join(csrc, 'sd_viewnet_plan.cpp'),
                    os.path.join(ROOT, 'tools', 'fcn_plan_dump.cpp'), '-o', exe], check=True, timeout=600)
    return exe


@pytest.fixture(scope='module')
def plan_dump(tmp_path_factory):
    return _build_dump(tmp_path_factory.mktemp('fcn_plan_dump'), ['-O2'])


def _write_net(path, in_channels, blocks, dec_last, n_class, floats, lens=None):
    floats = np.asarray(floats, np.float32)
    flat = [c for b in blocks for c in b]
    lens = [len(b) for b in blocks] if lens is None else lens
    with open(path, 'wb') as f:
        f.write(b'SDFCN01\0' + struct.pack('<9iq', in_channels, dec_last, n_class, len(flat), *lens, floats.size))
        f.write(np.asarray(flat, np.int32).tobytes() + floats.tobytes())


def _spec_net(path, spec, arrs):
    _write_net(path, spec.in_channels, spec.blocks, spec.dec_last, spec.n_class, np.concatenate([a.ravel() for a in arrs]))


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def _unpacked_want(spec, arrs, store):
    """The input with the 3 x 3 weights rounded to the storage type and (scale, shift) in place of the four BatchNorm tensors."""
    sr = R.StepRef(spec, arrs, store)
    q = lambda a: to_storage(torch.from_numpy(a), store).float().numpy().ravel()
    want = []
    for w, b in sr.convs:
        want += [q(w), b.ravel()]
    for d, (w, b, *_) in enumerate(sr.deconvs):
        sc, sh = sr.bn_constants(d)
        want += [q(w), b.ravel(), sc.numpy(), sh.numpy()]
    return np.concatenate(want + [sr.cls[0].ravel(), sr.cls[1].ravel()])


@pytest.mark.parametrize('name', NETS)
@pytest.mark.parametrize('store', K.STORES)
def test_packing_round_trip(plan_dump, tmp_path, name, store):
    """Fragment order, channel padding, the parity split of the transposed convolutions, the BatchNorm constants: read back by the lane
    map and the tap tables, the blob is the input with the 3 x 3 weights rounded to the storage type and nothing else; every weight is
    found exactly once and every padding element is zero."""
    spec, arrs, _ = K.inputs(name)
    _spec_net(tmp_path / 'n.bin', spec, arrs)
    out = _run(plan_dump, tmp_path / 'n.bin', '--dtypes', store, '--unpack', tmp_path / 'u.bin')
    assert out[0].startswith(f'dtype {store} rc 0')
    pads = [l for l in out if l.startswith('unpack op')]
    assert len(pads) == spec.n_ops - 1 and all(l.endswith('pad_nonzero 0 dup 0') for l in pads)
    got = np.fromfile(tmp_path / 'u.bin', np.float32)
    want = _unpacked_want(spec, arrs, store)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_batchnorm_constants():
    """scale = gamma / sqrt(var + 1e-5), shift = beta - mean scale: eval BatchNorm2d of torch within float32 rounding of its terms."""
    spec, arrs, _ = K.inputs('s')
    sr = R.StepRef(spec, arrs, 'f16')
    for d in range(5):
        _, _, gamma, beta, mean, var = (torch.from_numpy(a) for a in sr.deconvs[d])
        sc, sh = sr.bn_constants(d)
        x = torch.linspace(0, 6, 97).view(1, 1, -1, 1).repeat(1, len(gamma), 1, 1)
        want = torch.nn.functional.batch_norm(x.double(), mean.double(), var.double(), gamma.double(), beta.double(), False, 0., 1e-5)
        got = sc.double().view(1, -1, 1, 1) * x.double() + sh.double().view(1, -1, 1, 1)
        tol = 2.0 ** -23 * (sc.abs().double().view(1, -1, 1, 1) * x.double() + sh.abs().double().view(1, -1, 1, 1) + 1)
        assert ((got - want).abs() <= tol).all()


def test_plan_fields_and_workspace(plan_dump, tmp_path):
    spec, arrs, _ = K.inputs('g')
    _spec_net(tmp_path / 'n.bin', spec, arrs)
    out = _run(plan_dump, tmp_path / 'n.bin', '--dtypes', 'f16', '--geom', '128,256:10', '--geom', '512,1024:40', '--geom', '128,250', '--geom', '16,32')
    f = {int(l.split()[1]): dict(zip(l.split()[2::2], l.split()[3::2])) for l in out if l.startswith('op ')}
    assert len(f) == 16 and [f[i]['kind'] for i in range(16)] == ['0'] * 10 + ['1'] * 5 + ['2']
    assert [(f[i]['cin_p'], f[i]['cout_p'], f[i]['chunks'], f[i]['NT'], f[i]['groups']) for i in (0, 1, 2, 7, 10, 14)] == [
        ('4', '64', '1', '4', '1'), ('64', '64', '2', '4', '1'), ('64', '128', '2', '4', '2'), ('512', '512', '16', '4', '8'), ('512', '512', '16', '4', '8'),
        ('64', '32', '2', '2', '1')]
    assert [f[i]['pool'] for i in range(10)] == ['0', '1'] * 5 and f[0]['first'] == '1' and f[1]['first'] == '0'
    assert [f[10 + d]['skip'] for d in range(5)] == ['7', '5', '3', '1', '-1']
    geom = [l for l in out if l.startswith('geom ')]
    assert geom[0].startswith('geom 128 256 n 10 workspace ') and geom[0].endswith(f'macs {spec.macs_per_view(128, 256)}')
    # the buffers lie behind one another, 256-byte aligned, each n h w cp 2 bytes: every stored tensor has its own range
    outs = [l.split() for l in out if l.startswith('out ')]
    first = outs[:15]
    o = 0
    for l, (c, h, w) in zip(first, spec.shapes(128, 256)):
        assert [int(v) for v in l[2:5]] == [c, h, w] and int(l[-1]) == o
        o += -(-(10 * h * w * (-(-c // 8) * 8) * 2) // 256) * 256
    assert int(geom[0].split()[6]) == o
    # 40 planes of 512 x 1024: offsets beyond 2^32 (every byte offset is 64-bit)
    assert int(geom[1].split()[6]) > 2 ** 32 and int(outs[29][-1]) > 2 ** 32
    assert geom[2].startswith('geom 128 250 n 1 error: fcn: H and W must be multiples of 32') and geom[3].startswith('geom 16 32 n 1 error: fcn: H and W')


@pytest.mark.parametrize('change, msg', [
    (dict(in_channels=5), 'fcn: in_channels must be 1 to 4'), (dict(dec_last=600), 'fcn: dec_last must be 1 to 512'),
    (dict(n_class=17), 'fcn: n_class must be 1 to 16'), (dict(lens=[1, 1, 1, 1, 0]), 'fcn: block 4: 1 to 3 convolutions'),
    (dict(lens=[1, 4, 1, 1, 1]), 'fcn: block 1: 1 to 3 convolutions'), (dict(blocks=((8,), (8,), (600,), (8,), (8,))), 'fcn: convolution 2: channels must be 1 to 512'),
    (dict(drop=1), None), (dict(nan=True), 'fcn: non-finite weight at float 3'),
    (dict(big=65520.0), 'fcn: op 0: a weight overflows the storage type (use bf16, or rescale)'), (dict(dtype='f32'), 'fcn: act_dtype must be SD_F16 or SD_BF16'),
    (dict(negvar=True), 'fcn: op 5: BatchNorm running_var + eps is not positive')])
def test_refused_plan(plan_dump, tmp_path, change, msg):
    kw = dict(in_channels=3, blocks=((8,), (8,), (8,), (8,), (8,)), dec_last=8, n_class=2)
    kw.update({k: v for k, v in change.items() if k in kw})
    spec_ok = FcnSpec(3, ((8,),) * 5, 8, 2)
    n = sum(int(np.prod(s)) for s in spec_ok.param_shapes().values())
    floats = np.full(n - change.get('drop', 0), 0.25, np.float32)
    if change.get('nan'):
        floats[3] = np.nan
    if change.get('big'):
        floats[3] = change['big']      # the first value that rounds to an fp16 infinity
    if change.get('negvar'):
        conv_floats = 3 * 8 * 9 + 8 + 4 * (8 * 8 * 9 + 8)
        floats[conv_floats + 8 * 8 * 9 + 4 * 8 + 2] = -1.0      # running_var of the first decoder step (op 5)
    if msg is None:
        msg = f'fcn: weights hold {n - 1} floats, the description needs {n}'
    _write_net(tmp_path / 'n.bin', floats=floats, lens=change.get('lens'), **kw)
    dt = change.get('dtype', 'f16')
    assert _run(plan_dump, tmp_path / 'n.bin', '--dtypes', dt) == [f'dtype {dt} rc {SD_ERR_INVALID} error: {msg}']


def test_plan_builder_under_sanitizers(tmp_path):
    """The plan builder and tools/fcn_plan_dump.cpp as a stand-alone host program under the address and undefined behaviour
    sanitizers, on the specs of the cases: packing, unpacking, shapes and workspaces run clean and give the unsanitized output."""
    exe = _build_dump(tmp_path, ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer'])
    for name in ('s', 'o1', 'v'):
        spec, arrs, _ = K.inputs(name)
        _spec_net(tmp_path / f'{name}.bin', spec, arrs)
        r = subprocess.run([exe, str(tmp_path / f'{name}.bin'), '--geom', '32,64:3', '--geom', '512,1024:40', '--geom', '33,64', '--unpack', str(tmp_path / 'u.bin')],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr
        assert np.array_equal(np.fromfile(tmp_path / 'u.bin', np.float32), _unpacked_want(spec, arrs, 'f16'))
    floats = np.full(10, 0.25, np.float32)      # far too few weights: refused before anything is read
    _write_net(tmp_path / 'short.bin', 3, ((8,),) * 5, 8, 2, floats)
    r = subprocess.run([exe, str(tmp_path / 'short.bin')], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == '' and 'weights hold 10 floats' in r.stdout


# -- the constants of the GPU test ------------------------------------------------------------------------------------------------
def _chain_cref(name, mode, store):
    spec, arrs, views = K.inputs(name, mode)
    sr = R.StepRef(spec, arrs, store)
    worst = [0.0]

    def visit(idx, kind, args):
        fn = getattr(sr, kind)
        y64, S = fn(*args)
        y32, _ = fn(*args, dtype=torch.float32)
        worst[0] = max(worst[0], ((y32.double() - y64).abs() / (2.0 ** -24 * S.clamp_min(1e-300))).max().item())

    sr.chain(R.planes_of(views), visit)
    return worst[0]


@pytest.mark.parametrize('store', K.STORES)
def test_accumulation_constant(store):
    """c_ref = the largest |ref32 - ref64| / (2^-24 S) over every op of every case; printed, and within what the cases file records."""
    worst = {}
    for name in K.CASES:
        for mode in (K.MODES if name == 's' else ('shapes',)):
            worst[f'{name}:{mode}'] = _chain_cref(name, mode, store)
    print(store, {k: round(v, 3) for k, v in worst.items()})
    # the recorded constant is the measured one (torch's float32 summation order may move the last digits)
    assert 0.9 * K.C_REF[store] <= max(worst.values()) <= 1.02 * K.C_REF[store]
    assert K.C[store] == 4 * K.C_REF[store]


@pytest.mark.parametrize('name', K.E2E)
def test_tolerance_and_left_out(name):
    """T = 4 x the largest |emulation - float32 restatement| of the case, both on the stored weights, recomputed; the share of pixels the
    fp16 end-to-end label comparison leaves out (restatement margin below 2 T) is at most 10 % and as recorded."""
    spec, arrs, views = K.inputs(name)
    planes = R.planes_of(views)
    for store in K.STORES:
        l32 = K.restatement(name, store)
        em = R.forward_emul(spec, arrs, planes, store)
        d = float(np.abs(em - l32).max())
        rms = float(np.sqrt((l32.astype(np.float64) ** 2).mean()))
        m = R.top2_margin(l32)
        left = float((m < 2 * K.T[store][name]).mean())
        print(name, store, 'emulation diff', d, 'T', K.T[store][name], 'logit rms', round(rms, 3), 'margin < 2 T', round(left, 4), 'argmax disagreements',
              float((em.argmax(1) != l32.argmax(1)).mean()))
        assert 0.95 * K.EMUL_DIFF[store][name] <= d <= 1.05 * K.EMUL_DIFF[store][name]
        assert K.T[store][name] == 4 * K.EMUL_DIFF[store][name]
        assert 1.0 < rms < 4.0
        if store == 'f16':
            assert left <= 0.10 and abs(left - K.LEFT_OUT_E2E[name]) <= 0.005


def test_one_op_label_check_covers_the_cases():
    """The one-op label check leaves out pixels whose float64 top-2 margin is below twice the fp32 one-op bound: at most 0.1 % of the
    pixels of every case, on the stored tensors the float64 chain produces."""
    for store in K.STORES:
        for name in K.CASES:
            for mode in (K.MODES if name == 's' else ('shapes',)):
                spec, arrs, views = K.inputs(name, mode)
                sr = R.StepRef(spec, arrs, store)
                got = {}
                sr.chain(R.planes_of(views), lambda i, kind, args: got.update(x=args[0]) if kind == 'classify' else None)
                ref, S = sr.classify(got['x'])
                b = R.bound_f32(ref, S, K.C[store]).max(1).values.numpy()
                left = float((R.top2_margin(ref.numpy()) < 2 * b).mean())
                assert left <= 1e-3, (store, name, mode, left)


def test_restatement_chain_is_the_net():
    """StepRef's ops chained without rounding restate forward32 on the stored weights (float64 both: 1e-9)."""
    for name in ('s', 'o2'):
        spec, arrs, views = K.inputs(name)
        planes = R.planes_of(views)
        sr = R.StepRef(spec, arrs, 'f16')
        x, stored = np.ascontiguousarray(planes.transpose(0, 2, 3, 1)), []
        for i in range(sr.nc):
            x = sr.conv(i, x)[0].numpy()
            stored.append(x)
        for d in range(5):
            k = sr.skip_of(d)
            x = sr.deconv(d, x, stored[k] if k is not None else None)[0].numpy()
        got = sr.classify(x)[0].numpy()
        want = R.forward32(spec, arrs, planes, weights_as='f16', dtype=torch.float64)
        # (scale, shift) are float32 roundings of the float64 BatchNorm: 2^-24 relative per decoder step
        assert np.abs(got - want).max() < 1e-5


# -- the reference's own predict_views_semseg (golden g30) ------------------------------------------------------------------------
@pytest.mark.parametrize('name', [g[0] for g in K.GOLDEN])
def test_golden_semseg(name):
    """The generated inputs are the golden's; the golden model's 3 x 3 weights are exact in both storage types, so its labels -- the
    reference's ``predict_views_semseg``, layout included -- are the argmax of the float32 restatement except at near-ties (another
    float32 summation order); T of the golden cases is as recorded and the fp16 comparison leaves out at most 10 %."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g30_semseg.npz'))
    spec, arrs, views = K.golden_inputs(name)
    n_loc, _, nb_views, H, W = views.shape
    assert g[f'{name}_crc'] == K.crc(views, *arrs)
    for a in arrs:
        if a.ndim == 4 and a.shape[2:] == (3, 3):
            assert all(np.array_equal(to_storage(torch.from_numpy(a), st).numpy(), a.astype(np.float64)) for st in K.STORES)
    labels = g[f'{name}_labels']
    assert labels.shape == (n_loc, 1, nb_views, H, W) and labels.dtype == np.uint8
    planes = R.planes_of(views)
    l32 = R.forward32(spec, arrs, planes)
    clear = (R.top2_margin(l32) > 1e-4).reshape(n_loc, nb_views, H, W)[:, None]
    assert clear.mean() > 0.999
    assert np.array_equal(labels[clear], l32.argmax(1).reshape(n_loc, nb_views, H, W)[:, None][clear])
    for store in K.STORES:
        assert np.array_equal(R.forward32_stored(spec, arrs, planes, store), l32)      # the stored weights are the golden model's
        d = float(np.abs(R.forward_emul(spec, arrs, planes, store) - l32).max())
        print(name, store, 'emulation diff', d)
        assert 0.95 * K.GOLDEN_EMUL_DIFF[store][name] <= d <= 1.05 * K.GOLDEN_EMUL_DIFF[store][name]
        assert K.GOLDEN_T[store][name] == 4 * K.GOLDEN_EMUL_DIFF[store][name]
    assert (R.top2_margin(l32) < 2 * K.GOLDEN_T['f16'][name]).mean() <= 0.10
