"""CPU: the morphology embedding's spec and state-dict loader, the numpy drop-ins, the restatement (tests/_embedding_ref.py) against the
golden of the reference's own module (tests/golden/g31_embedding.npz), the table's offsets, the input checks that need no device, the
plan of the spec through tools/viewnet_plan_dump, and the constants the GPU test relies on (tests/_embedding_cases.py)."""
import dataclasses
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import _embedding_cases as K
import _embedding_ref as E
import _viewnet_ref as R
from _unet_step_ref import to_storage
from syconn_amd.cnn.viewnet_spec import CELLTYPE_CMN, TNET_REP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g31_embedding.npz'))


# -- spec -------------------------------------------------------------------------------------------------------------------------
def test_spec_geometry():
    s = TNET_REP()
    assert s.layers == ((13, 5, 2), (19, 5, 2), (25, 4, 1), (25, 4, 2), (30, 2, 2), (30, 2, 2), (31, 1, 1))
    assert s.linear_sizes == (372, 50, 25) and s.n_scalar == 0 and s.act == 'relu' and s.conv_ndim == 2 and s.in_channels == 4
    assert s.check_geometry(1, 128, 256) == [(62, 126), (29, 61), (26, 58), (11, 27), (5, 13), (2, 6), (2, 6)]
    lit = TNET_REP(fc_in=6076)
    assert lit.check_geometry(1, 512, 512) == [(254, 254), (125, 125), (122, 122), (59, 59), (29, 29), (14, 14), (14, 14)]
    assert 31 * 14 * 14 == 6076 and 31 * 2 * 6 == 372
    assert TNET_REP(z_dim=10).linear_sizes == (372, 50, 10)
    # the sizes each spec refuses: the other one's window, two views per sample
    for spec, geom, msg in ((s, (1, 512, 512), 'flattens to 6076'), (lit, (1, 128, 256), 'flattens to 372'), (s, (2, 128, 256), 'flattens to 744')):
        with pytest.raises(ValueError, match=msg):
            spec.check_geometry(*geom)
    # the minimum view: 92 x 92 flattens to 31 features; one pixel less in either extent leaves layer 5 without an output
    assert TNET_REP(fc_in=31).check_geometry(1, 92, 92)[-1] == (1, 1)
    for hw in ((91, 92), (92, 91)):
        with pytest.raises(ValueError, match='layer 5 has an empty output'):
            s.layer_shapes(*hw)
    with pytest.raises(ValueError, match='conv_ndim'):
        dataclasses.replace(s, conv_ndim=4)
    # the existing specs keep their 5-D weights
    assert CELLTYPE_CMN().conv_ndim == 3 and list(CELLTYPE_CMN().param_shapes().values())[0] == (20, 4, 1, 5, 5)
    assert list(s.param_shapes().values())[0] == (13, 4, 5, 5) and list(s.param_shapes().values())[-2:] == [(25, 50), (25,)]


def test_state_dict_loading():
    spec = K.GEOMS['min'][0]
    arrs = E.make_weights(spec, 1, 92, 92)
    flat = np.concatenate([a.ravel() for a in arrs])
    for prefix in ('', 'rep_net.'):      # the bare RepresentationNetwork and the whole TripletNet
        sd = E.state_dict_of(spec, arrs, prefix)
        assert list(sd)[0] == prefix + 'conv.0.weight' and sd[prefix + 'conv.0.weight'].dim() == 4
        got = spec.weights_from_state_dict(sd)
        assert np.array_equal(np.concatenate([a.ravel() for a in got]), flat)
    sd5 = E.state_dict_of(spec, arrs, ndim=3)
    assert np.array_equal(np.concatenate([a.ravel() for a in E.spec5(spec).weights_from_state_dict(sd5)]), flat)
    # a spec takes the convolution rank it names and no other
    with pytest.raises(ValueError, match=r'has shape \(13, 4, 1, 5, 5\), the spec needs \(13, 4, 5, 5\)'):
        spec.weights_from_state_dict(sd5)
    with pytest.raises(ValueError, match=r'has shape \(13, 4, 5, 5\), the spec needs \(13, 4, 1, 5, 5\)'):
        E.spec5(spec).weights_from_state_dict(E.state_dict_of(spec, arrs))
    sd = E.state_dict_of(spec, arrs)
    with pytest.raises(ValueError, match=r'fc.0.weight has shape \(50, 31\), the spec needs \(50, 372\)'):
        TNET_REP().weights_from_state_dict(sd)
    with pytest.raises(ValueError, match='14 tensors, the spec needs 18'):
        spec.weights_from_state_dict({k: v for k, v in sd.items() if not k.startswith('fc.')})
    bad = dict(sd)
    bad['fc.2.bias'] = torch.full((25,), float('nan'))
    with pytest.raises(ValueError, match='non-finite'):
        spec.weights_from_state_dict(bad)


# -- numpy drop-ins ----------------------------------------------------------------------------------------------------------------
def test_views2tripletinput_golden(gold):
    from syconn_amd.handler.prediction import views2tripletinput
    small = np.random.default_rng(K.GOLDEN_SEED).integers(0, 256, (3, 4, 2, 5, 7)).astype(np.uint8)
    assert K.crc(small) == gold['triplet_in_crc']
    got = views2tripletinput(small)
    assert got.dtype == gold['triplet_out'].dtype == np.float32 and got.shape == (3, 4, 3, 5, 7) and np.array_equal(got, gold['triplet_out'])


def test_config_paths():
    from syconn_amd.handler.config import DynConfig
    assert DynConfig('/nowhere/wd').mpath_tnet == '/nowhere/wd/models//tCMN/model.pts'


# -- the restatement against the reference's module ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(K.GOLDEN))
def test_restatement_against_golden(gold, name):
    """The generated inputs are the golden's; float32 restatement vs the reference's module on torch-CPU float32: another summation
    order only.  The node mapping restated in float64 with the lower row on ties is the reference's cKDTree result, ties included."""
    geom = K.GOLDEN[name][0]
    spec = K.GEOMS[geom][0]
    arrs = K.golden_weights(name)
    views, locs, nodes = K.golden_cell(name)
    assert K.crc(views, locs, nodes, *arrs) == gold[f'{name}_crc']
    lat = E.latent32(spec, arrs, views)
    assert lat.shape == gold[f'{name}_latent'].shape == (len(views), K.Z)
    d = np.abs(lat - gold[f'{name}_latent']).max()
    print(name, '|restatement - golden|', d, 'largest latent', np.abs(lat).max())
    assert d <= 1e-5
    # exact weights: the stored ones are the module's, for both storage types
    for s in K.STORES:
        assert np.array_equal(E.latent32(spec, arrs, views, s), lat)
    rows, tie = E.nearest_rows(locs, nodes * K.GOLDEN_SCALING)
    assert np.array_equal(rows, gold[f'{name}_view_ixs']) and np.array_equal(tie, gold[f'{name}_tie'])
    assert np.array_equal(gold[f'{name}_node_latent'], gold[f'{name}_latent'][gold[f'{name}_view_ixs']])
    if name == 'w372':
        assert tie.sum() >= 2 and len(nodes) == 36 and len(set(rows[tie])) > 1


def test_restatement_float64_chain():
    """StepRef's ops of the 5-D twin, chained without rounding, restate the float64 net (the step reference of the GPU test is the
    same network as the restatement)."""
    spec, H, W, arrs, views = K.inputs('min')
    sr = R.StepRef(E.spec5(spec), arrs, 'f16')
    x = np.ascontiguousarray(E._views5(views).transpose(0, 2, 3, 4, 1)).reshape(-1, H, W, 4)
    for i in range(sr.nl):
        x, _ = sr.layer(i, x)
    v = sr.head_input(x, None, 1)
    for j in range(sr.n_fc):
        v, _ = sr.linear(j, v)
    assert np.abs(v.numpy() - E.latent32(spec, arrs, views, dtype=torch.float64)).max() < 1e-9


# -- the constants of the GPU test ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('store', K.STORES)
def test_accumulation_constant(store):
    """c_ref of this net's layer shapes (k = 4 without a pool, k = 2 with a pool twice), measured as tests/test_viewnet_cpu.py measures
    it: it does not exceed the constant of tests/_viewnet_cases.py, whose bound the GPU test therefore uses."""
    worst = {}
    for name in K.GEOMS:
        spec, H, W, arrs, views = K.inputs(name)
        sr = R.StepRef(E.spec5(spec), arrs, store)
        x = np.ascontiguousarray(E._views5(views).transpose(0, 2, 3, 4, 1)).reshape(-1, H, W, 4)
        w = 0.0
        for i in range(sr.nl):
            r64, S = sr.layer(i, x)
            r32, _ = sr.layer(i, x, torch.float32)
            w = max(w, float(((r32.double() - r64).abs() / (2.0 ** -24 * S)).max()))
            x = to_storage(r64.float(), store)
        v = sr.head_input(x, None, 1).float()
        for j in range(sr.n_fc):
            r64, S = sr.linear(j, v)
            r32, _ = sr.linear(j, v, torch.float32)
            w = max(w, float(((r32.double() - r64).abs() / (2.0 ** -24 * S)).max()))
            v = r64.float()
        worst[name] = w
    print(store, {k: round(v, 3) for k, v in worst.items()})
    assert 0.9 * K.C_REF_MEASURED[store] <= max(worst.values()) <= 1.02 * K.C_REF_MEASURED[store]
    assert K.C_REF_MEASURED[store] <= K.C_REF[store] and K.C[store] == 4 * K.C_REF[store]


def _case_inputs(case):
    if case.startswith('golden_'):
        name = case[len('golden_'):]
        return K.GEOMS[K.GOLDEN[name][0]][0], K.golden_weights(name), K.golden_cell(name)[0]
    spec, _, _, arrs, views = K.inputs(case)
    return spec, arrs, views


@pytest.mark.parametrize('store', K.STORES)
@pytest.mark.parametrize('case', list(K.EMUL_DIFF))
def test_tolerance(case, store):
    """T = 4 x the largest |emulation - float32 restatement| of the case's latents, recomputed."""
    spec, arrs, views = _case_inputs(case)
    l32 = E.latent32(spec, arrs, views, store)
    d = float(np.abs(E.latent_emul(spec, arrs, views, store) - l32).max())
    print(case, store, 'emulation diff', d, 'T', K.T[case][store])
    assert 0.95 * K.EMUL_DIFF[case][store] <= d <= 1.05 * K.EMUL_DIFF[case][store]      # (torch's float32 summation order moves the last digits)
    assert K.T[case][store] == 4 * K.EMUL_DIFF[case][store]
    # the views of a case have latents that differ by far more than the tolerance
    assert np.abs(l32[0] - l32[1]).max() > 10 * K.T[case]['bf16']


def test_head_cases_tile_sizes():
    """The A/B cases force the tile sizes they are named for, by the header's rule; the two geometries of the issue give 8 and 4."""
    assert {n: K.tile_samples(c[0]) for n, c in K.HEAD_CASES.items()} == {n: c[2] for n, c in K.HEAD_CASES.items()} == dict(t8=8, t8s=8, t4=4, t1=1)
    assert K.tile_samples(TNET_REP()) == 8 and K.tile_samples(TNET_REP(fc_in=6076)) == 4
    for name, (spec, D, _) in K.HEAD_CASES.items():
        spec.check_geometry(D, K.HEAD_HW, K.HEAD_HW)
    assert K.head_counts(8, 1024) == [1, 7, 8, 9, 29, 8193] and K.head_counts(1, 1024) == [1, 2, 8, 1025]


# -- host side without a device ---------------------------------------------------------------------------------------------------------
def test_morphology_table_offsets():
    from syconn_amd.reps.super_segmentation_helper import MorphologyTable
    lat, nl = np.arange(15, dtype=np.float32).reshape(5, 3), np.arange(12, dtype=np.float32).reshape(4, 3)
    t = MorphologyTable([7, 8, 9], lat, [0, 2, 2, 5], nl, [0, 3, 3, 4], [1, 0, 1, 2])
    assert len(t) == 3 and t.latent_of(0).shape == (2, 3) and t.latent_of(1).shape == (0, 3) and np.array_equal(t.latent_of(2), lat[2:])
    assert np.array_equal(t.node_latent_of(2), nl[3:]) and t.view_ixs_of(0).tolist() == [1, 0, 1] and t.view_ixs.dtype == np.int64
    for lb, nb, ix in (([0, 2, 5], [0, 3, 3, 4], [1, 0, 1, 2]), ([0, 2, 2, 4], [0, 3, 3, 4], [1, 0, 1, 2]), ([0, 2, 2, 5], [0, 3, 2, 4], [1, 0, 1, 2]),
                       ([0, 2, 2, 5], [0, 3, 3, 4], [1, 0, 1]), ([1, 2, 2, 5], [0, 3, 3, 4], [1, 0, 1, 2])):
        with pytest.raises(ValueError, match='MorphologyTable'):
            MorphologyTable([7, 8, 9], lat, lb, nl, nb, ix)


def test_input_forms_without_device():
    """The shape rules of EmbeddingModel's inputs (checked before anything reaches the device) and the entry point's refusal."""
    from syconn_amd.handler.prediction import EmbeddingModel, ViewSamples
    m = object.__new__(EmbeddingModel)      # no device here: the input rules only
    v4, v5 = np.zeros((3, 4, 6, 5), np.uint8), np.zeros((3, 4, 2, 6, 5), np.uint8)
    s = m._view0(v4)
    assert s.views.shape == (3, 4, 1, 6, 5) and s.table.tolist() == [[0], [1], [2]] and s.table.dtype == np.int32
    s = m._view0(v5)
    assert s.views is v5 and s.table.tolist() == [[0], [2], [4]]      # view 0 of every location, read in place
    s = m._view0(np.zeros((3, 4, 6, 5), np.float32) - np.float32(0.5))      # normalised zeros
    assert s.views.dtype == np.uint8 and s.views.shape == (3, 4, 1, 6, 5)
    keep = ViewSamples(v5, np.array([[1], [3]], np.int32))
    assert m._view0(keep) is keep
    with pytest.raises(ValueError, match=r'must be \(n, 1\)'):
        m._view0(ViewSamples(v5, np.zeros((2, 2), np.int32)))
    with pytest.raises(ValueError, match='views must be'):
        m._view0(v4[0])
    with pytest.raises(NotImplementedError):
        m._view0(np.full((1, 4, 6, 5), 0.3001, np.float32))
    with pytest.raises(ValueError, match='triple'):
        m.predict_proba((v4, v4))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            EmbeddingModel(TNET_REP(), E.state_dict_of(TNET_REP(), E.make_weights(TNET_REP(), 1, 128, 256)))


def test_nearest_locations_checks():
    from syconn_amd.reps.super_segmentation_helper import nearest_locations
    assert nearest_locations(np.zeros((0, 3)), [0, 0], [], np.zeros((0, 3))).shape == (0,)
    with pytest.raises(ValueError, match='cell 8 has skeleton nodes but no rendering location'):
        nearest_locations(np.zeros((2, 3), np.float32), [0, 2, 2], [0, 1], np.zeros((2, 3)), ids=[7, 8])


# -- the plan of the spec ------------------------------------------------------------------------------------------------------------------
def test_plan_dump_of_the_spec(tmp_path):
    """tools/viewnet_plan_dump on TNET_REP: every layer's padded shapes and K steps, the LDS of every halo tile, the geometry's workspace
    and multiply-adds, and the refusal of the other window."""
    exe = str(tmp_path / 'viewnet_plan_dump')
    hipcc = '/opt/rocm/bin/hipcc'
    assert os.path.isfile(hipcc), 'hipcc is needed to build tools/viewnet_plan_dump.cpp'
    subprocess.run([hipcc, '-O2', '-std=c++17', os.path.join(ROOT, 'syconn_amd', 'csrc', 'sd_viewnet_plan.cpp'),
                    os.path.join(ROOT, 'tools', 'viewnet_plan_dump.cpp'), '-o', exe], check=True, timeout=600)
    spec, H, W, arrs, _ = K.inputs('g372')
    floats = np.concatenate([a.ravel() for a in arrs]).astype(np.float32)
    with open(tmp_path / 'n.bin', 'wb') as f:
        f.write(b'SDVNET1\0' + struct.pack('<5iq', len(spec.layers), len(spec.linear_sizes) - 1, 4, 0, 0, floats.size))
        f.write(np.asarray(spec.layers, np.int32).tobytes() + np.asarray(spec.linear_sizes, np.int32).tobytes() + floats.tobytes())
    r = subprocess.run([exe, str(tmp_path / 'n.bin'), '--dtypes', 'f16', '--geom', '1,128,256:800', '--geom', '1,512,512'], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert out[0].startswith('dtype f16 rc 0')
    f = {l.split()[1]: dict(zip(l.split()[2::2], l.split()[3::2])) for l in out if l.startswith('layer ')}
    # cin_p: 4 for the uint8 input, else channels rounded up to 8; NT = cout in tiles of 16; nks = taps x cin_p in steps of 32
    assert [(f[str(i)]['cin_p'], f[str(i)]['cout_p'], f[str(i)]['NT'], f[str(i)]['nks']) for i in range(7)] == [
        ('4', '16', '1', '4'), ('16', '24', '2', '13'), ('24', '32', '2', '12'), ('32', '32', '2', '16'), ('32', '32', '2', '4'),
        ('32', '32', '2', '4'), ('32', '32', '2', '1')]
    assert all(int(v['lds']) <= 65536 for v in f.values())
    geom = [l for l in out if l.startswith('geom ')]
    assert geom[0].startswith('geom 1 128 256 n 800 workspace ') and geom[0].endswith(f'macs {spec.macs_per_sample(1, 128, 256)}')
    assert geom[1] == 'geom 1 512 512 n 1 error: viewnet: the layers give 6076 features + 0 scalars, the first Linear takes 372'
