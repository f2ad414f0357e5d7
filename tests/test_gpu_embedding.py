"""The morphology embedding on the device: the sample-tiled head (``sd_viewnet_embed``) against the per-sample head
(``sd_viewnet_forward``) bit for bit, every layer and Linear of the representation network as one op against the float64 reference on
the device's own stored input, the latents against the float32 restatement and the golden of the reference's own module
(tests/golden/g31_embedding.npz), the input layouts and launch sets, flags, guard bands, argument checks, and the chain
``view_embedding_of_sso_nocache`` / ``embed_cells_table`` / ``collect_properties_from_ssv_partners`` / ``predict_celltype_multiview`` on
the synthetic cell of the view tests."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import _embedding_cases as K
import _embedding_ref as E
import _viewnet_cases as VK
import _viewnet_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _emb(spec, arrs, store, gpu, bs=800, prefix=''):
    from syconn_amd.handler.prediction import EmbeddingModel
    sd = E.state_dict_of(spec, arrs, prefix) if spec.conv_ndim == 2 else R.state_dict_of(spec, arrs)
    return EmbeddingModel(spec, sd, act_dtype=store, bs=bs, device=gpu)


def _planes(views):
    n, Cc, D, H, W = views.shape
    return np.ascontiguousarray(views.transpose(0, 2, 3, 4, 1)).reshape(n * D, H, W, Cc)


# -- the tiled head against the per-sample head ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('store', K.STORES)
@pytest.mark.parametrize('name', list(K.HEAD_CASES))
def test_tiled_head_equals_per_sample_head(gpu, name, store):
    """The same model, views and table through ``sd_viewnet_forward`` and ``sd_viewnet_embed``: logits and every buffer are the same
    bits at 1, TS - 1, TS, TS + 1, 3 TS + 5 samples and one sample past a full grid stride of tiles.  t8s has scalars, D = 3, LeakyReLU
    and two hidden Linear layers; t4 and t1 force the smaller tiles."""
    from syconn_amd import _lib as L
    from syconn_amd.handler.prediction import ViewModel, ViewSamples
    spec, D, arrs, pool, scal = K.head_inputs(name)
    ts = K.HEAD_CASES[name][2]
    sd = R.state_dict_of(spec, arrs)
    fwd = ViewModel(spec, sd, act_dtype=store, device=gpu)
    emb = _emb(spec, arrs, store, gpu)
    assert emb.tile_samples == ts == K.tile_samples(spec) and fwd._entry == 'sd_viewnet_forward' and emb._entry == 'sd_viewnet_embed'
    pool_d = torch.from_numpy(pool).to(gpu)
    nl, n_fc = len(spec.layers), len(spec.linear_sizes) - 1
    counts = K.head_counts(ts, L.SD_VIEWNET_HEAD_TILE_GRID)
    assert counts[-1] == ts * L.SD_VIEWNET_HEAD_TILE_GRID + 1 and {1, ts, ts + 1, 3 * ts + 5} <= set(counts)
    for n in counts:
        loc = (np.arange(n) * 5 + 3) % len(pool)
        sm = ViewSamples(pool_d, (loc[:, None] * D + np.arange(D)[None]).astype(np.int32))
        inp = (sm, scal[loc]) if spec.n_scalar else sm
        want = fwd.predict_proba(inp, bs=n)
        got = emb.forward_samples(inp, bs=n)
        assert want.shape == (n, spec.n_classes) and np.isfinite(want).all() and len(np.unique(want[:37], axis=0)) == min(n, 37)
        assert np.array_equal(got, want), (name, store, n)
        for j in range(n_fc):
            a, b = fwd.read_buffer(nl + j), emb.read_buffer(nl + j)
            assert a.shape == (n, spec.linear_sizes[j + 1]) and np.array_equal(a, b), (name, store, n, j)
        assert np.array_equal(emb.read_buffer(nl + n_fc - 1), got)      # the last Linear's buffer is the logits
        if n <= 3 * ts + 5:
            for i in range(nl):
                assert np.array_equal(fwd.read_buffer(i), emb.read_buffer(i))


# -- every layer and every Linear as one op; the latents -----------------------------------------------------------------------------
def _step_checks(model, spec, arrs, store, views5, latents):
    """Every op of the last launch set against StepRef on the device's own stored input, with the bound of tests/test_gpu_viewnet.py.
    -> the share of the bound each op used."""
    sr = R.StepRef(E.spec5(spec), arrs, store)
    assert model.num_ops == sr.n_ops()
    x, shares = _planes(views5), []
    for i in range(sr.nl):
        dev = torch.from_numpy(model.read_buffer(i)).double()
        ref, S = sr.layer(i, x)
        assert dev.shape == ref.shape, (i, dev.shape, ref.shape)
        assert torch.isfinite(dev).all()
        ratio = ((dev - ref).abs() / R.bound_stored(ref, S, K.C[store], store)).max().item()
        assert ratio <= 1, f'layer {i}: |dev - ref| is {ratio:.3f} of the bound'
        shares.append(ratio)
        x = dev.numpy()
    v = sr.head_input(x, None, 1).float()
    for j in range(sr.n_fc):
        dev = torch.from_numpy(model.read_buffer(sr.nl + j)).double()
        ref, S = sr.linear(j, v)
        assert dev.shape == ref.shape
        ratio = ((dev - ref).abs() / R.bound_f32(ref, S, K.C[store])).max().item()
        assert ratio <= 1, f'Linear {j}: |dev - ref| is {ratio:.3f} of the bound'
        shares.append(ratio)
        v = dev.float()
    assert np.array_equal(v.numpy(), latents)
    return shares


@pytest.mark.parametrize('store', K.STORES)
@pytest.mark.parametrize('name', list(K.GEOMS))
def test_steps_and_latents(gpu, name, store):
    """The three geometries -- 128 x 256 (TS = 8), the 92 x 92 minimum (nine samples: a full tile and a tile of one), 512 x 512 with the
    literal Linear(6076, 50) (TS = 4) --: all seven layers (layer 3: k = 4 without a pool; layers 5 and 6: k = 2 with a pool) and both
    Linear layers as single ops, and the latents within T of the float32 restatement on the stored weights."""
    spec, H, W, arrs, views = K.inputs(name)
    m = _emb(spec, arrs, store, gpu, prefix='rep_net.')
    assert m.tile_samples == (4 if name == 'g6076' else 8)
    lat = m.predict_proba(views)
    assert lat.shape == (len(views), K.Z) and lat.dtype == np.float32
    shares = _step_checks(m, spec, arrs, store, E._views5(views), lat)
    d = np.abs(lat - E.latent32(spec, arrs, views, store)).max()
    print(f'{name} {store}: shares of the bound {[round(s, 3) for s in shares]}; |latent - float32| {d:.5f} of T = {K.T[name][store]:.5f}')
    assert d <= K.T[name][store]


# -- the golden of the reference's own functions -----------------------------------------------------------------------------------------
class _Skel:
    """The part of a cell the embedding functions touch besides the mesh."""
    view_caching = True

    def __init__(self, nodes, scaling, views=None, locs=None):
        self.skeleton, self.scaling, self.view_dict, self.saved = {'nodes': nodes}, scaling, {}, 0
        self._views, self._locs = views, locs

    def load_views(self, view_key=None):
        return self._views if view_key is None else self.view_dict[view_key]

    def sample_locations(self):
        return [self._locs[:2], self._locs[2:]]      # per supervoxel, as the reference hands them out

    def load_skeleton(self):
        pass

    def save_skeleton(self):
        self.saved += 1


@pytest.mark.parametrize('store', K.STORES)
@pytest.mark.parametrize('name', list(K.GOLDEN))
def test_golden(gpu, name, store):
    """Both geometries through ``predict_views_embedding``: the latents within the CPU-measured T of the reference module's, the node
    -> location map (``view_ixs``) the reference's own cKDTree result bit for bit, ties included, and ``node_latent = latent[view_ixs]``
    exactly."""
    from syconn_amd.reps.super_segmentation_object import predict_views_embedding
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g31_embedding.npz'))
    spec = K.GEOMS[K.GOLDEN[name][0]][0]
    arrs = K.golden_weights(name)
    views, locs, nodes = K.golden_cell(name)
    assert K.crc(views, locs, nodes, *arrs) == g[f'{name}_crc']
    m = _emb(spec, arrs, store, gpu, prefix='rep_net.')
    T = K.T['golden_' + name][store]
    lat = m.predict_proba(views)
    d = np.abs(lat - g[f'{name}_latent']).max()
    print(f'golden {name} {store}: |latent - reference| {d:.5f} of T = {T:.5f}; {int(g[f"{name}_tie"].sum())} ties among {len(nodes)} nodes')
    assert d <= T
    cell = _Skel(nodes, K.GOLDEN_SCALING, views, locs)
    node_latent = predict_views_embedding(cell, m)
    assert cell.saved == 1 and cell.skeleton['latent_morph'] is node_latent and node_latent.dtype == np.float32
    ixs = cell.skeleton['view_ixs']
    assert ixs.dtype == np.int64 and np.array_equal(ixs, g[f'{name}_view_ixs'])
    assert np.array_equal(node_latent, lat[ixs])
    assert np.abs(node_latent - g[f'{name}_node_latent']).max() <= T
    # the stored view_ixs are reused (the reference's branch): put the nodes elsewhere, the map stays
    cell.skeleton['nodes'] = nodes[::-1].copy()
    assert np.array_equal(predict_views_embedding(cell, m, pred_key_appendix='_x'), node_latent) and 'latent_morph_x' in cell.skeleton
    # stale indices (another number of views, or of nodes) are an IndexError on the host, as the reference's latent[ixs] is
    for stale in (np.where(np.arange(len(ixs)) == 3, len(views), ixs), np.where(np.arange(len(ixs)) == 0, -1, ixs), ixs[:-1]):
        cell.skeleton['view_ixs'] = stale
        with pytest.raises(IndexError, match='view_ixs'):
            predict_views_embedding(cell, m)


# -- layout and calls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('store', K.STORES)
def test_input_forms_and_launch_sets(gpu, store):
    """The renderer's 5-D tensor read in place (host and device) = the sliced 4-D copy = the normalised float32 views = a sample table =
    the reference's triple; launch sets of 1, 7 and all samples: the same bits."""
    from syconn_amd.handler.prediction import ViewSamples, naive_view_normalization_new
    spec, H, W, arrs, views = K.inputs('min')
    m = _emb(spec, arrs, store, gpu)
    n = len(views)
    v0 = np.ascontiguousarray(views[:, :, 0])
    want = m.predict_proba(v0)
    assert len(np.unique(want, axis=0)) == n
    vd = torch.from_numpy(views).to(gpu)
    for form in (views, vd, torch.from_numpy(v0), naive_view_normalization_new(v0), ViewSamples(vd, np.arange(0, 2 * n, 2, dtype=np.int32)[:, None])):
        assert np.array_equal(m.predict_proba(form), want)
    assert not np.array_equal(m.predict_proba(np.ascontiguousarray(views[:, :, 1])), want)      # view 1 is another picture
    assert np.array_equal(m.predict_proba(ViewSamples(vd, np.arange(1, 2 * n, 2, dtype=np.int32)[:, None])), m.predict_proba(np.ascontiguousarray(views[:, :, 1])))
    x = naive_view_normalization_new(v0)
    res = m.predict_proba((x, np.zeros_like(x), np.zeros_like(x)))
    assert isinstance(res, tuple) and len(res) == 5 and [r is None for r in res] == [True, True, False, True, True] and np.array_equal(res[2], want)
    _, _, latent, _, _ = m.predict_proba([x, None, None])
    assert np.array_equal(latent, want)
    for bs in (1, 7, n, 4 * n):
        assert np.array_equal(m.predict_proba(vd, bs=bs), want), bs
    assert m.read_buffer(len(spec.layers) + 1).shape == (n, K.Z)
    assert np.array_equal(m.predict_device(vd).cpu().numpy(), want) and m.predict_device(vd).is_cuda
    # the last launch set of bs = 7 holds samples 7, 8
    m.predict_proba(vd, bs=7)
    assert np.array_equal(m.read_buffer(len(spec.layers) + 1), want[7:])


def test_table_out_of_range(gpu):
    from syconn_amd.handler.prediction import ViewSamples
    spec, D, arrs, pool, _ = K.head_inputs('t8')
    m = _emb(spec, arrs, 'f16', gpu)
    table = np.arange(11, dtype=np.int32)[:, None]
    want = m.predict_proba(ViewSamples(pool, table))
    for bad in (37, -1, 2 ** 31 - 1):
        t = table.copy()
        t[9, 0] = bad      # in the partial second tile
        with pytest.raises(IndexError, match=r'outside \[0, 37\)'):
            m.predict_proba(ViewSamples(pool, t))
    assert np.array_equal(m.predict_proba(ViewSamples(pool, table)), want)      # ... and the model still works


def test_f16_overflow_flag(gpu):
    """First-layer weights scaled so that the largest stored activation of layer 0 passes 65504 (about 75,000): fp16 storage raises and
    names bf16, bf16 runs; scaled to about 64,700 nothing is flagged.  The gains follow from the float64 reference of layer 0, whose
    largest value is linear in the gain."""
    from syconn_amd import _lib as L
    spec, D, _, pool, _ = K.head_inputs('t8')
    views = pool[:9]
    x = _planes(views)

    def top(gain):
        arrs = R.make_weights(spec, 41, D, K.HEAD_HW, K.HEAD_HW, gain=gain)
        assert np.abs(arrs[0]).max() < 30000
        return arrs, float(R.StepRef(spec, arrs, 'f16').layer(0, x)[0].max())

    (_, t1), (_, t2) = top(1.0), top(2.0)
    slope, offset = t2 - t1, 2 * t1 - t2      # top(gain) = slope gain + offset while the same pixel stays the largest
    over, t = top((75000.0 - offset) / slope)
    assert 70000 < t < 80000
    with pytest.raises(L.ActivationOverflowError, match="act_dtype='bf16'"):
        _emb(spec, over, 'f16', gpu).predict_proba(views)
    assert np.isfinite(_emb(spec, over, 'bf16', gpu).predict_proba(views)).all()
    under, t = top((64700.0 - offset) / slope)
    assert 64000 < t < 65400
    m = _emb(spec, under, 'f16', gpu)
    assert np.isfinite(m.predict_proba(views)).all()
    stored = m.read_buffer(0)
    assert np.isfinite(stored).all() and 64000 < stored.max() <= 65504


def _layout(spec, n, D, H, W):
    """The workspace layout of syconn_amd/csrc/sd_viewnet_plan.cpp -> [(offset, used bytes)], total."""
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
@pytest.mark.parametrize('name, n', [('t8s', 11), ('t8', 1), ('t4', 7)])
def test_guard_bands(gpu, name, n, store):
    """A partial last tile (11 = 8 + 3, 7 = 4 + 3) and a tile of one: nothing is written behind the workspace, the logits, a layer's
    buffer or a hidden vector."""
    from syconn_amd import _dev as dv
    from syconn_amd import _lib as L
    spec, D, arrs, pool, scal = K.head_inputs(name)
    m = _emb(spec, arrs, store, gpu)
    H = W = K.HEAD_HW
    views, sc = pool[:n], scal[:n]
    want = m.forward_samples((views, sc) if spec.n_scalar else views)
    ranges, total = _layout(spec, n, D, H, W)
    assert L.load().sd_viewnet_workspace_bytes(m._h, n, D, H, W) == total
    ws = torch.full((total + 4096,), 0xA5, dtype=torch.uint8, device=gpu)
    logits = torch.full((n * spec.n_classes + 64,), -7.0, dtype=torch.float32, device=gpu)
    flags = torch.full((6,), 9, dtype=torch.int32, device=gpu)
    table = torch.arange(n * D, dtype=torch.int32, device=gpu)
    dv.call('sd_viewnet_embed', gpu, m._h, torch.from_numpy(views).to(gpu), n * D, D, H, W, table, n, D,
            torch.from_numpy(sc).to(gpu) if spec.n_scalar else None, logits, ws, total, flags)
    torch.cuda.synchronize(gpu)
    assert np.array_equal(logits[:n * spec.n_classes].cpu().numpy().reshape(n, -1), want)
    assert (logits[n * spec.n_classes:] == -7.0).all() and (ws[total:] == 0xA5).all()
    assert flags.cpu().tolist() == [0, 0, 9, 9, 9, 9]
    ends = [o for o, _ in ranges[1:]] + [total]
    for (off, used), end in zip(ranges, ends):
        assert (ws[off + used:end] == 0xA5).all(), (off, used, end)


def test_argument_checks(gpu):
    """Every check of ``sd_viewnet_embed`` and ``sd_viewnet_embed_timed``; the timed entry gives the same bits and one time per launch."""
    from syconn_amd import _dev as dv
    from syconn_amd import _lib as L
    from syconn_amd.handler.prediction import EmbeddingModel
    spec, D, arrs, pool, scal = K.head_inputs('t8s')
    sd = R.state_dict_of(spec, arrs)
    with pytest.raises(ValueError, match='act_dtype'):
        EmbeddingModel(spec, sd, act_dtype='f32', device=gpu)
    with pytest.raises(ValueError, match='bs must be positive'):
        EmbeddingModel(spec, sd, bs=0, device=gpu)
    with pytest.raises(ValueError, match='has shape'):
        EmbeddingModel(spec, {k: (v[:-1] if k == 'fc.0.bias' else v) for k, v in sd.items()}, device=gpu)
    m = EmbeddingModel(spec, sd, device=gpu)
    assert m.bs == 800
    n, H, W = 11, K.HEAD_HW, K.HEAD_HW
    views, sc_h = pool[:n], scal[:n]
    want = m.forward_samples((views, sc_h))
    for msg, call in {'flattens to': lambda: m.predict_proba(views[:, :, 0]), 'takes 2 scalars': lambda: m.forward_samples(views),
                      'bs must be positive': lambda: m.forward_samples((views, sc_h), bs=0),
                      'views have 3 channels': lambda: m.forward_samples((views[:, :3], sc_h))}.items():
        with pytest.raises(ValueError, match=msg):
            call()
    vd, sc, tb = torch.from_numpy(views).to(gpu), torch.from_numpy(sc_h).to(gpu), torch.arange(n * D, dtype=torch.int32, device=gpu)
    ws = dv.scratch('sd_viewnet_workspace_bytes', gpu, m._h, n, D, H, W)
    lg, fl = torch.zeros((n, spec.n_classes), device=gpu), torch.zeros(2, dtype=torch.int32, device=gpu)
    good = [m._h, vd, n * D, D, H, W, tb, n, D, sc, lg, ws, ws.numel(), fl]
    lib = L.load()
    nl = len(spec.layers)
    ms = (C.c_float * (nl + 2))(*([-1.0] * (nl + 2)))
    for entry in ('sd_viewnet_embed', 'sd_viewnet_embed_timed'):
        timed = entry.endswith('_timed')

        def run(args):
            if timed:
                L.check(getattr(lib, entry)(*dv.pointers(args), dv.stream(gpu), ms), entry)
            else:
                dv.call(entry, gpu, *args)

        lg.zero_()
        run(good)
        assert np.array_equal(lg.cpu().numpy(), want) and fl.cpu().tolist() == [0, 0]
        for pos, val, msg in ((0, None, 'null'), (1, None, 'null'), (6, None, 'null'), (10, None, 'null'), (11, None, 'null'), (13, None, 'null'),
                              (9, None, 'scalars_dev is null'), (12, ws.numel() - 1, 'workspace smaller'), (3, 0, 'multiple of nb_views'),
                              (3, 2, 'multiple of nb_views'), (2, 0, 'multiple of nb_views'), (4, 5, 'empty output'), (8, 2, 'features'),
                              (7, 0, 'n_samples out of range'), (11, ws[1:], '16-byte aligned')):
            args = list(good)
            args[pos] = val
            with pytest.raises(ValueError, match=msg):
                run(args)
    assert all(0 <= t < 1000 for t in list(ms)[:-1]) and ms[nl + 1] == -1.0      # n_layers + 1 values, nothing behind them
    assert lib.sd_viewnet_embed_timed(*dv.pointers(good), dv.stream(gpu), None) == L.SD_ERR_INVALID
    assert lib.sd_viewnet_embed_tile_samples(None) == 0 and lib.sd_viewnet_embed_tile_samples(m._h) == 8
    # sd_viewnet_read_buffer after the embed entry
    dims = (C.c_int32 * 4)()
    for idx in (-1, nl + 3):
        assert lib.sd_viewnet_read_buffer(m._h, idx, ws.data_ptr(), lg.data_ptr(), n, D, H, W, None, dims, None) == L.SD_ERR_INVALID
    assert lib.sd_viewnet_read_buffer(m._h, nl + 1, ws.data_ptr(), lg.data_ptr(), n, D, H, W, None, dims, None) == 0 and list(dims) == [n, 1, 1, 11]
    out = np.empty((n, spec.n_classes), np.float32)
    assert lib.sd_viewnet_read_buffer(m._h, nl + 2, ws.data_ptr(), lg.data_ptr(), n, D, H, W, out.ctypes.data_as(C.POINTER(C.c_float)), dims, None) == 0
    assert np.array_equal(out, want)


# -- the chain on the synthetic cell of the view tests --------------------------------------------------------------------------------------
SCALE = np.array([50., 50., 50.], np.float32)


class _Cell(_Skel):
    def __init__(self, tris, verts, n_nodes, seed):
        rng = np.random.default_rng(seed)
        v = np.asarray(verts, np.float32).reshape(-1, 3)
        nodes = np.rint(v[rng.choice(len(v), n_nodes, replace=False)] / SCALE).astype(np.int64) + rng.integers(-2, 3, (n_nodes, 3))
        super().__init__(nodes, SCALE)
        self.mesh = (tris, verts)
        self.attr_dict, self.syn_props = {}, (rng.choice([-1, 1], 6), rng.uniform(0.1, 2, 6), rng.integers(0, 5, 6))

    def load_mesh(self, name):
        if name == 'mi':
            return (self.mesh[0][:len(self.mesh[0]) // 3], self.mesh[1])
        return (np.zeros(0, np.uint32), np.zeros((0, 3), np.float32))

    def sample_locations(self):
        return self._sample_locations

    def save_attributes(self, keys, values):
        pass


@pytest.fixture(scope='module')
def cells(gpu):
    spec_ = importlib.util.spec_from_file_location('views_probe', os.path.join(ROOT, 'tools', 'views_probe.py'))
    probe = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(probe)
    from syconn_amd.proc import meshes
    out = []
    for seed, shape, n_nodes in ((0, (256, 192, 128), 41), (1, (160, 128, 96), 23)):
        t = meshes.find_meshes_table(probe.make_cell(shape, seed), (0, 0, 0), scaling=(50.,) * 3, meshing_props={'normals': False}, device=gpu)
        out.append(_Cell(np.asarray(t.indices), np.asarray(t.vertices, np.float32), n_nodes, seed))
    return out


VIEW_KW = dict(ws=(256, 128), nb_views=2, comp_window=4000.0)


@pytest.mark.parametrize('store', K.STORES)
def test_view_embedding_end_to_end(gpu, cells, store):
    """``view_embedding_of_sso_nocache``: locations, render on the device, embed view 0, nearest location.  The stored node latents are
    ``latent[ixs]`` with ``ixs`` the float64 nearest location restated on the host (lower row on ties); the latents of the rendered
    views are within T of the float32 restatement on the downloaded views, T = 4 x |emulation - restatement| on those very views
    (CPU only, as tests/_embedding_cases.py measures it)."""
    from syconn_amd.reps.super_segmentation_helper import view_embedding_of_sso_nocache
    spec, H, W, arrs, _ = K.inputs('g372')
    m = _emb(spec, arrs, store, gpu)
    cell = cells[0]
    cell.view_dict.clear()
    saved = cell.saved
    out = view_embedding_of_sso_nocache(cell, m, device=gpu, **VIEW_KW)
    views_d = cell.view_dict['tmp_views']
    assert isinstance(views_d, torch.Tensor) and views_d.is_cuda and views_d.shape[1:] == (4, 2, 128, 256) and 20 <= len(views_d) <= 200
    locs = np.concatenate(cell.sample_locations())
    assert len(locs) == len(views_d) and cell.saved == saved + 1
    assert out.shape == (len(cell.skeleton['nodes']), K.Z) and out.dtype == np.float32 and cell.skeleton['latent_morph'] is out
    lat = m.predict_proba(views_d)
    ixs, tie = E.nearest_rows(locs, cell.skeleton['nodes'] * SCALE)
    assert np.array_equal(out, lat[ixs]) and len(np.unique(ixs)) > 5
    views = views_d.cpu().numpy()
    l32 = E.latent32(spec, arrs, views, store)
    T = 4 * np.abs(E.latent_emul(spec, arrs, views, store) - l32).max()
    d = np.abs(lat - l32).max()
    print(f'cell 0 {store}: {len(views)} locations, {len(ixs)} nodes ({int(tie.sum())} ties), |latent - float32| {d:.5f} of T = {T:.5f}')
    assert d <= T
    # overwrite=False: the cached views and locations are used again (nothing is rendered: the tensor is the same object)
    again = view_embedding_of_sso_nocache(cell, m, overwrite=False, pred_key_appendix='', device=gpu, **VIEW_KW)
    assert cell.view_dict['tmp_views'] is views_d and np.array_equal(again, out)
    other = view_embedding_of_sso_nocache(cell, m, pred_key_appendix='_ct', device=gpu, **VIEW_KW)
    assert np.array_equal(other, out) and 'tmp_views_ct' in cell.view_dict and 'latent_morph_ct' in cell.skeleton
    empty = _Skel(cell.skeleton['nodes'], SCALE)
    empty.mesh, empty.load_mesh = (np.zeros(0, np.uint32), np.zeros((0, 3), np.float32)), cell.load_mesh
    empty.view_dict['tmp_views'], empty._sample_locations = views_d[:0], [locs[:0]]
    empty.sample_locations = lambda: empty._sample_locations
    with pytest.raises(ValueError, match='no rendering location'):
        view_embedding_of_sso_nocache(empty, m, overwrite=False, device=gpu, **VIEW_KW)


class _Syn:
    def __init__(self, partners, rep, ratio):
        self.neuron_partners, self.rep_coords, self.syn_type_sym_ratio = partners, rep, ratio

    def __len__(self):
        return len(self.syn_type_sym_ratio)


@pytest.mark.parametrize('store', K.STORES)
def test_cells_table_equals_single_calls(gpu, cells, store):
    """Three cells through one pass (launch sets of 7 planes cut across the cells, one nearest-location call) = three single calls, bit
    for bit; the table's node latents in a ``CellTable`` give every synapse the latent of its partner's nearest skeleton node."""
    from syconn_amd.exec.exec_inference import run_morphology_embedding
    from syconn_amd.extraction.cs_processing_steps import CellTable, collect_properties_from_ssv_partners
    from syconn_amd.handler.multiviews import generate_rendering_locs
    from syconn_amd.proc.rendering import render_sso_coords
    from syconn_amd.reps.super_segmentation_helper import embed_cells_table, view_embedding_of_sso_nocache
    spec, H, W, arrs, _ = K.inputs('g372')
    m = _emb(spec, arrs, store, gpu)
    third = _Cell(cells[1].mesh[0], cells[1].mesh[1], 9, 5)
    trio = [cells[0], cells[1], third]
    views, locs = [], []
    for c, take in zip(trio, (slice(0, 23), slice(0, 11), slice(3, 8))):
        l = generate_rendering_locs(np.asarray(c.mesh[1]).reshape(-1, 3), 4000.0 / 3, device=gpu)[take]
        views.append(render_sso_coords(c, l, add_cellobjects=True, device=gpu, return_device=True, **VIEW_KW))
        locs.append(l)
    assert [len(v) for v in views] == [23, 11, 5]
    table = embed_cells_table(trio, m, views=views, locations=locs, bs=7, ids=[7, 8, 9])
    assert table.loc_begin.tolist() == [0, 23, 34, 39] and table.node_begin.tolist() == [0, 41, 64, 73] and len(table) == 3
    assert table.latent.shape == (39, K.Z) and table.node_latent.shape == (73, K.Z) and table.latent.dtype == table.node_latent.dtype == np.float32
    for k, (c, v, l) in enumerate(zip(trio, views, locs)):
        c.view_dict['tmp_views'], c._sample_locations = v, l[None]
        single = view_embedding_of_sso_nocache(c, m, overwrite=False, device=gpu, **VIEW_KW)
        assert np.array_equal(table.node_latent_of(k), single), k
        assert np.array_equal(table.latent_of(k), m.predict_proba(v))
        assert np.array_equal(table.view_ixs_of(k), E.nearest_rows(l, c.skeleton['nodes'] * SCALE)[0])
        assert np.array_equal(table.node_latent_of(k), table.latent_of(k)[table.view_ixs_of(k)])
    same = run_morphology_embedding(trio, m, ids=[7, 8, 9])      # views and locations from the cells, the model's own launch sets
    assert np.array_equal(same.node_latent, table.node_latent) and np.array_equal(same.view_ixs, table.view_ixs) and np.array_equal(same.latent, table.latent)
    # into the synapse properties
    verts = [np.asarray(c.mesh[1], np.float32).reshape(-1, 3) for c in trio]
    nodes = [c.skeleton['nodes'] for c in trio]
    ct = CellTable([7, 8, 9], np.concatenate(verts), np.concatenate(([0], np.cumsum([len(v) for v in verts]))),
                   {'spiness': np.zeros(sum(len(v) for v in verts), np.int32)}, np.concatenate(nodes), table.node_begin, {'latent_morph': table.node_latent})
    rng = np.random.default_rng(3)
    n_syn = 12
    partners = np.stack([rng.choice([7, 8, 9], n_syn), rng.choice([7, 8, 9], n_syn)], 1).astype(np.uint64)
    rep = np.stack([rng.integers(0, 256, n_syn), rng.integers(0, 192, n_syn), rng.integers(0, 128, n_syn)], 1).astype(np.int32)
    props = collect_properties_from_ssv_partners(_Syn(partners, rep, rng.uniform(0, 1, n_syn)), ct, scaling=SCALE, k=1, ds_vertices=1, ignore_labels=[],
                                                 pred_key_ax='ax', n_embedding=K.Z, sym_thresh=0.5, device=gpu)
    assert props.latent_morph.shape == (n_syn, 2, K.Z)
    for i in range(n_syn):
        for side in range(2):
            k = int(partners[i, side]) - 7
            row = E.nearest_rows(nodes[k] * SCALE.astype(np.float64), rep[i].astype(np.float64) * SCALE)[0][0]
            assert np.array_equal(props.latent_morph[i, side], table.node_latent_of(k)[row]), (i, side)


def test_celltype_multiview_with_tnet(gpu, cells):
    """``predict_celltype_multiview(model_tnet=EmbeddingModel)`` writes the cell type and then ``latent_morph`` + appendix, as the
    reference does; any other `model_tnet` object still raises before anything runs."""
    from syconn_amd.handler.prediction import ViewModel
    from syconn_amd.reps.super_segmentation_helper import view_embedding_of_sso_nocache
    from syconn_amd.reps.super_segmentation_object import predict_celltype_multiview
    cspec, _, _, _, carrs, _, _ = VK.inputs('cmn')
    cmn = ViewModel(cspec, R.state_dict_of(cspec, carrs), act_dtype='f16', device=gpu)
    spec, H, W, arrs, _ = K.inputs('g372')
    m = _emb(spec, arrs, 'f16', gpu)
    cell = cells[1]
    cell.view_dict.clear()
    cell.attr_dict.clear()
    cell.skeleton = {'nodes': cell.skeleton['nodes']}
    with pytest.raises(NotImplementedError):
        predict_celltype_multiview(cell, cmn, model_tnet=object())
    assert not cell.attr_dict and not cell.view_dict and list(cell.skeleton) == ['nodes']
    got = predict_celltype_multiview(cell, cmn, pred_key_appendix='_ct', model_tnet=m, onthefly_views=True, view_props=dict(comp_window=4000.0), device=gpu)
    assert got[0] == cell.attr_dict['celltype_cnn_e3_ct'] and 'tmp_views_ct' in cell.view_dict
    lm = cell.skeleton['latent_morph_ct']
    assert lm.shape == (len(cell.skeleton['nodes']), K.Z)
    assert np.array_equal(lm, view_embedding_of_sso_nocache(cell, m, pred_key_appendix='_ct', overwrite=False, device=gpu, ws=(256, 128), nb_views=2,
                                                            comp_window=4000.0))
