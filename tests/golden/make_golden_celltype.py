"""Golden vectors for the cell type step, produced by the REFERENCE'S OWN code, lifted by AST at generation time and run unchanged on
torch-CPU float32 / numpy / scipy: ``StackedConv2ScalarWithLatentAdd`` (/root/reference/syconn/cnn/cnn_celltype_cmn_j0251.py:22-60),
``sso_views_to_modelinput``, ``syn_sign_ratio_celltype`` and ``celltype_of_sso_nocache`` (reps/super_segmentation_helper.py:180-213,
:1981-2065, :1670-1755; its vote block :1733-1749 also alone, on crafted logits), ``naive_view_normalization_new`` and
``certainty_estimate`` (handler/prediction.py:1096-1097, :1197-1227).  Nothing compiled and no reference text is stored: outputs only,
and a CRC of the generated inputs and weights, so that a drift of the generators of tests/_viewnet_ref.py shows as itself.

    python tests/golden/make_golden_celltype.py      ->  tests/golden/g29_celltype.npz

Stated stand-ins (not reference code): elektronn3's ``Conv3DLayer`` = ``Conv3d(cin, cout, k)`` without padding -> ``MaxPool3d(pooling)`` ->
activation (syconn_amd/cnn/viewnet_spec.py says what of that the tree pins); ``InferenceModel.predict_proba`` = the module on float32
tensors; the cell object with its storages (views, attribute dict, synapse objects, ``attr_for_coords``), ``generate_rendering_locs`` and
``render_sso_coords`` (they hand out the generated locations / views), ``load_so_attr_bulk``, ``global_params.config``."""
import ast
import os
import sys
import types

import numpy as np
import scipy.special
import scipy.stats
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _viewnet_ref as R  # noqa: E402
from _viewnet_cases import GOLDEN_CELLS as CELLS, GOLDEN_WEIGHT_SEED as WEIGHT_SEED, crc, golden_cell_inputs as cell_inputs  # noqa: E402
from make_golden_cs import lift_function  # noqa: E402
from syconn_amd.cnn.viewnet_spec import CELLTYPE_CMN  # noqa: E402

REF = '/root/reference/syconn'


class Conv3DLayer(nn.Module):      # the stand-in
    def __init__(self, cin, cout, kernel_size, pooling, dropout_rate, act):
        super().__init__()
        self.conv, self.pool, self.act = nn.Conv3d(cin, cout, kernel_size), nn.MaxPool3d(pooling), act

    def forward(self, x):
        return self.act(self.pool(self.conv(x)))


def lift_class(path, name, ns):
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.ClassDef) and node.name == name:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, 'exec'), ns)
            return ns[name]
    raise KeyError(name)


def lift_vote_block(path):
    """The statements of celltype_of_sso_nocache from ``if da_equals_tan:`` to ``pred = np.argmax(major_dec)`` as a function of
    (res, da_equals_tan, n_classes) -> (pred, res)."""
    fn = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name == 'celltype_of_sso_nocache'][0]
    start = [i for i, n in enumerate(fn.body) if isinstance(n, ast.If) and ast.unparse(n.test) == 'da_equals_tan'][0]
    end = [i for i, n in enumerate(fn.body) if isinstance(n, ast.Assign) and ast.unparse(n) == 'pred = np.argmax(major_dec)'][0]
    body = fn.body[start:end + 1] + [ast.parse('return pred, res').body[0]]
    new = ast.parse('def vote(res, da_equals_tan, n_classes):\n    pass').body[0]
    new.body = body
    ns = {'np': np}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[new], type_ignores=[])), path, 'exec'), ns)
    return ns['vote']


def namespaces():
    pred = {'np': np, 'softmax': scipy.special.softmax, 'entropy': scipy.stats.entropy}
    for name in ('naive_view_normalization_new', 'certainty_estimate'):
        lift_function(f'{REF}/handler/prediction.py', name, pred)
    # celltype_of_sso_nocache imports the normalisation relatively: give the lifted functions a package to import it from
    for mod in ('refpkg', 'refpkg.reps', 'refpkg.handler'):
        sys.modules[mod] = types.ModuleType(mod)
        sys.modules[mod].__path__ = []
    hp = types.ModuleType('refpkg.handler.prediction')
    hp.naive_view_normalization_new = pred['naive_view_normalization_new']
    sys.modules['refpkg.handler.prediction'] = hp
    cfg = {'compartments': {'view_properties_semsegax': {'semseg_key': 'axoness'}, 'dist_axoness_averaging': 10000}}
    config = type('Cfg', (), {'__getitem__': lambda self, k: cfg[k], 'use_new_subfold': True, 'syntype_available': True})()
    ssh = {'np': np, '__package__': 'refpkg.reps', '__name__': 'refpkg.reps.super_segmentation_helper',
           'global_params': types.SimpleNamespace(config=config), 'log_reps': types.SimpleNamespace(debug=lambda *a: None),
           'generate_rendering_locs': lambda verts, ds: verts[:0], 'render_sso_coords': lambda sso, locs, **kw: sso._rendered,
           'load_so_attr_bulk': lambda sos, keys, **kw: {k: {so.id: so.attrs[k] for so in sos} for k in keys}}
    exec('from typing import *', ssh)
    for name in ('sso_views_to_modelinput', 'syn_sign_ratio_celltype', 'celltype_of_sso_nocache'):
        lift_function(f'{REF}/reps/super_segmentation_helper.py', name, ssh)
    net = {'torch': torch, 'nn': nn, 'Conv3DLayer': Conv3DLayer}
    lift_class(f'{REF}/cnn/cnn_celltype_cmn_j0251.py', 'StackedConv2ScalarWithLatentAdd', net)
    return pred, ssh, net['StackedConv2ScalarWithLatentAdd']


class Cell:
    """The stand-in of a SuperSegmentationObject: what the lifted functions touch."""
    view_caching = True
    sv_ids = [1]

    def __init__(self, views, syn, certainty_estimate):
        self._rendered, self._ce = views, certainty_estimate
        self.mesh = [np.zeros(0, np.uint32), np.zeros(3, np.float32), np.zeros(0, np.float32)]
        self.attr_dict, self.view_dict, self.saved = {}, {}, None
        sign, area, axs = syn
        self.syn_ssv = [types.SimpleNamespace(id=10 + i, attrs={'syn_sign': sign[i], 'mesh_area': area[i], 'rep_coord': [i, 0, 0]})
                        for i in range(len(sign))]
        self._axs = axs

    def load_attr_dict(self):
        pass

    def load_views(self, view_key=None):
        return self.view_dict[view_key]

    def lookup_in_attribute_dict(self, key):
        return None

    def attr_for_coords(self, coords, attr_keys):
        return [np.array([self._axs[int(c[0])] for c in coords])]

    def certainty_celltype(self, pred_key):      # reps/super_segmentation_object.py:3193-3220 without the cache
        return self._ce(self.attr_dict[pred_key + '_probas'], is_logit=True)

    def save_attributes(self, keys, values):
        self.saved = dict(zip(keys, values))


def main():
    torch.manual_seed(0)
    pred_ns, ssh, Net = namespaces()
    spec = CELLTYPE_CMN(7, 2)
    arrs = R.make_weights(spec, WEIGHT_SEED, 20, 128, 256)
    net = Net(in_channels=4, n_classes=7, n_scalar=2).eval()
    params = list(net.parameters())
    assert [tuple(p.shape) for p in params] == [tuple(s) for s in spec.param_shapes().values()]      # registration order = the spec's
    with torch.no_grad():
        for p, a in zip(params, arrs):
            p.copy_(torch.from_numpy(a))
    feats = {}
    net.seq.register_forward_hook(lambda m, i, o: feats.__setitem__('f', o.detach().numpy().copy()))

    class Model:      # InferenceModel.predict_proba without tiling: float32 tensors through the module
        def predict_proba(self, inp, bs=40):
            with torch.no_grad():
                return net(torch.from_numpy(np.ascontiguousarray(inp[0])).float(), torch.from_numpy(np.asarray(inp[1])).float()).numpy()

    out = {'weights_crc': crc(*arrs), 'names': np.array([c[0] for c in CELLS])}
    for name, n_loc, vpl, n_syn in CELLS:
        views, syn = cell_inputs(name, n_loc, vpl, n_syn)
        cell = Cell(views, syn, pred_ns['certainty_estimate'])
        before = views.copy()
        ssh['celltype_of_sso_nocache'](cell, Model(), ws=(256, 128), nb_views=vpl, comp_window=8000., nb_views_model=20)
        inp = ssh['sso_views_to_modelinput'](types.SimpleNamespace(sv_ids=[1], load_views=lambda view_key=None: before.copy()), 20)
        # the sample table: which plane of the unshuffled views every slot holds (planes are told apart by an index image)
        ids = np.arange(n_loc * vpl, dtype=np.uint8).reshape(n_loc, 1, vpl, 1, 1) * np.ones((1, 4, 1, 128, 256), np.uint8)
        table = ssh['sso_views_to_modelinput'](types.SimpleNamespace(sv_ids=[1], load_views=lambda view_key=None: ids.copy()), 20)[:, 0, :, 0, 0]
        ratios = [ssh['syn_sign_ratio_celltype'](cell, comp_types=[1, ]), ssh['syn_sign_ratio_celltype'](cell, comp_types=[0, ]),
                  ssh['syn_sign_ratio_celltype'](cell, weighted=False, comp_types=[1, ]), ssh['syn_sign_ratio_celltype'](cell, comp_types=[0, 2])]
        logits = Model().predict_proba((pred_ns['naive_view_normalization_new'](inp), np.array([ratios[:2]] * len(inp))))
        out.update({f'{name}_crc': crc(before, *syn), f'{name}_table': table.astype(np.int32), f'{name}_feat': feats['f'].astype(np.float32),
                    f'{name}_logits': logits, f'{name}_pred': np.int64(cell.attr_dict['celltype_cnn_e3']),
                    f'{name}_probas': cell.attr_dict['celltype_cnn_e3_probas'], f'{name}_cert': np.float64(cell.attr_dict['celltype_cnn_e3_certainty']),
                    f'{name}_ratios': np.array(ratios, np.float64)})
        assert cell.saved is not None and logits.shape == (len(table), 7)
        print(name, 'samples', len(table), 'pred', out[f'{name}_pred'], 'cert', out[f'{name}_cert'], 'ratios', ratios)
    # the vote block alone, on logits where adding logit 6 onto logit 1 changes an argmax
    vote = lift_vote_block(f'{REF}/reps/super_segmentation_helper.py')
    res = np.array([[0.1, 1.0, 0.0, 1.2, 0.0, 0.0, 0.9], [0.0, 2.0, 0.0, 0.0, 0.0, 0.0, -1.5], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 3.0],
                    [0.3, -0.2, 0.0, 2.5, 0.1, 0.0, 0.1]], np.float32)
    p1, r1 = vote(res.copy(), True, 7)
    p0, r0 = vote(res.copy(), False, 7)
    assert not np.array_equal(np.argmax(r1, 1), np.argmax(r0, 1))
    out.update(vote_in=res, vote_merged=r1, vote_pred_merged=np.int64(p1), vote_pred_plain=np.int64(p0),
               vote_cert=np.float64(pred_ns['certainty_estimate'](r1, is_logit=True)))
    path = os.path.join(HERE, 'g29_celltype.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
