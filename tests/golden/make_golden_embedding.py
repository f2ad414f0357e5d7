"""Golden vectors for the morphology embedding, produced by the REFERENCE'S OWN code, lifted by AST at generation time and run unchanged on
torch-CPU float32 / numpy / scipy: ``RepresentationNetwork`` and ``TripletNet`` (/root/reference/syconn/cnn/cnn_atn.py:21-55, :90-108; the
module imports elektronn3 at the top and cannot be imported), ``views2tripletinput`` and ``naive_view_normalization_new``
(handler/prediction.py:1189-1194, :1096-1097), ``view_embedding_of_sso_nocache`` (reps/super_segmentation_helper.py:1758-1817) and the
method ``predict_views_embedding`` (reps/super_segmentation_object.py:3032-3079).  Nothing compiled and no reference text is stored:
outputs only, and a CRC of the generated inputs and weights, so that a drift of the generators of tests/_embedding_cases.py shows as
itself.

    python tests/golden/make_golden_embedding.py      ->  tests/golden/g31_embedding.npz

Two geometries: ``lit`` is the module exactly as written, ``Linear(6076, 50)``, on 2 locations of 512 x 512; ``w372`` is the module with
only ``fc[0]`` replaced by the tree's commented ``Linear(372, 50)``, on 6 locations x 2 views of 128 x 256, with a skeleton of 36 nodes
of which five are constructed to be equidistant from two locations (a sixth tie comes from the seeded draws).

Stated stand-ins (not reference code): ``InferenceModel.predict_proba`` = the module in eval mode on the float32 triple, its outputs as
numpy; the cell object (mesh, skeleton, ``view_dict``, ``sample_locations``, ``load_views``, ``save_skeleton``);
``generate_rendering_locs`` and ``render_sso_coords`` (they hand out the generated locations / views); a ``cKDTree`` whose ``query``
maps the removed ``n_jobs`` keyword to ``workers``."""
import ast
import os
import sys
import types

import numpy as np
import scipy.spatial
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _embedding_cases as K  # noqa: E402
import _embedding_ref as E  # noqa: E402
from make_golden_celltype import lift_class  # noqa: E402
from make_golden_cs import lift_function  # noqa: E402

REF = '/root/reference/syconn'


def lift_method(path, cls, name, ns):
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.ClassDef) and node.name == cls:
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and sub.name == name:
                    sub.decorator_list = []
                    exec(compile(ast.Module(body=[sub], type_ignores=[]), path, 'exec'), ns)
                    return ns[name]
    raise KeyError(name)


class Tree(scipy.spatial.cKDTree):      # the shim: scipy dropped `n_jobs` for `workers`
    def query(self, x, n_jobs=1, **kw):
        return super().query(x, workers=n_jobs, **kw)


def namespaces():
    pred = {'np': np}
    for name in ('naive_view_normalization_new', 'views2tripletinput'):
        lift_function(f'{REF}/handler/prediction.py', name, pred)
    for mod in ('refpkg', 'refpkg.reps', 'refpkg.handler'):
        sys.modules[mod] = types.ModuleType(mod)
        sys.modules[mod].__path__ = []
    hp = types.ModuleType('refpkg.handler.prediction')
    hp.naive_view_normalization_new = pred['naive_view_normalization_new']
    sys.modules['refpkg.handler.prediction'] = hp
    spatial = types.SimpleNamespace(cKDTree=Tree)
    log = types.SimpleNamespace(debug=lambda *a: None, warning=lambda *a: None)
    ssh = {'np': np, 'spatial': spatial, '__package__': 'refpkg.reps', '__name__': 'refpkg.reps.super_segmentation_helper', 'log_reps': log,
           'generate_rendering_locs': lambda verts, ds: verts, 'render_sso_coords': lambda sso, locs, **kw: sso._rendered}
    exec('from typing import *', ssh)
    lift_function(f'{REF}/reps/super_segmentation_helper.py', 'view_embedding_of_sso_nocache', ssh)
    sso = {'np': np, 'spatial': spatial, '__package__': 'refpkg.reps', '__name__': 'refpkg.reps.super_segmentation_object', 'log_reps': log}
    lift_method(f'{REF}/reps/super_segmentation_object.py', 'SuperSegmentationObject', 'predict_views_embedding', sso)
    net = {'torch': torch, 'nn': nn, 'F': F}
    lift_class(f'{REF}/cnn/cnn_atn.py', 'RepresentationNetwork', net)
    lift_class(f'{REF}/cnn/cnn_atn.py', 'TripletNet', net)
    return pred, ssh, sso, net


class Cell:
    """The stand-in of a SuperSegmentationObject: what the lifted functions touch.  The mesh vertices ARE the rendering locations (the
    stand-in of generate_rendering_locs returns them)."""
    view_caching = True
    nb_cpus = 1
    version = '0'

    def __init__(self, views, locs, nodes):
        self._rendered, self._locs = views, locs
        self.mesh = [np.zeros(0, np.uint32), locs.reshape(-1).copy(), np.zeros(0, np.float32)]
        self.view_dict, self.skeleton, self.saved = {}, {'nodes': nodes.copy()}, 0
        self.scaling = K.GOLDEN_SCALING.copy()
        self._sample_locations = None

    def sample_locations(self):
        return self._sample_locations if self._sample_locations is not None else [self._locs]

    def load_views(self, view_key=None):
        return self._rendered

    def load_skeleton(self):
        pass

    def save_skeleton(self):
        self.saved += 1


def main():
    torch.manual_seed(0)
    pred_ns, ssh, sso_ns, net_ns = namespaces()
    out = {'names': np.array(list(K.GOLDEN))}
    for name, (geom, n_loc, vpl) in K.GOLDEN.items():
        spec, H, W, _ = K.GEOMS[geom]
        arrs = K.golden_weights(name)
        rep = net_ns['RepresentationNetwork'](n_in_channels=4, n_out_channels=K.Z, dr=0.1, leaky_relu=False)      # cnn_atn.py:113-114
        if spec.fc_in != 6076:
            rep.fc[0] = nn.Linear(spec.fc_in, 50)      # the tree's commented line 44
        tnet = net_ns['TripletNet'](rep).eval()
        sd = E.state_dict_of(spec, arrs, 'rep_net.')
        assert list(sd) == list(tnet.state_dict()) and [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in tnet.state_dict().values()]
        tnet.load_state_dict(sd)
        assert [tuple(s) for s in spec.param_shapes().values()] == [tuple(p.shape) for p in tnet.parameters()]      # registration order
        seen = {}

        class Model:      # InferenceModel.predict_proba: the module in eval mode on the triple
            def predict_proba(self, inp):
                with torch.no_grad():
                    res = tnet(*[torch.from_numpy(np.ascontiguousarray(a)).float() for a in inp])
                seen['latent'] = res[2].numpy().copy()
                return tuple(r.numpy() for r in res)

        views, locs, nodes = K.golden_cell(name)
        cell = Cell(views, locs, nodes)
        ssh['view_embedding_of_sso_nocache'](cell, Model(), ws=(W, H), nb_views=vpl, comp_window=8000.)
        latent = seen['latent']
        assert latent.shape == (n_loc, K.Z) and cell.saved == 1 and np.array_equal(cell._sample_locations[0], locs)
        cached = Cell(views, locs, nodes)
        sso_ns['predict_views_embedding'](cached, Model())
        ixs = np.asarray(cached.skeleton['view_ixs'])
        assert np.array_equal(cached.skeleton['latent_morph'], cell.skeleton['latent_morph']) and np.array_equal(seen['latent'], latent)
        assert np.array_equal(cell.skeleton['latent_morph'], latent[ixs])
        rows, tie = E.nearest_rows(locs, nodes * K.GOLDEN_SCALING)
        print(name, 'latent', latent.shape, 'nodes', len(nodes), 'ties', int(tie.sum()), 'tie rows (reference / lower row)', ixs[tie], rows[tie],
              'all rows equal the lower-row rule:', bool(np.array_equal(rows, ixs)))
        assert name != 'w372' or tie.sum() >= 2
        out.update({f'{name}_crc': K.crc(views, locs, nodes, *arrs), f'{name}_latent': latent.astype(np.float32), f'{name}_view_ixs': ixs.astype(np.int64),
                    f'{name}_node_latent': np.asarray(cell.skeleton['latent_morph'], np.float32), f'{name}_tie': tie})
    small = np.random.default_rng(K.GOLDEN_SEED).integers(0, 256, (3, 4, 2, 5, 7)).astype(np.uint8)
    out.update(triplet_in_crc=K.crc(small), triplet_out=pred_ns['views2tripletinput'](small))
    path = os.path.join(HERE, 'g31_embedding.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
