"""Golden vectors for the glia view step, produced by the REFERENCE'S OWN code, lifted by AST at generation time and run on numpy /
scipy: ``predict_views`` and ``multi_probas_saver`` (/root/reference/syconn/proc/sd_proc.py:1386-1432), ``gliapred_sso_nocache``
(reps/super_segmentation_helper.py:1495-1523) and ``single_conn_comp_img`` (proc/image.py:125-144).  Nothing compiled and no reference
text is stored: outputs only, and a CRC of the generated inputs (tests/_glia_views_ref.py), so that a drift of the generators shows as
itself.

    python tests/golden/make_golden_glia_views.py      ->  tests/golden/g32_glia_views.npz

Two changes are made to ``single_conn_comp_img``, both for the numpy of today: ``center = np.array(img.shape) / 2`` becomes ``// 2`` (a
float index, which the numpy of the reference's time truncated and current numpy refuses), and the one-element LIST ``ixs`` it indexes
with becomes a tuple (a list of one mask was read as a tuple then and is read as an array now).  Stated stand-ins (not reference
code): the model (``tests/_glia_views_ref.py: fake_proba``), the supervoxel and cell objects with their storages, ``sm.
start_multiprocess`` (a loop), ``flatten_list``, ``render_sso_coords`` (hands out the generated views)."""
import ast
import os
import sys
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _glia_views_ref as G  # noqa: E402
from make_golden_cs import lift_function  # noqa: E402

REF = '/root/reference/syconn'


def lift_single_conn_comp_img(ns):
    path = f'{REF}/proc/image.py'
    fn = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name == 'single_conn_comp_img'][0]
    done = set()
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign) and ast.unparse(node.targets[0]) == 'center' and isinstance(node.value, ast.BinOp):
            assert isinstance(node.value.op, ast.Div)
            node.value.op = ast.FloorDiv()
            done.add('center')
        if isinstance(node, ast.Assign) and ast.unparse(node.targets[0]) == 'ixs' and isinstance(node.value, ast.List):
            node.value = ast.Tuple(elts=node.value.elts, ctx=ast.Load())
            done.add('ixs')
    assert done == {'center', 'ixs'}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[])), path, 'exec'), ns)
    return ns['single_conn_comp_img']


class So:
    """The stand-in of a SegmentationObject: what the lifted functions touch."""

    def __init__(self, i):
        self.id, self.attr_dict, self.enable_locking = i, {}, False

    def save_attributes(self, keys, values):
        self.attr_dict.update(zip(keys, values))


class Model:
    def __init__(self):
        self.calls = 0

    def predict_proba(self, views, verbose=False):
        self.calls += 1
        return G.fake_proba(views)


def main():
    img_ns = {'np': np, 'ndimage': ndimage}
    scc = lift_single_conn_comp_img(img_ns)
    proc = {'np': np, 'single_conn_comp_img': scc,
            'sm': types.SimpleNamespace(start_multiprocess=lambda f, params, nb_cpus=1: [f(p) for p in params])}
    exec('from typing import *', proc)
    for name in ('multi_probas_saver', 'predict_views'):
        lift_function(f'{REF}/proc/sd_proc.py', name, proc)
    out = {}
    # the dozen planes
    planes = G.golden_planes()
    for k, (p, bg) in enumerate(planes):
        res = scc(p.copy(), background=bg) if bg != 1 else scc(p.copy())      # background 1 is the reference's default
        assert res.shape == p.shape and np.array_equal(res, np.rint(res)) and res.min() >= 0 and res.max() <= 255
        res3 = scc(p.copy()[None], background=bg)                              # any shape that squeezes to 2-D
        assert res3.shape == (1, *p.shape) and np.array_equal(res3[0], res)
        out[f'plane{k}'] = res.astype(np.uint8)
        out[f'plane{k}_crc'] = G.crc(p, np.int64(bg))
    out['n_planes'] = np.int64(len(planes))
    # predict_views: the partition, the filter, the stored key
    for C in (1, 4):
        for cc in (False, True):
            tag = f'pv_c{C}_cc{int(cc)}'
            views = G.golden_views(C)
            out[f'{tag}_crc'] = G.crc(*views)
            m = Model()
            probas = proc['predict_views'](m, [v.copy() for v in views], None, 'glia_probas', single_cc_only=cc, return_proba=True)
            assert m.calls == 1 and [len(p) for p in probas] == list(G.GOLDEN_COUNTS)
            out[f'{tag}_probas'] = np.concatenate(probas)
            out[f'{tag}_part'] = np.cumsum([0] + [len(p) for p in probas]).astype(np.int64)
            mine = [v.copy() for v in views]
            sos = [So(10 + i) for i in range(len(views))]
            assert proc['predict_views'](Model(), mine, sos, 'glia_probas_x', single_cc_only=cc, return_proba=False) is None
            assert all(list(so.attr_dict) == ['glia_probas_x'] for so in sos)
            assert all(np.array_equal(so.attr_dict['glia_probas_x'], p) for so, p in zip(sos, probas))
            out[f'{tag}_views'] = np.concatenate(mine)      # the reference filters the caller's arrays in place
        assert not np.array_equal(out[f'pv_c{C}_cc0_probas'], out[f'pv_c{C}_cc1_probas'])
    out['pv_key'] = np.array('glia_probas_x')
    # gliapred_sso_nocache
    seen = {}

    def render_sso_coords(sso, coords, **kw):
        seen.update(coords=np.array(coords), kw=dict(kw))
        return sso._rendered

    ssh = {'np': np, 'flatten_list': lambda l: [x for sub in l for x in sub], 'render_sso_coords': render_sso_coords,
           'predict_views': proc['predict_views']}
    exec('from typing import *', ssh)
    lift_function(f'{REF}/reps/super_segmentation_helper.py', 'gliapred_sso_nocache', ssh)
    views = G.golden_views(1, seed=77)
    rng = np.random.default_rng(5)
    coords = [rng.uniform(0, 1000, (n, 3)).astype(np.float32) for n in G.GOLDEN_COUNTS]
    svs = [So(20 + i) for i in range(len(views))]
    cell = types.SimpleNamespace(version='tmp', nb_cpus=1, svs=svs, _rendered=np.concatenate(views),
                                 sample_locations=lambda cache=False: [c.copy() for c in coords])
    ssh['gliapred_sso_nocache'](cell, Model(), verbose=False)
    assert seen['kw'] == dict(verbose=False, add_cellobjects=False, return_rot_mat=False) and np.array_equal(seen['coords'], np.concatenate(coords))
    assert all(list(sv.attr_dict) == ['glia_probas'] for sv in svs)
    out['gp_crc'] = G.crc(*views)
    out['gp_probas'] = np.concatenate([sv.attr_dict['glia_probas'] for sv in svs])
    out['gp_counts'] = np.array([len(sv.attr_dict['glia_probas']) for sv in svs], np.int64)
    path = os.path.join(HERE, 'g32_glia_views.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
