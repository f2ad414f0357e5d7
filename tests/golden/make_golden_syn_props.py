"""Golden vectors for the synapse properties (``classify_synssv_objects``, ``collect_properties_from_ssv_partners``, ``export_matrix``),
produced by the REFERENCE'S OWN code: ``_collect_properties_from_ssv_partners_thread``, ``_from_cell_to_syn_dict``,
``_classify_synssv_objects_thread`` and ``export_matrix`` (/root/reference/syconn/extraction/cs_processing_steps.py:109-229, :1129-1161,
:1434-1499), the methods ``semseg_for_coords`` and ``attr_for_coords`` (reps/super_segmentation_object.py:2190-2240, :2923-3003) and
``colorcode_vertices`` (reps/rep_helper.py:281-334) are lifted by AST at generation time and run unchanged, scipy's cKDTree and
sklearn's forest included.  The datasets, objects, ``AttributeDict``, ``joblib`` and ``global_params.config`` are in-memory stand-ins.
Nothing compiled and no reference text is stored: inputs and outputs only, as flat arrays.

    python tests/golden/make_golden_syn_props.py      ->  tests/golden/g21_syn_props.npz

Two notes.  The reference passes ``n_jobs=`` to ``cKDTree.query``, which scipy 1.15 no longer accepts: the stand-in tree forwards it
as ``workers``.  For a cell without skeleton nodes ``attr_for_coords`` returns ``-1 * np.ones((n, 2))``, which the caller unpacks into
two names: that only works for a cell with exactly two synapses, and leaves the scalar -1 as the cell's ``latent_morph`` entries.
Such a cell has two synapses here, and when the columns are flattened the scalar -1 becomes ``[inf] * ndim_embedding``, the rule
``attr_for_coords`` itself applies to a missing ``latent_morph`` (:2996-3002).

Two cases, prefixes ``a_`` and ``b_``; k 50, ds_vertices 1, ignore_labels [4, 5], ndim_embedding 4, sym_thresh 0.225.
``a``: scaling (10, 10, 20), every vertex on the 1/8 nm lattice: every squared distance is exact in float64.  Checked in ``main``: no
query has two equal d^2 among its first k + 1 neighbours; a cell with fewer than k vertices left after ``ignore_labels``; cells with
exactly 64 and 65 vertices, with one vertex, without mesh, without skeleton; a skeleton without the axoness key and one without
``latent_morph``; a vote tie decided by the first occurrence; a synapse whose partners give different values;
``syn_type_sym_ratio`` exactly at ``sym_thresh``; a ``spinehead_vol`` entry present and absent.
``b``: scaling (9, 9, 20), random float32 vertices, some negative; no query has two of its first k + 1 d^2 within a relative 1e-6.

Per case, inputs: ``syn_ids`` / ``syn_partners`` (n, 2) / ``syn_rep`` / ``syn_ratio`` / ``mesh_area`` / ``features`` (n, 14), ``scaling``
(float32); the cells: ``cell_ids`` / ``cell_celltypes`` (-1: none), ``cell_verts`` / ``cell_vert_begin`` / ``cell_spiness``, ``cell_nodes`` /
``cell_node_begin`` / ``cell_ax`` / ``cell_latent`` / ``cell_has_ax`` / ``cell_has_latent``, ``cell_sh_begin`` / ``cell_sh_ids`` / ``cell_sh_vol``;
the forest packed (``rf_*``; ``rf_proba`` = ``tree_.value``, which sklearn >= 1.3 stores as class fractions).  Outputs: ``syn_prob`` as
``_classify_synssv_objects_thread`` stored it, ``rf_predict_proba`` = sklearn's own output for all rows at once, the six columns
``_from_cell_to_syn_dict`` wrote, and ``csv`` / ``csv_half`` = the bytes of conn_mat.csv at threshold 0 and 0.5."""
import ast
import datetime
import os
import sys
import tempfile
import time
import types
from collections import Counter, defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_cs import lift_function  # noqa: E402
import _syn_props_ref as R  # noqa: E402

REF = '/root/reference/syconn'
K, DS, IGNORE, EMB, SYM = 50, 1, [4, 5], 4, 0.225
AX_KEY = 'axoness_avg10000'


def lift_method(path, cls, name, ns):
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.ClassDef) and node.name == cls:
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and sub.name == name:
                    sub.decorator_list = []
                    exec(compile(ast.Module(body=[sub], type_ignores=[]), path, 'exec'), ns)
                    return ns[name]
    raise KeyError(name)


class Maker:
    def __init__(self, seed, scale, lattice):
        self.rng, self.scale, self.lattice = np.random.default_rng(seed), np.array(scale, np.float32), lattice
        self.cells, self.syn = [], []

    def cloud(self, centre_nm, spread_nm, n):
        p = np.asarray(centre_nm, np.float64) + self.rng.normal(0, spread_nm, (n, 3))
        return (np.round(p * 8) / 8 if self.lattice else p).astype(np.float32)

    def cell(self, cid, centre_nm, n_vert, n_nodes, labels=None, celltype=None, ax=True, latent=True, spread_nm=600):
        rng = self.rng
        verts = self.cloud(centre_nm, spread_nm, n_vert)
        lab = rng.integers(0, 4, n_vert) if labels is None else np.asarray(labels)
        nodes = np.maximum(np.round((np.asarray(centre_nm) + rng.normal(0, spread_nm, (n_nodes, 3))) / self.scale), 0).astype(np.int64)
        attrs = {}
        if ax and n_nodes:
            attrs[AX_KEY] = rng.integers(0, 5, n_nodes)
        if latent and n_nodes:
            attrs['latent_morph'] = rng.normal(0, 1, (n_nodes, EMB)).astype(np.float32)
        self.cells.append(dict(id=cid, celltype=celltype, vertices=verts, vertex_labels={'spiness': lab.astype(np.int64)}, nodes=nodes,
                               node_attrs=attrs, spinehead_vol={}, centre=np.asarray(centre_nm, np.float64)))

    def synapse(self, a, b, rep=None, ratio=None):
        ca, cb = (next(c for c in self.cells if c['id'] == x) for x in (a, b))
        if rep is None:
            rep = np.maximum(np.round(((ca['centre'] + cb['centre']) / 2 + self.rng.normal(0, 300, 3)) / self.scale), 0)
        ratio = float(np.round(self.rng.random(), 3)) if ratio is None else ratio
        self.syn.append(((max(a, b), min(a, b)), np.asarray(rep, np.int32), ratio))
        return len(self.syn) - 1


def case_a():
    m = Maker(211, (10, 10, 20), True)
    rng = m.rng
    m.cell(1, (3000, 3000, 3000), 300, 40, labels=rng.integers(0, 6, 300), celltype=3)
    m.cell(2, (4500, 3000, 3000), 200, 25, labels=rng.integers(0, 6, 200), ax=False)           # skeleton without the axoness key, no celltype
    m.cell(3, (3000, 4500, 3000), 64, 12, celltype=5, latent=False)                            # exactly 64 vertices, no latent_morph
    m.cell(4, (4500, 4500, 3000), 65, 9, celltype=1)                                           # exactly 65
    m.cell(5, (3800, 3800, 4200), 1, 3, labels=[1], celltype=2)                                # one vertex
    m.cell(6, (3000, 3000, 4500), 0, 10, celltype=4)                                           # no mesh
    m.cell(7, (4500, 3000, 4500), 120, 0, celltype=6)                                          # no skeleton: exactly two synapses below
    lab8 = np.concatenate([rng.integers(4, 6, 50), rng.integers(0, 4, 30)])
    m.cell(8, (3000, 4500, 4500), 80, 15, labels=lab8[rng.permutation(80)], celltype=0)        # 30 < k vertices left
    # cell 9: four vertices at 100, 200, 300, 400 nm from the synapse below, labels 2, 1, 1, 2: two against two, 2 occurs first
    m.cell(9, (6000, 6000, 6000), 0, 6, celltype=7)
    m.cells[-1]['vertices'] = np.array([(6000, 6000, 6100), (6000, 6200, 6000), (6300, 6000, 6000), (6000, 6000, 5600)], np.float32)
    m.cells[-1]['vertex_labels'] = {'spiness': np.array([2, 1, 1, 2])}
    m.tie = m.synapse(9, 1, rep=(600, 600, 300), ratio=SYM)                                    # exactly at sym_thresh: sign 1
    pairs = [(1, 2), (1, 3), (2, 4), (3, 4), (5, 1), (5, 2), (6, 1), (6, 3), (7, 1), (7, 4), (8, 2), (8, 3), (8, 1), (4, 1), (2, 3), (9, 5),
             (1, 2), (3, 8), (5, 6), (4, 8)]
    for a, b in pairs:
        m.synapse(a, b)
    m.syn[3] = (m.syn[3][0], m.syn[3][1], 0.226)
    m.syn[4] = (m.syn[4][0], m.syn[4][1], 0.0)
    return m


def case_b():
    m = Maker(212, (9, 9, 20), False)
    rng = m.rng
    for cid in range(1, 7):
        centre = rng.uniform(-500, 3000, 3)
        m.cell(cid, centre, int(rng.integers(150, 400)), int(rng.integers(5, 40)), labels=rng.integers(0, 6, 400)[:0], celltype=int(rng.integers(0, 9)))
        c = m.cells[-1]
        c['vertex_labels'] = {'spiness': rng.integers(0, 6, len(c['vertices']))}
    ids = [c['id'] for c in m.cells]
    for _ in range(18):
        a, b = rng.choice(ids, 2, replace=False)
        m.synapse(int(a), int(b))
    return m


class Store(dict):
    def push(self):
        pass


def pack_forest(rfc):
    feature, threshold, left, right, proba, begin = [], [], [], [], [], [0]
    for est in rfc.estimators_:
        t, off = est.tree_, begin[-1]
        leaf = t.children_left < 0
        feature.append(np.where(leaf, 0, t.feature))
        threshold.append(np.where(leaf, 0.0, t.threshold))
        left.append(np.where(leaf, -1, t.children_left + off))
        right.append(np.where(leaf, -1, t.children_right + off))
        proba.append(t.value[:, 0, :])
        begin.append(off + t.node_count)
    return dict(feature=np.concatenate(feature).astype(np.int32), threshold=np.concatenate(threshold).astype(np.float64),
                left=np.concatenate(left).astype(np.int32), right=np.concatenate(right).astype(np.int32),
                proba=np.concatenate(proba).astype(np.float64), tree_begin=np.array(begin, np.int32), n_features=rfc.n_features_in_)


def run_case(m, seed):
    import scipy.spatial
    from sklearn.ensemble import RandomForestClassifier
    rng = m.rng
    scaling = m.scale
    n = len(m.syn)
    syn_ids = (2000 + rng.permutation(n)).astype(np.uint64)
    partners = np.array([s[0] for s in m.syn], np.uint64)
    syn_rep = np.array([s[1] for s in m.syn], np.int32)
    ratio = np.array([s[2] for s in m.syn], np.float64)
    mesh_area = np.round(rng.random(n) * 4, 3)
    # spine-head volumes: for about half of the (cell, synapse) sides
    for i in range(n):
        for cid in partners[i].tolist():
            if rng.random() < 0.5:
                next(c for c in m.cells if c['id'] == cid)['spinehead_vol'][int(syn_ids[i])] = float(np.float32(rng.random()))
    # the classifier: 14 feature columns shaped like synssv_o_features' (counts, sizes, distances up to 1e12)
    def feats(k):
        f = np.concatenate([rng.integers(100, 5000, (k, 1)), np.round(rng.random((k, 1)) * 4, 3)] +
                           [np.stack([rng.integers(0, 4, k), rng.integers(0, 3000, k), np.where(rng.random(k) < 0.3, 1e12, rng.random(k) * 1000)], 1)
                            for _ in range(4)], 1)
        return f.astype(np.float64)
    train = feats(300)
    y = ((train[:, 0] > 2000) ^ (train[:, 4] < 400) ^ (rng.random(300) < 0.2)).astype(np.int32)
    rfc = RandomForestClassifier(n_estimators=7, random_state=seed, n_jobs=1).fit(train, y)
    features = feats(n)
    by_id = {c['id']: c for c in m.cells}
    stores = {'/so/attr_dict.pkl': Store({i: dict(neuron_partners=partners[k], syn_type_sym_ratio=ratio[k]) for k, i in enumerate(syn_ids)})}

    class Tree:
        def __init__(self, data):
            self.t = scipy.spatial.cKDTree(data)

        def query(self, x, k=1, n_jobs=1, **kw):
            return self.t.query(x, k=k, workers=n_jobs, **kw)
    log = types.SimpleNamespace(debug=lambda *a: None, info=lambda *a: None, error=lambda *a: None, warning=lambda *a: None, warn=lambda *a: None)

    class Config(dict):
        working_dir, mpath_syn_rfc = '/nowhere', '/nowhere/rfc'
    cfg = Config(spines={'semseg2coords_spines': dict(k=K, ds_vertices=DS, ignore_labels=list(IGNORE))}, tcmn={'ndim_embedding': EMB},
                 compartments={'view_properties_semsegax': {'semseg_key': 'axoness'}, 'dist_axoness_averaging': 10000},
                 cell_objects={'sym_thresh': SYM, 'thresh_synssv_proba': 0.5})
    sso_ns = {'np': np, 'scipy': types.SimpleNamespace(spatial=types.SimpleNamespace(cKDTree=Tree)), 'defaultdict': defaultdict, 'log_reps': log}
    exec('from typing import *', sso_ns)
    helper_ns = {'np': np, 'spatial': types.SimpleNamespace(cKDTree=Tree), 'Counter': Counter, 'log_reps': log}
    sso_ns['colorcode_vertices'] = lift_function(f'{REF}/reps/rep_helper.py', 'colorcode_vertices', helper_ns)
    sso_path = f'{REF}/reps/super_segmentation_object.py'

    class SSO:
        semseg_for_coords = lift_method(sso_path, 'SuperSegmentationObject', 'semseg_for_coords', sso_ns)
        attr_for_coords = lift_method(sso_path, 'SuperSegmentationObject', 'attr_for_coords', sso_ns)

        def __init__(self, cid):
            c = by_id[int(cid)]
            self.id, self.size, self.rep_coord, self.scaling, self.nb_cpus, self.config = int(cid), 0, (0, 0, 0), scaling, 1, cfg
            self.ssv_dir = f'/nowhere/ssv/{int(cid)}'
            self.mesh = (np.zeros(0, np.uint32), c['vertices'].reshape(-1).copy(), np.zeros(0, np.float32))
            self.attr_dict = {'spinehead_vol': c['spinehead_vol']}
            if c['celltype'] is not None:
                self.attr_dict['celltype_cnn_e3'] = c['celltype']
            self.skeleton = dict(nodes=c['nodes'], **c['node_attrs'])
            self._labels = c['vertex_labels']

        def load_attr_dict(self):
            pass

        def load_skeleton(self):
            pass

        def label_dict(self, what):
            assert what == 'vertex'
            return self._labels

    class SSD:
        def __init__(self, working_dir=None, version=None, **kw):
            self.ssv_ids, self.config = np.array(sorted(by_id)), cfg

        def get_super_segmentation_object(self, ssv_id):
            return SSO(ssv_id)

    class Obj:
        def __init__(self, ix):
            self.id, self.attr_dict = ix, stores['/so/attr_dict.pkl'][ix]

        def load_attr_dict(self):
            pass

    class SD:
        def __init__(self, obj_type, working_dir=None, version=None, **kw):
            assert obj_type == 'syn_ssv'
            self.ids, self.rep_coords, self.so_dir_paths, self.scaling = syn_ids, syn_rep, ['/so'], scaling

        def load_numpy_data(self, name):
            if name == 'neuron_partners':
                return partners
            if name == 'mesh_area':
                return mesh_area
            return np.array([stores['/so/attr_dict.pkl'][i][name] for i in syn_ids])

        def get_segmentation_object(self, ix):
            return Obj(ix)

    def attribute_dict(path, **kw):
        return stores.setdefault(path, Store())
    ns = {'np': np, 'os': os, 'datetime': datetime, 'time': time, 'Logger': object}
    exec('from typing import *', ns)
    ns.update(segmentation=types.SimpleNamespace(SegmentationDataset=SD, SegmentationObject=object),
              super_segmentation=types.SimpleNamespace(SuperSegmentationDataset=SSD), global_params=types.SimpleNamespace(config=cfg),
              AttributeDict=attribute_dict, log_extraction=log, joblib=types.SimpleNamespace(load=lambda path: rfc),
              synssv_o_features=lambda o: features[int(np.flatnonzero(syn_ids == o.id)[0])].tolist())
    path = f'{REF}/extraction/cs_processing_steps.py'
    for name in ('_collect_properties_from_ssv_partners_thread', '_from_cell_to_syn_dict', '_classify_synssv_objects_thread', 'export_matrix'):
        lift_function(path, name, ns)
    ns['_classify_synssv_objects_thread']((['/so'], '/nowhere', 0))
    ns['_collect_properties_from_ssv_partners_thread'](('/nowhere', 0, 0, np.array(sorted(by_id))))
    ns['_from_cell_to_syn_dict']((['/so'], '/nowhere', 0, 0))
    attr = stores['/so/attr_dict.pkl']
    # the scalar -1 a cell without skeleton leaves as its latent_morph entry -> [inf] * ndim_embedding (see the module docstring)
    for i in syn_ids:
        attr[i]['latent_morph'] = [np.full(EMB, np.inf, np.float32) if np.ndim(v) == 0 and v == -1 else np.asarray(v, np.float32)
                                   for v in attr[i]['latent_morph']]
    csv = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, thr in (('csv', 0), ('csv_half', 0.5)):
            os.makedirs(f'{tmp}/{name}')
            ns['export_matrix'](dest_folder=f'{tmp}/{name}', threshold_syn=thr)
            csv[name] = np.frombuffer(open(f'{tmp}/{name}/conn_mat.csv', 'rb').read(), np.uint8)
    col = lambda key, dt: np.array([attr[i][key] for i in syn_ids], dt)
    forest = pack_forest(rfc)
    out = dict(syn_ids=syn_ids, syn_partners=partners, syn_rep=syn_rep, syn_ratio=ratio, mesh_area=mesh_area, features=features, scaling=scaling,
               syn_prob=col('syn_prob', np.float64), rf_predict_proba=rfc.predict_proba(features),
               partner_axoness=col('partner_axoness', np.int32), partner_spiness=col('partner_spiness', np.int32),
               partner_celltypes=col('partner_celltypes', np.int32), partner_spineheadvol=col('partner_spineheadvol', np.float32),
               latent_morph=col('latent_morph', np.float32), syn_sign=col('syn_sign', np.int64), **csv)
    for key in ('partner_axoness', 'partner_spiness', 'partner_celltypes', 'partner_spineheadvol'):
        assert np.array_equal(out[key], np.array([attr[i][key] for i in syn_ids], np.float64)), key      # the cast lost nothing
    out.update({f'rf_{k}': np.asarray(v) for k, v in forest.items()})
    assert np.array_equal(R.forest_proba(forest, features), out['rf_predict_proba']) and np.array_equal(out['syn_prob'], out['rf_predict_proba'][:, 1])
    cells = m.cells
    offs = lambda parts: np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.int64)
    sh = [sorted(c['spinehead_vol'].items()) for c in cells]
    out.update(cell_ids=np.array([c['id'] for c in cells], np.uint64), cell_celltypes=np.array([-1 if c['celltype'] is None else c['celltype'] for c in cells], np.int32),
               cell_verts=np.concatenate([c['vertices'] for c in cells]), cell_vert_begin=offs([c['vertices'] for c in cells]),
               cell_spiness=np.concatenate([c['vertex_labels']['spiness'] for c in cells]).astype(np.int32),
               cell_nodes=np.concatenate([c['nodes'] for c in cells]).astype(np.int32), cell_node_begin=offs([c['nodes'] for c in cells]),
               cell_ax=np.concatenate([c['node_attrs'].get(AX_KEY, np.zeros(len(c['nodes']), np.int64)) for c in cells]).astype(np.int32),
               cell_latent=np.concatenate([c['node_attrs'].get('latent_morph', np.zeros((len(c['nodes']), EMB), np.float32)) for c in cells]),
               cell_has_ax=np.array([AX_KEY in c['node_attrs'] for c in cells]), cell_has_latent=np.array(['latent_morph' in c['node_attrs'] for c in cells]),
               cell_sh_begin=offs(sh), cell_sh_ids=np.array([k for s in sh for k, _ in s], np.uint64), cell_sh_vol=np.array([v for s in sh for _, v in s], np.float32))
    assert out['latent_morph'].shape == (n, 2, EMB) and out['partner_axoness'].shape == (n, 2)
    return out


def check_case(c, exact):
    """No decision of the case hangs on rounding or on a tie between two d^2."""
    s = c['scaling'].astype(np.float64)
    cells = R.cells_from_case(c)
    if exact:
        v8 = c['cell_verts'].astype(np.float64) * 8
        assert np.array_equal(v8, np.round(v8)) and np.abs(v8).max() < 2 ** 24 and np.array_equal(s, np.round(s))
    by_id = {cell['id']: cell for cell in cells}
    for i in range(len(c['syn_ids'])):
        q = (c['syn_rep'][i].astype(np.float64) * s)[None]
        for cid in c['syn_partners'][i].tolist():
            cell = by_id[cid]
            if len(cell['vertices']):
                v, _ = R.spine_points(cell, DS, IGNORE)
                for pts, k in ((v, K), (cell['nodes'].astype(np.float64) * s, 1)):
                    if len(pts):
                        d2 = R.knn(pts, [0, len(pts)], None, [0], q, min(k, len(pts)), extra=1)[2]
                        assert not R.ambiguous(d2, 0.0 if exact else 1e-6).any(), (i, cid, k)


def main():
    out = {}
    for prefix, make, seed in (('a', case_a, 0), ('b', case_b, 1)):
        m = make()
        res = run_case(m, seed)
        check_case(res, exact=prefix == 'a')
        want = R.collect_properties(res['syn_partners'], res['syn_rep'], res['syn_ratio'], res['syn_ids'], R.cells_from_case(res), res['scaling'], K, DS,
                                    IGNORE, AX_KEY, EMB, SYM)
        for key, v in want.items():
            assert np.array_equal(v, res[key]), key
        out.update({f'{prefix}_{k}': v for k, v in res.items()})
        print(prefix, len(res['syn_ids']), 'synapses,', len(res['cell_ids']), 'cells,', len(res['cell_verts']), 'vertices,', len(res['cell_nodes']), 'nodes,',
              len(res['rf_feature']), 'forest nodes; spiness', res['partner_spiness'].reshape(-1).tolist())
        if prefix == 'a':
            a, part = res, res['syn_partners']
            left = {cell['id']: len(R.spine_points(cell, DS, IGNORE)[0]) for cell in R.cells_from_case(a)}
            assert left[8] == 30 and left[3] == 64 and left[4] == 65 and left[5] == 1 and left[6] == 0 and left[1] > K
            side = lambda cid: np.argwhere(part == cid)
            assert all((a['partner_spiness'][i, p], a['partner_celltypes'][i, p], a['partner_axoness'][i, p], a['partner_spineheadvol'][i, p]) == (0, 0, 0, 0)
                       and not a['latent_morph'][i, p].any() for i, p in side(6)) and len(side(6)) >= 2          # no mesh: zeros, celltype too
            assert len(side(7)) == 2 and all(a['partner_axoness'][i, p] == -1 and np.isinf(a['latent_morph'][i, p]).all() for i, p in side(7))
            assert all(a['partner_axoness'][i, p] == -1 and np.isfinite(a['latent_morph'][i, p]).all() for i, p in side(2))     # no axoness key
            assert all(a['partner_axoness'][i, p] >= 0 and np.isinf(a['latent_morph'][i, p]).all() for i, p in side(3))       # no latent_morph
            assert all(a['partner_celltypes'][i, p] == -1 for i, p in side(2))
            t = m.tie
            p9 = int(np.flatnonzero(part[t] == 9)[0])
            assert a['partner_spiness'][t, p9] == 2 and a['syn_ratio'][t] == SYM and a['syn_sign'][t] == 1          # two against two; at the threshold
            assert a['syn_sign'][3] == -1 and a['syn_sign'][4] == 1 and (a['syn_sign'] == -1).sum() > 3
            assert np.any(a['partner_spiness'][:, 0] != a['partner_spiness'][:, 1]) and np.any(a['partner_axoness'][:, 0] != a['partner_axoness'][:, 1])
            assert (a['partner_spineheadvol'] == -1).any() and (a['partner_spineheadvol'] > 0).any()
            assert len(np.unique(a['partner_spiness'])) >= 3
        else:
            assert res['cell_verts'].min() < 0
        assert 0 < (res['syn_prob'] > 0.5).sum() < len(res['syn_prob']) and len(res['csv_half']) < len(res['csv'])
    path = os.path.join(HERE, 'g21_syn_props.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
