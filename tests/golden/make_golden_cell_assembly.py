"""Golden vectors for the cell assembly (supervoxel graph -> cells, cell properties, organelle -> cell mapping, cell -> synapses),
produced by the REFERENCE'S OWN code: ``create_ccsize_dict`` (/root/reference/syconn/proc/graphs.py:220-249),
``_aggregate_segmentation_object_mappings_thread``, ``_apply_mapping_decisions_thread`` and ``map_synssv_objects_thread`` (proc/
ssd_proc.py:55-91, :126-279, :315-346) and the ``SuperSegmentationObject`` members ``calculate_size``, ``calculate_bounding_box`` and
``rep_coord`` (reps/super_segmentation_object.py:1148-1168, :713-727) are lifted by AST at generation time and run unchanged over
networkx and in-memory stand-ins for the dataset classes, ``prepare_so_attr_cache`` and ``get_segmentation_object(id).size``.  Nothing
compiled and no reference text is stored: inputs and outputs only, as flat arrays.

    python tests/golden/make_golden_cell_assembly.py      ->  tests/golden/g24_cell_assembly.npz

What cannot be lifted is done here over networkx with the reference's own calls (``G.remove_node(0)``, ``G.add_edge(ix, ix)``, the
filter loop, ``nx.connected_components``, ``cc_dict[np.min(cc)]``) and, for the per-supervoxel ratios of proc/sd_proc.py:1063-1084, by
tests/_cell_assembly_ref.py.  The reference's components are handed on with supervoxels ascending; its per-cell mapping lists are
sorted by organelle id with the ratios carried along.  ``_apply_mapping_decisions_thread`` is called with ONE object type at a time
(with several it uses the first type's thresholds for all).

``g_`` the graph: ``g_edges`` (e, 2) uint64, the table ``g_ids`` / ``g_sizes`` / ``g_rep`` / ``g_box_begin`` / ``g_boxes`` (m, 2, 3); three runs
r = ``a`` (scaling (10, 10, 20), min 5000, ``<=`` dropped), ``b`` (the same, ``<`` dropped), ``c`` (scaling (9.5, 9.5, 20.25), ``<=``):
``g_{r}_node_ids`` / ``_node_size`` (the lifted create_ccsize_dict) / ``_node_comp`` / ``_ssv_ids`` / ``_sv_begin`` / ``_sv_ids`` / ``_edges`` /
``_total_size``.  ``g_nobox_edges``: with it appended create_ccsize_dict raises ValueError.  The cases are asserted in ``graph_set``.
``p_`` cell properties of the cells ``p_sv_begin`` / ``p_sv_ids`` (explicit lists, the caller's order) over the ``g_`` table.
``m_`` the mapping: cells ``m_sv_begin`` / ``m_sv_ids`` (explicit lists); per kind k in (mi, sj) records ``m_{k}_sub`` / ``_sv`` / ``_count``,
table ``m_{k}_org_ids`` / ``_org_sizes``, ``m_{k}_thresholds`` (lower, upper, size) and the outputs ``_cell_begin`` / ``_ids`` / ``_ratios`` /
``_acc_begin`` / ``_acc_ids`` over the cells ascending by id.  The cases are asserted in ``mapping_set``.
``y_`` synapses: ``y_partners``, ``y_prob`` (float32), ``y_ids``, ``y_thresh``, ``y_ssv_ids`` -> ``y_begin`` / ``y_out``."""
import os
import sys
import types
from collections import Counter

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _cell_assembly_ref as R  # noqa: E402
from make_golden_cs import lift_function  # noqa: E402
from make_golden_syn_props import lift_method  # noqa: E402

REF = '/root/reference/syconn'
U = np.uint64
LOG = types.SimpleNamespace(debug=lambda *a: None, info=lambda *a: None, error=lambda *a: None, warning=lambda *a: None, critical=lambda *a: None)


# ---- the graph -------------------------------------------------------------------------------------------------------------------
def graph_set(rng):
    edges, table = [], {}                                                          # table: id -> (size, rep, [boxes])

    def sv(i, boxes, size=None):
        boxes = np.asarray(boxes, np.int64).reshape(-1, 2, 3)
        table[int(i)] = (int(rng.integers(1, 10 ** 6)) if size is None else size, boxes[0, 0] + 1, boxes)

    def small(i):                                                                  # a box of under 60 voxels per axis: never above 5000 nm alone
        lo = rng.integers(0, 2000, 3)
        sv(i, [[lo, lo + rng.integers(1, 60, 3)]])
    # 1: a path 100 .. 139 with the edges in descending order: sequential larger-under-smaller linking makes one chain 139 -> 138 -> ..
    for k in range(139, 100, -1):
        edges.append((k, k - 1))
    for k in range(100, 140):
        lo = np.array([50 * (k - 100), 0, 0])
        sv(k, [[lo, lo + 40]])
    # 2: a star of 1000 leaves
    for k in range(5001, 6001):
        edges.append((k, 5000) if k % 2 else (5000, k))
    for k in range(5000, 6001):
        small(k)
    # 3: duplicates and a self loop
    edges += [(6100, 6101), (6101, 6100), (6100, 6101), (6101, 6101), (6101, 6102)]
    for k in (6100, 6101, 6102):
        small(k)
    sv(6102, [[(0, 0, 0), (900, 20, 20)]])                                         # makes the component large
    # 4: edges to node 0; 7001 and 7002 stay apart
    edges += [(0, 7001), (7002, 0), (0, 0)]
    small(7001)
    sv(7002, [[(0, 0, 0), (10, 700, 10)]])
    # 5: ids at 2^63 and 2^64 - 1
    edges.append((2 ** 63, 2 ** 64 - 1))
    sv(2 ** 63, [[(0, 0, 0), (30, 30, 30)]])
    sv(2 ** 64 - 1, [[(1000, 1000, 1000), (1030, 1030, 1030)]])
    # 6: 8002 is an endpoint the table does not know, inside the component of 8001 and 8003
    edges += [(8001, 8002), (8002, 8003)]
    sv(8001, [[(0, 0, 0), (20, 20, 20)]])
    sv(8003, [[(600, 0, 0), (620, 20, 20)]])
    # 7: table ids without an edge
    small(8100)
    sv(8101, [[(0, 0, 0), (800, 10, 10)]])
    # 8: boxes from three chunks
    sv(8200, [[(100, 100, 100), (128, 128, 128)], [(128, 100, 100), (256, 128, 128)], [(256, 100, 110), (300, 120, 128)]])
    edges.append((8200, 8201))
    small(8201)
    # 9: extent (300, 400, 0) voxels: with scaling (10, 10, 20) exactly 5000.0 nm
    sv(9001, [[(100, 100, 5), (400, 500, 5)]])
    # a small component with edges: they leave the pruned graph
    edges += [(9100, 9101), (9101, 9102)]
    for k in (9100, 9101, 9102):
        sv(k, [[(10, 10, 10), (20 + k - 9100, 20, 20)]])
    perm = np.concatenate([np.arange(39), 39 + rng.permutation(len(edges) - 39)])          # the path first, in its order
    edges = np.array(edges, dtype=object)[perm]
    edges = np.array([[int(a), int(b)] for a, b in edges], U)
    ids = np.array(sorted(table), U)
    g = dict(g_edges=edges, g_ids=ids, g_sizes=np.array([table[int(i)][0] for i in ids], np.int64), g_rep=np.array([table[int(i)][1] for i in ids], np.int64),
             g_box_begin=np.concatenate(([0], np.cumsum([len(table[int(i)][2]) for i in ids]))).astype(np.int64),
             g_boxes=np.concatenate([table[int(i)][2] for i in ids]).astype(np.int64), g_nobox_edges=np.array([[9900, 9901]], U))
    # the cases
    assert (edges[:39, 0] == np.arange(139, 100, -1)).all() and (edges[:39, 1] == edges[:39, 0] - 1).all()
    assert (edges == 0).any() and (edges == U(2 ** 63)).any() and (edges == U(2 ** 64 - 1)).any() and (edges[:, 0] == edges[:, 1]).any()
    assert len(np.unique(np.sort(edges, 1), axis=0)) < len(edges)
    assert 8002 not in table and 8100 not in edges and np.diff(g['g_box_begin'])[list(ids).index(8200)] == 3
    return g


def run_graph(create_ccsize_dict, g, scaling, min_cc_size, strict, extra_edges=None):
    """run_create_rag :318-350 (strict) / run_create_neuron_ssd :70-80 over networkx, create_ccsize_dict lifted."""
    edges = g['g_edges'] if extra_edges is None else np.concatenate([g['g_edges'], extra_edges])
    ids = g['g_ids']
    G = nx.Graph()
    G.add_edges_from((U(a), U(b)) for a, b in edges)
    if 0 in G.nodes():
        G.remove_node(0)
    all_sv_ids_in_rag = np.array(list(G.nodes()), dtype=np.uint64)
    for ix in np.setdiff1d(ids, all_sv_ids_in_rag):
        G.add_edge(ix, ix)
    bbs = np.array(R.merged_boxes(g['g_box_begin'], g['g_boxes'])) * scaling
    sv_size_dict = {}
    for ii in range(len(ids)):
        sv_size_dict[ids[ii]] = bbs[ii]
    ccsize_dict = create_ccsize_dict(G, sv_size_dict)
    nodes = np.array(sorted(int(n) for n in G.nodes()), U)
    node_size = np.array([ccsize_dict[n] for n in nodes], np.float64)
    for ix in list(G.nodes()):
        if (ccsize_dict[ix] <= min_cc_size) if strict else (ccsize_dict[ix] < min_cc_size):
            G.remove_node(ix)
    size_of = dict(zip(ids.tolist(), g['g_sizes'].tolist()))
    total_size = 0
    for n in G.nodes():
        total_size += size_of.get(int(n), 0)
    cc_dict = {}
    for cc in nx.connected_components(G):
        cc_arr = np.array(list(cc), dtype=np.uint64)
        cc_dict[np.min(cc_arr)] = np.sort(cc_arr)
    ssv_ids = np.array(sorted(int(k) for k in cc_dict), U)
    inv = {int(s): int(k) for k, cc in cc_dict.items() for s in cc}
    kept_edges = np.array([bool(a in G and b in G) for a, b in edges], bool)
    return dict(node_ids=nodes, node_size=node_size, node_comp=np.array([inv.get(int(n), 0) for n in nodes], U), ssv_ids=ssv_ids,
                sv_begin=np.concatenate(([0], np.cumsum([len(cc_dict[k]) for k in ssv_ids]))).astype(np.int64),
                sv_ids=np.concatenate([cc_dict[k] for k in ssv_ids]), edges=edges[kept_edges].reshape(-1, 2), total_size=np.int64(total_size))


# ---- cell properties ---------------------------------------------------------------------------------------------------------------
def run_props(g, sv_begin, sv_ids):
    path = f'{REF}/reps/super_segmentation_object.py'
    ns = {'np': np}
    exec('from typing import *', ns)
    row = {int(i): k for k, i in enumerate(g['g_ids'])}
    mb = R.merged_boxes(g['g_box_begin'], g['g_boxes'])

    class SSO:
        calculate_size = lift_method(path, 'SuperSegmentationObject', 'calculate_size', ns)
        calculate_bounding_box = lift_method(path, 'SuperSegmentationObject', 'calculate_bounding_box', ns)
        rep_coord = property(lift_method(path, 'SuperSegmentationObject', 'rep_coord', ns))

        def __init__(self, svs):
            self.sv_ids, self._rep_coord, self._size, self._bounding_box = svs, None, None, None
            self.svs = [types.SimpleNamespace(rep_coord=g['g_rep'][row[int(s)]]) for s in svs]

        def lookup_in_attribute_dict(self, key):
            return None

        def load_so_attributes(self, obj_type, attr_keys):
            assert obj_type == 'sv'
            cols = dict(size=[g['g_sizes'][row[int(s)]] for s in self.sv_ids], bounding_box=[mb[row[int(s)]] for s in self.sv_ids])
            return [cols[k] for k in attr_keys]
    size, box, rep = [], [], []
    for a, b in zip(sv_begin[:-1], sv_begin[1:]):
        sso = SSO(sv_ids[a:b])
        sso.calculate_size()
        s0 = sso._size
        sso.calculate_bounding_box()
        assert s0 == sso._size and sso._bounding_box.dtype == np.int32
        size.append(s0)
        box.append(sso._bounding_box)
        rep.append(sso.rep_coord)
    return np.array(size, np.int64), np.array(box, np.int32), np.array(rep, np.int32)


# ---- mapping -----------------------------------------------------------------------------------------------------------------------
class FakeSSD:
    """In-memory SuperSegmentationDataset / SuperSegmentationObject storage: attr_dicts kept per cell."""
    store = None

    def __init__(self, *a, **kw):
        s = FakeSSD.store
        self.config, self.version_dict, self.mapping_dict, self._mapping_dict = s['config'], s['version_dict'], s['mapping_dict'], None
        self.version, self.working_dir, self.type = '0', '', 'ssv'

    def get_super_segmentation_object(self, ssv_id, caching=False):
        s = FakeSSD.store
        return types.SimpleNamespace(id=ssv_id, sv_ids=s['mapping_dict'].get(ssv_id), attr_dict=s['attr'][ssv_id], load_attr_dict=lambda: None,
                                     save_attr_dict=lambda: None, load_mesh=lambda k: None, typedsyns2mesh=lambda: None)


def lifted_ssd_proc(sizes_of, numpy_data=None):
    class SD:
        def __init__(self, obj_type, **kw):
            self.obj_type = obj_type

        def get_segmentation_object(self, i):
            return types.SimpleNamespace(size=sizes_of[self.obj_type][int(i)])

        def load_numpy_data(self, name):
            return numpy_data[name]

    def prepare_so_attr_cache(sd, svids, attrs):
        return FakeSSD.store['attr_cache']
    ns = {'np': np, 'Counter': Counter, 'tqdm': types.SimpleNamespace(tqdm=lambda it, **kw: it), 'log_proc': LOG,
          'super_segmentation': types.SimpleNamespace(SuperSegmentationDataset=FakeSSD), 'segmentation': types.SimpleNamespace(SegmentationDataset=SD),
          'prepare_so_attr_cache': prepare_so_attr_cache,
          'global_params': types.SimpleNamespace(config=types.SimpleNamespace(syntype_available=False))}
    p = f'{REF}/proc/ssd_proc.py'
    return (lift_function(p, '_aggregate_segmentation_object_mappings_thread', ns), lift_function(p, '_apply_mapping_decisions_thread', ns),
            lift_function(p, 'map_synssv_objects_thread', ns))


def mapping_set(rng):
    """-> cells (explicit lists), {kind: records, table, thresholds}."""
    lists, nxt = [], [10]

    def cell(n, shuffle=True):
        ids = np.arange(nxt[0], nxt[0] + n, dtype=U)
        nxt[0] += n + 5
        lists.append(rng.permutation(ids) if shuffle else ids)
        return lists[-1]
    mi_rec, mi_tab, sj_rec, sj_tab = [], {}, [], {}
    c_up = cell(3, False)                                                          # (1, 2, 3) / 12 in list order ...
    c_down = cell(3, False)[::-1].copy()                                           # ... and a list given the other way round: 3, 2, 1
    lists[-1] = c_down
    mi_tab[101], mi_tab[102] = 12, 12
    mi_rec += [(101, s, k) for s, k in zip(c_up, (1, 2, 3))] + [(102, s, k) for s, k in zip(c_down, (3, 2, 1))]
    c3 = cell(3, False)
    mi_tab[103] = 56
    mi_rec += [(103, s, k) for s, k in zip(c3, (9, 18, 1))]                        # 0.5000000000000001: mapped
    mi_tab[104] = 4
    mi_rec += [(104, c3[0], 1), (104, c3[1], 1)]                                   # exactly 0.5: not mapped
    mi_tab[105] = 10
    mi_rec += [(105, c3[0], 6), (105, c3[2], 6)]                                   # 1.2 with upper 1.: mapped
    mi_tab[106], mi_tab[107] = 3, 4                                                # the size threshold is 3: 106 stays out, 107 is mapped
    mi_rec += [(106, c3[1], 3), (107, c3[1], 4)]
    mi_rec += [(199, c3[0], 5)]                                                    # 199 is not in the size table
    mi_rec += [(103, 5, 7), (103, 0, 7)]                                           # supervoxel 5 is in no cell, 0 is background
    cell(4)                                                                        # a cell without mappings
    for j, n in enumerate((1, 63, 64, 65, 5000)):                                  # one (cell, organelle) run of n records
        c = cell(n)
        cnt = rng.integers(1, 10, n)
        mi_tab[200 + j] = int(cnt.sum()) + 3 if j % 2 else int(cnt.sum()) * 2 - 1
        mi_rec += [(200 + j, s, int(k)) for s, k in zip(c, cnt)]
        mi_rec += [(300 + j, s, 2) for s in c[::7]]                                # and a second organelle over every 7th supervoxel
        mi_tab[300 + j] = 2 * len(c[::7]) + 1
    # sj: 0.1 / 0.9
    ca, cb = lists[0], lists[1]
    sj_tab[401], sj_tab[402], sj_tab[403] = 10, 10, 10
    sj_rec += [(401, ca[0], 4), (401, cb[0], 5)]                                   # accepted by two cells
    sj_rec += [(402, ca[1], 10)]                                                   # 1.0 > 0.9: rejected by the upper ratio
    sj_rec += [(403, ca[2], 1)]                                                    # 0.1 is not above the lower ratio
    sj_rec += [(403, cb[2], 9)]                                                    # 0.9 <= 0.9: accepted
    out = {}
    for kind, rec, tab, thr in (('mi', mi_rec, mi_tab, (0.5, 1., 3)), ('sj', sj_rec, sj_tab, (0.1, 0.9, 3))):
        rec = np.array(rec, dtype=object)[rng.permutation(len(rec))]
        order = np.lexsort((rec[:, 1].astype(U), rec[:, 0].astype(U)))             # a MapTable: by organelle, then supervoxel
        rec = rec[order]
        oid = np.array(sorted(tab), U)
        out[kind] = dict(sub=rec[:, 0].astype(U), sv=rec[:, 1].astype(U), count=rec[:, 2].astype(np.int64), org_ids=oid,
                         org_sizes=np.array([tab[int(i)] for i in oid], np.int64), thresholds=np.array(thr, np.float64))
    sv_begin = np.concatenate(([0], np.cumsum([len(c) for c in lists]))).astype(np.int64)
    return sv_begin, np.concatenate(lists).astype(U), out


def run_mapping(sv_begin, sv_ids, kinds):
    ssv_ids, cb, cs = R.explicit_cells(sv_begin, sv_ids)
    mapping_dict = {int(c): cs[a:b] for c, a, b in zip(ssv_ids, cb[:-1], cb[1:])}
    sizes_of = {k: dict(zip(v['org_ids'].tolist(), v['org_sizes'].tolist())) for k, v in kinds.items()}
    aggregate, apply, _ = lifted_ssd_proc(sizes_of)
    out = {}
    for kind, v in kinds.items():
        md = R.sv_mapping_dicts(v['sub'], v['sv'], v['count'], v['org_ids'], v['org_sizes'])
        attr_cache = {f'mapping_{kind}_ids': {int(s): list(md.get(int(s), {}).keys()) for s in cs},
                      f'mapping_{kind}_ratios': {int(s): list(md.get(int(s), {}).values()) for s in cs}}
        lo, up, st = v['thresholds']
        cfg = {'cell_objects': {'lower_mapping_ratios': {kind: lo}, 'upper_mapping_ratios': {kind: up}, 'sizethresholds': {kind: st}}}
        FakeSSD.store = dict(config=cfg, version_dict={kind: 0}, mapping_dict=mapping_dict, attr_cache=attr_cache,
                             attr={c: dict(sv=1, rep_coord=1, bounding_box=1, size=1) for c in mapping_dict})
        args = (list(mapping_dict), '0', {kind: 0}, '', [kind], 'ssv')
        aggregate(args)
        apply(args)
        begin, ids, ratios, abegin, aids = [0], [], [], [0], []
        for c in mapping_dict:
            a = FakeSSD.store['attr'][c]
            i, r = np.array(a[f'mapping_{kind}_ids'], U), np.array(a[f'mapping_{kind}_ratios'], np.float64)
            o = np.argsort(i, kind='stable')
            ids.append(i[o]); ratios.append(r[o]); begin.append(begin[-1] + len(i))
            acc = np.sort(np.array(a[kind], U))
            aids.append(acc); abegin.append(abegin[-1] + len(acc))
        out[kind] = dict(cell_begin=np.array(begin, np.int64), ids=np.concatenate(ids), ratios=np.concatenate(ratios), acc_begin=np.array(abegin, np.int64),
                         acc_ids=np.concatenate(aids))
    return ssv_ids, out


def main():
    rng = np.random.default_rng(2401)
    g = graph_set(rng)
    ccsize = lift_function(f'{REF}/proc/graphs.py', 'create_ccsize_dict', {'np': np, 'nx': nx})
    runs = dict(a=(np.array([10., 10., 20.]), 5000, True), b=(np.array([10., 10., 20.]), 5000, False), c=(np.array([9.5, 9.5, 20.25]), 5000, True))
    res = {r: run_graph(ccsize, g, *v) for r, v in runs.items()}
    out = dict(g)
    for r, d in res.items():
        out[f'g_{r}_scaling'], out[f'g_{r}_min_cc_size'], out[f'g_{r}_strict'] = runs[r][0], np.float64(runs[r][1]), np.bool_(runs[r][2])
        out.update({f'g_{r}_{k}': v for k, v in d.items()})
    a, b, c = res['a'], res['b'], res['c']
    at = lambda d, n: d['node_size'][list(d['node_ids']).index(n)]
    assert at(a, 9001) == 5000.0 and 9001 not in a['ssv_ids'] and 9001 in b['ssv_ids']
    assert 100 in a['ssv_ids'] and 5000 in a['ssv_ids'] and 6100 in a['ssv_ids'] and 7002 in a['ssv_ids'] and 7001 not in a['ssv_ids']
    assert 2 ** 63 in a['ssv_ids'] and 8001 in a['ssv_ids'] and 8002 in a['sv_ids'] and 8101 in a['ssv_ids'] and 8100 not in a['ssv_ids']
    assert 0 not in a['node_ids'] and 9100 not in a['sv_ids'] and len(a['edges']) < len(g['g_edges']) - 3
    assert not np.array_equal(a['node_size'], c['node_size']) and (c['node_size'] != np.round(c['node_size'])).any()
    try:
        run_graph(ccsize, g, runs['a'][0], 5000, True, g['g_nobox_edges'])
        raise AssertionError('a component without a box must raise')
    except ValueError as e:
        assert 'Could not find a single bounding box' in str(e)
    # cell properties: the kept cells of run a without the one that holds the unknown supervoxel, each list reversed
    keep = [k for k in range(len(a['ssv_ids'])) if 8002 not in a['sv_ids'][a['sv_begin'][k]:a['sv_begin'][k + 1]]]
    lists = [a['sv_ids'][a['sv_begin'][k]:a['sv_begin'][k + 1]][::-1] for k in keep]
    out['p_sv_begin'] = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int64)
    out['p_sv_ids'] = np.concatenate(lists)
    out['p_size'], out['p_box'], out['p_rep'] = run_props(g, out['p_sv_begin'], out['p_sv_ids'])
    assert any(8200 in x for x in lists) and (out['p_rep'][0] == g['g_rep'][list(g['g_ids']).index(139)]).all()
    # mapping
    sv_begin, sv_ids, kinds = mapping_set(rng)
    ssv_ids, mres = run_mapping(sv_begin, sv_ids, kinds)
    out.update(m_sv_begin=sv_begin, m_sv_ids=sv_ids, m_ssv_ids=ssv_ids)
    for kind in kinds:
        out.update({f'm_{kind}_{k}': v for k, v in kinds[kind].items()})
        out.update({f'm_{kind}_{k}': v for k, v in mres[kind].items()})
    mi, sj = mres['mi'], mres['sj']
    ratio = lambda d, i: d['ratios'][d['ids'] == i]
    assert sorted(np.concatenate([ratio(mi, 101), ratio(mi, 102)]).tolist()) == [0.49999999999999994, 0.5]
    assert ratio(mi, 101)[0].tobytes() != ratio(mi, 102)[0].tobytes()
    assert ratio(mi, 103)[0] == 0.5000000000000001 and 103 in mi['acc_ids'] and ratio(mi, 104)[0] == 0.5 and 104 not in mi['acc_ids']
    assert ratio(mi, 105)[0] > 1 and 105 in mi['acc_ids'] and 106 not in mi['acc_ids'] and 107 in mi['acc_ids'] and 199 not in mi['ids']
    assert (np.diff(mi['cell_begin']) == 0).any() and len(ratio(mi, 103)) == 1
    assert (sj['acc_ids'] == 401).sum() == 2 and 402 not in sj['acc_ids'] and ratio(sj, 402)[0] == 1.0 and (sj['acc_ids'] == 403).sum() == 1
    runs_len = sorted(int((kinds['mi']['sub'] == 200 + j).sum()) for j in range(5))
    assert runs_len == [1, 63, 64, 65, 5000]
    # synapses
    y_ssv = np.array([3, 7, 9, 2 ** 63 + 5], U)
    n = 60
    partners = rng.choice(np.array([3, 7, 2 ** 63 + 5, 11], U), (n, 2))
    partners[4] = (7, 7)                                                           # a synapse of a cell with itself
    prob = rng.choice(np.array([0.2, 0.5, 0.75, 0.9], np.float32), n)
    prob[4] = 0.9
    ids = rng.permutation(np.arange(1000, 1000 + n)).astype(U)
    FakeSSD.store = dict(config=None, version_dict={}, mapping_dict={}, attr={int(c): {} for c in y_ssv})
    _, _, map_syn = lifted_ssd_proc({}, dict(neuron_partners=partners, syn_prob=prob, id=ids))
    map_syn(([int(c) for c in y_ssv], '0', {}, '', 'ssv', None, 0.5))
    lists = [np.asarray(FakeSSD.store['attr'][int(c)]['syn_ssv'], U) for c in y_ssv]
    out.update(y_partners=partners, y_prob=prob, y_ids=ids, y_thresh=np.float64(0.5), y_ssv_ids=y_ssv,
               y_begin=np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int64), y_out=np.concatenate(lists))
    assert (prob == 0.5).any() and not np.isin(ids[prob == 0.5], out['y_out']).any() and (out['y_out'] == ids[4]).sum() == 2 and len(lists[2]) == 0
    path = os.path.join(HERE, 'g24_cell_assembly.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
