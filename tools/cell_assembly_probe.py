"""Stage times of the cell assembly (csrc/sd_cell_assembly.hip) on ONE synthetic input: `--cells` cells (default 2000), each a random
tree of `--svs` supervoxels (default 100) with one box per supervoxel, `--organelles` organelles (default 20000) that each overlap 1 .. 6
supervoxels of one or two cells, and one synapse per 4 supervoxels between random cells.

    python tools/cell_assembly_probe.py [--out profiles/cell_assembly_probe.json]

Reports, as the minimum of three runs after one warm-up, from HIP events and without uploads: sd_svgraph_components, sd_cell_props,
sd_cell_mapping and sd_cell_synapses; the wall time of the host layer (``svgraph_components``, ``cell_properties``,
``apply_mapping_decisions``, ``map_synssv_objects``) with its uploads and copies; and, when
networkx can be imported, the reference's form in the same process on the same input: ``nx.connected_components`` with the loop of
``create_ccsize_dict`` and the node filter, and one ``Counter`` sum per cell with the decisions, with a check that cells and accepted
lists agree.  Both times are written side by side; no pass / fail rides on them."""
import argparse
import json
import os
import sys
import time
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE, MIN_CC, THRESHOLDS = (10., 10., 20.), 5000., (0.5, 1., 100.)
U = np.uint64


def make_input(n_cells, n_sv, n_org, seed=0):
    rng = np.random.default_rng(seed)
    n = n_cells * n_sv
    ids = np.arange(1, n + 1, dtype=U)
    k = np.arange(n) % n_sv
    parent = (np.arange(n) - k) + (rng.random(n) * np.maximum(k, 1)).astype(np.int64)           # a random earlier node of the same cell
    edges = np.stack([ids[parent[k > 0]], ids[k > 0]], 1)
    edges = edges[rng.permutation(len(edges))]
    lo = rng.integers(0, 4000, (n, 3))
    boxes = np.stack([lo, lo + rng.integers(1, 80, (n, 3))], 1)
    cell = rng.integers(0, n_cells, n_org)
    n_rec = rng.integers(1, 7, n_org)
    sub = np.repeat(np.arange(1, n_org + 1, dtype=U), n_rec)
    other = rng.random(len(sub)) < 0.2                                                           # a fifth of the overlaps lie in another cell
    rcell = np.where(other, rng.integers(0, n_cells, len(sub)), np.repeat(cell, n_rec))
    pair = np.unique(np.stack([sub, ids[rcell * n_sv + rng.integers(0, n_sv, len(sub))]], 1), axis=0)
    counts = rng.integers(20, 400, len(pair))
    org_sizes = np.bincount(pair[:, 0].astype(np.int64), weights=counts, minlength=n_org + 1)[1:].astype(np.int64) + rng.integers(0, 40, n_org)
    n_syn = n // 4
    partners = ids[rng.integers(0, n_cells, (n_syn, 2)) * n_sv]                                   # cell ids = their first supervoxel
    return dict(ids=ids, sizes=rng.integers(1, 10 ** 6, n), rep=lo, box_begin=np.arange(n + 1), boxes=boxes, edges=edges, sub=pair[:, 0], sv=pair[:, 1],
                counts=counts, org_ids=np.arange(1, n_org + 1, dtype=U), org_sizes=np.maximum(org_sizes, 1), partners=partners,
                prob=rng.random(n_syn).astype(np.float32), syn_ids=np.arange(n_syn, dtype=U) + U(1))


def reference_form(d):
    """networkx components + the loop of create_ccsize_dict + the filter; a Counter per cell + the decisions.  -> times, cells, accepted"""
    import networkx as nx
    t0 = time.perf_counter()
    G = nx.Graph()
    G.add_edges_from(d['edges'].tolist())
    for ix in np.setdiff1d(d['ids'], np.array(list(G.nodes()), U)).tolist():
        G.add_edge(ix, ix)
    bbs = dict(zip(d['ids'].tolist(), d['boxes'] * np.array(SCALE)))
    size = {}
    for cc in nx.connected_components(G):
        curr = np.concatenate([bbs[n] for n in cc if n in bbs])
        s = np.linalg.norm(np.max(curr, axis=0) - np.min(curr, axis=0), ord=2)
        for n in cc:
            size[n] = s
    for ix in list(G.nodes()):
        if size[ix] <= MIN_CC:
            G.remove_node(ix)
    cells = {min(cc): sorted(cc) for cc in nx.connected_components(G)}
    t1 = time.perf_counter()
    size_dc = dict(zip(d['org_ids'].tolist(), d['org_sizes'].tolist()))
    md = {}
    for sub, sv, cnt in zip(d['sub'].tolist(), d['sv'].tolist(), d['counts'].tolist()):
        md.setdefault(sv, {})[sub] = cnt / size_dc[sub]
    accepted = {}
    for c in sorted(cells):
        m = Counter()
        for sv in cells[c]:
            m += Counter(md.get(sv, {}))
        r = np.array(list(m.values()))
        mask = r > THRESHOLDS[0]
        accepted[c] = sorted(k for k, ok in zip(m.keys(), mask) if ok and size_dc[k] > THRESHOLDS[2])
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, cells, accepted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=2000)
    ap.add_argument('--svs', type=int, default=100)
    ap.add_argument('--organelles', type=int, default=20000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cell_assembly_probe.json'))
    args = ap.parse_args()
    import ctypes as C
    import torch
    from syconn_amd import _lib as L
    from syconn_amd.proc import graphs, ssd_proc
    from syconn_amd.proc.graphs import SvTable
    from syconn_amd.proc.sd_proc import MapTable, PropTable
    from syconn_amd.proc.ssd_proc import CellLists, map_synssv_objects
    dev, lib = torch.device('cuda', 0), L.load()
    L.check(lib.sd_init(0), 'sd_init')
    d = make_input(args.cells, args.svs, args.organelles)
    props = PropTable(d['ids'], d['sizes'], d['rep'], d['boxes'], d['box_begin'])
    tab = SvTable(props, dev)
    n_e, n_rec, n_org, n_syn = len(d['edges']), len(d['sub']), len(d['org_ids']), len(d['syn_ids'])
    m = tab.n + 2 * n_e
    res = dict(cells=args.cells, supervoxels=tab.n, edges=n_e, records=n_rec, organelles=n_org, synapses=n_syn, device=torch.cuda.get_device_name(0))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == U else np.ascontiguousarray(a)).to(dev)
    i64 = lambda k: torch.empty(max(k, 1), dtype=torch.int64, device=dev)
    e_d, sub_d, sv_d, cnt_d, oid_d, osz_d, par_d, sid_d = (up(d[k]) for k in ('edges', 'sub', 'sv', 'counts', 'org_ids', 'org_sizes', 'partners', 'syn_ids'))
    keep_d = up((d['prob'] > 0.5).astype(np.uint8))
    node_ids, node_comp, ssv_ids, sv_begin, sv_ids, edges_out = i64(m), i64(m), i64(m), i64(m + 1), i64(m), i64(2 * n_e)
    node_size = torch.empty(m, dtype=torch.float64, device=dev)
    cell_size, cell_box, cell_rep = i64(m), torch.empty((m, 6), dtype=torch.int32, device=dev), torch.empty((m, 3), dtype=torch.int32, device=dev)
    cell_begin, pair_org, acc_begin, acc_org, syn_begin, syn_out = i64(m + 1), i64(n_rec), i64(m + 1), i64(n_rec), i64(m + 1), i64(2 * n_syn)
    ratio, accepted = torch.empty(n_rec, dtype=torch.float64, device=dev), torch.empty(n_rec, dtype=torch.uint8, device=dev)
    org_n, org_first = (torch.empty(n_org, dtype=torch.int32, device=dev) for _ in range(2))
    counts_d = torch.zeros(8, dtype=torch.int64, device=dev)
    tmp = torch.empty(max(lib.sd_svgraph_components_temp_bytes(tab.n, n_e), lib.sd_cell_mapping_temp_bytes(n_rec, m), lib.sd_cell_synapses_temp_bytes(n_syn)),
                      dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sc = (C.c_double * 3)(*SCALE)
    shape = {}                                                       # cells and supervoxels the first stage kept: the later stages run on them

    def components():
        rc = lib.sd_svgraph_components(e_d.data_ptr(), n_e, tab.ids.data_ptr(), tab.sizes.data_ptr(), tab.box_begin.data_ptr(), tab.boxes.data_ptr(), tab.n,
                                       tab.n_boxes, sc, MIN_CC, 1, node_ids.data_ptr(), node_comp.data_ptr(), node_size.data_ptr(), ssv_ids.data_ptr(),
                                       sv_begin.data_ptr(), sv_ids.data_ptr(), edges_out.data_ptr(), counts_d.data_ptr(), tmp.data_ptr(), tmp.numel(), stream)
        c = counts_d.cpu().numpy()
        shape.update(n_cells=int(c[1]), n_sv=int(c[2]))
        return rc
    calls = dict(
        components_ms=components,
        props_ms=lambda: lib.sd_cell_props(sv_begin.data_ptr(), sv_ids.data_ptr(), shape['n_cells'], shape['n_sv'], tab.ids.data_ptr(), tab.sizes.data_ptr(),
                                           tab.rep.data_ptr(), tab.box_begin.data_ptr(), tab.boxes.data_ptr(), tab.n, tab.n_boxes, cell_size.data_ptr(),
                                           cell_box.data_ptr(), cell_rep.data_ptr(), counts_d.data_ptr(), stream),
        mapping_ms=lambda: lib.sd_cell_mapping(sub_d.data_ptr(), sv_d.data_ptr(), cnt_d.data_ptr(), n_rec, oid_d.data_ptr(), osz_d.data_ptr(), n_org,
                                               sv_begin.data_ptr(), sv_ids.data_ptr(), shape['n_cells'], shape['n_sv'], *THRESHOLDS, cell_begin.data_ptr(),
                                               pair_org.data_ptr(), ratio.data_ptr(), accepted.data_ptr(), acc_begin.data_ptr(), acc_org.data_ptr(),
                                               org_n.data_ptr(), org_first.data_ptr(), counts_d.data_ptr(), tmp.data_ptr(), tmp.numel(), stream),
        synapses_ms=lambda: lib.sd_cell_synapses(par_d.data_ptr(), keep_d.data_ptr(), sid_d.data_ptr(), n_syn, ssv_ids.data_ptr(), shape['n_cells'],
                                                 syn_begin.data_ptr(), syn_out.data_ptr(), counts_d.data_ptr(), tmp.data_ptr(), tmp.numel(), stream))
    cfg = {'cell_objects': {'lower_mapping_ratios': {'mi': THRESHOLDS[0]}, 'upper_mapping_ratios': {'mi': THRESHOLDS[1]}, 'sizethresholds': {'mi': THRESHOLDS[2]}}}
    runs = []
    for _ in range(4):                                              # the first run warms up (allocator, code objects)
        r = {}
        for name, call in calls.items():
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            rc = call()                                             # components_ms includes the read of its counts (one small copy)
            e[1].record()
            torch.cuda.synchronize(dev)
            assert rc == 0, lib.sd_last_error()
            r[name] = e[0].elapsed_time(e[1])
        t0 = time.perf_counter()
        comps = graphs.svgraph_components(d['edges'], props, SCALE, MIN_CC, True, dev)
        cells = CellLists(comps.ssv_ids, comps.sv_begin, comps.sv_ids)
        ssd_proc.cell_properties(cells, props, device=dev)
        mapping = ssd_proc.apply_mapping_decisions(cells, {'mi': MapTable(d['sub'], d['sv'], d['counts'])}, {'mi': PropTable(d['org_ids'], d['org_sizes'], None, None, None)},
                                                   config=cfg, device=dev)['mi']
        map_synssv_objects(cells, d['partners'], d['prob'], d['syn_ids'], 0.5, dev)
        r['host_layer_wall_ms'] = (time.perf_counter() - t0) * 1e3
        runs.append(r)
    res['runs'] = runs[1:]
    res['min_ms'] = {k: round(min(r[k] for r in runs[1:]), 3) for k in runs[0]}
    res.update(kept_cells=len(cells), kept_supervoxels=len(cells.sv_ids), pairs=len(mapping.ids), accepted=len(mapping.acc_ids))
    try:
        graph_ms, map_ms, ref_cells, ref_acc = reference_form(d)
        same_cells = sorted(ref_cells) == cells.ssv_ids.tolist() and all(ref_cells[c] == v.tolist() for c, v in cells.mapping_dict().items())
        by_cell = mapping.as_dicts()
        res.update(networkx_graph_ms=round(graph_ms, 1), counter_mapping_ms=round(map_ms, 1), cells_equal=bool(same_cells),
                   accepted_equal=bool(all(ref_acc[c] == by_cell[c][2] for c in ref_acc)))
    except ImportError:
        res['networkx_graph_ms'] = None
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(res) + '\n')
    print(json.dumps({k: v for k, v in res.items() if k != 'runs'}))


if __name__ == '__main__':
    main()
