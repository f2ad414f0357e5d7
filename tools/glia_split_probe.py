"""Times of the astrocyte splitting (csrc/sd_glia.hip) on ONE synthetic input: `--cells` cells (default 20000), each a random tree of
`--svs` supervoxels (default 50) with a few extra edges, boxes on a 100 nm lattice, 0 to 100 % glia supervoxels in runs along the tree, eight
views per supervoxel.

    python tools/glia_split_probe.py [--out profiles/glia_split_probe.json]

Reports, as the minimum of three runs after one warm-up, from HIP events and without uploads: sd_glia_pred and sd_glia_split (all four
passes, both component tables and both split graphs are one call); the wall time of the host layer (``glia_pred`` +
``split_glia_table``) with its uploads and copies; and, when networkx can be imported, the wall time of the rule of
``remove_glia_nodes`` stated over networkx (sub-graph copies, ``connected_components``, one box reduction per component) on the first
`--nx-cells` cells (default 500) of the same input, with a check that the neuron sets agree.  The times are written side by side; no
pass / fail rides on them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, THRESH = 2600.0, 0.25
U = np.uint64


def make_input(n_cells, n_sv, seed=0):
    rng = np.random.default_rng(seed)
    n = n_cells * n_sv
    ids = np.arange(1, n + 1, dtype=U)
    k = np.arange(n) % n_sv
    parent = (np.arange(n) - k) + np.maximum(k - 1 - (rng.random(n) * np.minimum(k, 3)).astype(np.int64), 0)      # one of the three nodes before it
    tree = np.stack([ids[parent[k > 0]], ids[k > 0]], 1)
    more = rng.integers(0, n, n // 5)
    extra = np.stack([ids[more], ids[more - more % n_sv + rng.integers(0, n_sv, len(more))]], 1)
    edges = np.concatenate([tree, extra])
    edges = edges[rng.permutation(len(edges))]
    lo = np.stack([k * 300 + rng.integers(0, 3, n) * 100, rng.integers(0, 10, n) * 100, rng.integers(0, 10, n) * 100], 1).astype(np.float64)
    boxes = np.stack([lo, lo + rng.integers(1, 8, (n, 3)) * 100], 1)
    share = rng.choice([0, 1, 3, 3, 3, 3, 5, 8, 10], n_cells).repeat(n_sv)                                         # tenths of a cell that are glia
    glia = (((k + rng.integers(0, n_sv, n_cells).repeat(n_sv)) // 5) % 10 < share).astype(np.uint8)              # runs of five along the tree
    p = np.where(glia[:, None] != 0, 0.75, 0.0625) + rng.integers(-128, 128, (n, 8)) / 4096.
    return dict(ids=ids, edges=edges, boxes=boxes, glia=glia, probas=p.astype(np.float32).reshape(-1), view_begin=np.arange(n + 1) * 8,
                sizes=rng.integers(1, 10 ** 6, n))


def networkx_form(d, n_cells, n_sv):
    """The rule of remove_glia_nodes over networkx, cell by cell.  -> ms, the neuron supervoxels of the cells"""
    import networkx as nx
    first = d['ids'][:n_cells * n_sv]
    e = d['edges'][(d['edges'][:, 0] <= first[-1]) & (d['edges'][:, 1] <= first[-1])]
    box, glia = dict(zip(first.tolist(), d['boxes'])), dict(zip(first.tolist(), d['glia'].tolist()))

    def sizes(g):
        out = {}
        for cc in nx.connected_components(g):
            cur = np.concatenate([box[n] for n in cc])
            s = np.linalg.norm(np.max(cur, axis=0) - np.min(cur, axis=0), ord=2)
            out.update({n: s for n in cc})
        return out
    t0 = time.perf_counter()
    G = nx.Graph()
    G.add_edges_from(e.tolist())
    neuron = []
    for cc in nx.connected_components(G):
        g = G.subgraph(cc)
        g_n = g.copy()
        g_n.remove_nodes_from([n for n in cc if glia[n]])
        if not any(v > T for v in sizes(g_n).values()):
            continue
        g_g = g.copy()
        g_g.remove_nodes_from([n for n in cc if not glia[n]])
        s_g = sizes(g_g)
        if not any(v > T for v in s_g.values()):
            neuron += list(cc)
            continue
        g_n = g.copy()
        g_n.remove_nodes_from([n for n in cc if glia[n] and not s_g[n] < T])
        neuron += [n for n, v in sizes(g_n).items() if not v < T]
    return (time.perf_counter() - t0) * 1e3, np.array(sorted(neuron), U)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=20000)
    ap.add_argument('--svs', type=int, default=50)
    ap.add_argument('--nx-cells', type=int, default=500)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'glia_split_probe.json'))
    args = ap.parse_args()
    import torch
    from syconn_amd import _dev as D
    from syconn_amd.proc import graphs
    dev = D.device('cuda:0')
    d = make_input(args.cells, args.svs)
    n, n_e = len(d['ids']), len(d['edges'])
    m = 2 * n_e
    res = dict(cells=args.cells, supervoxels=n, edges=n_e, views=len(d['probas']), min_size=T, device=torch.cuda.get_device_name(0))
    e_d, ids_d, box_d, p_d, vb_d, sz_d = (D.up(d[k], dev) for k in ('edges', 'ids', 'boxes', 'probas', 'view_begin', 'sizes'))
    u64s = lambda k: D.empty(k, D.i64, dev)
    outs = [u64s(m), u64s(m), D.empty(m, D.u8, dev), u64s(m), D.empty(m, D.f64, dev), D.empty(m, D.f64, dev), u64s(m), D.empty(m, D.u8, dev)]
    outs += [u64s(m), u64s(m), u64s(m + 1), u64s(m), u64s(m), u64s(m), u64s(m + 1), u64s(m), u64s(2 * n_e), u64s(2 * n_e)]
    cls_d, mean_d, counts_d, counts8 = D.empty(n, D.u8, dev), D.empty(n, D.f64, dev), D.counters(dev, 16), D.counters(dev)
    tmp = D.scratch('sd_glia_split_temp_bytes', dev, n, n_e, 0)
    calls = dict(
        glia_pred_ms=lambda: D.call('sd_glia_pred', dev, p_d, 0, vb_d, n, len(d['probas']), THRESH, 0, cls_d, mean_d, counts8),
        glia_split_ms=lambda: D.call('sd_glia_split', dev, e_d, n_e, None, 0, ids_d, box_d, cls_d, n, T, None, 0.0, sz_d, m, n_e, *outs, counts_d, tmp, tmp.numel()))
    runs = []
    for _ in range(4):                                              # the first run warms up (allocator, code objects)
        r = {}
        for name, call in calls.items():
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            call()
            e[1].record()
            torch.cuda.synchronize(dev)
            r[name] = e[0].elapsed_time(e[1])
        t0 = time.perf_counter()
        cls, _ = graphs.glia_pred(d['probas'], d['view_begin'], THRESH, False, dev)
        split = graphs.split_glia_table(d['edges'], d['ids'], d['boxes'], cls, T, sv_sizes=d['sizes'], device=dev)
        r['host_layer_wall_ms'] = (time.perf_counter() - t0) * 1e3
        runs.append(r)
    c = D.down(counts_d)
    assert not c[7] and not c[10] and not c[12] and np.array_equal(cls, d['glia'])
    res['runs'] = runs[1:]
    res['min_ms'] = {k: round(min(r[k] for r in runs[1:]), 3) for k in runs[0]}
    res.update(cells_by_outcome=list(split.n_cells_by_outcome), neuron_components=len(split.neuron), glia_components=len(split.glia),
               neuron_edges=len(split.neuron_edges), astrocyte_edges=len(split.astrocyte_edges))
    try:
        k = min(args.nx_cells, args.cells)
        ms, neuron = networkx_form(d, k, args.svs)
        mine = split.node_ids[(split.node_class == 0) & (split.node_ids <= d['ids'][k * args.svs - 1])]
        res.update(networkx_cells=k, networkx_wall_ms=round(ms, 1), neuron_sets_equal=bool(np.array_equal(mine, neuron)))
    except ImportError:
        res['networkx_wall_ms'] = None
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(res) + '\n')
    print(json.dumps({k: v for k, v in res.items() if k != 'runs'}))


if __name__ == '__main__':
    main()
