"""Stage times of the skeleton votes (csrc/sd_skeleton.hip) on ONE small synthetic input: `--cells` cells (default 20), each a skeleton
of 2000 nodes grown as a tree of long branches (a new node continues the last one with probability 0.97 and otherwise branches off
one of the last 300; steps of 100 nm with a persistent direction, rounded to voxels at scaling (10, 10, 20)), labels 0 .. 2 in runs
of random length, max_dist 10000.

    python tools/skeleton_vote_probe.py [--out profiles/skeleton_vote_probe.json]

Reports, as the minimum of three runs after one warm-up, from HIP events and without uploads: sd_skel_csr, sd_skel_vote and
sd_skel_components over all cells; the wall time of ``skeleton_majority_vote`` and ``skeleton_compartment_majority`` with their host
work (the edge weights) and copies; the device's counters; and, when networkx can be imported, the reference's form in the same
process on the same input: per node one ``nx.single_source_dijkstra_path(g, n, max_dist)`` and one ``np.unique`` over the first
`--ref-cells` cells, with a check that the votes agree.  Both times are written side by side; no pass / fail rides on them."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_NODES, SCALE, MAX_DIST = 2000, (10, 10, 20), 10000


def make_input(n_cells, seed=0):
    rng = np.random.default_rng(seed)
    nodes, edges, labels = [], [], []
    for _ in range(n_cells):
        p = np.zeros((N_NODES, 3))
        p[0] = rng.uniform(2000, 50000, 3)
        parent = np.zeros(N_NODES - 1, np.int64)
        step = rng.normal(0, 1, 3)
        for i in range(1, N_NODES):
            parent[i - 1] = i - 1 if rng.random() < 0.97 else rng.integers(max(0, i - 300), i)
            step = 0.8 * step / np.linalg.norm(step) + rng.normal(0, 0.4, 3)
            p[i] = p[parent[i - 1]] + 100 * step / np.linalg.norm(step)
        nodes.append(np.round(p / np.array(SCALE)).astype(np.int64))
        edges.append(np.stack([parent, np.arange(1, N_NODES)], 1))
        labels.append(np.repeat(rng.integers(0, 3, N_NODES // 20 + 1), rng.integers(5, 60, N_NODES // 20 + 1))[:N_NODES])
    begin = lambda parts: np.concatenate(([0], np.cumsum([len(x) for x in parts]))).astype(np.int64)
    return np.concatenate(nodes), begin(nodes), np.concatenate(edges), begin(edges), np.concatenate(labels).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=20)
    ap.add_argument('--ref-cells', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'skeleton_vote_probe.json'))
    args = ap.parse_args()
    import torch
    from syconn_amd import _lib as L
    from syconn_amd.reps import super_segmentation_helper as H
    dev, lib = torch.device('cuda', 0), L.load()
    nodes, nb, edges, eb, labels = make_input(args.cells)
    n, n_e, n_cells = len(nodes), len(edges), args.cells
    weights = H.skeleton_edge_weights(nodes, nb, edges, eb, np.array(SCALE)).astype(np.float64)
    res = dict(cells=n_cells, nodes=n, edges=n_e, max_dist=MAX_DIST, lds_nodes=L.SD_SKEL_LDS_NODES, device=torch.cuda.get_device_name(0))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nb_d, eb_d, e_d, w_d, cls_d = up(nb), up(eb), up(edges), up(weights), up(labels.astype(np.uint8))
    adj_begin, adj_nbr, adj_w = (torch.empty(k, dtype=t, device=dev) for k, t in ((n + 1, torch.int64), (2 * n_e, torch.int32), (2 * n_e, torch.float64)))
    vote_d, comp_d, reached_d = (torch.empty(n, dtype=t, device=dev) for t in (torch.uint8, torch.uint8, torch.int32))
    counts_d = torch.zeros(8, dtype=torch.int64, device=dev)
    tmp = torch.empty(max(lib.sd_skel_csr_temp_bytes(n_e), lib.sd_skel_vote_temp_bytes(n, N_NODES), lib.sd_skel_components_temp_bytes(n)),
                      dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    calls = dict(
        csr_ms=lambda: lib.sd_skel_csr(e_d.data_ptr(), eb_d.data_ptr(), nb_d.data_ptr(), n_cells, n, n_e, w_d.data_ptr(), adj_begin.data_ptr(),
                                       adj_nbr.data_ptr(), adj_w.data_ptr(), counts_d.data_ptr(), tmp.data_ptr(), tmp.numel(), stream),
        vote_ms=lambda: lib.sd_skel_vote(adj_begin.data_ptr(), adj_nbr.data_ptr(), adj_w.data_ptr(), 2 * n_e, nb_d.data_ptr(), n_cells, n, N_NODES,
                                         cls_d.data_ptr(), 3, float(MAX_DIST), vote_d.data_ptr(), reached_d.data_ptr(), counts_d.data_ptr(),
                                         tmp.data_ptr(), tmp.numel(), stream),
        components_ms=lambda: lib.sd_skel_components(e_d.data_ptr(), eb_d.data_ptr(), nb_d.data_ptr(), n_cells, n, n_e, cls_d.data_ptr(), 2, 1, 0,
                                                     comp_d.data_ptr(), counts_d.data_ptr(), tmp.data_ptr(), tmp.numel(), stream))
    runs = []
    for _ in range(4):                                              # the first run warms up (allocator, code objects)
        r = {}
        for name, call in calls.items():
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            rc = call()
            e[1].record()
            torch.cuda.synchronize(dev)
            assert rc == 0, lib.sd_last_error()
            r[name] = e[0].elapsed_time(e[1])
            if name == 'vote_ms':
                c = counts_d.cpu().numpy()
                counters = dict(sources_redone=int(c[0]), steps_lds=int(c[1]), steps_redo=int(c[2]))
        t0 = time.perf_counter()
        vote = H.skeleton_majority_vote(nodes, nb, edges, eb, labels, np.array(SCALE), MAX_DIST, dev)
        r['majority_vote_wall_ms'] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        H.skeleton_compartment_majority(nb, edges, eb, labels, device=dev)
        r['compartment_wall_ms'] = (time.perf_counter() - t0) * 1e3
        runs.append(r)
    assert np.array_equal(vote, vote_d.cpu().numpy())
    reached = reached_d.cpu().numpy()
    res['runs'] = runs[1:]
    res['min_ms'] = {k: round(min(r[k] for r in runs[1:]), 3) for k in runs[0]}
    res['counters'] = counters
    res['window_nodes'] = dict(min=int(reached.min()), median=float(np.median(reached)), max=int(reached.max()))
    try:
        import networkx as nx
        m = min(args.ref_cells, n_cells)
        t0 = time.perf_counter()
        ref = []
        for c in range(m):
            e = edges[eb[c]:eb[c + 1]]
            g = nx.Graph()
            g.add_nodes_from(range(nb[c + 1] - nb[c]))
            g.add_weighted_edges_from([(int(a), int(b), w) for (a, b), w in zip(e, weights[eb[c]:eb[c + 1]])])
            lab = labels[nb[c]:nb[c + 1]]
            for s in range(g.number_of_nodes()):
                neighs = np.array(list(nx.single_source_dijkstra_path(g, s, MAX_DIST).keys()), dtype=np.int64)
                vals, cnts = np.unique(lab[neighs], return_counts=True)
                ref.append(vals[np.argmax(cnts)])
        res.update(networkx_cells=m, networkx_nodes=int(nb[m]), networkx_per_node_ms=round((time.perf_counter() - t0) * 1e3, 1),
                   networkx_votes_differing=int(np.sum(np.array(ref) != vote[:nb[m]])))
    except ImportError:
        res['networkx_per_node_ms'] = None
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(res) + '\n')
    print(json.dumps({k: v for k, v in res.items() if k != 'runs'}))


if __name__ == '__main__':
    main()
