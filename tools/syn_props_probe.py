"""Stage times of the synapse properties (csrc/sd_syn_props.hip) on ONE synthetic dataset: 200 cells, each a mesh of 20000 float32
vertices (a random walk of 200 blobs, 100 vertices each, about 150 nm wide) with labels 0 .. 5 and a skeleton of 500 nodes; 20000
synapses between random pairs of cells, each at a vertex of its first partner (40000 sides); k = 50 over the vertices without labels 4
and 5, k = 1 over the nodes; a forest of 100 trees over 14 features (sklearn's, fitted on 2000 random rows, if sklearn can be
imported; else 100 random trees of depth 8) applied to the 20000 feature rows.

    python tools/syn_props_probe.py [--out profiles/syn_props_probe.json]

Reports, as the minimum of three runs after one warm-up, from HIP events: the build stage (cell boxes, keys, sort, tiles) and the
query stage of both kNN calls and the forest kernel, without uploads; the wall time of ``collect_properties_from_ssv_partners`` and
``classify_synssv_objects`` with their host work and copies; the device's tile counters; and, when scipy / sklearn can be imported,
the reference's form in the same process: one ``cKDTree`` per cell (built and queried with k = 50, then the Counter vote per query)
over the first `--ref-cells` cells, and ``predict_proba([row])`` per row over the first `--ref-rows` rows, with a check that both
agree with the device.  No pass / fail rides on the numbers."""
import argparse
import json
import os
import sys
import time
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_CELLS, N_BLOBS, PER_BLOB, N_NODES, N_SYN, K, N_TREES, SCALE = 200, 200, 100, 500, 20000, 50, 100, (10, 10, 20)


def make_input(seed=0):
    rng = np.random.default_rng(seed)
    cells = []
    for cid in range(1, N_CELLS + 1):
        centres = rng.uniform(5000, 60000, 3) + np.cumsum(rng.normal(0, 400, (N_BLOBS, 3)), 0)
        verts = (centres[:, None, :] + rng.normal(0, 75, (N_BLOBS, PER_BLOB, 3))).reshape(-1, 3).astype(np.float32)
        nodes = np.round(centres[rng.integers(0, N_BLOBS, N_NODES)] / np.array(SCALE, np.float64)) + rng.integers(-3, 4, (N_NODES, 3))
        cells.append(dict(id=cid, celltype=int(rng.integers(0, 9)), vertices=verts, vertex_labels={'spiness': rng.integers(0, 6, len(verts))},
                          nodes=np.maximum(nodes, 0), node_attrs={'axoness_avg10000': rng.integers(0, 5, N_NODES),
                                                                  'latent_morph': rng.normal(0, 1, (N_NODES, 10)).astype(np.float32)}))
    a = rng.integers(0, N_CELLS, N_SYN)
    b = (a + rng.integers(1, N_CELLS, N_SYN)) % N_CELLS
    rep = np.stack([np.round(cells[i]['vertices'][rng.integers(0, N_BLOBS * PER_BLOB)] / np.array(SCALE)) for i in a]).astype(np.int32)
    partners = np.stack([np.maximum(a, b) + 1, np.minimum(a, b) + 1], 1).astype(np.uint64)
    feats = np.concatenate([rng.integers(100, 5000, (N_SYN, 1)), rng.random((N_SYN, 1)) * 4, rng.integers(0, 3000, (N_SYN, 12))], 1).astype(np.float64)
    return cells, partners, rep, rng.random(N_SYN), feats


def make_forest(P, rng):
    try:
        from sklearn.ensemble import RandomForestClassifier
    except ImportError:
        depth, n = 8, 2 ** 9 - 1                                  # complete trees in breadth-first order
        i = np.arange(n)
        leaf = i >= 2 ** depth - 1

        def one():
            p = rng.random(n)
            return (np.where(leaf, 0, rng.integers(0, 14, n)), np.where(leaf, 0.0, rng.uniform(0, 3000, n)), np.where(leaf, -1, 2 * i + 1),
                    np.where(leaf, -1, 2 * i + 2), np.stack([p, 1 - p], 1))
        trees = [one() for _ in range(N_TREES)]
        off = n * np.arange(N_TREES)
        cat = lambda j, shift: np.concatenate([np.where(t[j] < 0, -1, t[j] + o) if shift else t[j] for t, o in zip(trees, off)])
        return P.PackedForest(cat(0, False), cat(1, False), cat(2, True), cat(3, True), cat(4, False), n * np.arange(N_TREES + 1), 14), None
    X = np.concatenate([rng.integers(100, 5000, (2000, 1)), rng.random((2000, 1)) * 4, rng.integers(0, 3000, (2000, 12))], 1).astype(np.float64)
    y = ((X[:, 0] > 2500) ^ (X[:, 4] < 1500) ^ (rng.random(2000) < 0.2)).astype(np.int32)
    rfc = RandomForestClassifier(n_estimators=N_TREES, random_state=0, n_jobs=1).fit(X, y)
    return P.PackedForest.from_sklearn(rfc), rfc


def timed_knn(lib, torch, dev, pts, begin, labels, q_cell, q_xyz, k):
    """Both stages of one sd_syn_props_knn over arrays that are on the device already.  -> (build ms, query ms, vote, counts)."""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pts_d, begin_d, qc_d, qx_d = up(pts), up(begin.astype(np.int64)), up(q_cell.astype(np.int32)), up(q_xyz)
    lab_d = None if labels is None else up(labels.astype(np.int32))
    vote_d = torch.empty(len(q_cell), dtype=torch.int32, device=dev)
    counts_d = torch.zeros(8, dtype=torch.int64, device=dev)
    tmp = torch.empty(lib.sd_syn_props_knn_temp_bytes(len(pts), len(begin) - 1), dtype=torch.uint8, device=dev)
    ms = []
    for stage in (1, 2):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        rc = lib.sd_syn_props_knn(pts_d.data_ptr(), int(pts.dtype == np.float32), begin_d.data_ptr(), len(begin) - 1, len(pts),
                                  None if lab_d is None else lab_d.data_ptr(), qc_d.data_ptr(), qx_d.data_ptr(), len(q_cell), k, stage, vote_d.data_ptr(),
                                  None, None, counts_d.data_ptr(), tmp.data_ptr(), tmp.numel(), torch.cuda.current_stream(dev).cuda_stream)
        e[1].record()
        torch.cuda.synchronize(dev)
        assert rc == 0, lib.sd_last_error()
        ms.append(e[0].elapsed_time(e[1]))
    counts = counts_d.cpu().numpy()
    assert counts[7] == 0
    return ms[0], ms[1], vote_d.cpu().numpy(), dict(tiles_visited=int(counts[0]), tiles_skipped=int(counts[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref-cells', type=int, default=20)
    ap.add_argument('--ref-rows', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'syn_props_probe.json'))
    args = ap.parse_args()
    import torch
    from syconn_amd import _lib as L
    from syconn_amd.extraction import cs_processing_steps as P
    dev, lib = torch.device('cuda', 0), L.load()
    cell_dicts, partners, rep, ratio, feats = make_input()
    cells = P.CellTable.from_cells(cell_dicts)
    forest, rfc = make_forest(P, np.random.default_rng(1))

    class Syn:
        neuron_partners, rep_coords, syn_type_sym_ratio = partners, rep, ratio

        def __len__(self):
            return N_SYN
    s64 = np.array(SCALE, np.float64)
    verts, lab, vbegin = P.spine_vertices(cells, np.ones(len(cells), bool), 'spiness', 1, [4, 5])
    row = partners.reshape(-1).astype(np.int64) - 1                 # cell ids are 1 .. N_CELLS in table order
    q_xyz = np.repeat(rep.astype(np.float64) * s64, 2, 0)
    res = dict(cells=N_CELLS, vertices=len(cells.vertices), vertices_voting=len(verts), nodes=len(cells.nodes), synapses=N_SYN, sides=2 * N_SYN, k=K,
               forest_trees=forest.n_trees, forest_nodes=len(forest.feature), forest='sklearn' if rfc is not None else 'random trees',
               device=torch.cuda.get_device_name(0))
    runs = []
    for _ in range(4):                                              # the first run warms up (allocator, code objects)
        r = {}
        r['vertices_build_ms'], r['vertices_query_ms'], vote, counts_v = timed_knn(lib, torch, dev, verts, vbegin, lab, row, q_xyz, K)
        r['nodes_build_ms'], r['nodes_query_ms'], near, counts_n = timed_knn(lib, torch, dev, cells.nodes * s64, cells.node_begin, None, row, q_xyz, 1)
        arrs = [torch.from_numpy(a).to(dev) for a in (feats, forest.feature, forest.threshold, forest.left, forest.right, forest.proba, forest.tree_begin)]
        out_d, cnt_d = torch.empty((N_SYN, 2), dtype=torch.float64, device=dev), torch.zeros(8, dtype=torch.int64, device=dev)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        rc = lib.sd_syn_props_forest(arrs[0].data_ptr(), N_SYN, 14, *(a.data_ptr() for a in arrs[1:]), forest.n_trees, len(forest.feature), 2,
                                     out_d.data_ptr(), cnt_d.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        e[1].record()
        torch.cuda.synchronize(dev)
        assert rc == 0
        r['forest_ms'] = e[0].elapsed_time(e[1])
        t0 = time.perf_counter()
        props = P.collect_properties_from_ssv_partners(Syn(), cells, SCALE, device=dev)
        r['collect_properties_wall_ms'] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        prob = P.classify_synssv_objects(feats, forest, dev)
        r['classify_wall_ms'] = (time.perf_counter() - t0) * 1e3
        runs.append(r)
    assert np.array_equal(props.partner_spiness.reshape(-1), vote) and np.array_equal(prob, out_d.cpu().numpy()[:, 1])
    res['runs'] = runs[1:]
    res['min_ms'] = {k: round(min(r[k] for r in runs[1:]), 3) for k in runs[0]}
    res['counters'] = dict(vertices=counts_v, nodes=counts_n)
    try:
        from scipy.spatial import cKDTree
        n = min(args.ref_cells, N_CELLS)
        sides = np.flatnonzero(row < n)
        t0 = time.perf_counter()
        ref = np.zeros(len(sides), np.int32)
        for c in range(n):
            mine = np.flatnonzero(row[sides] == c)
            v, l = verts[vbegin[c]:vbegin[c + 1]], lab[vbegin[c]:vbegin[c + 1]]
            _, ixs = cKDTree(v).query(q_xyz[sides[mine]], k=K, workers=1)
            for j, ix in zip(mine, ixs):
                ref[j] = Counter(l[ix]).most_common(1)[0][0]
            cKDTree(cells.nodes[cells.node_begin[c]:cells.node_begin[c + 1]] * s64).query(q_xyz[sides[mine]], k=1, workers=1)
        res.update(ckdtree_cells=n, ckdtree_sides=len(sides), ckdtree_ms=round((time.perf_counter() - t0) * 1e3, 1),
                   ckdtree_votes_differing=int(np.sum(ref != vote[sides])))   # float32 clouds: a near-tie may be ordered differently
    except ImportError:
        res['ckdtree_ms'] = None
    if rfc is not None:
        n = min(args.ref_rows, N_SYN)
        t0 = time.perf_counter()
        ref = np.array([rfc.predict_proba([f])[0][1] for f in feats[:n]])
        res.update(sklearn_rows=n, sklearn_per_row_ms=round((time.perf_counter() - t0) * 1e3, 1), sklearn_agrees=bool(np.array_equal(ref, prob[:n])))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(res) + '\n')
    print(json.dumps({k: v for k, v in res.items() if k != 'runs'}))


if __name__ == '__main__':
    main()
