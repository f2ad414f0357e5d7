"""Generates g33_skeleton_post.npz: inputs and outputs of the reference's own ``sparsify_skelcv``, ``skelcv2nxgraph``, ``nxgraph2skelcv``
(proc/skeleton.py:140-224), ``sparsify_skeleton_fast`` (reps/super_segmentation_helper.py:650-705), ``stitch_skel_nx`` (proc/graphs.py:
701-739) and the flow of ``kimimaro_mergeskels`` (proc/skeleton.py:116-122, without ``kimimaro.postprocess``), lifted by AST at generation
time over networkx and scipy's cKDTree with a stand-in class for ``cloudvolume.Skeleton``.  Only inputs and outputs are stored; no reference
text is.  Stitch inputs have no equal nearest distances (asserted in the kd-tree stand-in), so the tree's tie order never decides.
Run from the repository root with the reference tree at REF."""
import os
import sys
import time
import types

import networkx as nx
import numpy as np
from scipy import spatial

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_cs import lift_function  # noqa: E402

REF = '/root/reference/syconn'


class Skel:
    """Stand-in for cloudvolume.Skeleton: the three arrays, ``simple_merge`` (concatenation) and ``consolidate`` (equal vertices become one:
    distinct vertices in lexicographic order, radius of the first occurrence, edges renamed, no self loops, each once, ascending)."""

    def __init__(self, vertices=None, edges=None, radii=None):
        self.vertices = np.zeros((0, 3), np.float32) if vertices is None else np.asarray(vertices, np.float32).reshape(-1, 3)
        self.edges = np.zeros((0, 2), np.int64) if edges is None else np.asarray(edges, np.int64).reshape(-1, 2)
        self.radii = np.asarray(radii, np.float32).reshape(-1)

    @classmethod
    def simple_merge(cls, skels):
        v, e, r, n = [], [], [], 0
        for s in skels:
            v.append(s.vertices); e.append(s.edges + n); r.append(s.radii)
            n += len(s.vertices)
        return cls(np.concatenate(v), np.concatenate(e), np.concatenate(r))

    def consolidate(self):
        rows = {}
        for k, v in enumerate(self.vertices):
            rows.setdefault(tuple(float(x) for x in v), k)
        order = sorted(rows)
        new = {key: i for i, key in enumerate(order)}
        name = [new[tuple(float(x) for x in v)] for v in self.vertices]
        edges = sorted({(min(name[a], name[b]), max(name[a], name[b])) for a, b in self.edges.tolist() if name[a] != name[b]})
        return Skel(np.array(order, np.float32), edges, self.radii[[rows[key] for key in order]])


class Tree(spatial.cKDTree):
    def query(self, x, n_jobs=1):
        k = min(2, self.n)
        d, i = super().query(x, k=k)
        d, i = np.asarray(d).reshape(len(x), k), np.asarray(i).reshape(len(x), k)
        row = int(np.argmin(d[:, 0]))
        first = np.sort(d[:, 0])
        assert len(first) < 2 or first[0] < first[1], 'two nodes of the largest component are equally near the rest'
        assert k < 2 or d[row, 0] < d[row, 1], 'two rest nodes are equally near'
        return d[:, 0], i[:, 0]


def tree_skeleton(rng, n, step, branches, offset=0.0):
    v = [rng.uniform(0, 50, 3) + offset]
    e = []
    tips = [0]
    for k in range(1, n):
        src = tips[-1] if rng.random() > branches else int(rng.integers(0, k))
        v.append(v[src] + rng.normal(0, 1, 3) * step + np.array([step, 0, 0]))
        e.append((src, k))
        tips.append(k)
    return Skel(np.array(v), e, rng.uniform(10, 200, n))


def main():
    ns = {'np': np, 'nx': nx, 'spatial': types.SimpleNamespace(cKDTree=Tree), 'time': time, 'global_params': None, 'log_reps': None,
          'cloudvolume': types.SimpleNamespace(Skeleton=Skel, PrecomputedSkeleton=Skel)}
    exec('from typing import *', ns)
    p = f'{REF}/proc/skeleton.py'
    for name in ('skelcv2nxgraph', 'nxgraph2skelcv'):
        ns[name] = lift_function(p, name, ns)
    sparsify_skelcv = lift_function(p, 'sparsify_skelcv', ns)
    sparsify_fast = lift_function(f'{REF}/reps/super_segmentation_helper.py', 'sparsify_skeleton_fast', ns)
    stitch = lift_function(f'{REF}/proc/graphs.py', 'stitch_skel_nx', ns)
    rng = np.random.default_rng(3301)
    out = {}

    def put(key, s):
        out[key + '_v'], out[key + '_e'], out[key + '_r'] = s.vertices, s.edges, s.radii

    cases = [(tree_skeleton(rng, 120, 30, 0.05), np.array([1, 1, 1])), (tree_skeleton(rng, 200, 12, 0.1), np.array([1, 1, 1])),
             (tree_skeleton(rng, 90, 4, 0.08), np.array([10, 10, 20])), (tree_skeleton(rng, 60, 3, 0.0), np.array([9.5, 9.5, 20.0]))]
    out['n_sparsify'] = np.int64(len(cases))
    for k, (s, scale) in enumerate(cases):
        put(f'sp{k}_in', s)
        out[f'sp{k}_scale'] = scale
        put(f'sp{k}_out', sparsify_skelcv(Skel(s.vertices.copy(), s.edges.copy(), s.radii.copy()), scale=scale))
        put(f'sp{k}_fast', ns['nxgraph2skelcv'](sparsify_fast(ns['skelcv2nxgraph'](s), scal=scale)))
        assert len(out[f'sp{k}_out_v']) < len(s.vertices)
    stitch_in = []
    for k in range(3):
        parts = [tree_skeleton(rng, int(rng.integers(3, 40)), 60, 0.1, offset=rng.uniform(0, 4000, 3)) for _ in range(int(rng.integers(3, 7)))]
        if k == 2:
            parts += [tree_skeleton(rng, len(parts[0].vertices), 60, 0.1, offset=rng.uniform(0, 4000, 3))]      # two components of equal size
        stitch_in.append(Skel.simple_merge(parts))
    out['n_stitch'] = np.int64(len(stitch_in))
    for k, s in enumerate(stitch_in):
        put(f'st{k}_in', s)
        g = stitch(ns['skelcv2nxgraph'](s), n_jobs=1)
        assert nx.number_connected_components(g) == 1
        put(f'st{k}_out', ns['nxgraph2skelcv'](g))
    out['n_merge'] = np.int64(2)
    for k in range(2):
        a = tree_skeleton(rng, 50, 80, 0.05)
        a.vertices = np.round(a.vertices)
        b = tree_skeleton(rng, 30, 80, 0.05, offset=3000.0)
        b.vertices = np.round(b.vertices)
        b.vertices[:3] = a.vertices[-3:]                   # the pieces of two chunks share vertices at the seam
        c = tree_skeleton(rng, 12, 80, 0.0, offset=-2500.0)
        pieces = [a, b, c]
        out[f'mg{k}_n'] = np.int64(len(pieces))
        for j, s in enumerate(pieces):
            put(f'mg{k}_in{j}', s)
        skel = Skel.simple_merge(pieces).consolidate()     # the flow of kimimaro_mergeskels, :116-122
        put(f'mg{k}_out', ns['nxgraph2skelcv'](stitch(ns['skelcv2nxgraph'](skel), n_jobs=1)))
    np.savez_compressed(os.path.join(HERE, 'g33_skeleton_post.npz'), **out)
    print('wrote g33_skeleton_post.npz:', len(out), 'arrays')


if __name__ == '__main__':
    main()
