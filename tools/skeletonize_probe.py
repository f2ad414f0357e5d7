"""Probe of the skeletonisation chain (proc/skeleton.py: trace_chunk) on an MI355X: one synthetic branching cell in a 512 x 512 x 256 chunk.
Writes profiles/skeletonize_probe.json: stage times from HIP events (minimum of three runs; the chain is stateful, so a region is NOT
repeated up to 200 ms as the other probes do -- the short stages carry the launch and synchronisation overhead of one call), sweeps and
tiles per relaxation, the share of the invalidation box fill, and the time of the CPU restatement on a crop small enough to finish.
No ratio to the reference: kimimaro cannot run here.   python tools/skeletonize_probe.py [--small]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def branching_cell(shape, rng):
    """A trunk along x with side branches of falling radius: label 1, radii 3 .. 8 voxels."""
    X, Y, Z = shape
    seg = np.zeros(shape, np.uint64)
    zz, yy = np.meshgrid(np.arange(Z), np.arange(Y), indexing='ij')

    def tube(p0, p1, r):
        p0, p1 = np.array(p0, float), np.array(p1, float)
        n = int(np.abs(p1 - p0).max()) + 1
        for t in np.linspace(0, 1, n):
            c = p0 + (p1 - p0) * t
            lo = np.maximum(np.floor(c - r).astype(int), 0)
            hi = np.minimum(np.ceil(c + r).astype(int) + 1, shape)
            g = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a]) for a in range(3)], indexing='ij'), -1)
            seg[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]][((g - c) ** 2).sum(-1) <= r * r] = 1

    tube((10, Y // 2, Z // 2), (X - 10, Y // 2, Z // 2), 8)
    for k in range(12):
        x = 30 + k * (X - 60) // 12
        end = (x + rng.integers(-30, 30), rng.integers(12, Y - 12), rng.integers(12, Z - 12))
        tube((x, Y // 2, Z // 2), end, 5)
        tube(end, (min(max(end[0] + rng.integers(-60, 60), 8), X - 8), rng.integers(8, Y - 8), rng.integers(8, Z - 8)), 3)
    return seg


def main():
    import torch
    from syconn_amd.proc.skeleton import TEASAR_DEFAULTS, trace_chunk
    small = '--small' in sys.argv
    shape = (128, 128, 64) if small else (512, 512, 256)
    seg = branching_cell(shape, np.random.default_rng(7))
    seg_d = torch.from_numpy(seg.view(np.int64)).cuda()
    w = (10, 10, 20)
    runs, out = [], None
    for _ in range(3):
        t = {}
        t0 = time.perf_counter()
        out = trace_chunk(seg_d, w, dict(TEASAR_DEFAULTS), dust_threshold=1000, timings=t)
        t['wall_ms'] = (time.perf_counter() - t0) * 1e3
        runs.append(t)
    stage_ms = {k: min(r[k] for r in runs) for k in runs[0]}
    res = dict(shape=list(shape), anisotropy=list(w), teasar=dict(TEASAR_DEFAULTS), foreground_voxels=int(out['sizes'].sum()), components=int(len(out['sizes'])),
               nodes=int(len(out['node_voxel'])), rounds=(len(out['stats']) - 3), stage_ms_min_of_3=stage_ms, runs=runs,
               relaxations=[dict(sweeps=s, tiles=tl, tiles_per_sweep=(tl / s if s else 0)) for s, tl in out['stats']],
               note='round_target_walk_invalidate holds the per-node box fill of the invalidation; regions are not repeated (stateful chain)')
    # the CPU restatement on a crop small enough to finish
    import _skeletonize_ref as R
    crop = seg[:48, shape[1] // 2 - 12:shape[1] // 2 + 12, shape[2] // 2 - 12:shape[2] // 2 + 12].copy()
    t0 = time.perf_counter()
    r = R.skeletonize(crop, w, dust_threshold=100, scale=2.0, const=500.0, max_paths=100)
    res['cpu_restatement'] = dict(crop=list(crop.shape), foreground_voxels=int((crop > 0).sum()), seconds=time.perf_counter() - t0, rounds=len(r['targets']))
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    path = os.path.join(ROOT, 'profiles', 'skeletonize_probe_small.json' if small else 'skeletonize_probe.json')
    with open(path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ('shape', 'foreground_voxels', 'nodes', 'rounds', 'stage_ms_min_of_3', 'cpu_restatement')}))


if __name__ == '__main__':
    main()
