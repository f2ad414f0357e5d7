"""Stage times of the surface meshes (csrc/sd_mesh.hip) on ONE synthetic organelle chunk: `--shape` voxels (default 512 x 512 x 256) with
one ellipsoid of its own label in every 32 x 32 x 16 cell (made on the device), meshed at ds (4, 4, 2) and (1, 1, 1) with pad 1.

    python tools/mesh_probe.py [--out profiles/mesh_probe.json]

Reports per ds, as the minimum of three runs after one warm-up, from HIP events and without uploads: ``sd_mesh_count`` (one pass over
the volume) and ``sd_mesh_build`` (count pass, scans, emit pass, two sorts, vertices, indices, boxes and areas); the wall time of
``find_meshes_table`` with the ids given (uploads of the tables, the two calls, the copies of the result to the host); vertices,
triangles and objects; and the bytes of label volume the three voxel passes would read if every padded voxel were fetched once per pass
(8 bytes per voxel and pass -- an algorithmic figure: hardware counters are not collected here, and the eightfold re-read of a voxel
by its neighbours is served by the caches or not, which this probe does not tell).  No pass / fail rides on the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCALING = np.array([10., 10., 20.])


def make_chunk(shape, dev):
    import torch
    ax = [torch.arange(n, device=dev) for n in shape]
    cell = [32, 32, 16]
    d2 = sum((((a % c) - c / 2 + 0.5) / (0.35 * c)) ** 2 for a, c in zip(torch.meshgrid(*ax, indexing='ij'), cell))
    idx = [a // c for a, c in zip(torch.meshgrid(*ax, indexing='ij'), cell)]
    n = [-(-s // c) for s, c in zip(shape, cell)]
    lab = (idx[0] * n[1] + idx[1]) * n[2] + idx[2] + 1
    return torch.where(d2 < 1, lab, torch.zeros_like(lab)).contiguous()


def main():
    import torch
    from syconn_amd import _dev as D
    from syconn_amd.proc.meshes import _source_tables, find_meshes_table
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=[512, 512, 256])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_probe.json'))
    args = ap.parse_args()
    dev = D.device()
    vol = make_chunk(args.shape, dev)
    ids = np.unique(D.down(torch.unique(vol), view=np.uint64))
    ids = ids[ids != 0]
    ids_dev = D.up(ids, dev)
    X, Y, Z = args.shape
    out = dict(shape=args.shape, objects=int(len(ids)), device=torch.cuda.get_device_name(dev), runs={})

    def timed(fn):
        best = None
        for k in range(4):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if k:
                best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
        return best
    for ds in ((4, 4, 2), (1, 1, 1)):
        tabs = _source_tables((X, Y, Z), 1, np.asarray(ds, np.float64))
        NX, NY, NZ = (len(t) for t in tabs)
        tx, ty, tz = (D.up(t, dev) for t in tabs)
        s_ds = SCALING * np.asarray(ds, np.float64)
        cnt = D.counters(dev)
        count = lambda: D.call('sd_mesh_count', dev, vol, X, Y, Z, tx, ty, tz, NX, NY, NZ, ids_dev, len(ids), cnt)
        ms_count = timed(count)
        c = D.down(cnt)
        nv, nt, n = int(c[0]), int(c[1]), len(ids)
        vb, tb = D.empty(n + 1, D.i64, dev), D.empty(n + 1, D.i64, dev)
        verts, tris = D.empty((nv, 3), torch.float32, dev), D.empty((nt, 3), D.i32, dev)
        bb, area = D.empty((n, 6), torch.float32, dev), D.empty(n, D.f64, dev)
        tmp = D.scratch('sd_mesh_build_temp_bytes', dev, NX, NY, NZ, nv, nt)
        build = lambda: D.call('sd_mesh_build', dev, vol, X, Y, Z, tx, ty, tz, NX, NY, NZ, ids_dev, n, D.f64x3(s_ds), D.f64x3(-s_ds), nv, nt, vb, tb, verts,
                               tris, bb, area, cnt, tmp, tmp.numel())
        ms_build = timed(build)
        assert not D.down(cnt)[2:].any()
        wall = []
        for _ in range(3):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            t = find_meshes_table(vol, (0, 0, 0), pad=1, ds=ds, scaling=SCALING, device=dev, ids=ids)
            wall.append((time.perf_counter() - t0) * 1e3)
        assert len(t.vertices) == nv and len(t.indices) == nt
        out['runs']['x'.join(str(d) for d in ds)] = dict(
            padded_shape=[NX, NY, NZ], vertices=nv, triangles=nt, sd_mesh_count_ms=ms_count, sd_mesh_build_ms=ms_build, scratch_bytes=int(tmp.numel()),
            find_meshes_table_wall_ms=min(wall), label_bytes_per_padded_voxel_if_fetched_once_per_pass=24, voxel_passes=3,
            note='bytes are algorithmic (8 per voxel and pass), not from hardware counters')
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
