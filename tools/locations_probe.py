"""Times of the rendering locations (csrc/sd_locations.hip) on two inputs: the synthetic cell of tools/views_probe.py (one object: a
branched tube meshed by the project's own ``find_meshes_table``) and a table of `--objects` small random clouds.

    python tools/locations_probe.py [--out profiles/locations_probe.json]

Reports per input and rule (voxel: ``sd_locations_voxel``, surface: ``sd_locations_surface``, both with ds_factor 2000), as the minimum of
three runs after one warm-up, from HIP events and without uploads: the sizing call (boxes, keys, the two sorts, the runs), the emitting
call (all of that again, then the locations), and their difference, which is what the emit kernels cost.  Beside them the wall time of
the surface rule in its scipy form (one ``cKDTree`` and one ``histogramdd`` per object, written out below) on the same input, on the
host this probe runs on.  The numbers are recorded; none is asserted, and no ratio to the reference's batch job is claimed: it writes
storages and spreads supervoxels over processes, and cannot run next to this probe."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def surface_scipy(v, bins, r):
    """The surface rule of one object over scipy's tree and numpy's histogram."""
    from scipy.spatial import cKDTree
    bs = np.asarray(bins, np.float32)
    off = v.min(0)
    c = v - off
    tree = cKDTree(c)
    nb = np.maximum(1, np.ceil(c.max(0) / bs).astype(np.int32))
    hist, _ = np.histogramdd(c, bins=nb)
    centres = (np.argwhere(hist != 0) + 0.5) * bs
    picked = c[tree.query(centres)[1]]
    return np.array([c[m].mean(0) + off for m in tree.query_ball_point(picked, r=r)], np.float32)


def small_objects(n_obj, seed=3):
    rng = np.random.default_rng(seed)
    k = rng.integers(30, 101, n_obj)
    begin = np.concatenate(([0], np.cumsum(k))).astype(np.uint64)
    centre = rng.uniform(0, 2e5, (n_obj, 3))
    v = (np.round((np.repeat(centre, k, axis=0) + rng.uniform(-2500, 2500, (int(begin[-1]), 3))) * 2) / 2).astype(np.float32)
    return begin, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=[256, 192, 128])
    ap.add_argument('--voxel', type=float, default=50.0)
    ap.add_argument('--objects', type=int, default=5000)
    ap.add_argument('--ds', type=float, default=2000.0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'locations_probe.json'))
    args = ap.parse_args()
    import torch
    from views_probe import make_cell
    from syconn_amd import _dev as D
    from syconn_amd.proc import meshes
    dev = D.device('cuda:0')
    cell = meshes.find_meshes_table(make_cell(tuple(args.shape)), (0, 0, 0), scaling=(args.voxel,) * 3, meshing_props={'normals': False}, device=dev)
    inputs = {'cell': (cell.vert_begin, cell.vertices), 'small_objects': small_objects(args.objects)}
    ds = args.ds
    res = dict(volume=list(args.shape), voxel_nm=args.voxel, ds_factor=ds, device=torch.cuda.get_device_name(0), inputs={})
    bins3 = (C.c_float * 3)(ds, ds, ds)
    for name, (begin, verts) in inputs.items():
        n_obj, n_v = len(begin) - 1, len(verts)
        v_d, b_d = D.up(verts, dev), D.up(begin, dev)
        loc_begin, cnt = D.empty(n_obj + 1, D.i64, dev), D.counters(dev)
        out = dict(objects=n_obj, vertices=n_v)
        for rule in ('voxel', 'surface'):
            entry = 'sd_locations_' + rule
            head = (v_d, 1, b_d, n_obj, n_v, ds, loc_begin) if rule == 'voxel' else (v_d, b_d, n_obj, n_v, bins3, ds / 2, loc_begin)
            tmp = D.scratch(entry + '_temp_bytes', dev, n_v, n_obj)
            D.call(entry, dev, *head, None, 0, cnt, tmp, tmp.numel())
            c = D.down(cnt)
            assert not c[4] and not c[5] and not c[7]
            n = int(c[0])
            loc = D.empty((n, 3), D.f64 if rule == 'voxel' else torch.float32, dev)
            calls = dict(sizing_ms=lambda: D.call(entry, dev, *head, None, 0, cnt, tmp, tmp.numel()),
                         emitting_ms=lambda: D.call(entry, dev, *head, loc, n, cnt, tmp, tmp.numel()))
            runs = []
            for _ in range(4):                                      # the first run warms up (allocator, code objects)
                r = {}
                for key, call in calls.items():
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    e[0].record()
                    call()
                    e[1].record()
                    torch.cuda.synchronize(dev)
                    r[key] = e[0].elapsed_time(e[1])
                runs.append(r)
            c = D.down(cnt)
            assert not c[1] and int(c[0]) == n
            m = {k: round(min(r[k] for r in runs[1:]), 3) for k in runs[0]}
            m['emit_kernels_ms'] = round(m['emitting_ms'] - m['sizing_ms'], 3)
            out[rule] = dict(locations=n, min_ms=m, runs=runs[1:])
            if rule == 'surface':
                out[rule].update(tiles_visited=int(c[2]), tiles_skipped=int(c[3]))
                b = begin.astype(np.int64)
                t0 = time.perf_counter()
                host = [surface_scipy(verts[b[k]:b[k + 1]], (ds, ds, ds), ds / 2) for k in range(n_obj) if b[k + 1] > b[k]]
                out[rule]['scipy_form_wall_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
                out[rule]['scipy_form_locations'] = int(sum(len(h) for h in host))
        res['inputs'][name] = out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(res) + '\n')
    for name, out in res['inputs'].items():
        print(name, json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != 'runs'} if isinstance(v, dict) else v) for k, v in out.items()}))


if __name__ == '__main__':
    main()
