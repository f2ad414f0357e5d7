"""Times of the view raster (csrc/sd_views.hip) on ONE synthetic cell: a branched tube drawn into a label volume of `--shape` voxels of
`--voxel` nm, meshed by the project's own ``find_meshes_table``; every `--every`-th vertex (default: every 10th) of the mesh is a rendering location; the
default window (256 x 128 pixels, 8000 nm, 2 views).

    python tools/views_probe.py [--out profiles/views_probe.json]

Reports, as the minimum of three runs after one warm-up, from HIP events and without uploads: the rotations, the triangle grid
(sd_views_index), the candidate lists (sd_views_candidates: the sizing call and the emitting call), the depth raster with its filter
(sd_views_render) and the index raster (sd_views_render_index); depth views per second from the raster time alone; the mean
candidates per location.  No pass / fail rides on the times; the reference renders with OpenGL, which cannot run next to this probe, so no
ratio to it exists."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_cell(shape, seed=0):
    """A label volume (x, y, z) uint64 with one object: three tubes of varying radius from a common soma."""
    rng = np.random.default_rng(seed)
    vol = np.zeros(shape, np.uint64)
    s = np.array(shape, np.float64)

    def ball(c, r):
        lo, hi = np.maximum(np.floor(c - r).astype(int), 1), np.minimum(np.ceil(c + r).astype(int) + 1, np.array(shape) - 1)
        g = np.stack(np.meshgrid(*[np.arange(a, b) for a, b in zip(lo, hi)], indexing='ij'), -1)
        vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]][((g - c) ** 2).sum(-1) <= r * r] = 1
    soma = s * [0.2, 0.5, 0.5]
    ball(soma, 0.12 * s.min())
    for end in ([0.95, 0.15, 0.3], [0.95, 0.55, 0.75], [0.9, 0.9, 0.35]):
        t = np.linspace(0, 1, 400)[:, None]
        path = soma + t * (s * end - soma) + 0.06 * s.min() * np.sin(2 * np.pi * t * rng.uniform(1, 3, 3) + rng.uniform(0, 6, 3))
        for k, c in enumerate(path):
            ball(c, 3.5 + 2.5 * np.sin(k / 23.0) ** 2)
    return vol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=[256, 192, 128])
    ap.add_argument('--voxel', type=float, default=50.0)
    ap.add_argument('--every', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'views_probe.json'))
    args = ap.parse_args()
    import torch
    from syconn_amd import _dev as D
    from syconn_amd.proc import meshes, rendering
    dev = D.device('cuda:0')
    table = meshes.find_meshes_table(make_cell(tuple(args.shape)), (0, 0, 0), scaling=(args.voxel,) * 3, meshing_props={'normals': False}, device=dev)
    verts, tris = table.vertices, table.indices
    coords = verts[::args.every].copy()
    ws, nb_views, cw = (256, 128), 2, 8000.0
    W, H = ws
    n, n_v, n_t = len(coords), len(verts), len(tris)
    res = dict(volume=list(args.shape), voxel_nm=args.voxel, vertices=n_v, triangles=n_t, locations=n, ws=list(ws), nb_views=nb_views, comp_window=cw,
               device=torch.cuda.get_device_name(0))
    vm = rendering.ViewMesh(tris, verts, device=dev)
    lib = D.L.load()
    c_d = D.up(coords, dev)
    f64n = lambda v: (C.c_double * len(v))(*[float(x) for x in v])
    ang = np.deg2rad(rendering.view_angles(nb_views))
    E, cos_v, sin_v, w7 = f64n(vm.edge_lengths(cw)), f64n(np.cos(ang)), f64n(np.sin(ang)), f64n(rendering.gauss_weights())
    cnt = D.counters(dev)
    stride = meshes.rot_vertex_stride(n_v)
    rot_d = D.empty((n, 16), D.f64, dev)
    rot_tmp = D.scratch('sd_views_rotations_temp_bytes', dev, n_v, stride)
    ix = D.empty(int(lib.sd_views_index_bytes(n_t)), D.u8, dev)
    ix_tmp = D.scratch('sd_views_index_temp_bytes', dev, n_t)
    begin = D.empty(n + 1, D.i64, dev)
    c_tmp = D.scratch('sd_views_candidates_temp_bytes', dev, n)
    norm = (vm.center3, float(vm.max_dist))
    D.call('sd_views_index', dev, vm.verts, n_v, vm.tris, n_t, *norm, ix, ix.numel(), cnt, ix_tmp, ix_tmp.numel())
    D.call('sd_views_candidates', dev, ix, n_t, c_d, n, *norm, E, begin, None, 0, cnt, c_tmp, c_tmp.numel())
    n_cand = int(D.down(cnt)[0])
    cand = D.empty(n_cand, D.i32, dev)
    views = torch.empty((n, nb_views, H, W), dtype=torch.uint8, device=dev)
    iviews = torch.empty((n, nb_views, H, W), dtype=torch.int32, device=dev)
    r_tmp = D.scratch('sd_views_render_temp_bytes', dev, n, nb_views)
    head = (vm.verts, n_v, vm.tris, n_t, ix, c_d, n, rot_d, *norm, E, cos_v, sin_v, nb_views, W, H)
    calls = dict(
        rotations_ms=lambda: D.call('sd_views_rotations', dev, vm.verts, n_v, stride, c_d, n, *norm, float(np.float32(cw / vm.max_dist)), rot_d, None, cnt,
                                    rot_tmp, rot_tmp.numel()),
        index_ms=lambda: D.call('sd_views_index', dev, vm.verts, n_v, vm.tris, n_t, *norm, ix, ix.numel(), cnt, ix_tmp, ix_tmp.numel()),
        candidates_ms=lambda: (D.call('sd_views_candidates', dev, ix, n_t, c_d, n, *norm, E, begin, None, 0, cnt, c_tmp, c_tmp.numel()),
                               D.call('sd_views_candidates', dev, ix, n_t, c_d, n, *norm, E, begin, cand, n_cand, cnt, c_tmp, c_tmp.numel())),
        raster_filter_ms=lambda: D.call('sd_views_render', dev, *head, w7, begin, cand, n_cand, views, views.numel(), cnt, r_tmp, r_tmp.numel()),
        index_raster_ms=lambda: D.call('sd_views_render_index', dev, *head, begin, cand, n_cand, iviews, iviews.numel(), cnt, r_tmp, r_tmp.numel()))
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
        runs.append(r)
    c = D.down(cnt)
    assert not c[1] and not c[3]
    res['runs'] = runs[1:]
    res['min_ms'] = {k: round(min(r[k] for r in runs[1:]), 3) for k in runs[0]}
    res['depth_views_per_s'] = round(n * nb_views / (res['min_ms']['raster_filter_ms'] * 1e-3), 1)
    res['candidates'] = n_cand
    res['mean_candidates_per_location'] = round(n_cand / max(n, 1), 1)
    v = views.cpu().numpy()
    res['drawn_pixel_share'] = round(float((v != 255).mean()), 4)
    res['zero_matrices'] = int((~D.down(rot_d).any(1)).sum())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(res) + '\n')
    print(json.dumps({k: v for k, v in res.items() if k != 'runs'}))


if __name__ == '__main__':
    main()
