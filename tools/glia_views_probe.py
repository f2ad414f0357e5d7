"""Times of the glia view step on ONE synthetic cell built the way tools/views_probe.py builds its cell: the branched tube of
``make_cell`` in a label volume of `--shape` voxels of `--voxel` nm, cut into `--svs` supervoxels along x, meshed by the project's own
``find_meshes_table``; seeded weights (no trained glia model exists here); the default window (256 x 128 pixels, 8000 nm, 2 views).

    python tools/glia_views_probe.py [--out profiles/glia_views_probe.json]

Reports, as the minimum of three runs after one warm-up, from HIP events: the rendering locations (``sample_locations_sso``), the
rasteriser (``render_sso_coords(add_cellobjects=False)``), the network (the logits of ``GliaViewModel``), the softmax
(``sd_glia_view_probas``), the centre filter (``sd_views_center_component`` on the rendered planes, background 255), each repeated
inside its timed region until the region lasts about `--min-ms` milliseconds, per call; and the wall time of ``predict_glia_table``
(host clock around work that ends in a download).  It is a tool, not a test: no pass / fail rides on the times."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


class Sv:
    def __init__(self, i, mesh, rep, scaling):
        self.id, self.mesh, self.rep_coord, self.scaling, self.attr_dict = int(i), mesh, rep, scaling, {}


class Cell:
    def __init__(self, svs):
        self.svs = svs
        ind, vert, n = [], [], 0
        for sv in svs:
            ind.append(np.asarray(sv.mesh[0], np.uint32) + np.uint32(n))
            vert.append(np.asarray(sv.mesh[1], np.float32))
            n += len(sv.mesh[1]) // 3
        self.mesh = [np.concatenate(ind), np.concatenate(vert), np.zeros(0, np.float32)]

    def load_mesh(self, name):
        return [np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.float32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=[256, 192, 128])
    ap.add_argument('--voxel', type=float, default=50.0)
    ap.add_argument('--svs', type=int, default=16)
    ap.add_argument('--ds', type=float, default=400.0)
    ap.add_argument('--min-ms', type=float, default=200.0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'glia_views_probe.json'))
    args = ap.parse_args()
    import torch
    import _viewnet_ref as R
    from syconn_amd import _dev as D
    from syconn_amd.cnn.viewnet_spec import GLIA_CMN
    from syconn_amd.handler.prediction import GliaViewModel, glia_view_probas
    from syconn_amd.proc import meshes
    from syconn_amd.proc.image import center_component_planes
    from syconn_amd.proc.rendering import render_sso_coords
    from syconn_amd.reps.super_segmentation_helper import predict_glia_table, sample_locations_sso
    spec_ = importlib.util.spec_from_file_location('views_probe', os.path.join(ROOT, 'tools', 'views_probe.py'))
    probe = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(probe)
    dev = D.device('cuda:0')
    vol = probe.make_cell(tuple(args.shape))
    slab = (np.arange(args.shape[0]) * args.svs // args.shape[0] + 1).astype(np.uint64)
    vol = vol * slab[:, None, None]
    scaling = (args.voxel,) * 3
    table = meshes.find_meshes_table(vol, (0, 0, 0), scaling=scaling, meshing_props={'normals': False}, device=dev)
    cell = Cell([Sv(i, table.mesh_of(i), (0, 0, 0), scaling) for i in table.ids])
    spec = GLIA_CMN()
    model = GliaViewModel(spec, R.state_dict_of(spec, R.make_weights(spec, 321, 2, 128, 256)), device=dev)
    locs = np.concatenate(sample_locations_sso(cell, args.ds, device=dev))
    views = render_sso_coords(cell, locs, add_cellobjects=False, device=dev, return_device=True)
    logits = model.predict_device(views, apply_softmax=False)
    res = dict(volume=list(args.shape), voxel_nm=args.voxel, supervoxels=len(cell.svs), vertices=len(cell.mesh[1]) // 3, ds_factor=args.ds,
               locations=len(locs), view_bytes=views.numel(), launch_set=model.bs, act_dtype=model.act_dtype, device=torch.cuda.get_device_name(0))
    calls = dict(locations_ms=lambda: sample_locations_sso(cell, args.ds, device=dev),
                 raster_ms=lambda: render_sso_coords(cell, locs, add_cellobjects=False, device=dev, return_device=True),
                 network_ms=lambda: model.predict_device(views, apply_softmax=False),
                 softmax_ms=lambda: glia_view_probas(logits),
                 center_filter_ms=lambda: center_component_planes(views, 255))

    def timed(call, reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        for _ in range(reps):
            call()
        e[1].record()
        torch.cuda.synchronize(dev)
        return e[0].elapsed_time(e[1]) / reps

    reps = {}
    for name, call in calls.items():      # warm-up, and the repetitions that make a region last about --min-ms
        timed(call, 1)
        reps[name] = int(min(max(1, np.ceil(args.min_ms / max(timed(call, 2), 1e-3))), 100000))
    runs = [{name: timed(call, reps[name]) for name, call in calls.items()} for _ in range(3)]
    walls = []
    for _ in range(4):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        t = predict_glia_table([cell], model, ds_factor=args.ds, device=dev)
        walls.append((time.perf_counter() - t0) * 1e3)
    res.update(repetitions=reps, runs=runs, min_ms={k: round(min(r[k] for r in runs), 4) for k in calls},
               predict_glia_table_wall_ms=round(min(walls[1:]), 2), predict_glia_table_wall_runs_ms=[round(w, 2) for w in walls[1:]],
               glia_share=float(t.glia.mean()), locations_per_s_wall=round(len(locs) / (min(walls[1:]) * 1e-3), 1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(res) + '\n')
    print(json.dumps({k: v for k, v in res.items() if k != 'runs'}))


if __name__ == '__main__':
    main()
