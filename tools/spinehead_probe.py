"""Stage times of the spine head volumes (csrc/sd_spinehead.hip with the EDT, flood and kNN entries it calls) per window, at the
reference's own ``ctx_vol`` (200, 200, 100) with scaling (10, 10, 20): windows of 400 x 400 x 200 voxels, 200^3 after the zoom.  One
synthetic cell: a shaft with spines (necks and heads of 12 - 20 voxels radius) in a 600 x 600 x 300 dataset, its surface voxels as mesh
vertices labelled shaft / neck / head; one window per head.

    python tools/spinehead_probe.py [--windows 3] [--ctx 200 200 100] [--out profiles/spinehead_probe.json]

Per window, interleaved in one process, the minimum of three runs: the device stages from HIP events (mask, fill holes, EDT, peaks; the
vertex boxes, the vote; markers + flood + selection) and the wall time of the whole window; and the reference's per-synapse CPU form = the
restatement tests/_spinehead_ref.py (scipy zoom / fill holes / EDT / label / cKDTree, the Python flood of oracle/objseg_ref.py, which is
far slower than skimage's compiled one: its share is reported separately so that it can be left out of the ratio).  Checks that both
give the same voxel count.  No pass / fail rides on the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SCALING, K = np.array([10, 10, 20]), 50


def make_input(ctx, n_heads, seed=0):
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    ds = SCALING[2] // SCALING
    shape = tuple(int(v) for v in 3 * np.asarray(ctx))
    iso = [(np.arange(n) + 0.5) / d for n, d in zip(shape, ds)]
    X, Y, Z = np.meshgrid(*iso, indexing='ij', sparse=True)
    ext = np.array(shape) / ds
    own = ((Y - ext[1] / 2) ** 2 + (Z - ext[2] / 2) ** 2) <= (0.06 * ext[2]) ** 2 + 0 * X           # the shaft along x
    lab = np.where(own, 2, -1).astype(np.int8)
    reps = []
    for h in range(n_heads):
        c = np.array([ext[0] * (h + 1) / (n_heads + 1), ext[1] / 2 + rng.uniform(0.15, 0.22) * ext[1] * (1 if h % 2 else -1), ext[2] / 2 + rng.uniform(-0.1, 0.1) * ext[2]])
        r = rng.uniform(0.04, 0.07) * ext[2]
        ball = ((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) <= r * r
        neck = (((X - c[0]) ** 2 + (Z - c[2]) ** 2) <= (0.3 * r) ** 2) & ((Y - c[1]) * (Y - ext[1] / 2) <= 0)
        lab[ball & ~own] = 1
        own |= ball
        lab[neck & ~own] = 0
        own |= neck
        reps.append(np.floor(c * ds).astype(np.int64))
    vol = np.where(own, np.uint64(7), np.uint64(0))
    surf = own & ~ndimage.binary_erosion(own)
    pos = np.transpose(np.nonzero(surf))
    verts = ((pos + 0.5) * SCALING + rng.uniform(-3, 3, pos.shape)).astype(np.float32)
    return vol, verts, lab[tuple(pos.T)].astype(np.int64), np.array(reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--ctx', type=int, nargs=3, default=[200, 200, 100])
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spinehead_probe.json'))
    args = ap.parse_args()
    import torch
    import _spinehead_ref as R
    from oracle import objseg_ref
    from syconn_amd.extraction import spinehead as SH
    ctx = np.array(args.ctx)
    vol, verts_nm, labels, reps = make_input(ctx, args.windows)
    verts = verts_nm / SCALING
    dev = torch.device('cuda', 0)
    size = (2 * ctx).astype(np.int32)
    ds = SCALING[2] // SCALING
    tabs_h = [SH.zoom_source_table(int(size[a]), ds[a]) for a in range(3)]
    runner = SH.WindowRunner([len(t) for t in tabs_h], batch=1, device=dev)
    tabs = [torch.from_numpy(t).to(dev) for t in tabs_h]
    seg_d = torch.from_numpy(vol.view(np.int64)).to(dev)
    sv_d = torch.tensor([7], dtype=torch.int64, device=dev)
    verts_d, lab_d = torch.from_numpy(verts).to(dev), torch.from_numpy(labels.astype(np.int32)).to(dev)
    res = dict(ctx_vol=ctx.tolist(), window=[len(t) for t in tabs_h], n_vertices=int(len(verts)), windows=[])

    def device_window(rep):
        off = np.maximum(rep - ctx, 0)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        runner.buf.zero_()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ev[0].record()
        runner.fill_holes(runner.window_mask(seg_d, (0, 0, 0), off, tabs, sv_d), 0)
        ev[1].record()
        runner.edt(0)
        runner.find_peaks(0)
        ev[2].record()
        pts, lab, begin = runner.box_vertices(verts_d, lab_d, off[None], size)
        if len(pts):
            runner.vote(1, pts, lab, ds.astype(np.float64), K)
        ev[3].record()
        if len(pts):
            runner.flood_select(0, rep - off, off, SCALING.astype(np.float64))
        ev[4].record()
        out = runner.res32[0].cpu().numpy()
        wall = time.perf_counter() - t0
        ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]
        return dict(mask_fill_ms=ms[0], edt_peaks_ms=ms[1], vertices_vote_ms=ms[2], flood_select_ms=ms[3], wall_ms=wall * 1e3), int(out[2]), int(out[1])

    def cpu_window(rep):
        off = np.maximum(rep - ctx, 0)
        flood_s = [0.0]
        inner = objseg_ref.watershed_ref

        def timed(*a):
            t = time.perf_counter()
            r = inner(*a)
            flood_s[0] += time.perf_counter() - t
            return r
        R.watershed_ref = timed
        try:
            t0 = time.perf_counter()
            st = R.window_stages(R.load_window(vol, (0, 0, 0), off, size), [7], ds, verts, labels, off, size, rep - off, SCALING, K)
            wall = time.perf_counter() - t0
        finally:
            R.watershed_ref = inner
        return dict(cpu_ms=wall * 1e3, cpu_python_flood_ms=flood_s[0] * 1e3), int(st.get('n_voxels', 0))
    for rep in reps:
        device_window(rep)                                         # warm-up
        runs, n_dev, n_cpu, n_peaks = [], None, None, 0
        for _ in range(args.runs):                                 # both sides interleaved
            d, n_dev, n_peaks = device_window(rep)
            c, n_cpu = cpu_window(rep)
            runs.append({**d, **c})
        best = {k: round(min(r[k] for r in runs), 3) for k in runs[0]}
        best.update(head_voxels=n_dev, peaks=n_peaks, equal=bool(n_dev == n_cpu),
                    ratio_cpu_without_flood_to_device=round((best['cpu_ms'] - best['cpu_python_flood_ms']) / best['wall_ms'], 2))
        res['windows'].append(best)
        print(json.dumps(best))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
