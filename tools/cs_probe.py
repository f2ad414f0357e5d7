"""Per-stage device times (the sd_* launches only, buffers allocated beforehand) of the contact-site steps on a synthetic chunk: (512 + 2 * 6 + 12, ..) voxels = one default 512^3 chunk
with the worker's halo (overlap 6 + stencil offset (6, 6, 3)), ~2000 jittered-grid Voronoi cells (random uint32 ids), 1 % background
speckle.  Prints one JSON line; ``--out`` also writes it to a file.

    python tools/cs_probe.py [--reps 3] [--out profiles/cs_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from syconn_amd import _lib as L  # noqa: E402
from syconn_amd.extraction.cs_extraction_steps import plan_sites, run_sites  # noqa: E402
from syconn_amd.extraction.find_object_properties import detect_seg_boundaries  # noqa: E402


def voronoi_cells(shape, grid, dev, seed=0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    cell = [s / n for s, n in zip(shape, grid)]
    pts = (torch.stack(torch.meshgrid(*[torch.arange(n) for n in grid], indexing='ij'), -1).float()
           + torch.rand(*grid, 3, generator=g)) * torch.tensor(cell)
    ids = torch.randperm(2 ** 31 - 1, generator=g)[:pts[..., 0].numel()].to(torch.int64) * 2 + 1
    pts, ids = pts.to(dev), ids.view(grid).to(dev)
    seg = torch.empty(shape, dtype=torch.int32, device=dev)
    ys, zs = torch.arange(shape[1], device=dev).float(), torch.arange(shape[2], device=dev).float()
    for x in range(shape[0]):
        gx = min(int(x / cell[0]), grid[0] - 1)
        best = torch.full(shape[1:], float('inf'), device=dev)
        lab = torch.zeros(shape[1:], dtype=torch.int64, device=dev)
        for i in range(max(gx - 1, 0), min(gx + 2, grid[0])):
            p = pts[i].reshape(-1, 3)
            d = (p[:, 0, None, None] - x) ** 2 + (p[:, 1, None, None] - ys[None, :, None]) ** 2 + (p[:, 2, None, None] - zs[None, None, :]) ** 2
            v, a = d.min(0)
            upd = v < best
            best = torch.where(upd, v, best)
            lab = torch.where(upd, ids[i].reshape(-1)[a], lab)
        seg[x] = (lab & 0xffffffff).to(torch.int32)
    seg[torch.rand(shape, device=dev) < 0.01] = 0
    return seg


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return r, min(ts)


def lane_use(edges, st, tile=(8, 8, 16)):
    """Boundary centres per 8 x 8 x 16 output block of k_contact_partners and the share of its 256 lanes that the centre list
    keeps busy (a block with n centres runs ceil(n / 256) rounds of 256 lanes)."""
    h = [s // 2 for s in st]
    o = [n - s + 1 for n, s in zip(edges.shape, st)]
    c = edges[h[0]:h[0] + o[0], h[1]:h[1] + o[1], h[2]:h[2] + o[2]].to(torch.int32)
    pad = [(-n) % t for n, t in zip(o, tile)]
    c = torch.nn.functional.pad(c, (0, pad[2], 0, pad[1], 0, pad[0]))
    n = c.reshape(c.shape[0] // tile[0], tile[0], c.shape[1] // tile[1], tile[1], c.shape[2] // tile[2], tile[2]).sum((1, 3, 5))
    n = n.flatten().double()
    rounds = torch.ceil(n / 256)
    return float(n.mean()), float(n.sum() / (256 * rounds).sum().clamp(min=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    lib = L.load()
    st = (13, 13, 7)
    shape = (512 + 12 + 12, 512 + 12 + 12, 512 + 12 + 6)
    seg = voronoi_cells(shape, (13, 13, 12), dev)
    X, Y, Z = shape
    stream = torch.cuda.current_stream(dev).cuda_stream
    # device times of the sd_* launches only: buffers are allocated before the timed region
    edges = torch.empty(shape, dtype=torch.uint8, device=dev)
    _, t_b = timed(lambda: L.check(lib.sd_seg_boundaries(seg.data_ptr(), X, Y, Z, edges.data_ptr(), stream)), args.reps)
    cs = torch.empty(tuple(n - s + 1 for n, s in zip(shape, st)), dtype=torch.int64, device=dev)
    ws = torch.zeros(lib.sd_contact_partners_workspace_bytes(), dtype=torch.uint8, device=dev)
    _, t_p = timed(lambda: L.check(lib.sd_contact_partners(edges.data_ptr(), seg.data_ptr(), X, Y, Z, *st, cs.data_ptr(),
                                                           ws.data_ptr(), ws.numel(), stream)), args.reps)
    ovf_blocks = int(ws[:4].view(torch.int32).item())
    n_blocks = int(np.prod([-(-n // t) for n, t in zip(cs.shape, (8, 8, 16))]))
    centres, lanes = lane_use(edges, st)
    n_close, n_dil = max(st) // 2, 2
    plan, t_plan = timed(lambda: plan_sites(cs, n_close, dev), 1)       # site boxes: segstats + host batching (host syncs)
    out = torch.empty_like(cs)
    wsc = torch.empty(max(plan.ws_bytes, 1), dtype=torch.uint8, device=dev)
    _, t_c = timed(lambda: run_sites(cs, plan, n_close, n_dil, out, wsc), args.reps)
    res = dict(shape=list(shape), stencil=list(st), cells=13 * 13 * 12, boundary_fraction=float(edges.float().mean()),
               contact_voxels=int((cs != 0).sum()), sites=len(plan.ids), site_box_voxels=plan.box_voxels,
               site_box_voxels_per_chunk_voxel=round(plan.box_voxels / cs.numel(), 2), close_batches=len(plan.batches),
               partner_blocks=n_blocks, partner_blocks_with_overflow=ovf_blocks, boundary_centres_per_block=round(centres, 1),
               partner_lane_use=round(lanes, 3),
               ms_boundaries=round(t_b, 3), ms_partners=round(t_p, 3), ms_site_plan_host=round(t_plan, 3),
               ms_close_dilate_kernels=round(t_c, 3), device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
