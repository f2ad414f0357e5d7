"""Per-stage device times (the sd_* launches only, buffers allocated beforehand) of the contact-site steps on a synthetic chunk: (512 + 2 * 6 + 12, ..) voxels = one default 512^3 chunk
with the worker's halo (overlap 6 + stencil offset (6, 6, 3)), ~2000 jittered-grid Voronoi cells (random uint32 ids), 1 % background
speckle.  Prints one JSON line; ``--out`` also writes it to a file.

    python tools/cs_probe.py [--reps 3] [--out profiles/cs_probe.json]
    python tools/cs_probe.py --driver [--reps 3] [--out profiles/cs_driver_probe.json]

``--driver``: wall time of contact-site extraction over a dataset of 2 x 2 x 2 chunks (256 x 256 x 128 each, KnossosDatasets in a
temporary directory on tmpfs when there is one), minimum of ``--reps`` runs: (a) the per-chunk worker over all chunks plus the host
merge of its files (tests/_cs_driver_ref.py), (b) ``extract_contact_sites``; for (b) also per stage.
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
    ap.add_argument('--part2-out', default=None, help='also time the part-2 stages (sj mask, type masks, statistics, voxel lists, '
                                                      'host copies, one worker chunk) and write them here')
    ap.add_argument('--driver', action='store_true', help='time the dataset driver against the per-chunk worker + host merge')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    lib = L.load()
    if args.driver:
        return driver_probe(dev, args)
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
    if args.part2_out:
        del edges, ws, wsc
        part2(out, n_close, dev, args)


def part2(contacts, overlap, dev, args):
    """The stages after the closing on the closed contact volume (a 512^3 core inside `overlap`) and a synthetic sj map with ~1 %
    foreground.  Kernel-only rows time the sd_* launches; rows marked _host include host syncs and allocations."""
    from syconn_amd.extraction.cs_extraction_steps import binary_morphology, syntype_masks
    from syconn_amd.extraction.find_object_properties import CsSyntypeScan, cs_syntype_dicts
    from syconn_amd.extraction.object_extraction_steps import get_aniso_struct
    lib = L.load()
    shape = tuple(int(s) for s in contacts.shape)
    g = torch.Generator(device=dev).manual_seed(1)
    pool = torch.nn.functional.avg_pool3d(torch.rand((1, 1) + shape, generator=g, device=dev), 5, 1, 2)[0, 0]
    sj_raw = torch.where(pool > 0.56, 200, 10).to(torch.uint8)
    del pool
    ops = ['binary_opening', 'binary_closing', 'binary_erosion']
    struct = get_aniso_struct(np.array([10, 10, 20]))
    sj, t_sj = timed(lambda: binary_morphology(sj_raw, ops, struct, threshold=255 * 0.19047619, return_device=True, device=dev),
                     args.reps)
    labels = torch.randint(0, 4, shape, generator=g, device=dev, dtype=torch.int64)
    (asym, sym), t_types = timed(lambda: syntype_masks(labels, 3, 1, device=dev), args.reps)
    del labels
    core = tuple(s - 2 * overlap for s in shape)
    sc = CsSyntypeScan(dev)
    res, t_all = timed(lambda: sc.run(contacts, sj, asym, sym, offset=(0, 0, 0), origin=(overlap,) * 3, extent=core, want_cores=True),
                       args.reps)
    stream = torch.cuda.current_stream(dev).cuda_stream
    cs_core, syn_core = res.cs_core, res.syn_core
    _, t_scan = timed(lambda: L.check(lib.sd_cs_syntype_scan(contacts.data_ptr(), L.SD_U64, sj.data_ptr(), asym.data_ptr(), sym.data_ptr(),
                                                             *shape, *(overlap,) * 3, *core, sc.table.data_ptr(), sc.cap,
                                                             cs_core.data_ptr(), syn_core.data_ptr(), sc.status.data_ptr(), stream)),
                      args.reps)
    _, t_scan_nocore = timed(lambda: L.check(lib.sd_cs_syntype_scan(contacts.data_ptr(), L.SD_U64, sj.data_ptr(), asym.data_ptr(),
                                                                    sym.data_ptr(), *shape, *(overlap,) * 3, *core, sc.table.data_ptr(),
                                                                    sc.cap, None, None, sc.status.data_ptr(), stream)), args.reps)
    import ctypes as C
    n, ns = int(res.rec.shape[0]), int(res.voxels.shape[0])
    vox = torch.empty((max(ns, 1), 3), dtype=torch.int64, device=dev)
    offs = (C.c_int64 * 3)(0, 0, 0)
    _, t_vox = timed(lambda: L.check(lib.sd_cs_syntype_voxels(contacts.data_ptr(), L.SD_U64, sj.data_ptr(), *shape, *(overlap,) * 3,
                                                              res.rec.data_ptr(), n, ns, offs, vox.data_ptr(), sc.status.data_ptr(),
                                                              stream)), args.reps)

    def to_host():
        a = cs_core.permute(2, 1, 0).contiguous().cpu()
        b = syn_core.permute(2, 1, 0).contiguous().cpu()
        return a, b, res.host()
    _, t_copy = timed(to_host, args.reps)
    t0 = __import__('time').perf_counter()
    cs_syntype_dicts(*res.host())
    t_dicts = (__import__('time').perf_counter() - t0) * 1e3
    # one worker chunk with KnossosDataset I/O (a smaller chunk: 256 x 256 x 128, written to a temporary dataset first)
    t_worker = worker_chunk(dev)
    out = dict(core=list(core), sites=n, syn_sites=int((res.rec[:, 14] > 0).sum()), syn_voxels=ns,
               sj_foreground=float(sj.float().mean()), scan_table_slots=sc.cap,
               ms_sj_threshold_morphology_host=round(t_sj, 3), ms_type_masks_host=round(t_types, 3),
               ms_stats_pass_kernel=round(t_scan, 3), ms_stats_pass_kernel_without_cores=round(t_scan_nocore, 3),
               ms_voxel_lists_kernel=round(t_vox, 3), ms_stats_voxels_records_host=round(t_all, 3),
               ms_copies_to_host=round(t_copy, 3), ms_dicts_host=round(t_dicts, 3), worker_chunk=[256, 256, 128],
               ms_worker_chunk_with_kd_io=round(t_worker, 1), device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.part2_out) or '.', exist_ok=True)
    with open(args.part2_out, 'w') as f:
        f.write(line + '\n')


def worker_chunk(dev):
    import tempfile
    import time
    import yaml
    from syconn_amd import global_params
    from syconn_amd.extraction.cs_extraction_steps import _contact_site_extraction_thread
    from syconn_amd.knossos import Chunk, KnossosDataset
    chunk, halo = (256, 256, 128), (12, 12, 9)
    box = tuple(c + 2 * h for c, h in zip(chunk, halo))
    with tempfile.TemporaryDirectory() as tmp:
        def kd(path, seg=None, raw=None):
            k = KnossosDataset().initialize_without_conf(path, box, (10, 10, 20), 'probe', mags=[1])
            if seg is not None:
                k.save_seg(offset=(0, 0, 0), mags=[1], data=np.ascontiguousarray(seg.swapaxes(0, 2)), data_mag=1)
            if raw is not None:
                k.save_raw(offset=(0, 0, 0), mags=[1], data=np.ascontiguousarray(raw.swapaxes(0, 2)), data_mag=1)
        cells = voronoi_cells(box, (4, 4, 2), dev, seed=2).cpu().numpy().view(np.uint32).astype(np.uint64)
        sj = (torch.nn.functional.avg_pool3d(torch.rand((1, 1) + box, device=dev), 5, 1, 2)[0, 0] > 0.56).to(torch.uint8) * 200
        kd(f'{tmp}/cells', seg=cells)
        kd(f'{tmp}/sj', raw=sj.cpu().numpy())
        kd(f'{tmp}/wd/knossosdatasets/cs_seg/')
        kd(f'{tmp}/wd/knossosdatasets/syn_seg/')
        with open(f'{tmp}/wd/config.yml', 'w') as f:
            yaml.safe_dump({'scaling': [10, 10, 20], 'paths': {'kd_sj': f'{tmp}/sj'}}, f)
        saved = global_params.wd
        global_params.wd = f'{tmp}/wd'
        try:
            ch = [Chunk(0, halo, chunk, (0, 0, 0))]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _contact_site_extraction_thread((ch, f'{tmp}/cells', 0, f'{tmp}/props', None))
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        finally:
            global_params.wd = saved


def driver_probe(dev, args):
    """(a) ``_contact_site_extraction_thread`` over all chunks (one job, the parent path) + the host merge of its files against
    (b) ``extract_contact_sites`` on the same dataset, and the stages of (b) from a timed copy of its chunk loop."""
    import shutil
    import tempfile
    import time
    import yaml
    from syconn_amd import global_params
    from syconn_amd.extraction import cs_extraction_steps as S
    from syconn_amd.knossos import ChunkDataset, KnossosDataset
    from syconn_amd.handler import basics
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import _cs_driver_ref as D
    chunk, cube, grid = (256, 256, 128), (128, 128, 128), (2, 2, 2)
    box = tuple(c * g for c, g in zip(chunk, grid))
    min_vx = global_params.config['cell_objects']['min_obj_vx']
    tmp = tempfile.mkdtemp(dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
    saved = global_params.wd
    try:
        def kd(path, seg=None, raw=None):
            k = KnossosDataset()
            k._cube_shape = cube
            k.initialize_without_conf(path, box, (10, 10, 20), 'probe', mags=[1])
            if seg is not None:
                k.save_seg(offset=(0, 0, 0), mags=[1], data=np.ascontiguousarray(seg.swapaxes(0, 2)), data_mag=1)
            if raw is not None:
                k.save_raw(offset=(0, 0, 0), mags=[1], data=np.ascontiguousarray(raw.swapaxes(0, 2)), data_mag=1)
        cells = voronoi_cells(box, (8, 8, 4), dev, seed=2).cpu().numpy().view(np.uint32).astype(np.uint64)
        g = torch.Generator(device=dev).manual_seed(1)
        sj = torch.where(torch.nn.functional.avg_pool3d(torch.rand((1, 1) + box, generator=g, device=dev), 5, 1, 2)[0, 0] > 0.52, 200, 10)
        types = torch.randint(0, 4, box, generator=g, device=dev, dtype=torch.int64).cpu().numpy().view(np.uint64)
        kd(f'{tmp}/cells', seg=cells)
        kd(f'{tmp}/sj', raw=sj.to(torch.uint8).cpu().numpy())
        kd(f'{tmp}/types', seg=types)
        del cells, sj, types
        wd = f'{tmp}/wd'
        os.makedirs(wd)
        with open(f'{wd}/config.yml', 'w') as f:
            yaml.safe_dump({'scaling': [10, 10, 20], 'syntype_avail': True,
                            'paths': {'kd_seg': f'{tmp}/cells', 'kd_sj': f'{tmp}/sj', 'kd_sym': f'{tmp}/types', 'kd_asym': f'{tmp}/types'},
                            'cell_objects': {'sym_label': 1, 'asym_label': 3}}, f)
        global_params.wd = wd
        cset = ChunkDataset().initialize(basics.kd_factory(f'{tmp}/cells'), box, chunk, '', box_coords=[0, 0, 0], fit_box_size=True)
        chunks = [cset.chunk_dict[k] for k in sorted(cset.chunk_dict)]

        def parent_path():
            for t in ('cs', 'syn'):
                shutil.rmtree(f'{wd}/knossosdatasets/{t}_seg/', ignore_errors=True)
                kd(f'{wd}/knossosdatasets/{t}_seg/')
            shutil.rmtree(f'{tmp}/props', ignore_errors=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            S._contact_site_extraction_thread((chunks, f'{tmp}/cells', 0, f'{tmp}/props', None))
            t1 = time.perf_counter()
            cs, syn = D.merge_workers([D.load_worker_files(f'{tmp}/props', 0)], min_vx['cs'], min_vx['syn'])
            return (t1 - t0), (time.perf_counter() - t1), cs, syn

        def driver():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cs_t, syn_t = S.extract_contact_sites(chunk_size=chunk, cube_shape=cube, max_n_jobs=1, overwrite=True, as_tables=True)
            return time.perf_counter() - t0, cs_t, syn_t

        def driver_stages():
            """The chunk loop of ``extract_contact_sites`` with a clock on every stage (same classes, same order)."""
            kds = []
            for t in ('cs', 'syn'):
                shutil.rmtree(f'{wd}/knossosdatasets/{t}_seg/', ignore_errors=True)
                k = KnossosDataset()
                k._cube_shape = cube
                k.initialize_without_conf(f'{wd}/knossosdatasets/{t}_seg/', box, (10, 10, 20), 'probe', mags=[1], create_pyk_conf=True,
                                          create_knossos_conf=False)
                kds.append(k)
            body = S._ChunkExtractor(f'{tmp}/cells', None, dev)
            t_load = [0.0]
            for k in (body.kd, body.kd_sj, body.kd_sym, body.kd_asym):
                for name in ('load_seg', 'load_raw'):
                    def wrap(fn):
                        def timed_load(*a, **kw):
                            t = time.perf_counter()
                            r = fn(*a, **kw)
                            t_load[0] += time.perf_counter() - t
                            return r
                        return timed_load
                    setattr(k, name, wrap(getattr(k, name)))
            merger = S.ContactSiteMerger(min_vx, dev)
            writer = S._CoreWriter(dev, *kds)
            ev = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t_body = t_submit = 0.0
            for ch in chunks:
                t = time.perf_counter()
                res, off = body.run(ch)
                t_body += time.perf_counter() - t
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                merger.add_chunk(res, off)
                b.record()
                ev.append((a, b))
                t = time.perf_counter()
                writer.submit(res, off)
                t_submit += time.perf_counter() - t
                del res
            t_loop = time.perf_counter() - t0
            writer.close()
            t_drain = time.perf_counter() - t0 - t_loop
            torch.cuda.synchronize()
            t = time.perf_counter()
            n = [int(v) for v in merger.cursors.cpu().numpy()]
            cs_t, syn_t = merger.finish()
            t_finish = time.perf_counter() - t
            wall = time.perf_counter() - t0
            return dict(ms_wall=wall * 1e3, ms_chunk_loop=t_loop * 1e3, ms_chunk_body_host_view=t_body * 1e3, ms_kd_loads_in_body=t_load[0] * 1e3,
                        ms_append_kernels_per_chunk=[round(a.elapsed_time(b), 3) for a, b in ev], ms_submit_cores_host=t_submit * 1e3,
                        ms_writer_save_seg_overlapped=writer.busy_s * 1e3, ms_writer_drain_after_loop=t_drain * 1e3,
                        ms_merge_and_table_download=t_finish * 1e3, records=n, kd_load_share_of_wall=t_load[0] / wall)

        def merge_only():
            """Device time of the two merges and host time of the downloads, on the records of one more pass."""
            body = S._ChunkExtractor(f'{tmp}/cells', None, dev)
            merger = S.ContactSiteMerger(min_vx, dev)
            for ch in chunks:
                res, off = body.run(ch)
                merger.add_chunk(res, off)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            merger.finish()
            b.record()
            torch.cuda.synchronize()
            return dict(ms_finish_host=(time.perf_counter() - t0) * 1e3, ms_finish_device_span=a.elapsed_time(b))

        S.extract_contact_sites(chunk_size=chunk, cube_shape=cube, max_n_jobs=1, overwrite=True, as_tables=True)      # warm-up: allocator, tables
        a_runs, b_runs = [], []
        for _ in range(args.reps):
            w, m, cs_a, syn_a = parent_path()
            a_runs.append((w + m, w, m))
            t, cs_t, syn_t = driver()
            b_runs.append(t)
        D.assert_same(cs_t.as_dict(), cs_a, 'cs')                 # both paths computed the same thing
        D.assert_same(syn_t.as_dict(), syn_a, 'syn')
        stages = min((driver_stages() for _ in range(args.reps)), key=lambda d: d['ms_wall'])
        stages.update(merge_only())
        a_tot = [r[0] for r in a_runs]
        best_a = min(a_runs)
        res = dict(box=list(box), chunk=list(chunk), chunks=len(chunks), tmpdir_on_tmpfs=tmp.startswith('/dev/shm'), cs_objects=len(cs_t),
                   syn_objects=len(syn_t), syn_voxels=int(len(syn_t.voxels)),
                   a_worker_plus_host_merge_ms=[round(v * 1e3, 1) for v in a_tot], a_min_ms=round(best_a[0] * 1e3, 1),
                   a_min_worker_ms=round(best_a[1] * 1e3, 1), a_min_host_merge_ms=round(best_a[2] * 1e3, 1),
                   a_spread_ms=round((max(a_tot) - min(a_tot)) * 1e3, 1),
                   b_extract_contact_sites_ms=[round(v * 1e3, 1) for v in b_runs], b_min_ms=round(min(b_runs) * 1e3, 1),
                   b_over_a=round(min(b_runs) / best_a[0], 3),
                   b_stages={k: ([round(x, 3) for x in v] if isinstance(v, list) and v and isinstance(v[0], float) else
                                 (round(v, 3) if isinstance(v, float) else v)) for k, v in stages.items()},
                   device=torch.cuda.get_device_name(0))
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
            with open(args.out, 'w') as f:
                f.write(line + '\n')
    finally:
        global_params.wd = saved
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
