"""Stage times of the synapse agglomeration (``extraction.cs_processing_steps.combine_and_split_syn``) on a synthetic input: a few
thousand cell pairs, 1 to 8 fragments per pair, blobs of 10^2 .. 10^4 voxels.

    python tools/syn_ssv_probe.py [--pairs 3000] [--seed 0] [--ref-pairs 40] [--out profiles/syn_ssv_probe.json]

Reports, as the minimum of three runs: the device stages from HIP events (cells, link, number, statistics), the host preparation
(filter, gather of the voxel runs, upload) and the host edge; the share of neighbouring cell pairs that needed a voxel test; and the
time of the CPU restatement (tests/_syn_ssv_ref.py: cKDTree + csgraph, what the tests compare with) on the first `--ref-pairs` pairs
whose groups have at most 3000 voxels, in the same process.  No pass / fail rides on the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SCALE, GAP, MIN_VX = (10, 10, 20), 250, 100


def blob(rng, centre, n_target):
    """An ellipsoid flattened in z (a synaptic cleft) with about n_target voxels and 15 % holes."""
    r = (n_target / (4.19 * 0.25)) ** (1 / 3)
    rad = np.maximum(np.array([r, r * rng.uniform(0.6, 1.0), max(r * 0.25, 1.0)]), 1.0)
    ext = np.ceil(rad).astype(int)
    g = np.stack(np.meshgrid(*[np.arange(-e, e + 1) for e in ext], indexing='ij'), -1).reshape(-1, 3)
    g = g[((g / rad) ** 2).sum(1) <= 1.0]
    g = g[rng.random(len(g)) > 0.15]
    return (g + centre).astype(np.uint32)


def make_input(n_pairs, seed):
    rng = np.random.default_rng(seed)
    ids, lists, mapping = [], [], {}
    for p in range(n_pairs):
        cell_a, cell_b = 2 * p + 2, 2 * p + 3
        base = rng.integers(200, 20000, 3)
        n_frag = int(rng.integers(1, 9))
        for f in range(n_frag):
            sv_a, sv_b = 16 * p + 2 * f + 16, 16 * p + 2 * f + 17
            mapping[sv_a], mapping[sv_b] = cell_a, cell_b
            # fragments of a pair lie within ~1.5 um of each other: some merge, some stay apart
            centre = base + rng.integers(-70, 71, 3) * (1, 1, 0) + (0, 0, int(rng.integers(-20, 21)))
            size = int(10 ** rng.uniform(2, 4 if f == 0 else 3.3))
            vox = blob(rng, centre, size)
            if len(vox):
                ids.append((sv_a << 32) + sv_b)
                lists.append(vox)
    return ids, lists, mapping


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=3000)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--ref-pairs', type=int, default=40)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'syn_ssv_probe.json'))
    args = ap.parse_args()
    import torch
    import _syn_ssv_ref as S
    from syconn_amd.extraction import cs_processing_steps as P
    dev = torch.device('cuda', 0)
    ids, lists, mapping = make_input(args.pairs, args.seed)
    table = S.Table(ids, lists, np.full(len(ids), 0.25), np.full(len(ids), 0.5))
    res = dict(pairs=args.pairs, fragments=len(ids), voxels=int(table.vox_begin[-1]), scaling=SCALE, cs_gap_nm=GAP, min_obj_vx=MIN_VX,
               device=torch.cuda.get_device_name(0))
    runs = []
    for rep in range(4):                                                 # the first run warms up (allocator, code objects)
        t0 = time.perf_counter()
        keys, begin, rows = P.filter_relevant_syn(table.ids, mapping)
        vb = table.vox_begin
        run_start, run_len = vb[:-1][rows], np.diff(vb)[rows]
        b = np.concatenate(([0], np.cumsum(run_len)))
        src = np.repeat(run_start - b[:-1], run_len) + np.arange(b[-1])
        vox = table.voxels[src]
        vox_frag = np.repeat(np.arange(len(rows), dtype=np.uint32), run_len)
        frag_group = np.repeat(np.arange(len(keys), dtype=np.uint32), np.diff(begin))
        t1 = time.perf_counter()
        agg = P._Agglomerator(vox.astype(np.int32), vox_frag, frag_group, len(keys), SCALE, GAP, dev)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        for k, stage in enumerate((1, 2, 4)):
            agg.components(stage)
            ev[k + 1].record()
        counts = agg.read_counts()
        t3 = time.perf_counter()
        ev_s = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev_s[0].record()
        st = agg.stats(MIN_VX)                                           # includes the download of the result
        ev_s[1].record()
        torch.cuda.synchronize(dev)
        t4 = time.perf_counter()
        comp_group = frag_group[vox_frag[st['comp_rep_flat']]].astype(np.int64)
        t = P.build_syn_ssv_table(keys, begin, table.ids[rows], table.sym_prop[rows], table.asym_prop[rows], comp_group, st['comp_sizes'],
                                  st['comp_bbox'], vox[st['comp_rep_flat']], st['pair_comp'], st['pair_frag'], st['pair_cnt'], st['voxels'],
                                  SCALE, MIN_VX, 0.225)
        t5 = time.perf_counter()
        runs.append(dict(host_filter_gather_ms=(t1 - t0) * 1e3, upload_ms=(t2 - t1) * 1e3, cells_ms=ev[0].elapsed_time(ev[1]),
                         link_ms=ev[1].elapsed_time(ev[2]), number_ms=ev[2].elapsed_time(ev[3]),
                         stats_with_download_ms=ev_s[0].elapsed_time(ev_s[1]), stats_wall_ms=(t4 - t3) * 1e3,
                         host_edge_ms=(t5 - t4) * 1e3, total_ms=(t5 - t0) * 1e3))
    timed = runs[1:]
    res['runs'] = timed
    res['min_ms'] = {k: round(min(r[k] for r in timed), 3) for k in timed[0]}
    c = [int(v) for v in counts]
    res.update(cell=agg.cell.tolist(), components=c[0], rows=len(t), cells=c[1], neighbour_cells_found=c[2], too_far_by_boxes=c[3],
               joined_by_boxes=c[4], already_joined=c[5], voxel_tested=c[6], voxel_tested_share=round(c[6] / max(c[2], 1), 4))
    # the CPU restatement on a stated subset, in this process
    groups = S.groups_from_arrays(table.ids, table.voxels, table.vox_begin, table.sym_prop, table.asym_prop, keys, begin, rows)
    subset = [g for g in groups if sum(len(f[1]) for f in g[1]) <= 3000][:args.ref_pairs]
    t0 = time.perf_counter()
    want, _ = S.combine(subset, SCALE, GAP, MIN_VX, 0.225)
    res.update(cpu_restatement_pairs=len(subset), cpu_restatement_voxels=int(sum(len(f[1]) for g in subset for f in g[1])),
               cpu_restatement_ms=round((time.perf_counter() - t0) * 1e3, 1), cpu_restatement_rows=len(want))
    # the same subset through the device path, for a like-for-like figure (and a check that both agree)
    frags = [f for g in subset for f in g[1]]
    sub_t = S.Table([f[0] for f in frags], [f[1] for f in frags], [f[2] for f in frags], [f[3] for f in frags])
    t0 = time.perf_counter()
    got = P.combine_and_split_syn(sub_t, mapping, scaling=SCALE, cs_gap_nm=GAP, min_obj_vx=MIN_VX, sym_thresh=0.225, device=dev)
    res['device_path_same_subset_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    S.assert_rows_equal(got.as_dict(), want, 'probe subset')
    res['subset_agrees'] = True
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(res) + '\n')
    print(json.dumps({k: v for k, v in res.items() if k != 'runs'}))


if __name__ == '__main__':
    main()
