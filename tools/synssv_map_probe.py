"""Stage times of the organelle mapping (``extraction.cs_processing_steps.map_objects_from_synssv_partners``) on a synthetic input:
`--cells` cells, `--synapses` synapses between random pairs of them (flattened blobs of 10^2 .. 10^4 voxels), per synapse and partner
one to three mitochondria (tubes of 10^3 .. 10^5 mesh vertices) and one to four vesicle clouds (spheres of 100 .. 400 vertices).

    python tools/synssv_map_probe.py [--cells 100] [--synapses 300] [--seed 0] [--ref-synapses 25] [--out profiles/synssv_map_probe.json]

Reports, as the minimum of three runs: the device stages from HIP events (candidate pairs per type, both calls and the count read
in between; the sampled-voxel preparation; the query per type, with the download of its result), the host preparation (sort by cell,
upload) and the host edge; the device's counters; and the time of the reference's form -- one cKDTree per synapse side, queried per
candidate organelle -- on the first `--ref-synapses` synapses in the same process (scipy if it can be imported, else the numpy
restatement tests/_synssv_map_ref.py), with a check that both agree.  No pass / fail rides on the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SCALE, R, D, F = (10, 10, 20), {'mi': 1000, 'vc': 500}, 4000, 2
S64 = np.array(SCALE, np.float64)


def blob(rng, centre, n_target):
    """An ellipsoid flattened in z (a synaptic cleft) with about n_target voxels and 15 % holes."""
    r = (n_target / (4.19 * 0.25)) ** (1 / 3)
    rad = np.maximum(np.array([r, r * rng.uniform(0.6, 1.0), max(r * 0.25, 1.0)]), 1.0)
    ext = np.ceil(rad).astype(int)
    g = np.stack(np.meshgrid(*[np.arange(-e, e + 1) for e in ext], indexing='ij'), -1).reshape(-1, 3)
    g = g[((g / rad) ** 2).sum(1) <= 1.0]
    g = g[rng.random(len(g)) > 0.15]
    return (g + centre).astype(np.uint32)


def tube(rng, start_nm, n_vert):
    """A bent tube of radius ~150 nm: rings of 16 vertices along a random walk."""
    n_ring = max(n_vert // 16, 2)
    step = rng.normal(0, 1, 3)
    step /= np.linalg.norm(step)
    axis = start_nm + np.cumsum(step * 25.0 + rng.normal(0, 4.0, (n_ring, 3)), 0)
    ang = np.arange(16) * (2 * np.pi / 16)
    u = np.cross(step, (0.0, 0.0, 1.0)) + 1e-3
    u /= np.linalg.norm(u)
    w = np.cross(step, u)
    ring = 150.0 * (np.cos(ang)[:, None] * u + np.sin(ang)[:, None] * w)
    return (axis[:, None, :] + ring[None]).reshape(-1, 3).astype(np.float32)


def sphere(rng, centre_nm, n_vert):
    p = rng.normal(0, 1, (n_vert, 3))
    return (centre_nm + 60.0 * p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)


def make_input(n_cells, n_syn, seed):
    import _synssv_map_ref as M
    rng = np.random.default_rng(seed)
    partners, rep, vox = [], [], []
    org = {t: dict(cells=[], sizes=[], rep=[], verts=[]) for t in ('mi', 'vc')}
    for _ in range(n_syn):
        a, b = rng.choice(np.arange(1, n_cells + 1), 2, replace=False)
        centre = rng.integers(2000, 60000, 3)
        v = blob(rng, centre, int(10 ** rng.uniform(2, 4)))
        if not len(v):
            v = centre[None].astype(np.uint32)
        partners.append((max(a, b), min(a, b)))
        vox.append(v)
        rep.append(v[len(v) // 2])
        c_nm = v.astype(np.float64).mean(0) * S64
        for cell in (a, b):
            for _ in range(int(rng.integers(1, 4))):
                p = tube(rng, c_nm + rng.normal(0, 700, 3), int(10 ** rng.uniform(3, 5)))
                org['mi']['cells'].append(cell); org['mi']['sizes'].append(int(rng.integers(10 ** 4, 10 ** 6)))
                org['mi']['rep'].append(np.round(p[len(p) // 2] / S64)); org['mi']['verts'].append(p)
            for _ in range(int(rng.integers(1, 5))):
                p = sphere(rng, c_nm + rng.normal(0, 400, 3), int(rng.integers(100, 400)))
                org['vc']['cells'].append(cell); org['vc']['sizes'].append(int(rng.integers(10 ** 2, 10 ** 4)))
                org['vc']['rep'].append(np.round(p.mean(0) / S64)); org['vc']['verts'].append(p)
    tables = {t: M.table_from_lists(np.arange(len(o['cells'])) + 1, o['cells'], o['sizes'], np.maximum(np.array(o['rep']), 0), o['verts'])
              for t, o in org.items()}
    return dict(partners=np.array(partners, np.uint64), rep=np.array(rep, np.int32), vox=np.concatenate(vox),
                vox_begin=np.concatenate(([0], np.cumsum([len(v) for v in vox]))), tables=tables)


class Syn:
    def __init__(self, c, n=None):
        n = len(c['partners']) if n is None else n
        self.neuron_partners, self.rep_coords = c['partners'][:n], c['rep'][:n]
        self.vox_begin = c['vox_begin'][:n + 1]
        self.voxels, self.sizes = c['vox'][:self.vox_begin[-1]], np.diff(self.vox_begin)

    def __len__(self):
        return len(self.sizes)


def reference_form(c, n, tables):
    """One tree per synapse side's synapse, queried per candidate organelle: ``_map_objects_from_synssv``'s loop.  -> per type the
    (close, len, min d) of every pair in (side, organelle row) order, and which tree was used."""
    import _synssv_map_ref as M
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    out = {}
    for t, tab in tables.items():
        side_begin, pair_obj = M.candidates(c['partners'][:n], c['rep'][:n], tab, SCALE, D)
        rows = []
        for side in range(2 * n):
            objs = pair_obj[side_begin[side]:side_begin[side + 1]]
            if not len(objs):
                continue
            P = M.sampled_points(c['vox'], c['vox_begin'], side // 2, SCALE, F)
            tree = cKDTree(P) if cKDTree else None
            for o in objs.tolist():
                V = M.sampled_vertices(tab, o, F)
                if tree is not None:
                    ds, _ = tree.query(V, distance_upper_bound=R[t])
                else:
                    d2 = M.sq_dist(V, P).min(1)
                    ds = np.where(d2 < R[t] ** 2, np.sqrt(d2), np.inf)
                rows.append((int(np.sum(ds < np.inf)), len(ds), float(np.min(ds))))
        out[t] = rows
    return out, 'scipy cKDTree' if cKDTree else 'numpy brute force'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=100)
    ap.add_argument('--synapses', type=int, default=300)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--ref-synapses', type=int, default=25)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'synssv_map_probe.json'))
    args = ap.parse_args()
    import torch
    from syconn_amd.extraction import cs_processing_steps as P
    dev = torch.device('cuda', 0)
    c = make_input(args.cells, args.synapses, args.seed)
    tables = {t: P.OrganelleTable(tab['ids'], tab['cells'], tab['sizes'], tab['rep'], tab['verts'], tab['vert_begin']) for t, tab in c['tables'].items()}
    syn = Syn(c)
    res = dict(cells=args.cells, synapses=len(syn), voxels=int(c['vox_begin'][-1]), scaling=SCALE, max_vert_dist_nm=R, max_rep_coord_dist_nm=D,
               sample_fact=F, organelles={t: len(tab) for t, tab in tables.items()}, vertices={t: len(tab.vertices) for t, tab in tables.items()},
               device=torch.cuda.get_device_name(0))
    runs = []
    for rep in range(4):                                                 # the first run warms up (allocator, code objects)
        r = {}
        t0 = time.perf_counter()
        mapper = P._ObjectMapper(syn, S64, F, dev)
        torch.cuda.synchronize(dev)
        r['host_upload_synapses_ms'] = (time.perf_counter() - t0) * 1e3
        cands, ev = {}, {}
        for t in tables:
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            t0 = time.perf_counter()
            e[0].record()
            cands[t] = mapper.candidates(tables[t], D)               # sort by cell and upload on the host, both calls, the downloads
            e[1].record()
            torch.cuda.synchronize(dev)
            r[f'pairs_{t}_wall_ms'] = (time.perf_counter() - t0) * 1e3
            r[f'pairs_{t}_ms'] = e[0].elapsed_time(e[1])
        mapper.reserve(max(cd['P'] for cd in cands.values()))
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        mapper.prepare()
        e[1].record()
        torch.cuda.synchronize(dev)
        r['voxels_ms'] = e[0].elapsed_time(e[1])
        pairs, counters = {}, {}
        for t in tables:
            t0 = time.perf_counter()
            cands[t]['vert_d'], cands[t]['vtb_d'] = torch.from_numpy(tables[t].vertices).to(dev), torch.from_numpy(tables[t].vert_begin).to(dev)
            torch.cuda.synchronize(dev)
            r[f'upload_{t}_vertices_ms'] = (time.perf_counter() - t0) * 1e3
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            pairs[t], counters[t] = mapper.query(cands[t], R[t])         # with the download of the pair values
            e[1].record()
            torch.cuda.synchronize(dev)
            r[f'query_{t}_ms'] = e[0].elapsed_time(e[1])
        t0 = time.perf_counter()
        mapping = P.build_synssv_mapping(len(syn), tables, pairs)
        r['host_edge_ms'] = (time.perf_counter() - t0) * 1e3
        r['device_ms'] = r['voxels_ms'] + sum(r[f'pairs_{t}_ms'] + r[f'query_{t}_ms'] for t in tables)
        runs.append(r)
    timed = runs[1:]
    res['runs'] = timed
    res['min_ms'] = {k: round(min(r[k] for r in timed), 3) for k in timed[0]}
    res['counters'] = counters
    res['pairs'] = {t: int(len(pairs[t].pair_obj)) for t in tables}
    res['brute_force_point_tests'] = {t: int((pairs[t].pair_len * (-(-np.diff(c['vox_begin']) // F))[np.repeat(np.arange(2 * len(syn)),
                                      np.diff(pairs[t].side_begin)) // 2]).sum()) for t in tables}
    # the reference's form on a stated subset, in this process, and the device path on the same subset
    n = min(args.ref_synapses, len(syn))
    t0 = time.perf_counter()
    ref, tree = reference_form(c, n, c['tables'])
    res.update(cpu_form=tree, cpu_form_synapses=n, cpu_form_pairs={t: len(v) for t, v in ref.items()},
               cpu_form_ms=round((time.perf_counter() - t0) * 1e3, 1))
    sub = Syn(c, n)
    t0 = time.perf_counter()
    got = P.map_objects_from_synssv_partners(sub, tables, SCALE, max_vert_dist_nm=R, max_rep_coord_dist_nm=D, sample_fact=F, device=dev)
    res['device_path_same_subset_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    for t in tables:
        pl = got.pairs[t]
        assert [(int(a), int(b)) for a, b in zip(pl.pair_close, pl.pair_len)] == [(a, b) for a, b, _ in ref[t]], t
        assert np.sqrt(pl.pair_min_d2).tolist() == [d for _, _, d in ref[t]], t
    res['subset_agrees'] = True
    res['cpu_form_over_device_path'] = round(res['cpu_form_ms'] / max(res['device_path_same_subset_ms'], 1e-3), 2)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(res) + '\n')
    print(json.dumps({k: v for k, v in res.items() if k != 'runs'}))
    del mapping


if __name__ == '__main__':
    main()
