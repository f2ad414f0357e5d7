"""Brute-force numpy restatement of the organelle mapping (``map_objects_from_synssv_partners``), in own words and without scipy,
pinned to golden g20 by tests/test_synssv_map_cpu.py; and a Python model of the device form of csrc/sd_synssv_map.hip (sorted
sampled voxels in tiles of 64 with boxes, the margin box tests, the split of a pair into work items of T sampled vertices).

A *side* is (synapse row i, partner slot p) = 2 i + p.  Organelle tables are dicts ``ids, cells, sizes, rep, verts, vert_begin``."""
import numpy as np

T_ITEM = 1024
TILE = 64


def table(ids, cells, sizes, rep, verts, vert_begin):
    return dict(ids=np.asarray(ids, np.uint64), cells=np.asarray(cells, np.uint64), sizes=np.asarray(sizes, np.int64),
                rep=np.asarray(rep, np.int32).reshape(-1, 3), verts=np.asarray(verts, np.float32).reshape(-1, 3),
                vert_begin=np.asarray(vert_begin, np.int64))


def table_from_lists(ids, cells, sizes, rep, vert_lists):
    vl = [np.asarray(v, np.float32).reshape(-1, 3) for v in vert_lists]
    return table(ids, cells, sizes, rep, np.concatenate(vl) if vl else np.zeros((0, 3), np.float32),
                 np.concatenate(([0], np.cumsum([len(v) for v in vl]))))


def sq_dist(A, B):
    """((dx dx) + dy dy) + dz dz for every row of A (k, 3) against every row of B (l, 3): each product and sum rounded on its own."""
    d = A[:, None, :] - B[None, :, :]
    return ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def scale64(scaling):
    return np.asarray(scaling, np.float32).astype(np.float64)


def candidates(partners, syn_rep, tab, scaling, D):
    """-> side_begin (2 n + 1), pair_obj: per side the rows of its cell's organelles whose scaled rep distance is <= D, ascending."""
    s = scale64(scaling)
    partners = np.asarray(partners, np.uint64).reshape(-1, 2)
    begin, objs = [0], []
    for side in range(2 * len(partners)):
        cell = partners[side // 2, side % 2]
        rows = np.flatnonzero(tab['cells'] == cell) if cell != 0 else np.zeros(0, np.int64)
        if len(rows):
            d2 = sq_dist(tab['rep'][rows].astype(np.float64) * s, (np.asarray(syn_rep)[side // 2].astype(np.float64) * s)[None])[:, 0]
            rows = rows[d2 <= float(D) * float(D)]
        objs += rows.tolist()
        begin.append(len(objs))
    return np.array(begin, np.int64), np.array(objs, np.int64)


def sampled_points(vox, vox_begin, i, scaling, f):
    return np.asarray(vox)[vox_begin[i]:vox_begin[i + 1]][::f].astype(np.float64) * scale64(scaling)


def sampled_vertices(tab, o, f):
    return tab['verts'][tab['vert_begin'][o]:tab['vert_begin'][o + 1]][::f].astype(np.float64)


def pair_values(partners, syn_rep, vox, vox_begin, tab, scaling, R, D, f=2):
    """The pair list of one type by brute force.  -> dict side_begin, pair_obj, pair_close, pair_len, pair_min_d2, and ``product`` =
    sampled vertices x sampled voxels summed over the pairs (what a search without pruning tests)."""
    side_begin, pair_obj = candidates(partners, syn_rep, tab, scaling, D)
    close, length, best, product = [], [], [], 0
    r2 = float(R) * float(R)
    for side in range(len(side_begin) - 1):
        P = sampled_points(vox, vox_begin, side // 2, scaling, f)
        for o in pair_obj[side_begin[side]:side_begin[side + 1]].tolist():
            V = sampled_vertices(tab, o, f)
            if not len(V):
                raise ValueError(f'object {int(tab["ids"][o])} (row {o}) is a candidate but has no mesh vertices')
            nearest = sq_dist(V, P).min(1)
            inside = nearest < r2
            close.append(int(inside.sum()))
            length.append(len(V))
            best.append(float(nearest[inside].min()) if inside.any() else np.inf)
            product += len(V) * len(P)
    return dict(side_begin=side_begin, pair_obj=pair_obj, pair_close=np.array(close, np.int64), pair_len=np.array(length, np.int64),
                pair_min_d2=np.array(best, np.float64), product=product)


def columns(n_syn, tab, pv):
    """The three columns of one type from its pair values: per side the estimated voxel counts of its organelles in list order, how
    many are positive, their sum cut to an integer, and the root of the smallest squared distance (1e12 without one)."""
    n_objs, n_vxs, min_dst = np.zeros(2 * n_syn, np.int32), np.zeros(2 * n_syn, np.int32), np.full(2 * n_syn, 1e12, np.float32)
    sb = pv['side_begin']
    for side in range(2 * n_syn):
        sl = slice(sb[side], sb[side + 1])
        if sl.start == sl.stop:
            continue
        est = np.array([(c / l) * sz for c, l, sz in zip(pv['pair_close'][sl], pv['pair_len'][sl], tab['sizes'][pv['pair_obj'][sl]])], np.float64)
        n_objs[side] = int((est > 0).sum())
        total = float(np.sum(est))
        if total >= 2.0 ** 31:
            raise ValueError('n_vxs does not fit int32')
        n_vxs[side] = int(total)
        d = float(np.sqrt(pv['pair_min_d2'][sl].min()))
        min_dst[side] = np.float32(d) if d < 1e12 else np.float32(1e12)
    return n_objs.reshape(n_syn, 2), n_vxs.reshape(n_syn, 2), min_dst.reshape(n_syn, 2)


def map_objects(partners, syn_rep, vox, vox_begin, tables, scaling, R, D=4000, f=2, pair_fn=None):
    """All types.  `R` a dict by type or a number.  -> {type: dict(n_objs, n_vxs, min_dst, **pair values)}."""
    out = {}
    n = len(np.asarray(partners).reshape(-1, 2))
    for t, tab in tables.items():
        pv = (pair_fn or pair_values)(partners, syn_rep, vox, vox_begin, tab, scaling, R[t] if isinstance(R, dict) else R, D, f)
        a, b, c = columns(n, tab, pv)
        out[t] = dict(pv, n_objs=a, n_vxs=b, min_dst=c)
    return out


def features(sizes, mesh_area, res):
    """(n, 14): size, mesh area, then per partner slot the mi and the vc triple."""
    cols = [np.asarray(sizes, np.float64), np.asarray(mesh_area, np.float64)]
    for p in (0, 1):
        for t in ('mi', 'vc'):
            cols += [res[t]['n_objs'][:, p].astype(np.float64), res[t]['n_vxs'][:, p].astype(np.float64), res[t]['min_dst'][:, p].astype(np.float64)]
    return np.stack(cols, 1)


# ---- the device form ---------------------------------------------------------------------------------------------------------------
def box_d2(V, lo, hi):
    d = np.maximum(0.0, np.maximum(lo[None] - V, V - hi[None]))
    return (d * d).sum(1)


def sorted_tiles(vox_s, scaling):
    """The sampled voxels of one synapse (integer rows) -> float64 points sorted by the coarse key (boxes of 4 voxels relative to the
    smallest coordinates, z slowest), and the (lo, hi) box of every tile of 64."""
    v = np.asarray(vox_s, np.int64)
    c = np.minimum((v - v.min(0)) >> 2, 1023)
    key = (c[:, 2] << 20) | (c[:, 1] << 10) | c[:, 0]
    pts = (v.astype(np.float64) * scale64(scaling))[np.argsort(key, kind='stable')]
    return pts, [(pts[a:a + TILE].min(0), pts[a:a + TILE].max(0)) for a in range(0, len(pts), TILE)]


def pair_values_device_model(partners, syn_rep, vox, vox_begin, tab, scaling, R, D, f=2, counters=None):
    """``pair_values`` the way the kernels go about it; `counters` (a dict) receives the device's counters."""
    side_begin, pair_obj = candidates(partners, syn_rep, tab, scaling, D)
    r2 = float(R) * float(R)
    r2_hi = r2 * (1.0 + 1e-9)
    cnt = dict(pairs=len(pair_obj), work_items=0, vertices_rejected=0, tiles_skipped=0, tiles_staged=0, point_tests=0)
    close, length, best_d2, product = [], [], [], 0
    prepared = {}
    for side in range(len(side_begin) - 1):
        i = side // 2
        if side_begin[side] == side_begin[side + 1]:
            continue
        if i not in prepared:
            prepared[i] = sorted_tiles(np.asarray(vox)[vox_begin[i]:vox_begin[i + 1]][::f], scaling)
        pts, tiles = prepared[i]
        lo, hi = pts.min(0), pts.max(0)
        for o in pair_obj[side_begin[side]:side_begin[side + 1]].tolist():
            V_all = sampled_vertices(tab, o, f)
            if not len(V_all):
                raise ValueError(f'object {int(tab["ids"][o])} (row {o}) is a candidate but has no mesh vertices')
            product += len(V_all) * len(pts)
            c_pair, m_pair = 0, np.inf
            for a in range(0, len(V_all), T_ITEM):                              # one block per item
                cnt['work_items'] += 1
                V = V_all[a:a + T_ITEM]
                alive = box_d2(V, lo, hi) < r2_hi
                cnt['vertices_rejected'] += int((~alive).sum())
                best = np.full(len(V), np.inf)
                for k, (tlo, thi) in enumerate(tiles):
                    want = alive & (box_d2(V, tlo, thi) < np.minimum(r2_hi, best * (1.0 + 1e-9)))
                    if not want.any():
                        cnt['tiles_skipped'] += 1
                        continue
                    cnt['tiles_staged'] += 1
                    tile = pts[k * TILE:(k + 1) * TILE]
                    best[want] = np.minimum(best[want], sq_dist(V[want], tile).min(1))
                    cnt['point_tests'] += int(want.sum()) * len(tile)
                inside = alive & (best < r2)
                c_pair += int(inside.sum())
                if inside.any():
                    m_pair = min(m_pair, float(best[inside].min()))
            close.append(c_pair)
            length.append(len(V_all))
            best_d2.append(m_pair)
    if counters is not None:
        counters.update(cnt)
    return dict(side_begin=side_begin, pair_obj=pair_obj, pair_close=np.array(close, np.int64), pair_len=np.array(length, np.int64),
                pair_min_d2=np.array(best_d2, np.float64), product=product)


# ---- synthetic inputs ---------------------------------------------------------------------------------------------------------------
def random_case(rng, n_syn=12, n_cells=5, scaling=(10, 10, 20), extent=6, per_cell=(1, 4), n_vert=(3, 200), spread_nm=900, blob_nm=250,
                fractional=True, types=('mi', 'vc')):
    """Synapses as shuffled blobs near the origin (so that vertices go negative), organelles as clouds around them."""
    s = scale64(scaling)
    partners, rep, vox = [], [], []
    for k in range(n_syn):
        a, b = rng.choice(np.arange(1, n_cells + 1), 2, replace=False)
        shape = rng.integers(1, extent + 1, 3)
        g = np.stack(np.meshgrid(*[np.arange(x) for x in shape], indexing='ij'), -1).reshape(-1, 3) + rng.integers(0, 400, 3)
        g = g[rng.random(len(g)) < 0.8] if len(g) > 3 else g
        g = g[rng.permutation(len(g))]
        partners.append((max(a, b), min(a, b)))
        vox.append(g.astype(np.uint32))
        rep.append(g[len(g) // 2])
    tables = {}
    for t in types:
        ids, cells, sizes, reps, verts = [], [], [], [], []
        for k in range(n_syn):
            centre = vox[k].astype(np.float64).mean(0) * s
            for cell in partners[k] + (0, n_cells + 1):                         # and unassigned / foreign organelles nearby
                for _ in range(int(rng.integers(per_cell[0], per_cell[1]))):
                    p = centre + rng.normal(0, spread_nm, 3) + rng.normal(0, blob_nm, (int(rng.integers(n_vert[0], n_vert[1])), 3))
                    p = p if fractional else np.round(p)
                    ids.append(10 * len(ids) + 3)
                    cells.append(cell)
                    sizes.append(int(rng.integers(0, 4000)))
                    reps.append(np.maximum(np.round(p.mean(0) / s), 0))
                    verts.append(p.astype(np.float32))
        order = rng.permutation(len(ids))
        tables[t] = table_from_lists(np.array(ids)[order], np.array(cells)[order], np.array(sizes)[order], np.array(reps)[order],
                                     [verts[j] for j in order])
    return dict(partners=np.array(partners, np.uint64), rep=np.array(rep, np.int32), vox=np.concatenate(vox),
                vox_begin=np.concatenate(([0], np.cumsum([len(v) for v in vox]))), sizes=np.array([len(v) for v in vox], np.int64),
                tables=tables, scaling=np.asarray(scaling, np.float32))


def assert_result_equal(got, want, what=''):
    """`got` / `want`: dicts with n_objs, n_vxs, min_dst and the pair list."""
    for k in ('side_begin', 'pair_obj', 'pair_close', 'pair_len'):
        assert np.array_equal(np.asarray(got[k], np.int64), want[k]), (what, k)
    assert np.asarray(got['pair_min_d2'], np.float64).tobytes() == want['pair_min_d2'].tobytes(), (what, 'pair_min_d2')
    for k in ('n_objs', 'n_vxs'):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k)
    assert got['min_dst'].dtype == np.float32 and got['min_dst'].tobytes() == want['min_dst'].tobytes(), (what, 'min_dst')


def mapping_result(mapping, t):
    """A ``SynSsvMapping``'s type `t` in the shape of ``map_objects``'s."""
    pl = mapping.pairs[t]
    return dict(side_begin=pl.side_begin, pair_obj=pl.pair_obj, pair_close=pl.pair_close, pair_len=pl.pair_len, pair_min_d2=pl.pair_min_d2,
                n_objs=getattr(mapping, f'n_{t}_objs'), n_vxs=getattr(mapping, f'n_{t}_vxs'), min_dst=getattr(mapping, f'min_dst_{t}_nm'))
