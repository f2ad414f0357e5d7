"""CPU restatement of the TEASAR rules of DESIGN.md section 7 (the skeletonisation step): plain Python / numpy in the stated precisions,
a heap Dijkstra for every field and a brute-force distance to the boundary.  Written from the rules, not from any kimimaro text (kimimaro
is not part of the reference tree); the device must equal this bit for bit.  Volumes are (X, Y, Z), z fastest; a voxel is its raster index.

``defect`` plants a deviation for the tests that check the cases can tell: 'fma' fuses scale * pw + far in the penalty, 'tie_last' lets the
LARGEST raster index win ties of the parent step and of the target."""
import heapq
from fractions import Fraction

import numpy as np

F32 = np.float32
OFFS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]      # ascending raster order


def components(seg, dust_threshold=1):
    """comp int32 (1 .. N in raster order of the first voxel, dust 0), sizes, labels, first (index 0 unused)."""
    X, Y, Z = seg.shape
    flat = seg.reshape(-1)
    raw = np.zeros(flat.size, np.int64)
    groups = []
    for i in np.flatnonzero(flat):
        if raw[i]:
            continue
        lab = flat[i]
        raw[i] = len(groups) + 1
        stack, members = [int(i)], []
        while stack:
            v = stack.pop()
            members.append(v)
            x, r = divmod(v, Y * Z)
            y, z = divmod(r, Z)
            for dx, dy, dz in OFFS:
                xx, yy, zz = x + dx, y + dy, z + dz
                if 0 <= xx < X and 0 <= yy < Y and 0 <= zz < Z:
                    j = (xx * Y + yy) * Z + zz
                    if flat[j] == lab and not raw[j]:
                        raw[j] = raw[i]
                        stack.append(j)
        groups.append(np.array(sorted(members), np.int64))
    comp = np.zeros(flat.size, np.int32)
    sizes, labels, first = [0], [0], [-1]
    for m in groups:      # (found in raster order of their first voxel)
        if m.size < dust_threshold:
            continue
        comp[m] = len(sizes)
        sizes.append(m.size); labels.append(int(flat[m[0]])); first.append(int(m[0]))
    return comp.reshape(seg.shape), np.array(sizes, np.uint64), np.array(labels, np.uint64), np.array(first, np.int32)


def d2_brute(comp, w):
    """uint64: min over the voxels q of the array with another component number of sum (w_a (v_a - q_a))^2; 2^64 - 1 without such a voxel."""
    out = np.zeros(comp.shape, np.uint64)
    coords = np.stack(np.meshgrid(*[np.arange(n) for n in comp.shape], indexing='ij'), -1).reshape(-1, 3).astype(np.int64) * np.asarray(w, np.int64)
    flat, o = comp.reshape(-1), out.reshape(-1)
    for c in range(1, int(flat.max()) + 1 if flat.size else 1):
        V, Q = np.flatnonzero(flat == c), np.flatnonzero(flat != c)
        if Q.size == 0:
            o[V] = np.uint64(2 ** 64 - 1)
            continue
        for s in range(0, V.size, 256):
            d = coords[V[s:s + 256], None, :] - coords[None, Q, :]
            o[V[s:s + 256]] = (d * d).sum(-1).min(1).astype(np.uint64)
    return out


def dbf_of(d2):
    return np.sqrt(d2.astype(np.float64)).astype(F32)      # (2^64 - 1 -> 2^64 -> finite float32; the device writes +inf and raises a count)


class Grid:
    def __init__(self, comp, w):
        self.shape = comp.shape
        self.X, self.Y, self.Z = comp.shape
        self.comp = comp.reshape(-1)
        self.w = [int(a) for a in w]
        self.len = [F32(np.sqrt(np.float64(sum((self.w[a] * o[a]) ** 2 for a in range(3))))) for o in OFFS]

    def neighbours(self, v):
        """(raster index, offset class) of the same-component neighbours of v, in ascending raster order."""
        x, r = divmod(v, self.Y * self.Z)
        y, z = divmod(r, self.Z)
        c = self.comp[v]
        for k, (dx, dy, dz) in enumerate(OFFS):
            xx, yy, zz = x + dx, y + dy, z + dz
            if 0 <= xx < self.X and 0 <= yy < self.Y and 0 <= zz < self.Z:
                j = (xx * self.Y + yy) * self.Z + zz
                if self.comp[j] == c:
                    yield j, k


def daf_heap(g, source):
    """float32 field of the component of `source`: {voxel: value}."""
    d = {source: F32(0)}
    heap, done = [(F32(0), source)], set()
    while heap:
        du, u = heapq.heappop(heap)
        if u in done:
            continue
        done.add(u)
        for j, k in g.neighbours(u):
            cand = F32(du + g.len[k])
            if j not in d or cand < d[j]:
                d[j] = cand
                heapq.heappush(heap, (cand, j))
    return d


def daf_sweeps(g, source, members):
    """The same fixed point by naive sweeps until nothing changes (the fixed-point claim)."""
    d = {v: F32(np.inf) for v in members}
    d[source] = F32(0)
    changed = True
    while changed:
        changed = False
        for v in members:
            for j, k in g.neighbours(v):
                cand = F32(d[j] + g.len[k])
                if cand < d[v]:
                    d[v] = cand
                    changed = True
    return d


def penalty(dbf, daf, M, daf_max, scale, e, defect=None):
    b = 1.0 - float(dbf) / M
    pw = b
    for _ in range(e - 1):
        pw = pw * b
    far = float(daf) / float(daf_max) if float(daf_max) > 0.0 else 0.0
    if defect == 'fma':
        return float(Fraction(scale) * Fraction(pw) + Fraction(far))
    return scale * pw + far


def dist_heap(g, p, start):
    """float64 fixed point of dist(v) = min_u fl64(dist(u) + p(v)) from the start values {voxel: value} (inf where absent)."""
    d = dict(start)
    heap = [(val, v) for v, val in d.items() if val < np.inf]
    heapq.heapify(heap)
    done = set()
    while heap:
        du, u = heapq.heappop(heap)
        if u in done or du > d[u]:
            continue
        done.add(u)
        for j, _ in g.neighbours(u):
            cand = du + p[j]
            if cand < d.get(j, np.inf):
                d[j] = cand
                heapq.heappush(heap, (cand, j))
    return d


def dist_sweeps(g, p, start, members):
    d = {v: start.get(v, np.inf) for v in members}
    changed = True
    while changed:
        changed = False
        for v in members:
            for j, _ in g.neighbours(v):
                cand = d[j] + p[v]
                if cand < d[v]:
                    d[v] = cand
                    changed = True
    return d


def skeletonize(seg, w, dust_threshold=1, scale=4.0, const=0.0, pdrf_scale=100000.0, pdrf_exponent=4, max_paths=100, defect=None, cold=False):
    """All stages.  Returns a dict: comp, sizes, labels, first, d2, dbf, dbf_max, daf0, root, daf, daf_max, targets [round][c], dist / valid
    snapshots after every round (`dist_rounds`, `valid_rounds`; dist is +inf outside the components), absorbed, void, and per component the
    `nodes` (raster indices, ascending), `edges` (indices inside the component), `radii`, `vertices`.  cold=True recomputes dist from
    infinity after every round instead of continuing from its values."""
    comp, sizes, labels, first = components(seg, dust_threshold)
    n = len(sizes) - 1
    g = Grid(comp, w)
    d2 = d2_brute(comp, w)
    dbf = dbf_of(d2)
    cf, dbf_f = comp.reshape(-1), dbf.reshape(-1)
    nvox = cf.size
    members = [None] + [np.flatnonzero(cf == c).tolist() for c in range(1, n + 1)]
    daf0 = np.full(nvox, np.inf, F32); daf = np.full(nvox, np.inf, F32)
    dist = np.full(nvox, np.inf, np.float64); valid = (cf > 0).astype(np.uint8)
    p = np.zeros(nvox, np.float64)
    root = np.full(n + 1, -1, np.int32); dbf_max = np.zeros(n + 1, F32); daf_max = np.zeros(n + 1, F32)
    parent = np.full(nvox, -1, np.int32)
    void = np.zeros(n + 1, np.int32)
    absorbed = 0
    for c in range(1, n + 1):
        m = members[c]
        dbf_max[c] = dbf_f[m].max()
        for v, val in daf_heap(g, int(first[c])).items():
            daf0[v] = val
        root[c] = max(m, key=lambda v: (daf0[v], -v))
        for v, val in daf_heap(g, int(root[c])).items():
            daf[v] = val
        daf_max[c] = daf[m].max()
        M = float(dbf_max[c]) ** 1.01
        for v in m:
            p[v] = penalty(dbf_f[v], daf[v], M, daf_max[c], float(pdrf_scale), pdrf_exponent, defect)
        for v, val in dist_heap(g, p, {int(root[c]): 0.0}).items():
            dist[v] = val
    targets, dist_rounds, valid_rounds = [], [], []
    s32, c32 = F32(scale), F32(const)
    for rnd in range(max_paths):
        tg = np.full(n + 1, -1, np.int32)
        for c in range(1, n + 1):
            if void[c]:
                continue
            m = [v for v in members[c] if valid[v]]
            if m:
                tg[c] = max(m, key=(lambda v: (daf[v], v)) if defect == 'tie_last' else (lambda v: (daf[v], -v)))
        if (tg < 0).all():
            break
        targets.append(tg)
        for c in range(1, n + 1):
            if void[c]:
                continue
            new = []
            if rnd == 0:
                parent[root[c]] = root[c]
                new.append(int(root[c]))
            u = int(tg[c])
            while u >= 0 and dist[u] > 0.0:
                best, bn = np.inf, -1
                for j, _ in g.neighbours(u):
                    if dist[j] < best or (defect == 'tie_last' and dist[j] == best):
                        best, bn = dist[j], j
                if bn < 0 or not best < dist[u]:
                    absorbed += 1
                    void[c] = 1
                    break
                parent[u] = bn
                new.append(u)
                u = bn
            start = {}
            for v in new:
                dist[v] = 0.0
                r = F32(F32(s32 * dbf_f[v]) + c32)
                if not r >= 0:
                    continue
                x, rr = divmod(v, g.Y * g.Z)
                y, z = divmod(rr, g.Z)
                h = [int(min(np.floor(float(r) / g.w[a]), 4096)) for a in range(3)]
                box = valid.reshape(g.shape)[max(x - h[0], 0):x + h[0] + 1, max(y - h[1], 0):y + h[1] + 1, max(z - h[2], 0):z + h[2] + 1]
                box[comp[max(x - h[0], 0):x + h[0] + 1, max(y - h[1], 0):y + h[1] + 1, max(z - h[2], 0):z + h[2] + 1] == c] = 0
            m = members[c]
            if cold:
                start = {v: 0.0 for v in m if dist[v] == 0.0}
            else:
                start = {v: dist[v] for v in m}
            for v, val in dist_heap(g, p, start).items():
                dist[v] = val
        dist_rounds.append(dist.reshape(g.shape).copy())
        valid_rounds.append(valid.reshape(g.shape).copy())
    out = dict(comp=comp, sizes=sizes, labels=labels, first=first, d2=d2, dbf=dbf, dbf_max=dbf_max, daf0=daf0.reshape(g.shape), root=root,
               daf=daf.reshape(g.shape), daf_max=daf_max, p=p.reshape(g.shape), targets=targets, dist_rounds=dist_rounds, valid_rounds=valid_rounds,
               absorbed=absorbed, void=void, parent=parent.reshape(g.shape), nodes=[None], edges=[None], radii=[None], vertices=[None])
    wv = np.asarray(w, np.int64)
    for c in range(1, n + 1):
        nodes = np.array([v for v in members[c] if parent[v] >= 0 and not void[c]], np.int64)
        index = {int(v): k for k, v in enumerate(nodes)}
        edges = np.array([(index[int(v)], index[int(parent[v])]) for v in nodes if v != root[c]], np.int32).reshape(-1, 2)
        xyz = np.stack(np.unravel_index(nodes, g.shape), -1).astype(np.int64).reshape(-1, 3)
        out['nodes'].append(nodes); out['edges'].append(edges); out['radii'].append(dbf_f[nodes]); out['vertices'].append((xyz * wv).astype(F32))
    return out

