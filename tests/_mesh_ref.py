"""Plain numpy restatement of the device meshing (sd_mesh.hip, syconn_amd/proc/meshes.py), written from the rule and the order the
contract states and from nothing else: the triangle table is built here, not read from the generated header.

Numbering: corner = dx + 2 dy + 4 dz; edge = axis * 4 + j over the four corners with coordinate 0 on the axis, ascending.
Order: vertices ascend by ((x NY + y) NZ + z) * 3 + axis of the grid edge's lower voxel in the padded array, triangles by cube in C order,
then table order.  ``Mesher`` and ``mesh_surface_area`` are the stand-ins for zmesh and skimage that the golden generator injects into
the reference's own ``find_meshes`` / ``mesh_area_calc``."""
import itertools
from collections import Counter

import numpy as np
from scipy.ndimage import zoom

CP = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)])
EDGES = [(c, c | (1 << a)) for a in range(3) for c in range(8) if CP[c][a] == 0]
EID = {e: i for i, e in enumerate(EDGES)}
EMID = np.array([(CP[a] + CP[b]) / 2 for a, b in EDGES])


def _eid(c0, c1):
    return EID[(min(c0, c1), max(c0, c1))]


def rule_table():
    """The 256 triangle lists of the rule (module docstring of tools/gen_mc_table.py states it in words)."""
    faces = []
    for a in range(3):
        b, c = [(1, 2), (0, 2), (0, 1)][a]
        for s in (0, 1):
            cyc = []
            for u, v in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[a], p[b], p[c] = s, u, v
                cyc.append(p[0] + 2 * p[1] + 4 * p[2])
            n = np.zeros(3)
            n[a] = 1 if s else -1
            faces.append((cyc, n))
    T = [[] for _ in range(256)]
    for cfg in range(1, 255):
        ins = [(cfg >> c) & 1 for c in range(8)]
        nxt = {}
        for cyc, n in faces:
            f = [ins[c] for c in cyc]
            if sum(f) in (0, 4):
                continue
            for i in range(4):
                if f[i] and not f[i - 1]:                       # a maximal run of inside corners starts at i
                    j = i
                    while f[(j + 1) % 4]:
                        j += 1
                    ea, eb = _eid(cyc[i - 1], cyc[i]), _eid(cyc[j % 4], cyc[(j + 1) % 4])
                    pa, pb = EMID[ea], EMID[eb]
                    if np.dot(np.cross(n, pb - pa), CP[cyc[i]] - pa) > 0:
                        nxt[eb] = ea                             # the side on which a single voxel's volume is positive
                    else:
                        nxt[ea] = eb
        seen = set()
        for st in sorted(nxt):
            if st in seen:
                continue
            loop, cur = [st], nxt[st]
            seen.add(st)
            while cur != st:
                loop.append(cur)
                seen.add(cur)
                cur = nxt[cur]
            T[cfg] += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    return T


TABLE = rule_table()


def vertex_keys(m):
    """The canonical vertex set of the boolean volume m as ascending keys: one vertex per grid edge whose voxels differ."""
    NX, NY, NZ = m.shape
    keys = []
    for a in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        q = np.argwhere(m[tuple(lo)] != m[tuple(hi)]).astype(np.int64)
        keys.append(((q[:, 0] * NY + q[:, 1]) * NZ + q[:, 2]) * 3 + a)
    return np.sort(np.concatenate(keys))


def key_positions(keys, shape):
    """Half-integer grid positions (n, 3) float64 of vertex keys."""
    NX, NY, NZ = shape
    keys = np.asarray(keys, np.int64)
    a, v = keys % 3, keys // 3
    g = np.stack([v // (NY * NZ), (v // NZ) % NY, v % NZ], 1).astype(np.float64)
    g[np.arange(len(keys)), a] += 0.5
    return g


def marching_cubes(m):
    """-> (keys ascending int64, triangles (n, 3) uint32 into them) of the boolean volume m, in the contract's order."""
    NX, NY, NZ = m.shape
    keys = vertex_keys(m)
    if min(m.shape) < 2:
        return keys, np.zeros((0, 3), np.uint32)
    cfg = np.zeros((NX - 1, NY - 1, NZ - 1), np.int64)
    for c in range(8):
        dx, dy, dz = CP[c]
        cfg |= m[dx:NX - 1 + dx, dy:NY - 1 + dy, dz:NZ - 1 + dz].astype(np.int64) << c
    tris = []
    for x, y, z in np.argwhere((cfg != 0) & (cfg != 255)):
        for t in TABLE[cfg[x, y, z]]:
            tri = []
            for e in t:
                c0 = EDGES[e][0]
                tri.append((((x + CP[c0][0]) * NY + y + CP[c0][1]) * NZ + z + CP[c0][2]) * 3 + e // 4)
            tris.append(tri)
    tris = np.array(tris, np.int64).reshape(-1, 3)
    idx = np.searchsorted(keys, tris)
    assert (keys[idx] == tris).all()
    return keys, idx.astype(np.uint32)


def padded_volume(chunk, pad, ds):
    """The reference's own preparation (proc/meshes.py:969-975): scipy's zoom, then numpy's edge pad."""
    if ds is not None:
        chunk = zoom(chunk, 1 / np.array(ds), order=0)
    if pad > 0:
        chunk = np.pad(chunk, 1, mode='edge')
    return chunk


def find_meshes_table(chunk, offset, pad=0, ds=None, scaling=(10., 10., 20.)):
    """The whole contract on the host: dict(ids, vert_begin, tri_begin, vertices (n, 3) float32, indices (n, 3) uint32, mesh_bb, mesh_area)."""
    chunk = np.asarray(chunk)
    ids = np.unique(chunk)
    ids = ids[ids != 0].astype(np.uint64)
    scaling = np.array(scaling, np.float64)
    s_ds = scaling * (np.array(ds, np.float64) if ds is not None else 1.0)
    off = np.asarray(offset, np.float64) * scaling - (pad * s_ds if pad > 0 else 0.0)
    vol = padded_volume(chunk, pad, ds)
    verts, tris, vb, tb, bbs, areas = [], [], [0], [0], [], []
    for i in ids:
        keys, t = marching_cubes(vol == i)
        v = np.maximum(key_positions(keys, vol.shape) * s_ds + off, 0).astype(np.float32)
        verts.append(v); tris.append(t)
        vb.append(vb[-1] + len(v)); tb.append(tb[-1] + len(t))
        bbs.append([v.min(0), v.max(0)] if len(v) else np.zeros((2, 3), np.float32))
        areas.append(mesh_surface_area(v, t) / 1e6)
    return dict(ids=ids, vert_begin=np.array(vb, np.uint64), tri_begin=np.array(tb, np.uint64),
                vertices=np.concatenate(verts).reshape(-1, 3) if verts else np.zeros((0, 3), np.float32),
                indices=np.concatenate(tris).reshape(-1, 3) if tris else np.zeros((0, 3), np.uint32),
                mesh_bb=np.array(bbs, np.float32).reshape(-1, 2, 3), mesh_area=np.array(areas, np.float64))


# ---- stand-ins for zmesh.Mesher and skimage.measure.mesh_surface_area ---------------------------------------------------------------
def mesh_surface_area(verts, faces):
    """0.5 * sum |cross| in float64."""
    p = np.asarray(verts, np.float64).reshape(-1, 3)[np.asarray(faces).reshape(-1, 3).astype(np.int64)]
    a, b = p[:, 0] - p[:, 1], p[:, 0] - p[:, 2]
    return np.sqrt((np.cross(a, b) ** 2).sum(axis=1)).sum() / 2.


class _Mesh:
    def __init__(self, vertices, faces):
        self.vertices, self.faces, self.normals = vertices, faces, None


class Mesher:
    """zmesh.Mesher's interface over the unsimplified surface: vertices in nm (voxel i at coordinate i times the voxel size), float64."""

    def __init__(self, voxel_res):
        self.res, self.vol = np.array(voxel_res, np.float64), None

    def mesh(self, vol_zyx):
        self.vol = np.asarray(vol_zyx).swapaxes(0, 2)

    def ids(self):
        u = np.unique(self.vol)
        return [i for i in u if i != 0]

    def get_mesh(self, obj_id, normals=False, simplification_factor=0, max_simplification_error=0):
        assert not normals
        keys, t = marching_cubes(self.vol == obj_id)
        return _Mesh(key_positions(keys, self.vol.shape) * self.res, t)

    def erase(self, obj_id):
        pass

    def clear(self):
        self.vol = None


# ---- properties of a mesh -------------------------------------------------------------------------------------------------------------
def edge_balance(tris):
    """(closed, manifold): every directed edge has its reverse as often; no directed edge twice."""
    d = Counter()
    for a, b, c in np.asarray(tris).reshape(-1, 3).tolist():
        for e in ((a, b), (b, c), (c, a)):
            d[e] += 1
    return all(d[(b, a)] == n for (a, b), n in d.items()), all(n == 1 for n in d.values())


def signed_volume(verts, tris):
    p = np.asarray(verts, np.float64).reshape(-1, 3)[np.asarray(tris).reshape(-1, 3).astype(np.int64)]
    return np.einsum('ij,ij->i', p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6


def euler(n_verts, tris):
    t = np.asarray(tris).reshape(-1, 3).astype(np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    return n_verts - len(np.unique(e, axis=0)) + len(t)


if __name__ == '__main__':
    print('max', max(len(t) for t in TABLE), 'total', sum(len(t) for t in TABLE))
    one = np.zeros((3, 3, 3), bool); one[1, 1, 1] = True
    k, t = marching_cubes(one)
    print('voxel', len(k), len(t), signed_volume(key_positions(k, one.shape), t), edge_balance(t))
    box = np.zeros((6, 5, 4), bool); box[1:5, 1:4, 1:3] = True
    k, t = marching_cubes(box)
    print('box', len(k), len(t), signed_volume(key_positions(k, box.shape), t), euler(len(k), t))
    g = np.indices((15, 15, 15)) - 7
    ball = (g ** 2).sum(0) <= 25
    k, t = marching_cubes(ball)
    print('ball', len(k), len(t), signed_volume(key_positions(k, ball.shape), t), euler(len(k), t), edge_balance(t))
    del itertools
