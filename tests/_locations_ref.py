"""The two rules of the rendering locations in numpy, by brute force: what csrc/sd_locations.hip computes, per object.

``generate_rendering_locs`` is the NORMATIVE form of the voxel rule: the reference calls open3d's ``PointCloud.voxel_down_sample``
(handler/multiviews.py:339-355), which is not installed where this suite runs, so the rule is stated here as open3d publishes it and is
pinned by nothing else.  ``surface_samples`` restates reps/rep_helper.py:376-417; tests/golden/g28_locations.npz holds what the
reference's own function returns, and tests/test_locations_cpu.py compares the two bit for bit.

Choices where the reference leaves one: the voxel rule's locations ascend by voxel (ix, iy, iz), x most significant (open3d: the order of
a hash map); among vertices at exactly the same distance from a bin centre the lowest index is the nearest (cKDTree: its own order)."""
import numpy as np

MAX_CELLS = 1 << 21                      # voxels / bins of one object per axis (SD_LOCATIONS_MAX_CELLS)


def seq_sum(rows, dtype):
    """The rows added one after another in `dtype`, starting from the first."""
    return np.cumsum(np.asarray(rows, dtype), axis=0, dtype=dtype)[-1]


def generate_rendering_locs(verts, ds_factor) -> np.ndarray:
    ds = float(ds_factor)
    if not (ds > 0 and np.isfinite(ds)):
        raise ValueError('voxel size must be positive')
    p = np.asarray(verts).astype(np.float64).reshape(-1, 3)
    if not np.isfinite(p).all():
        raise ValueError('a vertex is not finite')
    if len(p) == 0:
        return np.zeros((0, 3), np.float64)
    vmin = p.min(0) - 0.5 * ds
    ix = np.floor((p - vmin) / ds)
    if ix.max() >= MAX_CELLS:
        raise ValueError('more voxels per axis than the key packing allows')
    ix = ix.astype(np.int64)
    key = (ix[:, 0] << 42) | (ix[:, 1] << 21) | ix[:, 2]
    order = np.argsort(key, kind='stable')                                       # within a voxel: ascending vertex index
    cuts = np.flatnonzero(np.diff(key[order])) + 1
    out = []
    for run in np.split(order, cuts):
        s = seq_sum(np.concatenate((np.zeros((1, 3)), p[run])), np.float64)   # open3d accumulates from a zero vector
        out.append(s / float(len(run)))
    return np.array(out, np.float64).reshape(-1, 3)


def surface_bins(c, mx, nb):
    """numpy >= 2's histogramdd bin of every row of the float32 `c`: per axis the number of float32 edges <= c, minus one."""
    bins = np.zeros(c.shape, np.int64)
    for a in range(3):
        if mx[a] == 0:
            continue                                                             # edges -0.5 | 0.5: one bin
        step = np.float32(mx[a] / np.float32(nb[a]))
        e = (np.arange(nb[a] + 1, dtype=np.float32) * step).astype(np.float32)
        e[-1] = mx[a]
        bins[:, a] = np.minimum(np.searchsorted(e, c[:, a], side='right') - 1, nb[a] - 1)      # c == mx: the last bin
    return bins


def sq_dist(a, b):
    d = a - b
    return ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def surface_samples(coords, bin_sizes=(2000, 2000, 2000), max_nb_samples=5000, r=1000, return_parts=False):
    v = np.asarray(coords)
    if v.dtype != np.float32:
        raise NotImplementedError('float32 vertices only')
    v = v.reshape(-1, 3)
    if not np.isfinite(v).all():
        raise ValueError('a vertex is not finite')
    if len(v) == 0:
        return np.zeros((0, 3), np.float32)
    bs = np.array(bin_sizes, dtype=np.float32)
    off = v.min(0)
    c = (v - off).astype(np.float32)
    mx = c.max(0)
    with np.errstate(over='ignore', invalid='ignore'):
        q = np.ceil(mx / bs)
    if not (q <= MAX_CELLS).all():
        raise ValueError('more bins per axis than the key packing allows')
    nb = np.maximum(1, q.astype(np.int32))
    occupied = np.unique(surface_bins(c, mx, nb), axis=0)                          # C order of (bx, by, bz)
    centres = (occupied + 0.5) * bs.astype(np.float64)
    c64 = c.astype(np.float64)
    r2 = float(r) * float(r)
    out = np.zeros((len(centres), 3), np.float32)
    nearest, sizes = [], []
    for n, q in enumerate(centres):
        ix = int(np.argmin(sq_dist(c64, q)))                                     # the first minimum: the lowest index
        members = np.flatnonzero(sq_dist(c64, c64[ix]) <= r2)                    # ascending
        out[n] = seq_sum(c[members], np.float32) / np.float32(len(members)) + off
        nearest.append(ix); sizes.append(len(members))
    if return_parts:
        return out, occupied, np.array(nearest), np.array(sizes), nb
    return out


def sample_table(vert_begin, verts, rule, **kw):
    """(loc_begin uint64 (n + 1), locations) of every object of the table: 'voxel' (ds=...) in float64, 'surface' (bin_sizes=..., r=...)
    in float32."""
    vb = np.asarray(vert_begin).astype(np.int64)
    verts = np.asarray(verts).reshape(-1, 3)
    parts = []
    for k in range(len(vb) - 1):
        o = verts[vb[k]:vb[k + 1]]
        parts.append(generate_rendering_locs(o, kw['ds']) if rule == 'voxel' else surface_samples(o, kw['bin_sizes'], r=kw['r']))
    dt = np.float64 if rule == 'voxel' else np.float32
    begin = np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.uint64)
    return begin, (np.concatenate(parts) if parts else np.zeros((0, 3), dt)).astype(dt).reshape(-1, 3)


def sample_locations(verts, rep_coord, scaling, ds_factor=None, use_new_renderings_locs=True):
    """SegmentationObject.sample_locations (reps/segmentation.py:718-732) without the storage."""
    verts = np.asarray(verts).reshape(-1, 3)
    if len(verts) == 0:
        return (np.array([rep_coord, ], dtype=np.float32) * scaling).astype(np.float32)
    if ds_factor is None:
        ds_factor = 2000
    if use_new_renderings_locs:
        return generate_rendering_locs(verts, ds_factor).astype(np.float32)
    return surface_samples(verts, [ds_factor] * 3, r=ds_factor / 2).astype(np.float32)
