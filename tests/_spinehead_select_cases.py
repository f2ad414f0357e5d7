"""Hand-built ``flood`` volumes for the head selection (``sd_spinehead_select``; reference ``reps/super_segmentation_helper.py:2171-2196``),
shared by tests/test_spinehead_cpu.py (the restatement against cKDTree) and tests/test_gpu_spinehead_select.py (the kernel against the
restatement).  A case is a dict ``flood (x, y, z) int32, c, offset (int64[3]), scaling (array, dtype kept)``; everything is seeded.

The volumes of the distance families are (64, 64, 16) with every object below z = 10 and ``c[2] = 4``: the z part of
``labels[c - 10 : c + 11]`` wraps to ``[10:15]``, so the slice is empty whatever x and y are and the nearest object decides."""
import numpy as np

SHAPE = (64, 64, 16)
VOXEL_SIZES = [(9.1, 9.1, 22.5), (11.24, 11.24, 28.0), (13.3, 13.3, 40.0)]
CONTROL = (10.0, 10.0, 20.0)                       # every product exact: fused or not, difference first or not, the same bits
# (id, voxel size as the array SuperSegmentationObject.scaling is): float64, and float32 that numpy widens in its products
SCALINGS = [(f'{s[0]}-{t.__name__}', np.array(s, t)) for s in VOXEL_SIZES for t in (np.float64, np.float32)] + [('10-control', np.array(CONTROL, np.float64))]
OFFSETS = [(1234, 877, 300), (20480, 9000, 5120)]  # window offsets of the size real datasets have
RANDOM_SEEDS = range(40)                           # of random_objects, per offset: every one decided for every voxel size (test_spinehead_cpu.py)
N_MIRRORED, N_NEAR = 120, 40
# (c, offset) of the near-ties: mirrored pairs whose exact tie an unsymmetric c or a window offset may break in the reference's rounding
NEAR_TIES = [((30, 27, 4), (0, 0, 0)), ((30, 30, 4), OFFSETS[0]), ((30, 27, 4), OFFSETS[1])]


def _case(flood, c, offset, scaling):
    return dict(flood=flood, c=np.array(c, np.int64), offset=np.array(offset, np.int64), scaling=scaling)


def mirrored_pairs(n, seed):
    """`n` of the 1140 offsets (a, b, k), 11 <= a < b <= 30, k < 6, in a seeded order, every k and both ends of a and b among them."""
    every = [(a, b, k) for a in range(11, 31) for b in range(a + 1, 31) for k in range(6)]
    rng = np.random.default_rng(seed)
    first = [(11, 12, 0), (11, 30, 5), (29, 30, 3), (12, 27, 1), (17, 18, 2), (20, 25, 4)]
    rest = [every[i] for i in rng.permutation(len(every)) if every[i] not in first]
    return (first + rest)[:n]


def mirrored(c, offset, scaling, n=120, seed=1):
    """Two single-voxel objects at c + (a, b, k) and c + (b, a, k): raster order gives the first id 1.  With c[0] == c[1], equal x and y
    voxel sizes and offset 0 the two are exact ties in the reference's arithmetic; otherwise its rounding decides."""
    out = []
    for a, b, k in mirrored_pairs(n, seed):
        flood = np.zeros(SHAPE, np.int32)
        flood[c[0] + a, c[1] + b, c[2] + k] = 1
        flood[c[0] + b, c[1] + a, c[2] + k] = 1
        out.append(_case(flood, c, offset, scaling))
    return out


def random_objects(seed, offset, scaling, c=(30, 27, 4)):
    """2 to 6 objects of 1 to 5 voxels (a self-avoiding walk each), 11 to 25 voxels from c in x / y (Chebyshev), below z = 10."""
    rng = np.random.default_rng(seed)
    flood = np.zeros(SHAPE, np.int32)
    ok = lambda p: 11 <= max(abs(p[0] - c[0]), abs(p[1] - c[1])) <= 25 and 0 <= p[2] < 10
    for _ in range(int(rng.integers(2, 7))):
        while True:
            p = (c[0] + int(rng.integers(-25, 26)), c[1] + int(rng.integers(-25, 26)), int(rng.integers(0, 10)))
            if ok(p):
                break
        flood[p] = 1
        for _ in range(int(rng.integers(0, 5))):
            step = np.zeros(3, np.int64)
            step[rng.integers(3)] = rng.choice((-1, 1))
            q = tuple(int(v) for v in np.array(p) + step)
            if ok(q):
                flood[q] = 1
                p = q
    return _case(flood, c, offset, scaling)


# ---- the slice rule ------------------------------------------------------------------------------------------------------------------
EXTENTS = (9, 17, 20, 21, 22, 33)


def axis_pairs():
    """Every (extent n, component of c) with c from {0, 3, 9, 10, 11, n - 12, n - 11, n - 10, n - 1} that exists for n."""
    return [(n, v) for n in EXTENTS for v in sorted({v for v in (0, 3, 9, 10, 11, n - 12, n - 11, n - 10, n - 1) if 0 <= v < n})]


def blob_flood(shape, rng):
    """flood == 1 blobs (boxes, balls, sprinkles) cut and surrounded by voxels of flood 0, 2 and 9, which the selection ignores."""
    g = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing='ij'), -1)
    head = rng.random(shape) < 0.03
    for _ in range(int(rng.integers(3, 9))):
        p, r = rng.integers(0, shape), rng.integers(1, 4, 3)
        if rng.random() < 0.5:
            head |= np.all(np.abs(g - p) <= r, -1)
        else:
            head |= (((g - p) / r) ** 2).sum(-1) <= 1.0
    flood = np.where(head, 1, rng.choice(np.array([0, 2, 9]), shape, p=[0.8, 0.1, 0.1])).astype(np.int32)
    cut = rng.random(shape) < 0.08
    flood[cut] = rng.choice(np.array([0, 2, 9]), int(cut.sum()))
    return flood


def slice_cases(rounds=3, seed=11, scaling=None, offset=OFFSETS[0]):
    """Every (extent, c component) pair on every axis `rounds` times, the axes shuffled against each other."""
    scaling = np.array(VOXEL_SIZES[0], np.float64) if scaling is None else scaling
    rng = np.random.default_rng(seed)
    pairs = axis_pairs()
    out = []
    for _ in range(rounds):
        perm = [rng.permutation(len(pairs)) for _ in range(3)]
        for i in range(len(pairs)):
            (X, cx), (Y, cy), (Z, cz) = (pairs[perm[a][i]] for a in range(3))
            out.append(_case(blob_flood((X, Y, Z), rng), (cx, cy, cz), offset, scaling))
    return out


def directed_slice_cases(scaling=None, offset=OFFSETS[0]):
    """-> list of (name, case, (chosen id, its voxels, nb_obj)) worked out by hand."""
    scaling = np.array(VOXEL_SIZES[0], np.float64) if scaling is None else scaling
    out = []
    # c = (16, 10, 10) in (33, 22, 21): the slice is [6:27, 0:21, 0:21]
    f = np.zeros((33, 22, 21), np.int32)
    f[12, 5, 3:6] = 1                                  # id 1: 3 voxels, all in the slice
    f[24:33, 5, 4] = 1                                 # id 2: 9 voxels, x = 24, 25, 26 in the slice
    out.append(('equal counts: the lower id, not the larger object', _case(f.copy(), (16, 10, 10), offset, scaling), (1, 3, 2)))
    f[:] = 0
    f[0:8, 5, 4] = 1                                   # id 1: 8 voxels, x = 6, 7 in the slice
    f[12, 5, 3:6] = 1                                  # id 2: 3 voxels, all in the slice
    out.append(('larger overall, smaller in the slice, loses', _case(f.copy(), (16, 10, 10), offset, scaling), (2, 3, 2)))
    # a slice that is empty because it wraps (c[0] = 3 of 33: [26:14]); id 2 owns the voxel nearest to c
    f[:] = 0
    f[0:3, 0, 0] = 1
    f[5, 12, 10] = 1
    out.append(('empty by wrapping: the nearest', _case(f.copy(), (3, 10, 10), offset, scaling), (2, 1, 2)))
    # a slice that wraps yet holds voxels (c[0] = 8 of 17: [15:17]): the object in it wins over the larger one around c
    f = np.zeros((17, 22, 21), np.int32)
    f[7:10, 9:12, 9:12] = 1                            # id 1: 27 voxels around c, none in the slice
    f[16, 3, 3] = 1                                    # id 2: one voxel, in the slice
    out.append(('wraps, not empty', _case(f.copy(), (8, 10, 10), offset, scaling), (2, 1, 2)))
    return out


def checkerboard():
    """16^3, every second voxel: 2048 isolated objects, 32 distinct labels in every wave of 64 consecutive voxels."""
    return (np.indices((16, 16, 16)).sum(0) % 2 == 0).astype(np.int32)
