"""GPU: the rendering locations past one grid stride of every kernel of csrc/sd_locations.hip (1024 blocks of 256 items; 4096 blocks of 4
waves for the kernels with one wave per object or location), against closed forms, with guard bands behind every buffer
(tests/_locations_gpu.py)."""
import numpy as np
import pytest

import _locations_gpu as G
from syconn_amd import _lib as L

pytestmark = pytest.mark.gpu
F = np.float32
N_OBJ = 300000


@pytest.fixture(scope='module')
def small_objects():
    """300,000 objects of 1 - 3 vertices: multiples of 0.5 anywhere ('any'), or on a line along x with a spacing of 10 ('line')."""
    rng = np.random.default_rng(11)
    k = rng.integers(1, 4, N_OBJ)
    begin = np.concatenate(([0], np.cumsum(k))).astype(np.uint64)
    owner = np.repeat(np.arange(N_OBJ), k)
    j = np.arange(len(owner)) - begin[:-1].astype(np.int64)[owner]              # the vertex's number inside its object
    anyv = (rng.integers(-4000, 4001, (len(owner), 3)) * 0.5).astype(F)
    base = rng.integers(-1000, 1001, (N_OBJ, 3)).astype(F)
    line = base[owner].copy()
    line[:, 0] += (10 * j).astype(F)
    assert N_OBJ > L.SD_LOCATIONS_WAVE_GRID * 4 and len(owner) > L.SD_LOCATIONS_GRID * 256
    return dict(k=k, begin=begin, owner=owner, j=j, any=anyv, line=line)


def in_order(rows, begin, k, dtype, zero_first):
    """Per object ((v0 + v1) + v2) in `dtype` (after 0 + v0 with `zero_first`), vectorised over the objects."""
    b = begin[:-1].astype(np.int64)
    r = rows.astype(dtype)
    s = r[b] + dtype(0) if zero_first else r[b].copy()
    for step in (1, 2):
        m = k > step
        s[m] = s[m] + r[b[m] + step]
    return s


def test_many_small_objects_voxel(gpu, small_objects):
    o = small_objects
    # one voxel per object: the mean, added in vertex order in float64
    c, begin, loc = G.run(gpu, 'voxel', o['any'], o['begin'], ds=1e7)
    assert int(c[0]) == N_OBJ and np.array_equal(begin, np.arange(N_OBJ + 1, dtype=np.uint64))
    want = in_order(o['any'], o['begin'], o['k'], np.float64, True) / o['k'][:, None].astype(np.float64)
    assert G.same_bits(loc, want)
    # one voxel per vertex: the vertices themselves, x ascends with the vertex number
    c, begin, loc = G.run(gpu, 'voxel', o['line'], o['begin'], ds=1.0)
    assert np.array_equal(begin, o['begin']) and G.same_bits(loc, o['line'].astype(np.float64))


def test_many_small_objects_surface(gpu, small_objects):
    o = small_objects
    # one bin and one ball per object: the float32 mean of c = v - off in vertex order, + off
    c, begin, loc = G.run(gpu, 'surface', o['any'], o['begin'], bins=(1e6, 1e6, 1e6), r=1e6)
    assert int(c[0]) == N_OBJ and np.array_equal(begin, np.arange(N_OBJ + 1, dtype=np.uint64))
    off = np.minimum.reduceat(o['any'], o['begin'][:-1].astype(np.int64), axis=0)
    cc = (o['any'] - off[o['owner']]).astype(F)
    want = (in_order(cc, o['begin'], o['k'], F, False) / o['k'][:, None].astype(F)).astype(F) + off
    assert G.same_bits(loc, want)
    # bins of 5 over vertices 10 apart, r = 0: every vertex is the nearest one of its own bin's centre and alone in its ball
    c, begin, loc = G.run(gpu, 'surface', o['line'], o['begin'], bins=(5, 5, 5), r=0)
    assert np.array_equal(begin, o['begin']) and G.same_bits(loc, o['line'])
    assert c[2] > 0


@pytest.fixture(scope='module')
def lattice():
    g = np.arange(128, dtype=F)
    v = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    assert len(v) == 2097152
    return np.ascontiguousarray(v)


def test_lattice_voxel(gpu, lattice):
    """ds = 4, vmin = -2: the indices 0, 1 | 2 .. 5 | ... | 122 .. 125 | 126, 127 per axis, 33 voxels whose means are 0.5, 3.5, 7.5, ...,
    123.5, 126.5; the sums of small integers are exact in any order, the ORDER of the locations is what this checks at scale."""
    begin = np.array([0, 0, len(lattice), len(lattice)], np.uint64)               # an empty object on either side
    c, got_begin, loc = G.run(gpu, 'voxel', lattice, begin, ds=4.0)
    axis = np.concatenate(([0.5], 4.0 * np.arange(1, 32) - 0.5, [126.5]))
    want = np.stack(np.meshgrid(axis, axis, axis, indexing='ij'), -1).reshape(-1, 3)
    assert got_begin.tolist() == [0, 0, 33 ** 3, 33 ** 3] and G.same_bits(loc, want)


def test_lattice_surface(gpu, lattice):
    """Bins of 16 over an extent of 127: 8 bins per axis with the float32 step 15.875, all occupied; the centres 8, 24, ..., 120 are
    lattice points, so each is its own nearest vertex, and the 33 lattice points within r = 2 of it are symmetric about it: exact float32
    sums whose mean is the centre."""
    begin = np.array([0, len(lattice)], np.uint64)
    c, got_begin, loc = G.run(gpu, 'surface', lattice, begin, bins=(16, 16, 16), r=2)
    axis = (np.arange(8, dtype=F) + F(0.5)) * F(16)
    want = np.stack(np.meshgrid(axis, axis, axis, indexing='ij'), -1).reshape(-1, 3).astype(F)
    assert got_begin.tolist() == [0, 512] and G.same_bits(loc, want)
    assert c[3] > c[2] > 0                                                        # most tiles are skipped by their boxes
