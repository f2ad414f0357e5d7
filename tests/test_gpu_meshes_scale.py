"""GPU: csrc/sd_mesh.hip past one grid stride of every kernel (SD_MESH_GRID = 256 blocks of 256 threads: 65,536 voxel items, records,
pieces or objects per step; 16,384 objects per step of the wave-per-object kernel).  A 128 x 128 x 64 lattice of isolated voxels with
distinct labels, 131,072 objects, checked analytically: every object is an octahedron of 6 vertices and 8 triangles around its voxel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U = np.uint64
SCALING = np.array([10., 10., 20.])
LATTICE = (64, 64, 32)                                      # voxels at the odd coordinates of a (129, 129, 65) volume: none on a face


@pytest.fixture(scope='module')
def lattice():
    n = int(np.prod(LATTICE))
    vol = np.zeros((129, 129, 65), U)
    vol[1::2, 1::2, 1::2] = np.arange(1, n + 1, dtype=U).reshape(LATTICE)          # ids ascend in C order
    return vol


def check_octahedra(t, vol, offset):
    from syconn_amd import _lib as L
    n = len(t)
    assert n * 8 > L.SD_MESH_GRID * 256 and n > L.SD_MESH_GRID * 256                 # records and objects past one stride
    assert np.array_equal(t.ids, np.unique(vol)[1:])
    assert np.array_equal(t.vert_begin, np.arange(n + 1, dtype=U) * U(6)) and np.array_equal(t.tri_begin, np.arange(n + 1, dtype=U) * U(8))
    centre = (np.argwhere(vol != 0) + np.asarray(offset)).astype(np.float64)       # C order = id order
    v = t.vertices.reshape(n, 6, 3).astype(np.float64)
    # key order of the six grid edges around voxel c: (x - 1, axis 0), (y - 1, axis 1), (z - 1, axis 2), then (c, axis 0), (c, axis 1), (c, axis 2)
    shift = np.array([[-.5, 0, 0], [0, -.5, 0], [0, 0, -.5], [.5, 0, 0], [0, .5, 0], [0, 0, .5]])
    assert np.array_equal(v, (centre[:, None, :] + shift[None]) * SCALING)
    tri = t.indices.reshape(n, 8, 3)
    assert (tri == tri[0]).all() and tri.max() == 5
    p = v[0][tri[0]]
    assert np.einsum('ij,ij->i', p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6 == pytest.approx(SCALING.prod() / 6)      # outward
    sx, sy, sz = SCALING
    area = 8 * 0.5 * np.sqrt((sy * sz / 4) ** 2 + (sx * sz / 4) ** 2 + (sx * sy / 4) ** 2) / 1e6
    assert (np.abs(t.mesh_area - area) <= 8 * 2.0 ** -52 * area).all()
    assert np.array_equal(t.mesh_bb[:, 0], ((centre - .5) * SCALING).astype(np.float32)) and np.array_equal(t.mesh_bb[:, 1], ((centre + .5) * SCALING).astype(np.float32))


def test_lattice_of_isolated_voxels(gpu, lattice):
    from syconn_amd.proc.meshes import find_meshes_table
    t = find_meshes_table(lattice, (0, 0, 0), scaling=SCALING, device=gpu)
    assert len(t) == 131072 and len(t.vertices) == 6 * 131072 and len(t.indices) == 8 * 131072
    check_octahedra(t, lattice, (0, 0, 0))


def test_merge_of_four_chunks_is_their_concatenation(gpu, lattice):
    from syconn_amd.proc.meshes import MeshTable, find_meshes_table
    parts = [find_meshes_table(np.ascontiguousarray(lattice[32 * c:32 * c + 33]), (32 * c, 0, 0), scaling=SCALING, device=gpu) for c in range(4)]
    assert [len(p) for p in parts] == [32768] * 4
    merged = MeshTable.merge(parts[::-1], device=gpu)        # the list order does not matter where no object has two pieces
    check_octahedra(merged, lattice, (0, 0, 0))
    cat = lambda k: np.concatenate([getattr(p, k) for p in parts])
    for k in ('ids', 'vertices', 'indices', 'mesh_bb', 'mesh_area'):
        assert getattr(merged, k).tobytes() == cat(k).tobytes(), k
    twice = MeshTable.merge([parts[0], parts[0]], device=gpu)                      # every object in two pieces: second copy shifted by 6
    assert len(twice) == 32768 and np.array_equal(twice.vert_begin, np.arange(32769, dtype=U) * U(12))
    tri = twice.indices.reshape(32768, 16, 3)
    assert np.array_equal(tri[:, 8:], tri[:, :8] + 6) and np.array_equal(twice.vertices.reshape(32768, 2, 6, 3)[:, 1], parts[0].vertices.reshape(32768, 6, 3))
    assert (np.abs(twice.mesh_area - 2 * parts[0].mesh_area) <= 16 * 2.0 ** -52 * twice.mesh_area).all()
