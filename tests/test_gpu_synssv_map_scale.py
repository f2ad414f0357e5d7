"""GPU: the organelle mapping on an analytic lattice past every launch cap of csrc/sd_synssv_map.hip: more sides than one grid stride
of the pair kernel (4096 blocks of four waves) and more work items than one grid of the query kernel (8192 blocks).

Synapse i (cells 2 i + 2 and 2 i + 1) is a 2 x 2 x 2 blob in scan order at scaling (10, 10, 20): with ``sample_fact`` 2 its sampled
voxels are the z layer of its corner.  Its smaller cell owns one organelle of 8 vertices straight above the corner voxel, at heights
h + 0 .. h + 7 nm: the sampled ones are at distances h, h + 2, h + 4, h + 6.  With R = 500: h = 100 + 99 (i mod 5) gives 4 close
vertices, except h = 496 which gives 2 (500 is exactly R: not close); every 7th organelle is at h = 600, beyond R."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 9000
R = 500


def test_lattice_past_the_launch_caps(gpu):
    from syconn_amd.extraction.cs_processing_steps import OrganelleTable, map_objects_from_synssv_partners
    assert 2 * N > 4096 * 4 and N > 8192
    i = np.arange(N)
    corner = np.stack([40 * (i % 100), 40 * (i // 100), 5 + i % 3], 1)
    blob = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing='ij'), -1).reshape(-1, 3)
    vox = (corner[:, None, :] + blob[None]).reshape(-1, 3).astype(np.uint32)
    partners = np.stack([2 * i + 2, 2 * i + 1], 1).astype(np.uint64)

    class Syn:
        neuron_partners, rep_coords, voxels, vox_begin, sizes = partners, corner.astype(np.int32), vox, 8 * np.arange(N + 1), np.full(N, 8)

        def __len__(self):
            return N
    h = np.where(i % 7 == 0, 600, 100 + 99 * (i % 5)).astype(np.float64)
    base = corner * np.array((10.0, 10.0, 20.0))
    verts = np.repeat(base, 8, 0)
    verts[:, 2] += np.repeat(h, 8) + np.tile(np.arange(8.0), N)
    sizes = 8 * (1 + i % 3)
    order = np.random.default_rng(5).permutation(N)               # table order is not cell order
    table = OrganelleTable((10 ** 6 + i)[order], (2 * i + 1)[order], sizes[order], corner[order], verts.reshape(N, 8, 3)[order].reshape(-1, 3),
                           8 * np.arange(N + 1))
    m, stats = map_objects_from_synssv_partners(Syn(), {'vc': table}, (10, 10, 20), max_vert_dist_nm=R, device=gpu, return_stats=True)
    close = np.where(h == 600, 0, np.where(h == 496, 2, 4))
    pl = m.pairs['vc']
    assert stats['vc']['pairs'] == N and stats['vc']['work_items'] == N
    assert np.array_equal(pl.side_begin, np.arange(2 * N + 1) // 2)                             # one pair on every slot-1 side
    row_of = np.empty(N, np.int64)
    row_of[order] = np.arange(N)
    assert np.array_equal(pl.pair_obj, row_of) and np.array_equal(pl.pair_len, np.full(N, 4)) and np.array_equal(pl.pair_close, close)
    assert np.array_equal(pl.pair_min_d2, np.where(close > 0, h * h, np.inf))
    assert not m.n_vc_objs[:, 0].any() and np.array_equal(m.n_vc_objs[:, 1], (close > 0).astype(np.int32))
    assert np.array_equal(m.n_vc_vxs[:, 1], (close * sizes) // 4) and not m.n_vc_vxs[:, 0].any()
    assert np.array_equal(m.min_dst_vc_nm[:, 1], np.where(close > 0, h, 1e12).astype(np.float32))
    assert np.all(m.min_dst_vc_nm[:, 0] == np.float32(1e12))
