"""CPU: the restatement of the rendering locations (tests/_locations_ref.py) against what the reference's own ``surface_samples``
returned (tests/golden/g28_locations.npz), bit for bit; the voxel rule on hand-computed cases; the argument checks of the host layer
that need no device; the new entries fail loudly without a GPU."""
import os

import numpy as np
import pytest

import _locations_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(HERE, 'golden', 'g28_locations.npz'))


def test_surface_restatement_equals_the_reference_bit_for_bit(gold):
    assert int(gold['n']) == 6
    for k in range(int(gold['n'])):
        got = R.surface_samples(gold[f's{k}_verts'], gold[f's{k}_bins'], r=float(gold[f's{k}_r']))
        want = gold[f's{k}_out']
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f'cloud {k}'
        assert np.array_equal(got, R.surface_samples(gold[f's{k}_verts'], gold[f's{k}_bins'], max_nb_samples=1, r=float(gold[f's{k}_r'])))


def test_voxel_rule_by_hand():
    # ds = 10, vmin = -5: x = 4.5 is voxel 0, x = 5 lies on the boundary and belongs to voxel 1, x = 14.5 too, x = 15 is voxel 2
    v = np.array([[15, 0, 0], [0, 0, 0], [5, 0, 0], [4.5, 0, 0], [14.5, 0, 0]], np.float64)
    got = R.generate_rendering_locs(v, 10)
    assert got.dtype == np.float64
    assert np.array_equal(got, [[(0 + 4.5) / 2, 0, 0], [(5 + 14.5) / 2, 0, 0], [15, 0, 0]])
    # the order: x most significant, then y, then z
    v = np.array([[0, 0, 20], [0, 20, 0], [20, 0, 0], [0, 0, 0]], np.float32)
    assert np.array_equal(R.generate_rendering_locs(v, 10), [[0, 0, 0], [0, 0, 20], [0, 20, 0], [20, 0, 0]])
    # all in one voxel: the mean, added in vertex order; one voxel per vertex: the vertices, sorted
    v = np.array([[1, 2, 3], [2, 4, 6], [6, 6, 6]], np.float64)
    assert np.array_equal(R.generate_rendering_locs(v, 100), [[3, 4, 5]])
    assert np.array_equal(R.generate_rendering_locs(v[::-1], 0.5), v)
    assert R.generate_rendering_locs(np.zeros((0, 3)), 5).shape == (0, 3)
    # a voxel size float32 does not hold: the division is float64's
    v = np.array([[0, 0, 0], [500.05, 0, 0], [500.04, 0, 0]], np.float64)
    assert np.array_equal(R.generate_rendering_locs(v, 1000.1), [[500.04 / 2, 0, 0], [500.05, 0, 0]])


def test_voxel_rule_errors_and_limit():
    v = np.array([[0, 0, 0], [R.MAX_CELLS - 1, 0, 0]], np.float64)
    assert len(R.generate_rendering_locs(v, 1.0)) == 2                             # voxel 2^21 - 1: the last one the key holds
    v[1, 0] = R.MAX_CELLS
    with pytest.raises(ValueError):
        R.generate_rendering_locs(v, 1.0)
    for ds in (0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            R.generate_rendering_locs(np.zeros((2, 3)), ds)
    with pytest.raises(ValueError):
        R.generate_rendering_locs(np.array([[0, np.nan, 0]]), 1.0)


def test_in_order_sums_are_not_pairwise_sums():
    """What gives the sum tests of the GPU suite their teeth: the sequential sums differ from numpy's pairwise ones."""
    rng = np.random.default_rng(1)
    p = rng.uniform(0, 1, (5000, 3)) + 1e6
    pair = np.array([np.sum(np.ascontiguousarray(p[:, a])) for a in range(3)])
    assert not np.array_equal(R.seq_sum(p, np.float64), pair)
    q = p.astype(np.float32)
    assert not np.array_equal(R.seq_sum(q, np.float32), np.array([np.sum(np.ascontiguousarray(q[:, a])) for a in range(3)]))


def test_host_argument_checks():
    from syconn_amd.handler.multiviews import generate_rendering_locs
    from syconn_amd.proc.locations import LocationTable, sample_locations_table
    from syconn_amd.reps.rep_helper import surface_samples
    v = np.zeros((4, 3), np.float32)
    for ds in (0, -2000, np.nan, np.inf, (1, 2, 3)):
        with pytest.raises(ValueError):
            generate_rendering_locs(v, ds)
        with pytest.raises(ValueError):
            sample_locations_table((np.arange(1), [0, 4], v), ds_factor=ds)
    bad = v.copy()
    bad[2, 1] = np.inf
    with pytest.raises(ValueError):
        generate_rendering_locs(bad, 10)
    with pytest.raises(ValueError):
        surface_samples(bad)
    with pytest.raises(NotImplementedError):
        surface_samples(v.astype(np.float64))
    with pytest.raises(ValueError):
        surface_samples(v[:0])
    for kw in (dict(bin_sizes=(0, 1, 1)), dict(bin_sizes=(1, 1)), dict(bin_sizes=(1, np.nan, 1)), dict(r=-1), dict(r=np.inf)):
        with pytest.raises(ValueError):
            surface_samples(v, **kw)
    with pytest.raises(ValueError):                                                # offsets that do not match the ids / the vertices
        sample_locations_table((np.arange(2), [0, 4], v))
    with pytest.raises(ValueError):
        sample_locations_table((np.arange(1), [0, 3], v))
    with pytest.raises(ValueError):
        sample_locations_table((np.arange(2), [0, 5, 4], v))
    with pytest.raises(ValueError):                                                # an empty object without rep_coords / scaling
        sample_locations_table((np.arange(2), [0, 0, 4], v))
    with pytest.raises(ValueError):
        sample_locations_table((np.arange(2), [0, 0, 4], v), rep_coords=np.zeros((2, 3)))
    with pytest.raises(NotImplementedError):
        sample_locations_table((np.arange(1), [0, 4], v.astype(np.float64)), use_new_renderings_locs=False)
    with pytest.raises(ValueError):
        sample_locations_table(v)
    with pytest.raises(ValueError):
        LocationTable(np.arange(2), [0, 1], np.zeros((1, 3), np.float32))
    t = LocationTable([7, 3], [0, 2, 3], np.arange(9, dtype=np.float32).reshape(3, 3))
    loc, begin = t.locations_of([3, 5, 7, 3])
    assert begin.tolist() == [0, 1, 1, 3, 4] and np.array_equal(loc, t.locations[[2, 0, 1, 2]])
    assert len(t) == 2 and np.array_equal(t.as_dict()[7], t.locations[:2])


def test_config_key():
    from syconn_amd import global_params
    assert global_params.config['views']['use_new_renderings_locs'] is True


def test_entries_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is visible')
    from syconn_amd.handler.multiviews import generate_rendering_locs
    from syconn_amd.proc.locations import sample_locations_table
    from syconn_amd.proc.rendering import render_sampled_views
    from syconn_amd.reps.rep_helper import surface_samples
    from syconn_amd.reps.super_segmentation_helper import sample_locations_sso
    v = np.zeros((4, 3), np.float32)

    class Sv:
        mesh, rep_coord, scaling = [np.zeros(0, np.uint32), v.reshape(-1), np.zeros(0, np.float32)], (0, 0, 0), (10, 10, 20)

    class Cell:
        svs, mesh = [Sv()], Sv.mesh

    for call in (lambda: generate_rendering_locs(v, 10), lambda: surface_samples(v), lambda: sample_locations_table((np.arange(1), [0, 4], v)),
                 lambda: sample_locations_sso(Cell()), lambda: render_sampled_views(Cell())):
        with pytest.raises(RuntimeError):
            call()
