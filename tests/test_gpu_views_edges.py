"""GPU: the raster of csrc/sd_views.hip on its own structure edges (tests/_views_edge_cases.py; tests/test_views_edges_cpu.py shows on
the CPU that each input sits where it claims) -- depth and index views bit for bit against the numpy restatement (tests/_views_ref.py),
through the C ABI with a guard band behind every buffer (tests/_views_gpu.py)."""
import os

import numpy as np
import pytest

import _views_edge_cases as EC
import _views_gpu as G
import _views_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g27_views.npz')
SD_OK, SD_ERR_INVALID = 0, -1


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def run(gpu, case, index, mesh=None):
    """The case on the device, compared with the restatement -> (views, the restatement's views, the mesh)."""
    m = G.Mesh(gpu, case.v, case.t, np.zeros(3), 1.0) if mesh is None else mesh
    assert m.rc == SD_OK and not m.counts.any()
    want, dropped = case.ref(index)
    rc, c, got = m.render(case.coords, case.rot, R.EDGE_CW, case.nb_views, case.ws, index=index, cos_sin=case.cos_sin)
    assert rc == SD_OK and c[2] == dropped and c[3] == 0
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), f'{(got != want).sum()} of {got.size} pixels differ'
    return got, want, m


# ---- 1. the tiled all-zero rule: k_vw_zero_rule writes, and only the views whose every tile is zero ----------------------------------------
@pytest.mark.parametrize('name', EC.NAMES['zero_rule'])
def test_tiled_zero_rule(gpu, name):
    got, _, _ = run(gpu, EC.cases('zero_rule')[name], False)
    if name == 'all_zero':
        assert (got == 255).all()
    elif name == 'corner_nonzero':
        assert (got == 0).sum() == 33120                                            # the zeros of three all-zero tiles stay zeros
    else:
        assert (got[0] == 255).all() and (got[1] == 0).sum() == 33120 * got.shape[1] and (got[2] == 255).all()


# ---- 2. the 2^22 bound and the depth cut-off, exactly --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', EC.NAMES['bound'])
@pytest.mark.parametrize('index', [False, True])
def test_exact_bounds(gpu, name, index):
    case = EC.cases('bound')[name]
    got, _, _ = run(gpu, case, index)
    dropped = case.ref(index)[1]
    bg = R.BG_INDEX if index else 255
    if name == 'at_bound':
        assert dropped == 1 and (not index or (got != bg).sum() == 36)
    if name == 'below_bound':
        assert dropped == 0 and (not index or (got != bg).all())
    if name == 'at_bound_tiled':
        assert dropped == len(case.coords) * case.nb_views                          # once per (location, view), not once per tile
    if name == 'last_depth':
        assert (got != bg).sum() == (36 if index else 0)
    if name == 'past_last_depth':
        assert (got == bg).all()


# ---- 3. a pixel box of 64 samples is drawn by one lane, of 65 by the wave ------------------------------------------------------------------
@pytest.mark.parametrize('name', EC.NAMES['split'])
@pytest.mark.parametrize('index', [False, True])
def test_lane_or_wave(gpu, name, index):
    got, _, _ = run(gpu, EC.cases('split')[name], index)
    if index:
        assert (got != R.BG_INDEX).sum() == (64 if name == 'box_64' else 65)


# ---- 4. large triangles and depth ties across the tile seams -------------------------------------------------------------------------------
@pytest.mark.parametrize('name', EC.NAMES['seam'])
@pytest.mark.parametrize('index', [False, True])
def test_seams_under_large_triangles(gpu, name, index):
    got, _, _ = run(gpu, EC.cases('seam')[name], index)
    if index and name == 'coplanar':
        assert set(np.unique(got)) == {2, 7, R.BG_INDEX}                            # the lower-numbered triangle keeps a tie, in every tile


# ---- 5. more candidates than the block has threads -----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lattice(gpu):
    return G.Mesh(gpu, *EC.lattice_mesh(), np.zeros(3), 1.0)


@pytest.mark.parametrize('ws', EC.LATTICE_WS)
@pytest.mark.parametrize('index', [False, True])
def test_candidate_loop_runs_more_than_once(gpu, lattice, ws, index):
    case = EC.lattice_case(ws)
    rc, c, begin, cand, _, _ = lattice.candidates(case.coords, case.E)
    print(f'lattice: candidates per location {np.diff(begin.astype(np.int64)).tolist()} of {len(lattice.tris)} triangles')
    assert rc == SD_OK and c[1] == 0 and (np.diff(begin.astype(np.int64)) > 1024).all()       # more than the largest block
    run(gpu, case, index, mesh=lattice)


# ---- 6. windows narrower than the filter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ws', EC.TINY_WS)
@pytest.mark.parametrize('index', [False, True])
def test_tiny_windows(gpu, ws, index):
    for name in EC.TINY_NAMES:
        run(gpu, EC.tiny_case(name, ws), index)


# ---- 7. view counts ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tube(gpu, gold):
    g = gold
    return G.Mesh(gpu, g['m_verts'], g['m_tris'], g['m_center'], g['m_max_dist'])


@pytest.mark.parametrize('nb_views', [2, 16])
@pytest.mark.parametrize('index', [False, True])
def test_two_and_sixteen_views(gold, tube, nb_views, index):
    g = gold
    want, dropped = EC.tube_ref(g, nb_views, index)
    rc, c, got = tube.render(g['m_coords'][:2], g['m_rot'][:2], float(g['m_comp_window']), nb_views, (32, 16), index=index)
    assert rc == SD_OK and c[2] == dropped == 0 and c[3] == 0
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)
    assert len(np.unique(got.reshape(2 * nb_views, -1), axis=0)) == 2 * nb_views


@pytest.mark.parametrize('index', [False, True])
def test_seventeen_views_are_refused(gold, tube, index):
    g = gold
    rc, c, _ = tube.render(g['m_coords'][:2], g['m_rot'][:2], float(g['m_comp_window']), 17, (32, 16), index=index)
    assert rc == SD_ERR_INVALID
