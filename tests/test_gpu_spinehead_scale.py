"""GPU: the smallest inputs that take every kernel of csrc/sd_spinehead.hip (and ``sd_edt_squared``) past one grid stride.  The kernels keep
no LDS table, so the grid caps of include/syconn_dense.h are the only size thresholds:
  SD_SPINEHEAD_VOX_GRID  x 256 = 2 097 152 voxels  -> a window of 129 x 131 x 127 = 2 146 173 voxels (mask, fill, peaks, markers, select);
  SD_SPINEHEAD_ID_GRID   x 256 =   262 144 rows    -> the id tables of that window hold 2 146 173 / 2 + 1026 rows;
  SD_SPINEHEAD_VERT_GRID x 256 =   262 144 pairs   -> 2 windows x 140 000 vertices;
  the query and marker kernels (VOX_GRID)          -> called on their own with 3 x 800 000 query slots / 2 146 173 peaks (a window cannot
                                                      hold that many maxima).
Too large for the restatement's Python flood, so the window is an analytic construction: a lattice of 8 x 8 x 8 separated balls of radius
5 at pitch 16.  Distances, peaks and voxel counts of every ball equal those of ONE ball in a 16^3 block (computed by the restatement),
every ball votes with the vertices at its own centre (label 1 where i + j + k is even, else 2), the head objects are the even balls in
raster order, and the ball around the synapse is chosen by the count, the ball next to a synapse at the origin by the distance.
Also: more windows than the driver's batch size."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _spinehead_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPE, PITCH, RADIUS, NB = (129, 131, 127), 16, 5, 8
N_VERT, MAX_PEAKS = 140000, 4096

Q_SLOTS = 800000


def test_grid_caps_are_passed():
    from syconn_amd import _lib as L
    nvox = SHAPE[0] * SHAPE[1] * SHAPE[2]
    assert nvox > L.SD_SPINEHEAD_VOX_GRID * 256 and nvox // 2 + 1026 > L.SD_SPINEHEAD_ID_GRID * 256
    assert 2 * N_VERT > L.SD_SPINEHEAD_VERT_GRID * 256 and 3 * Q_SLOTS > L.SD_SPINEHEAD_VOX_GRID * 256
    assert nvox < L.SD_SPINEHEAD_VOX_GRID * 256 * 1.05            # ... and by as little as an odd, ragged extent allows
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'syconn_dense.h')).read()
    for name in ('VOX', 'VERT', 'ID'):
        assert f'#define SD_SPINEHEAD_{name}_GRID {getattr(L, f"SD_SPINEHEAD_{name}_GRID")}\n' in hdr


def test_ball_lattice_past_every_grid_stride(gpu):
    import torch
    from syconn_amd.extraction import spinehead as SH
    g = np.indices((PITCH,) * 3) - PITCH // 2
    ball = ((g ** 2).sum(0) <= RADIUS * RADIUS).astype(np.uint8)
    one = R.window_stages(ball.astype(np.uint64) * 5, [5], (1, 1, 1), np.array([[8.5, 8.5, 8.5]]), np.array([1]), np.zeros(3, np.int64), np.array((PITCH,) * 3),
                          (8, 8, 8), np.array([10, 10, 10]), 1)
    assert one['nb_obj'] == 1 and one['n_voxels'] == ball.sum() == 515 and len(one['peaks']) >= 1
    vol = np.zeros(SHAPE, np.uint64)
    d2 = np.zeros(SHAPE, np.int32)
    vol[:NB * PITCH, :NB * PITCH, :NB * PITCH // 1][:, :, :SHAPE[2]] = np.tile(ball, (NB, NB, NB))[:, :, :SHAPE[2]] * np.uint64(5)
    d2[:NB * PITCH, :NB * PITCH, :SHAPE[2]] = np.tile(one['d2'], (NB, NB, NB))[:, :, :SHAPE[2]]
    assert vol[:, :, -1].sum() == 0                               # the last balls end at z = 125: none is cut
    ijk = np.indices((NB,) * 3).reshape(3, -1).T
    even = ijk.sum(1) % 2 == 0
    # vertices: N_VERT of them spread over the ball centres (a small cloud each, inside the ball), labelled by the ball's parity
    rng = np.random.default_rng(11)
    owner = rng.integers(0, len(ijk), N_VERT)
    owner[:len(ijk)] = np.arange(len(ijk))
    verts = ijk[owner] * PITCH + 8.5 + rng.uniform(-0.4, 0.4, (N_VERT, 3))
    labels = np.where(even[owner], 1, 2).astype(np.int32)
    runner = SH.WindowRunner(SHAPE, batch=2, max_peaks=MAX_PEAKS, device=gpu)
    tabs = [torch.arange(n, dtype=torch.int32, device=runner.dev) for n in SHAPE]
    seg_d = torch.from_numpy(vol.view(np.int64)).to(runner.dev)
    sv_d = torch.tensor([5], dtype=torch.int64, device=runner.dev)
    cs = np.array([[40, 40, 40], [5, 5, 5]], np.int64)            # ball (2, 2, 2) by the count; the slice wraps empty: ball (0, 0, 0) by the distance
    keep = []
    res = runner.run_batch(seg_d, (0, 0, 0), np.zeros((2, 3), np.int64), tabs, sv_d, torch.from_numpy(verts).to(runner.dev),
                           torch.from_numpy(labels).to(runner.dev), np.array(SHAPE, np.int32), np.ones(3), 1, cs, np.array([10.0, 10.0, 10.0]), keep)
    n_balls, per_ball = len(ijk), len(one['peaks'])
    rank = np.cumsum(even)                                        # ids of the head objects: the even balls in raster (= lexicographic) order
    for w, ball_ix in ((0, (2 * NB + 2) * NB + 2), (1, 0)):
        assert res[w].tolist() == [n_balls * 515, n_balls * per_ball, 515, rank[ball_ix], int(even.sum()), N_VERT], w
        k = keep[w]
        assert torch.equal(k['filled'], torch.from_numpy((vol > 0).astype(np.uint8)).to(runner.dev))
        assert torch.equal(k['d2'], torch.from_numpy(d2).to(runner.dev))
        want_peaks = (ijk[:, None, :] * PITCH + one['peaks'][None, :, :]).reshape(-1, 3)
        want_peaks = want_peaks[np.lexsort(want_peaks.T[::-1])]
        assert np.array_equal(k['peaks'].cpu().numpy(), want_peaks)
        parity = (want_peaks // PITCH).sum(1) % 2
        assert np.array_equal(k['votes'].cpu().numpy(), np.where(parity == 0, 1, 2))
        flood = k['flood'].cpu().numpy()
        cell_par = (np.indices(SHAPE) // PITCH).sum(0) % 2
        assert np.array_equal(flood, np.where(vol > 0, np.where(cell_par == 0, 1, 2), 0))


def test_more_windows_than_the_batch(gpu):
    g = dict(np.load(os.path.join(HERE, 'golden', 'g22_spinehead.npz')))
    from syconn_amd.extraction import spinehead as SH
    case = R.case_from_golden(g, 'a_')
    cell = case['cells'][0]
    ids, rep = R.synapses_of(case, cell['id'])
    head = R.spinehead_filter(cell, rep, case['scaling'], case['k'], 1, (4, 5), R.AX_KEY)
    ids, rep = ids[head], rep[head]
    verts = np.asarray(cell['vertices'], np.float32) / np.array(case['scaling'])
    sem = cell['vertex_labels']['spiness']
    keep = ~np.isin(sem, (4, 5))
    assert len(ids) >= 5
    runs = [SH.spinehead_windows(case['seg'], cell['sv_ids'], rep, verts[keep], sem[keep], case['scaling'], case['ctx_vol'], case['k'], gpu, batch=b)
            for b in (2, 1, 8)]
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    vols = SH.head_volume(runs[0][:, 2], np.array(case['scaling']), np.array(case['scaling'])[2] // np.array(case['scaling']))
    want = case['expected'][cell['id']]
    assert {int(i): v for i, v, e in zip(ids, vols, runs[0][:, 5]) if e} == want


def test_query_and_marker_kernels_past_one_grid_stride(gpu):
    import ctypes as C
    import torch
    from syconn_amd import _lib as L
    lib = L.load()
    L.check(lib.sd_init(0), 'sd_init')
    stream = torch.cuda.current_stream(gpu).cuda_stream
    rng = np.random.default_rng(4)
    n_win, cap = 3, Q_SLOTS + 5
    peaks = rng.integers(0, 200, (n_win, cap, 3)).astype(np.int32)
    n_peaks = np.array([Q_SLOTS, 17, Q_SLOTS + 5], np.int32)     # full, nearly empty, more peaks than slots
    ds = (2.0, 2.0, 1.0)
    p_d, n_d = torch.from_numpy(peaks).to(gpu), torch.from_numpy(n_peaks).to(gpu)
    q_cell = torch.empty(n_win * Q_SLOTS, dtype=torch.int32, device=gpu)
    q_xyz = torch.empty((n_win * Q_SLOTS, 3), dtype=torch.float64, device=gpu)
    L.check(lib.sd_spinehead_queries(p_d.data_ptr(), n_d.data_ptr(), n_win, cap, Q_SLOTS, (C.c_double * 3)(*ds), q_cell.data_ptr(), q_xyz.data_ptr(), stream),
            'sd_spinehead_queries')
    live = np.arange(Q_SLOTS)[None, :] < n_peaks[:, None]
    assert np.array_equal(q_cell.cpu().numpy().reshape(n_win, Q_SLOTS), np.where(live, np.arange(n_win)[:, None], n_win))
    assert np.array_equal(q_xyz.cpu().numpy().reshape(n_win, Q_SLOTS, 3), np.where(live[..., None], peaks[:, :Q_SLOTS] * np.array(ds), 0.0))
    assert lib.sd_spinehead_queries(p_d.data_ptr(), n_d.data_ptr(), n_win, cap, cap + 1, (C.c_double * 3)(*ds), q_cell.data_ptr(), q_xyz.data_ptr(), stream) == L.SD_ERR_INVALID
    # markers: every voxel of the 2.1 M voxel window a peak, in a shuffled order
    nvox = SHAPE[0] * SHAPE[1] * SHAPE[2]
    order = rng.permutation(nvox)
    pk = np.stack(np.unravel_index(order, SHAPE), 1).astype(np.int32)
    votes = rng.integers(-1, 10, nvox).astype(np.int32)
    markers = torch.empty(SHAPE, dtype=torch.int32, device=gpu)
    L.check(lib.sd_spinehead_markers(torch.from_numpy(pk).to(gpu).data_ptr(), torch.tensor([nvox], dtype=torch.int32, device=gpu).data_ptr(),
                                     torch.from_numpy(votes).to(gpu).data_ptr(), nvox, *SHAPE, markers.data_ptr(), stream), 'sd_spinehead_markers')
    want = np.zeros(nvox, np.int32)
    want[order] = np.maximum(votes, 0)
    assert np.array_equal(markers.cpu().numpy().ravel(), want)
