"""GPU: ``sd_spinehead_select`` called directly through the C ABI on hand-built ``flood`` volumes (tests/_spinehead_select_cases.py)
against ``select_head`` of tests/_spinehead_ref.py, which states the selection in the reference's own words
(``reps/super_segmentation_helper.py:2171-2196``): the nearest-object branch with non-integer voxel sizes, exact ties, window offsets and
near-ties that the reference's rounding decides; numpy's wrap-once-then-clip slice on every axis with the count rule; degenerate and
dense inputs.  Every comparison is an equality.  The workspace of every call is followed by a guard band that must stay untouched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _spinehead_ref as R  # noqa: E402
import _spinehead_select_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 4096
IDS = [n for n, _ in K.SCALINGS]


class Select:
    """Queues calls on the current stream; the results of all of them come back in one copy (``results``)."""

    def __init__(self, gpu, n_calls):
        import torch
        from syconn_amd import _lib as L
        self.torch, self.L, self.lib, self.gpu = torch, L, L.load(), gpu
        self.res = torch.full((n_calls, 3), -7, dtype=torch.int32, device=gpu)
        self.n, self.ws, self.held = 0, {}, []

    def workspace(self, shape):
        if shape not in self.ws:
            nb = int(self.lib.sd_spinehead_workspace_bytes(*shape))
            assert nb > 0
            ws = self.torch.empty(nb + GUARD, dtype=self.torch.uint8, device=self.gpu)
            ws[nb:] = 0xA5
            self.ws[shape] = (ws, nb)
        return self.ws[shape]

    def __call__(self, case, objects=False):
        torch = self.torch
        flood = torch.from_numpy(np.ascontiguousarray(case['flood'], dtype=np.int32)).to(self.gpu)
        shape = tuple(int(v) for v in flood.shape)
        ws, nb = self.workspace(shape)
        obj = torch.full(shape, -7, dtype=torch.int32, device=self.gpu) if objects else None
        i64x3 = lambda v: (C.c_int64 * 3)(*[int(x) for x in v])
        sc = (C.c_double * 3)(*[float(x) for x in np.asarray(case['scaling']).astype(np.float64)])      # (a float32 size widens exactly)
        self.L.check(self.lib.sd_spinehead_select(flood.data_ptr(), *shape, i64x3(case['c']), i64x3(case['offset']), sc,
                                                  None if obj is None else obj.data_ptr(), self.res[self.n].data_ptr(), ws.data_ptr(), nb,
                                                  torch.cuda.current_stream().cuda_stream), 'sd_spinehead_select')
        self.held.append(flood)
        self.n += 1
        return obj

    def results(self):
        """-> (calls, 3) int64: voxels of the chosen object, the chosen id, nb_obj; checks every guard band."""
        out = self.res[:self.n].cpu().numpy().astype(np.int64)
        for shape, (ws, nb) in self.ws.items():
            assert bool((ws[nb:] == 0xA5).all()), f'sd_spinehead_select wrote behind sd_spinehead_workspace_bytes{shape}'
        return out


def expected(case):
    info = {}
    objects, nb_obj, chosen, n_vox = R.select_head(case['flood'], case['c'], case['offset'], case['scaling'], info)
    return info, objects, [n_vox, chosen, nb_obj]


def report(name, what, got, want):
    """The figure a failing run is read for: how many cases differ."""
    bad = [i for i in range(len(want)) if got[i].tolist() != want[i]]
    print(f'{what} [{name}]: {len(bad)} of {len(want)} cases differ' + (f', first {bad[0]}: got {got[bad[0]].tolist()}, want {want[bad[0]]}' if bad else ''))
    return bad


@pytest.mark.parametrize('name,scaling', K.SCALINGS, ids=IDS)
def test_mirrored_exact_ties_give_the_lowest_id(gpu, name, scaling):
    """B1: window offset 0, c = (30, 30, 4), single voxels at c + (a, b, k) and c + (b, a, k).  Exact ties in the reference's arithmetic
    (asserted through the restatement, not assumed): id 1 and one voxel, for every pair.  A fused sum tells the two apart by one ulp."""
    cases = K.mirrored((30, 30, 4), (0, 0, 0), scaling, K.N_MIRRORED, seed=1)
    assert len(cases) >= 100
    run = Select(gpu, len(cases))
    for case in cases:
        info, _, want = expected(case)
        assert info['branch'] == 'nearest' and not info['decided'] and want == [1, 1, 2]
        run(case)
    got = run.results()
    assert not report(name, 'mirrored ties', got, [[1, 1, 2]] * len(cases))


@pytest.mark.parametrize('name,scaling', K.SCALINGS, ids=IDS)
def test_nearest_object_with_window_offsets(gpu, name, scaling):
    """B2: 2 to 6 random objects around an unsymmetric c, window offsets of real size: every case decided in the reference's arithmetic,
    the expected id cKDTree's.  Then the near-ties: mirrored pairs around an unsymmetric c or behind an offset, where the reference's own
    rounding of the scaled points decides (or, where its products are exact, the tie stays and the lowest id is due)."""
    cases = [K.random_objects(seed, off, scaling) for off in K.OFFSETS for seed in K.RANDOM_SEEDS]
    n_random = len(cases)
    for c, off in K.NEAR_TIES:
        cases += K.mirrored(c, off, scaling, K.N_NEAR, seed=2)
    run = Select(gpu, len(cases))
    want = []
    for i, case in enumerate(cases):
        info, _, w = expected(case)
        assert info['branch'] == 'nearest'
        if i < n_random:
            assert info['decided'] and w[1] == info['ref_id'], (name, i)
        want.append(w)
        run(case)
    got = run.results()
    bad = report(name, 'random objects', got[:n_random], want[:n_random]) + report(name, 'near-ties', got[n_random:], want[n_random:])
    assert not bad


def test_slice_rule(gpu):
    """B3: extents from {9, 17, 20, 21, 22, 33} and every c component that meets a bound of ``c - 10 : c + 11`` on every axis; blobs of
    flood 1 among voxels of flood 0, 2 and 9.  Chosen id, voxel count, nb_obj and the objects volume are ``select_head``'s; the directed
    cases also give what was worked out by hand."""
    directed = K.directed_slice_cases()
    cases = [case for _, case, _ in directed] + K.slice_cases()
    run = Select(gpu, len(cases))
    want, objs = [], []
    for case in cases:
        info, objects, w = expected(case)
        want.append(w)
        objs.append((objects, run(case, objects=True)))
    got = run.results()
    for i, (name, _, hand) in enumerate(directed):
        assert got[i].tolist() == [hand[1], hand[0], hand[2]] == want[i], name
    assert not report('slice', 'slice rule', got, want)
    for i, (objects, obj_d) in enumerate(objs):
        assert np.array_equal(obj_d.cpu().numpy(), objects), i


def test_degenerate_and_dense(gpu):
    """B4: no voxel of flood 1: [0, 1, 0]; one object: id 1 wherever c is; the 16^3 checkerboard: 2048 objects of one voxel, 32 distinct
    labels in every wave of the counting kernel, the chosen id once by the slice and once by the distance."""
    sc, off = np.array(K.VOXEL_SIZES[0], np.float64), np.array(K.OFFSETS[0], np.int64)
    case = lambda flood, c: dict(flood=flood, c=np.array(c, np.int64), offset=off, scaling=sc)
    none = np.zeros((21, 9, 17), np.int32)
    none[3:6, 2, 1:9] = 2
    none[10, 4, 4] = 9
    one = np.zeros((21, 9, 17), np.int32)
    one[2:5, 1:4, 3] = 1
    one[4, 3, 3:12] = 1
    one[15, 5, 5] = 2
    cs = [(0, 0, 0), (3, 2, 5), (10, 4, 8), (20, 8, 16), (11, 3, 3), (40, 40, 40), (-30, 2, 2)]
    board = K.checkerboard()
    cases = [case(none, c) for c in cs[:3]] + [case(one, c) for c in cs] + [case(board, (12, 12, 12)), case(board, (40, 38, 7))]
    run = Select(gpu, len(cases))
    objs = [run(c, objects=True) for c in cases]
    got = run.results()
    assert got[:3].tolist() == [[0, 1, 0]] * 3
    assert got[3:3 + len(cs)].tolist() == [[17, 1, 1]] * len(cs)
    for c, o in zip(cases[:-2], objs[:-2]):
        assert np.array_equal(o.cpu().numpy(), ndimage.label(c['flood'] == 1)[0])
    labels, nb = ndimage.label(board == 1)
    assert nb == 2048
    for i in (-2, -1):
        info, objects, want = expected(cases[i])
        assert info['branch'] == ('slice', 'nearest')[i] and want[0] == 1 and want[2] == 2048 and want[1] > 1
        assert got[i].tolist() == want
        o = objs[i].cpu().numpy()
        assert np.array_equal(o, labels) and np.array_equal(np.bincount(o.ravel())[1:], np.ones(2048, np.int64))      # all counts are 1
    assert labels[2, 2, 2] == got[-2, 1]                          # the lowest id inside [2:16]^3 among equal counts
