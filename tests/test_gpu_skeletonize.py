"""GPU: every stage of the skeletonisation chain (csrc/sd_skeletonize.hip through proc/skeleton.py) against the CPU restatement of the
same rules (tests/_skeletonize_ref.py), bit for bit, on the cases of tests/_skeletonize_cases.py; limits, guard bands and argument errors."""
import ctypes as C_
import os

import numpy as np
import pytest

import _skeletonize_cases as C
import _skeletonize_ref as R

pytestmark = pytest.mark.gpu
CASES = {c[0]: c for c in C.cases()}
_REF, _DEV = {}, {}


def ref(name):
    if name not in _REF:
        _, seg, kw, _ = CASES[name]
        kw = dict(kw)
        _REF[name] = R.skeletonize(seg, kw.pop('w'), **kw)
    return _REF[name]


def dev_kwargs(kw):
    kw = dict(kw)
    return dict(anisotropy=kw.pop('w'), dust_threshold=kw.pop('dust_threshold'), max_paths=kw.pop('max_paths'), teasar_params=kw)


def dev(name):
    from syconn_amd.proc.skeleton import trace_chunk
    if name not in _DEV:
        stages = {}
        out = trace_chunk(CASES[name][1], stages=stages, **dev_kwargs(CASES[name][2]))
        _DEV[name] = (out, stages)
    return _DEV[name]


def bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f'{what}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}'
    assert a.tobytes() == b.tobytes(), f'{what}: {int((a.view(np.uint8) != b.view(np.uint8)).sum())} bytes differ'


@pytest.mark.parametrize('name', list(CASES))
def test_components_and_distance_to_boundary(name):
    r, (_, s) = ref(name), dev(name)
    for k in ('comp', 'sizes', 'labels', 'first', 'd2', 'dbf', 'dbf_max'):
        bits(s[k], r[k], k)


@pytest.mark.parametrize('name', list(CASES))
def test_roots_and_fields(name):
    r, (_, s) = ref(name), dev(name)
    for k in ('daf0', 'root', 'daf', 'daf_max', 'p'):
        a, b = s[k], r[k]
        if k == 'root':
            a, b = a[1:], b[1:]
        bits(a, b, k)


@pytest.mark.parametrize('name', list(CASES))
def test_rounds_targets_dist_and_valid(name):
    r, (_, s) = ref(name), dev(name)
    assert len(s['targets']) == len(r['targets'])
    for k in range(len(r['targets'])):      # after 1, 2, ... and all rounds
        bits(s['targets'][k][1:], r['targets'][k][1:], f'targets of round {k + 1}')
        bits(s['dist_rounds'][k], r['dist_rounds'][k], f'dist after round {k + 1}')
        bits(s['valid_rounds'][k], r['valid_rounds'][k], f'valid after round {k + 1}')
    bits(s['parent'], r['parent'], 'parent')


@pytest.mark.parametrize('name', list(CASES))
def test_nodes_edges_radii(name):
    r, (o, _) = ref(name), dev(name)
    n = len(r['sizes']) - 1
    assert o['absorbed'] == 0 and not o['void'].any() and len(o['node_begin']) == n + 1
    for c in range(1, n + 1):
        n0, n1, e0, e1 = o['node_begin'][c - 1], o['node_begin'][c], o['edge_begin'][c - 1], o['edge_begin'][c]
        bits(o['node_voxel'][n0:n1].astype(np.int64), r['nodes'][c], f'nodes of {c}')
        bits(o['edges'][e0:e1], r['edges'][c], f'edges of {c}')
        bits(o['radii'][n0:n1], r['radii'][c], f'radii of {c}')
        bits(o['vertices'][n0:n1], r['vertices'][c], f'vertices of {c}')


def test_relaxation_statistics_are_reported():
    o, _ = dev('tile_seams')
    assert len(o['stats']) == 3 + len(ref('tile_seams')['targets']) and all(sw >= 1 and tiles >= sw for sw, tiles in o['stats'])
    assert max(sw for sw, _ in o['stats']) > 2      # the tube crosses seams: more than one sweep over its tiles


# ---- limits -------------------------------------------------------------------------------------------------------------------------------
def test_capacities_one_short_with_guard_bands(monkeypatch):
    """max_comps and max_nodes one below the need raise with the need; every output and scratch buffer of the chain is followed by a band
    of poison that must come back untouched (also from the runs that stop at the capacity)."""
    import torch
    from syconn_amd import _dev as D
    from syconn_amd.proc.skeleton import trace_chunk
    bands = []

    def guarded(n, dtype, dev_):
        shape = n if isinstance(n, tuple) else (n,)
        rows = max(shape[0], 1)
        per = int(np.prod(shape[1:])) if len(shape) > 1 else 1
        guard = 64
        full = torch.empty((rows + guard) * per, dtype=dtype, device=dev_)
        full.view(torch.uint8)[:] = 0xA5
        bands.append(full[rows * per:])
        return full[:rows * per].view((rows,) + tuple(shape[1:]))

    def guarded_copy(t):
        g = guarded(tuple(t.shape), t.dtype, t.device)
        g.copy_(t)
        return g

    up, counters = D.up, D.counters
    monkeypatch.setattr(D, 'empty', guarded)
    monkeypatch.setattr(D, 'up', lambda a, dev_: guarded_copy(up(a, dev_)))                  # the uploaded tables (seg, M, the lookup)
    monkeypatch.setattr(D, 'counters', lambda dev_, n=8: guarded_copy(counters(dev_, n)))      # the count blocks
    monkeypatch.setattr(D, 'scratch', lambda name, dev_, *sizes: guarded(max(int(getattr(D.L.load(), name)(*sizes)), 1), torch.uint8, dev_))
    _, seg, kw, _ = CASES['multi_label']
    r = ref('multi_label')
    need_nodes = sum(len(x) for x in r['nodes'][1:])
    with pytest.raises(RuntimeError, match=f'{len(r["sizes"]) - 1} components'):
        trace_chunk(seg, max_comps=len(r['sizes']) - 2, **dev_kwargs(kw))
    with pytest.raises(RuntimeError, match=f'{need_nodes} nodes'):
        trace_chunk(seg, max_nodes=need_nodes - 1, **dev_kwargs(kw))
    o = trace_chunk(seg, max_comps=len(r['sizes']) - 1, max_nodes=need_nodes, **dev_kwargs(kw))
    assert len(o['node_voxel']) == need_nodes
    bits(o['node_voxel'].astype(np.int64), np.concatenate(r['nodes'][1:]), 'nodes at the exact capacity')
    # the same results over buffers that start as 0xA5 (here) and as whatever the allocator hands out (the cached run): nothing is read before it is written
    stages = {}
    again = trace_chunk(CASES['tile_seams'][1], stages=stages, **dev_kwargs(CASES['tile_seams'][2]))
    first, first_stages = dev('tile_seams')
    for k in ('node_begin', 'edge_begin', 'node_voxel', 'vertices', 'radii', 'edges'):
        bits(again[k], first[k], k)
    for k in ('d2', 'daf', 'p', 'parent'):
        bits(stages[k], first_stages[k], k)
    bits(stages['dist_rounds'][-1], first_stages['dist_rounds'][-1], 'dist')
    torch.cuda.synchronize()
    assert len(bands) > 20
    for b in bands:
        assert bool((b.view(torch.uint8) == 0xA5).all()), 'a guard band was written'


def test_a_component_without_boundary_is_an_error():
    from syconn_amd.proc.skeleton import trace_chunk
    with pytest.raises(ValueError, match='no voxel of another component'):
        trace_chunk(np.ones((3, 4, 5), np.uint64), (1, 1, 1), dust_threshold=1)


def test_empty_and_all_dust_volumes():
    from syconn_amd.proc.skeleton import skeletonize_chunk_table, trace_chunk
    o = trace_chunk(np.zeros((3, 4, 5), np.uint64), (1, 1, 1))
    assert len(o['labels']) == 0 and o['node_begin'].tolist() == [0]
    assert len(skeletonize_chunk_table(CASES['minimal'][1], (1, 1, 1), dust_threshold=3)) == 0


# ---- argument errors: rejected before anything is launched ---------------------------------------------------------------------------------
def test_every_argument_error():
    import torch
    from syconn_amd import _dev as D
    from syconn_amd import _lib as L
    dev_ = D.device()
    lib = L.load()
    X, Y, Z, n = 4, 5, 6, 2
    nv = X * Y * Z
    t = {k: torch.zeros(nv, dtype=dt, device=dev_) for k, dt in (('seg', D.i64), ('comp', D.i32), ('d2', D.i64), ('dbf', torch.float32), ('f64', D.f64), ('u8', D.u8))}
    tab = {k: torch.zeros(n + 2, dtype=dt, device=dev_) for k, dt in (('i64', D.i64), ('i32', D.i32), ('f32', torch.float32), ('f64', D.f64))}
    big = torch.zeros(64, dtype=D.i64, device=dev_)
    counts = D.counters(dev_)
    temp = D.scratch('sd_skeletonize_temp_bytes', dev_, X, Y, Z)
    etemp = D.scratch('sd_skeletonize_emit_temp_bytes', dev_, 8)
    w, w0, wbig = D.i32x3((1, 1, 1)), D.i32x3((1, 0, 1)), D.i32x3((1, 1, L.SD_SKELETONIZE_MAX_ANISOTROPY + 1))
    P = lambda x: x.data_ptr()
    cap = L.SD_SKELETONIZE_MAX_EXTENT

    def comps(seg=P(t['seg']), dims=(X, Y, Z), comp=P(t['comp']), cap_=n, tb=temp.numel(), tp=P(temp), cnt=P(counts)):
        return lib.sd_skeletonize_components(seg, *dims, 1, comp, P(tab['i64']), P(tab['i64']), P(tab['i32']), cap_, cnt, tp, tb, 0)

    def d2(dims=(X, Y, Z), w_=w, tb=temp.numel(), out=P(t['d2'])):
        return lib.sd_skeletonize_d2(P(t['comp']), *dims, w_, n, out, P(t['dbf']), P(tab['f32']), P(counts), P(temp), tb, 0)

    def start(dims=(X, Y, Z), f64=0, src=P(tab['i32']), tb=temp.numel()):
        return lib.sd_skeletonize_field_start(P(t['comp']), *dims, src, n, P(t['f64']), f64, P(temp), tb, 0)

    def relax(dims=(X, Y, Z), w_=w, sweeps=6, field=P(t['f64']), tb=temp.numel()):
        return lib.sd_skeletonize_relax(P(t['comp']), *dims, w_, field, None, sweeps, P(counts), P(temp), tb, 0)

    def argmax(nvox=nv, keys=P(big), idx=P(tab['i32'])):
        return lib.sd_skeletonize_argmax(P(t['comp']), P(t['dbf']), None, nvox, n, idx, None, keys, 0)

    def pen(e=4, scale=1.0, m=P(tab['f64']), nvox=nv):
        return lib.sd_skeletonize_penalty(P(t['comp']), P(t['dbf']), P(t['dbf']), nvox, n, m, P(tab['f32']), scale, e, P(t['f64']), 0)

    def rnd(dims=(X, Y, Z), w_=w, n_=n, scale=1.0, const=0.0, tgt=P(tab['i32']), tb=temp.numel()):
        return lib.sd_skeletonize_round(P(t['comp']), *dims, w_, P(t['dbf']), P(t['f64']), P(t['u8']), P(t['comp']), tgt, None, P(tab['i64']), n_, scale, const,
                                        P(tab['i32']), P(counts), P(temp), tb, 0)

    def emit(dims=(X, Y, Z), w_=w, n_=n, cap_=8, tb=temp.numel(), eb=etemp.numel(), root=P(tab['i32'])):
        return lib.sd_skeletonize_emit(P(t['comp']), *dims, w_, P(t['comp']), P(t['dbf']), root, P(tab['i32']), n_, cap_, P(big), P(big), P(big), P(big), P(big),
                                       P(big), P(counts), P(temp), tb, P(etemp), eb, 0)

    bad = [comps(seg=None), comps(comp=None), comps(cnt=None), comps(dims=(0, Y, Z)), comps(dims=(cap + 1, 1, 1)), comps(cap_=0), comps(tb=temp.numel() - 1), comps(tp=None),
           d2(dims=(X, 0, Z)), d2(dims=(1, cap + 1, 1)), d2(w_=w0), d2(w_=wbig), d2(w_=None), d2(tb=0), d2(out=None),
           start(dims=(X, Y, -1)), start(f64=2), start(src=None), start(tb=0),
           relax(dims=(X, Y, cap + 1)), relax(w_=w0), relax(sweeps=0), relax(sweeps=L.SD_SKELETONIZE_MAX_SWEEPS + 1), relax(field=None), relax(tb=0),
           argmax(nvox=0), argmax(nvox=2 ** 31), argmax(keys=None), argmax(idx=None),
           pen(e=0), pen(e=L.SD_SKELETONIZE_MAX_EXPONENT + 1), pen(scale=-1.0), pen(scale=float('nan')), pen(m=None), pen(nvox=0),
           rnd(dims=(0, 0, 0)), rnd(w_=wbig), rnd(n_=0), rnd(scale=-1.0), rnd(scale=float('inf')), rnd(const=float('nan')), rnd(tgt=None), rnd(tb=0),
           emit(dims=(X, cap + 1, Z)), emit(w_=w0), emit(n_=0), emit(cap_=0), emit(tb=0), emit(eb=0), emit(root=None)]
    assert all(rc == L.SD_ERR_INVALID for rc in bad), bad
    assert b'sd_skeletonize_emit' in lib.sd_last_error()
    assert lib.sd_skeletonize_temp_bytes(cap + 1, 1, 1) == 0 and lib.sd_skeletonize_temp_bytes(0, 1, 1) == 0 and lib.sd_skeletonize_emit_temp_bytes(0) == 0
    assert lib.sd_skeletonize_temp_bytes(cap, 1, 1) > 0      # the cap itself is legal
    torch.cuda.synchronize()
    assert not counts.any()


# ---- the table on top ---------------------------------------------------------------------------------------------------------------------
def _expected_table(seg, kw):
    from syconn_amd.proc.skeleton import Skeleton, SkeletonTable
    kw = dict(kw)
    r = R.skeletonize(seg, kw.pop('w'), **kw)
    sk = {}
    for cell in np.unique(r['labels'][1:]):
        rows = [c for c in range(1, len(r['labels'])) if r['labels'][c] == cell]
        shift = np.concatenate(([0], np.cumsum([len(r['nodes'][c]) for c in rows])))
        sk[int(cell)] = Skeleton(np.concatenate([r['vertices'][c] for c in rows]) + np.float32(100), np.concatenate([r['edges'][c].astype(np.int64) + shift[k] for k, c in enumerate(rows)]),
                                 np.concatenate([r['radii'][c] for c in rows]))
    return SkeletonTable.from_skeletons(sk)


@pytest.mark.parametrize('resident', [False, True])
def test_chunk_table_with_and_without_lookup(resident):
    import torch
    from syconn_amd.proc.skeleton import relabel_lookup, skeletonize_chunk_table
    _, seg, kw, _ = CASES['multi_label']
    a = dev_kwargs(kw)
    arg = torch.from_numpy(seg.view(np.int64)).cuda() if resident else seg
    plain = skeletonize_chunk_table(arg, a['anisotropy'], 100, a['teasar_params'], a['dust_threshold'], max_paths=a['max_paths'])
    want = _expected_table(seg, kw)
    assert plain.ids.tolist() == [5, 9, 11]
    for k, v in want.as_dict().items():
        bits(plain.as_dict()[k], v, k)
    sv, ssv = [5, 9, 11], [50, 50, 60]      # 5 and 9 become one cell (their corner contact now joins them), the dust label 4 is not in the lookup
    looked = skeletonize_chunk_table(arg, a['anisotropy'], 100, a['teasar_params'], a['dust_threshold'], sv, ssv, max_paths=a['max_paths'])
    want = _expected_table(relabel_lookup(seg, sv, ssv), kw)
    assert looked.ids.tolist() == [50, 60] and len(looked.skeleton_of(50).vertices) > 0
    for k, v in want.as_dict().items():
        bits(looked.as_dict()[k], v, k)


def test_every_cell_is_a_forest_of_trees_and_feeds_the_vote():
    """The chain into the skeleton consumers: the table's columns are what skeleton_majority_vote takes."""
    from syconn_amd.proc.skeleton import skeletonize_chunk_table
    from syconn_amd.reps.super_segmentation_helper import skeleton_majority_vote
    _, seg, kw, _ = CASES['branch_cross']
    a = dev_kwargs(kw)
    t = skeletonize_chunk_table(seg, (10, 10, 20), 0, a['teasar_params'], 1, max_paths=100)
    assert len(t) == 1 and len(t.edges) == len(t.nodes) - 1
    cols = t.to_cell_columns((10, 10, 20))
    labels = (np.arange(len(t.nodes)) % 2).astype(np.int64)
    voted = skeleton_majority_vote(cols['nodes'], cols['node_begin'], cols['edges'], cols['edge_begin'], labels, (10, 10, 20), max_dist=1e9)
    assert len(voted) == len(t.nodes) and len(np.unique(voted)) == 1      # the whole tree is one window: one winner


# ---- the drop-in, the chunk driver and the chain into map_myelin_global -------------------------------------------------------------------
def _two_cells():
    """A (40, 36, 20) volume: cell 50 = supervoxels 5 and 6 (a long bent tube through every cube), cell 60 = supervoxel 9 (a Y), supervoxel 4
    in no cell."""
    seg = np.zeros((40, 36, 20), np.uint64)
    C.draw(seg, [(2, 2, 3), (36, 2, 3), (36, 30, 3)], 5, 1)
    C.draw(seg, [(36, 30, 3), (36, 30, 17), (5, 30, 17)], 6, 1)
    C.draw(seg, [(4, 12, 10), (20, 12, 10), (30, 6, 10)], 9, 1)
    C.draw(seg, [(20, 12, 10), (30, 20, 12)], 9, 1)
    C.draw(seg, [(3, 20, 3), (9, 20, 3)], 4, 1)
    return seg, [5, 6, 9], [50, 50, 60]


TP = dict(scale=1.0, const=30.0, pdrf_scale=100000.0, pdrf_exponent=4, max_paths=100)


def test_kimimaro_skelgen_equals_restatement_then_golden_checked_host_functions():
    from syconn_amd.proc import skeleton as S
    seg, sv, ssv = _two_cells()
    size, off = np.array([24, 36, 20]), np.array([16, 0, 0])
    got = S.kimimaro_skelgen(seg, size, off, dust_threshold=10, scaling=(10, 10, 20), sv_ids=sv, ssv_ids=ssv, teasar_params=TP)
    cube = S.relabel_lookup(seg[16:40], sv, ssv)
    r = R.skeletonize(cube, (10, 10, 20), dust_threshold=10, **TP)
    assert sorted(got) == [50, 60] and r['absorbed'] == 0
    for cell in (50, 60):
        rows = [c for c in range(1, len(r['labels'])) if r['labels'][c] == cell]
        shift = np.concatenate(([0], np.cumsum([len(r['nodes'][c]) for c in rows])))
        raw = S.Skeleton(np.concatenate([r['vertices'][c] for c in rows]), np.concatenate([r['edges'][c].astype(np.int64) + shift[k] for k, c in enumerate(rows)]),
                         np.concatenate([r['radii'][c] for c in rows]))
        want = S.sparsify_skelcv(S.downsample(raw, 10), scale=np.array([1, 1, 1]))
        bits(got[cell].vertices, want.vertices + (off * np.array([10, 10, 20])).astype(np.int32), f'vertices of {cell}')
        bits(got[cell].edges, want.edges, f'edges of {cell}')
        bits(got[cell].radii, want.radii, f'radii of {cell}')
        assert 0 < len(want.vertices) < len(raw.vertices)
    # with downsampling: the order-0 zoom, the anisotropy scaling * ds
    ds = S.kimimaro_skelgen(seg, np.array([40, 36, 20]), np.zeros(3, int), ds=np.array([2, 2, 1]), dust_threshold=10, scaling=(10, 10, 20), sv_ids=sv, ssv_ids=ssv, teasar_params=TP)
    r2 = R.skeletonize(S._zoom0(S.relabel_lookup(seg, sv, ssv), np.array([2., 2., 1.])), (20, 20, 20), dust_threshold=10, **TP)
    assert sorted(ds) == sorted(set(int(x) for x in r2['labels'][1:]))


def _one_tree(skel):
    from syconn_amd.proc.skeleton import _Graph
    return len(skel.vertices) >= 1 and len(skel.edges) == len(skel.vertices) - 1 and len(_Graph.of(skel).components()) == 1


def test_chunk_driver_on_a_box_that_is_no_multiple_of_the_cube():
    from syconn_amd.exec.exec_skeleton import run_kimimaro_skeletonization, run_skeleton_generation
    seg, sv, ssv = _two_cells()
    kw = dict(scaling=(10, 10, 20), cube_size=(16, 16, 16), ds=(1, 1, 1), sv_ids=sv, ssv_ids=ssv, dust_threshold=5, teasar_params=TP)
    t = run_kimimaro_skeletonization(seg, **kw)                       # 3 x 3 x 2 cubes over 40 x 36 x 20
    assert t.ids.tolist() == [50, 60]
    for cell in (50, 60):
        s = t.skeleton_of(cell)
        assert _one_tree(s), f'cell {cell}: {len(s.vertices)} nodes, {len(s.edges)} edges'
        lo, hi = s.vertices.min(0), s.vertices.max(0)
        assert (lo >= 0).all() and (hi <= np.array([400, 360, 400])).all()
    assert t.skeleton_of(50).vertices[:, 0].max() - t.skeleton_of(50).vertices[:, 0].min() > 250      # the tube spans the cubes
    whole = run_kimimaro_skeletonization(seg, **dict(kw, cube_size=(64, 64, 64)))
    assert whole.ids.tolist() == [50, 60] and all(_one_tree(whole.skeleton_of(c)) for c in (50, 60))
    part = run_skeleton_generation(seg, cube_of_interest_bb=((0, 0, 0), (40, 36, 8)), **kw)      # a partial box: only what lies in z < 8
    assert part.ids.tolist() == [50] and part.skeleton_of(50).vertices[:, 2].max() < 8 * 20


def test_chain_into_map_myelin_global(gpu, tmp_path):
    from syconn_amd import global_params
    from syconn_amd.exec.exec_skeleton import run_kimimaro_skeletonization
    from syconn_amd.handler.config import generate_default_conf
    from syconn_amd.knossos import KnossosDataset
    seg, sv, ssv = _two_cells()
    wd = str(tmp_path / 'wd')
    os.makedirs(wd, exist_ok=True)
    generate_default_conf(wd, scaling=(10., 10., 20.))
    mag = 2
    vol = np.zeros((10, 18, 20), np.uint8)                             # (z, y, x) at mag 2: myelin where x >= 20 at mag 1
    vol[:, :, 10:] = 255
    kd = KnossosDataset()
    kd.initialize_without_conf(wd + '/knossosdatasets/myelin/', np.array(vol.shape[::-1]) * mag, (10., 10., 20.), 'myelin', mags=[1, mag])
    kd.save_raw(offset=(0, 0, 0), mags=[mag], data=vol, data_mag=mag, fast_resampling=True, upsample=False)
    global_params.wd = wd
    try:
        t, cols = run_kimimaro_skeletonization(seg, scaling=(10, 10, 20), cube_size=(16, 16, 16), ds=(1, 1, 1), sv_ids=sv, ssv_ids=ssv, dust_threshold=5,
                                               teasar_params=TP, map_myelin=True, max_dist=1, mag=mag, cube_edge_avg=np.array([1, 1, 1]))
    finally:
        global_params.wd = None
    assert set(cols) == {'myelin', 'myelin_avg1'} and len(cols['myelin']) == len(t.nodes)
    assert np.array_equal(cols['myelin'], (t.nodes[:, 0] / 10 >= 20).astype(np.uint8)) and cols['myelin'].any() and not cols['myelin'].all()
    assert np.array_equal(cols['myelin_avg1'], cols['myelin'])      # a window of 1 nm holds the node alone
