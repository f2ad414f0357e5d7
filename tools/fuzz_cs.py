"""GPU box: randomized sweep of the contact-site stage -- boundaries, partner stencil, closing + dilation and the syn statistics on
random shapes, odd stencils the entry point admits and id pools from 2 ids to "every voxel its own id", against the numpy / scipy
restatement of tests/_cs_ref.py and tests/_cs_syntype_ref.py.  Not part of the suite.
usage: fuzz_cs.py [seconds] [seed]"""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _cs_ref, _cs_syntype_ref
from syconn_amd.extraction.cs_extraction_steps import close_and_dilate_cs
from syconn_amd.extraction.find_object_properties import cs_syntype, cs_syntype_dicts, detect_cs, detect_seg_boundaries

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rng = np.random.default_rng(seed)
dev = torch.device('cuda', 0)


def admitted(st):
    return np.prod([t + s - 1 for t, s in zip((8, 8, 16), st)]) * 4 <= 64 * 1024 and np.prod(st) <= 4096


t0, n, hit = time.time(), 0, {}
while time.time() - t0 < budget:
    st = tuple(int(rng.choice([1, 3, 5, 7, 9, 13, 15, 19])) for _ in range(3))
    if not admitted(st):
        continue
    ext = tuple(int(rng.choice([1, 2, 7, 8, 9, 15, 16, 17, 24, 33])) for _ in range(3))
    shape = tuple(e + s - 1 for e, s in zip(ext, st))
    pool = int(rng.choice([2, 5, 9, 10, 12, 40, 0]))                   # 0: every voxel its own id
    if pool == 0 and np.prod(shape) > 20000:                           # the restatement loops over the ids
        pool = 400
    m = pool or int(np.prod(shape))
    ids = rng.permutation(np.unique(rng.integers(1, 2 ** 32, 2 * m + 8, dtype=np.uint64))[:m]).astype(np.uint32)
    if rng.random() < 0.5:
        ids[0] = 2 ** 32 - 1
    seg = ids[rng.integers(0, len(ids), shape)] if pool else ids.reshape(shape).copy()
    if rng.random() < 0.5:                                             # coherent blocks instead of noise
        seg = np.ascontiguousarray(np.kron(seg[::3, ::3, ::3], np.ones((3, 3, 3), np.uint32))[:shape[0], :shape[1], :shape[2]])
    seg[rng.random(shape) < rng.choice([0.0, 0.1, 0.6])] = 0
    case = (seed, n, st, ext, pool)
    edges = _cs_ref.seg_boundaries(seg)
    assert np.array_equal(detect_seg_boundaries(seg, device=dev), edges), ('boundaries', case)
    want = _cs_ref.contact_partners(edges, seg, st)
    got = detect_cs(seg, st, device=dev)
    assert np.array_equal(got, want), ('partners', case, int(np.flatnonzero(got.ravel() != want.ravel())[0]))
    nc, k = int(rng.integers(0, 8)), int(rng.integers(0, 4))
    ws = int(rng.choice([1, 1 << 12, 1 << 28]))
    closed = _cs_ref.close_dilate(want, nc, k)
    got = close_and_dilate_cs(want, nc, k, device=dev, ws_budget=ws)
    assert np.array_equal(got, closed), ('closing', case, nc, k, ws, int(np.flatnonzero(got.ravel() != closed.ravel())[0]))
    vals = np.array([0, 1, 2, 255], np.uint8)
    syn, asym, sym = (vals[rng.integers(0, 4, closed.shape)] for _ in range(3))
    org = tuple(int(rng.integers(0, s)) for s in closed.shape)
    wext = tuple(int(rng.integers(1, s - o + 1)) for s, o in zip(closed.shape, org))
    crop = tuple(slice(o, o + e) for o, e in zip(org, wext))
    vol = closed if rng.random() < 0.5 else (closed & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ref = _cs_syntype_ref.extract_cs_syntype(vol[crop], syn[crop], asym[crop], sym[crop], (5, 6, 7))
    res = cs_syntype_dicts(*cs_syntype(vol, syn, asym, sym, offset=(5, 6, 7), device=dev, origin=org, extent=wext).host())
    assert res == ref and list(res[4]) == list(ref[4]), ('syntype', case, org, wext, vol.dtype)
    hit[(st, pool)] = hit.get((st, pool), 0) + 1
    n += 1
print(f'fuzz_cs: {n} cases ok in {time.time() - t0:.0f} s; (stencil, pool) combinations hit: {len(hit)}')
