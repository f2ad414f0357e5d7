"""Golden vectors for the legacy rule of the rendering locations, produced by the REFERENCE'S OWN ``surface_samples``
(/root/reference/syconn/reps/rep_helper.py:376-417), lifted by AST at generation time and run unchanged over numpy and scipy
(``spatial.cKDTree``, ``np.histogramdd``).  Nothing compiled and no reference text is stored: inputs and outputs only.

    python tests/golden/make_golden_locations.py      ->  tests/golden/g28_locations.npz

The voxel rule (``generate_rendering_locs``) has no golden: the reference calls open3d, which is not installed here; tests/_locations_ref.py
is its normative statement.

``n``: the number of clouds; per cloud k ``s{k}_verts`` float32 (m, 3) -- multiples of 0.5 plus a large offset, as marching-cubes vertices
are --, ``s{k}_bins`` (3), ``s{k}_r``, ``s{k}_out`` float32: the reference's result.  The generator ASSERTS the conditions under which the
reference alone is well defined: the two smallest squared distances of every bin centre differ (no cKDTree tie; a cloud with a tie is
drawn again), every squared distance is exact in float64 (so ``d^2 <= r^2`` does not depend on rounding), and ``max_nb_samples=1``
changes nothing (the threshold branch of the reference is dead).  It also asserts that the restatement agrees bit for bit."""
import os
import sys
from fractions import Fraction

import numpy as np
import scipy.spatial

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _locations_ref as R  # noqa: E402
from make_golden_cs import lift_function  # noqa: E402

REF = '/root/reference/syconn'


def namespace():
    ns = {'np': np, 'spatial': scipy.spatial}
    exec('from typing import *', ns)
    lift_function(f'{REF}/reps/rep_helper.py', 'surface_samples', ns)
    return ns


def well_defined(verts, bins, r):
    """No tie for the nearest vertex of any occupied bin's centre, and exact squared distances."""
    _, occupied, nearest, _, _ = R.surface_samples(verts, bins, r=r, return_parts=True)
    c = (verts - verts.min(0)).astype(np.float32).astype(np.float64)
    centres = (occupied + 0.5) * np.array(bins, np.float32).astype(np.float64)
    for q in centres:
        d = np.sort(R.sq_dist(c, q))
        if len(d) > 1 and d[0] == d[1]:
            return False
    # exactness: the float64 sums against rational arithmetic, for every centre and every nearest vertex
    for q in list(centres) + [c[i] for i in nearest]:
        d = R.sq_dist(c, q)
        for row, dv in zip(c, d):
            exact = sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(row, q))
            assert Fraction(float(dv)) == exact
    return True


def cloud(rng, n, extent, offset, flat_axis=None):
    half = rng.integers(0, [2 * e + 1 for e in extent], (n, 3)).astype(np.float64) * 0.5
    if flat_axis is not None:
        half[:, flat_axis] = half[0, flat_axis]
    v = (half + np.asarray(offset, np.float64)).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), half + np.asarray(offset, np.float64))      # float32 holds them exactly
    return v


def main():
    rng = np.random.default_rng(2801)
    ns = namespace()
    ref = ns['surface_samples']
    specs = [dict(n=300, extent=(5000, 3000, 2500), offset=(81920.0, 40960.5, 20480.0), bins=(2000, 2000, 2000), r=1000),
             dict(n=200, extent=(900, 700, 800), offset=(123456.5, 65432.0, 1000.5), bins=(300, 300, 300), r=150.0),
             dict(n=400, extent=(4000, 4000, 100), offset=(0.0, 512.0, 70000.0), bins=(1500, 1000, 2000), r=700),
             dict(n=250, extent=(3000, 2000, 2600), offset=(50000.0, 50000.0, 50000.0), bins=(1000, 1000, 1000), r=500, flat_axis=1),
             dict(n=64, extent=(100, 100, 100), offset=(1e5, 2e5, 3e5), bins=(2000, 2000, 2000), r=1000),
             dict(n=350, extent=(7000, 1000, 1000), offset=(16384.0, 8.5, 99.0), bins=(1000, 1000, 1000), r=2000.5)]
    out = {'n': np.int64(len(specs))}
    for k, sp in enumerate(specs):
        for attempt in range(100):
            v = cloud(rng, sp['n'], sp['extent'], sp['offset'], sp.get('flat_axis'))
            if well_defined(v, sp['bins'], sp['r']):
                break
        else:
            raise AssertionError(f'cloud {k}: no draw without a tie')
        got = ref(v, sp['bins'], r=sp['r'])
        assert got.dtype == np.float32 and got.shape[1] == 3 and len(got) >= 1
        assert np.array_equal(got, ref(v, sp['bins'], max_nb_samples=1, r=sp['r']))            # max_nb_samples has no effect
        mine = R.surface_samples(v, sp['bins'], r=sp['r'])
        assert mine.dtype == got.dtype and np.array_equal(mine.view(np.uint32), got.view(np.uint32)), f'cloud {k}: the restatement differs'
        out.update({f's{k}_verts': v, f's{k}_bins': np.array(sp['bins'], np.float64), f's{k}_r': np.float64(sp['r']), f's{k}_out': got})
        print(f'cloud {k}: {len(v)} vertices -> {len(got)} locations (draw {attempt})')
    path = os.path.join(HERE, 'g28_locations.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
