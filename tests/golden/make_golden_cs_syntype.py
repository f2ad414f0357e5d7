"""Golden vectors for the synapse statistics of contact sites and the sj morphology, produced by the REFERENCE'S OWN code:
``extract_cs_syntype`` of /root/reference/syconn/extraction/block_processing_C.pyx (:78-158) is cythonized and compiled into a
temporary directory at generation time (as make_golden_cs.py does), and ``apply_morphological_operations``,
``_multi_mop_findobjects``, ``_count_subsequent_mops`` and ``get_aniso_struct`` are lifted by AST from
/root/reference/syconn/proc/image.py (:358-438, 485-539) and run with scipy.  Only flat input and output arrays are stored.

    python tests/golden/make_golden_cs_syntype.py      ->  tests/golden/g16_cs_syntype.npz
"""
import os
import sys
import tempfile
import typing

import numpy as np
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_cs import REF, compile_block_processing, lift_function, voronoi  # noqa: E402


def flatten(res):
    """extract_cs_syntype's return value -> flat arrays, sites in ascending id order, voxel lists in the recorded order."""
    (rc, bb, sz), (src, sbb, ssz), asym, sym, vox = res
    out = {}
    for tag, (a, b, c) in (('cs', (rc, bb, sz)), ('syn', (src, sbb, ssz))):
        ids = sorted(c)
        out[f'{tag}_ids'] = np.array(ids, np.uint64)
        out[f'{tag}_rc'] = np.array([a[k] for k in ids], np.int64).reshape(-1, 3)
        out[f'{tag}_bb'] = np.array([b[k] for k in ids], np.int64).reshape(-1, 2, 3)
        out[f'{tag}_size'] = np.array([c[k] for k in ids], np.int64)
    for tag, d in (('asym', asym), ('sym', sym)):
        ids = sorted(d)
        out[f'{tag}_ids'] = np.array(ids, np.uint64)
        out[f'{tag}_cnt'] = np.array([d[k] for k in ids], np.int64)
    ids = sorted(vox)
    out['vox_ids'] = np.array(ids, np.uint64)
    out['vox_cnt'] = np.array([len(vox[k]) for k in ids], np.int64)
    out['vox'] = np.array([v for k in ids for v in vox[k]], np.int64).reshape(-1, 3)
    return out


def blobs(shape, rng, frac, sigma=1.5):
    """Smoothed noise thresholded at the (1 - frac) quantile: a 0/1 mask of roughly `frac` foreground."""
    n = scipy.ndimage.gaussian_filter(rng.random(shape), sigma)
    return (n > np.quantile(n, 1 - frac)).astype(np.uint8)


def main():
    rng = np.random.default_rng(16)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        bp = compile_block_processing(tmp)
        # ---- extract_cs_syntype cases: (name, cs_seg, syn, asym, sym, offset)
        cases = []
        big = [2 ** 32 + 7, 2 ** 33 + 1, 2 ** 63 + 5, 2 ** 64 - 2, 2 ** 32]
        vor = voronoi((64, 64, 32), 100, rng, np.concatenate([rng.integers(1, 2 ** 40, 95, dtype=np.uint64), np.array(big, np.uint64)]))
        vor[rng.random(100)[np.searchsorted(np.unique(vor), vor)] < 0.5] = 0                 # half of the sites are background
        syn = blobs(vor.shape, rng, 0.15) * rng.choice(np.array([1, 2, 255], np.uint8), vor.shape)
        asym = blobs(vor.shape, rng, 0.5) * rng.choice(np.array([1, 2], np.uint8), vor.shape)
        sym = blobs(vor.shape, rng, 0.5) * rng.choice(np.array([1, 2], np.uint8), vor.shape)
        cases.append(('vor64', vor.astype(np.uint64), syn, asym, sym, (0, 0, 0)))
        small = voronoi((12, 10, 9), 7, rng, [3, 4, 9, 11, 2 ** 31 + 3, 2 ** 32 - 1, 17]).astype(np.uint32)
        small[rng.random(small.shape) < 0.2] = 0
        sv = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), small.shape)
        av = rng.choice(np.array([0, 1, 2], np.uint8), small.shape)
        yv = rng.choice(np.array([0, 1, 2], np.uint8), small.shape)
        cases.append(('u32', small, sv, av, yv, (0, 0, 0)))
        cases.append(('u32_offset', small, sv, av, yv, (1000, -7, 2 ** 30)))
        cases.append(('u64_big', (small.astype(np.uint64) * np.uint64(2 ** 31 + 1)) | np.uint64(2 ** 63) * (small > 0),
                      sv, av, yv, (5, 6, 7)))
        cases.append(('empty_syn', small, np.zeros_like(sv), av, yv, (0, 0, 0)))
        cases.append(('background', np.zeros((5, 6, 7), np.uint32), np.ones((5, 6, 7), np.uint8), np.ones((5, 6, 7), np.uint8),
                      np.ones((5, 6, 7), np.uint8), (0, 0, 0)))
        one = np.zeros((4, 4, 4), np.uint64)
        one[2, 1, 3] = 2 ** 40 + 1
        cases.append(('single', one, np.full(one.shape, 2, np.uint8), np.ones(one.shape, np.uint8), np.full(one.shape, 2, np.uint8),
                      (3, 2, 1)))
        cases.append(('flat_z', small[:, :, 4:5].copy(), sv[:, :, 4:5].copy(), av[:, :, 4:5].copy(), yv[:, :, 4:5].copy(), (0, 0, 9)))
        cases.append(('flat_x', small[6:7].copy(), sv[6:7].copy(), av[6:7].copy(), yv[6:7].copy(), (0, 0, 0)))
        names = []
        for name, cs, s, a, y, off in cases:
            res = bp.extract_cs_syntype(cs, s, a, y, offset=np.array(off, np.int64))
            out[f'cst_{name}_cs'], out[f'cst_{name}_syn'], out[f'cst_{name}_asym'], out[f'cst_{name}_sym'] = cs, s, a, y
            out[f'cst_{name}_offset'] = np.array(off, np.int64)
            for k, v in flatten(res).items():
                out[f'cst_{name}_{k}'] = v
            names.append(name)
        out['cst_cases'] = np.array(names)

        # ---- sj morphology: apply_morphological_operations(mask, sj ops, mop_kwargs=dict(structure=get_aniso_struct(scaling)))
        image = os.path.join(REF, 'proc', 'image.py')
        ns = {'np': np, 'ndimage': scipy.ndimage, 'log_proc': None, 'tqdm': None, 'fill_voids': None}
        ns.update({k: getattr(typing, k) for k in ('List', 'Optional', 'Union', 'Tuple')})
        for fn in ('_count_subsequent_mops', '_multi_mop_findobjects', 'apply_morphological_operations', 'get_aniso_struct'):
            lift_function(image, fn, ns)
        ops = ['binary_opening', 'binary_closing', 'binary_erosion']
        masks = [('blob', blobs((40, 36, 20), rng, 0.08, 2.0)), ('noisy', blobs((24, 28, 16), rng, 0.3, 1.0)),
                 ('empty', np.zeros((10, 12, 8), np.uint8))]
        mnames = []
        for mname, m in masks:
            for scaling in ((10, 10, 20), (10, 10, 10), (8, 8, 30)):
                struct = ns['get_aniso_struct'](np.array(scaling))
                res = ns['apply_morphological_operations'](m.copy(), ops, mop_kwargs=dict(structure=struct)).astype('u1', copy=False)
                key = f'{mname}_{scaling[2] // scaling[0]}'
                out[f'mop_{key}_in'], out[f'mop_{key}_scaling'] = m, np.array(scaling, np.int64)
                out[f'mop_{key}_out'] = res
                mnames.append(key)
        out['mop_ops'] = np.array(ops)
        out['mop_cases'] = np.array(mnames)
    path = os.path.join(HERE, 'g16_cs_syntype.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
