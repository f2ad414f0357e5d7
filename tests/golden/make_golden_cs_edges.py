"""Golden vectors for the contact-site steps at the edges of the device kernels' structure, produced by the REFERENCE'S OWN code
exactly as ``make_golden_cs.py`` does (``process_block_nonzero`` cythonized into a temporary directory at generation time,
``detect_seg_boundaries`` and the closing loop lifted by AST; nothing compiled and no reference text is stored: inputs and
outputs only).

Stencil cases: volumes drawn from a pool of P ids (one of them 2^32 - 1) plus 10 % background.  P = 9 gives windows with exactly
8 distinct partners (the register table of k_contact_partners is full but holds), P = 10 exactly 9 (the first overflow), P = 12
more.  The output extents cover 1, 7, 8, 9, 15, 16, 17 (the 8 x 8 x 16 tile and its neighbours), a volume equal to the stencil
(one output) and the stencil (1, 1, 1) (all zero).  Closing cases: (n, k) = (0, 2), (1, 1), (12, 3), (6, 0) on a volume with sites
on all six faces, a one-voxel site, a site whose box is the whole volume and ids >= 2^63.

    python tests/golden/make_golden_cs_edges.py      ->  tests/golden/g17_cs_edges.npz
"""
import io
import os
import sys
import tempfile
import zipfile

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_cs import REF, bboxes_ascending, compile_block_processing, lift_closing_loop, lift_function  # noqa: E402

# name, pool size P, volume shape, stencil  (output extent = shape - stencil + 1)
STENCIL_CASES = [
    ('p9_s333', 9, (10, 11, 19), (3, 3, 3)),          # out  8,  9, 17
    ('p10_s333', 10, (10, 11, 19), (3, 3, 3)),        # out  8,  9, 17
    ('p12_s333', 12, (9, 18, 3), (3, 3, 3)),          # out  7, 16,  1
    ('p9_s531', 9, (21, 9, 16), (5, 3, 1)),           # out 17,  7, 16
    ('p10_s531', 10, (19, 3, 9), (5, 3, 1)),          # out 15,  1,  9
    ('p12_s531', 12, (12, 10, 7), (5, 3, 1)),         # out  8,  8,  7
    ('p9_s3d7', 9, (11, 28, 13), (3, 13, 7)),         # out  9, 16,  7
    ('p10_s3d7', 10, (3, 29, 22), (3, 13, 7)),        # out  1, 17, 16
    ('p12_s3d7', 12, (17, 19, 14), (3, 13, 7)),       # out 15,  7,  8
    ('p9_sdd7', 9, (29, 21, 23), (13, 13, 7)),        # out 17,  9, 17
    ('p10_sdd7', 10, (20, 27, 15), (13, 13, 7)),      # out  8, 15,  9
    ('p12_sdd7', 12, (19, 20, 22), (13, 13, 7)),      # out  7,  8, 16
    ('p10_eq_dd7', 10, (13, 13, 7), (13, 13, 7)),     # volume == stencil: one output
    ('p10_eq_333', 10, (3, 3, 3), (3, 3, 3)),
    ('p10_s111', 10, (9, 8, 17), (1, 1, 1)),          # a window of the centre alone: all zero
]
CLOSE_NK = [(0, 2), (1, 1), (12, 3), (6, 0)]


def pool_volume(rng, shape, p):
    """Every voxel one of `p` ids (2^32 - 1, ids >= 2^31 and small ones), 10 % background."""
    ids = np.concatenate([[2 ** 32 - 1, 2 ** 31 + 3], rng.choice(np.arange(1, 5000), p - 2, replace=False)]).astype(np.uint64)
    vol = ids[rng.integers(0, p, shape)]
    vol[rng.random(shape) < 0.1] = 0
    return vol


def site_volume(rng):
    s = np.zeros((44, 40, 36), np.uint64)
    s[0:2, 5:9, 6:9] = 21                                              # x = 0 face
    s[42:44, 14:19, 3:6] = (7 << 32) | 9                              # x = X - 1 face
    s[8:12, 0:2, 12:15] = 2 ** 63 + 5                                  # y = 0 face, id >= 2^63
    s[15:19, 38:40, 10:14] = 2 ** 64 - 2                               # y = Y - 1 face, the largest admitted id
    s[30:33, 9:12, 0:1] = 4                                            # z = 0 face
    s[4:8, 25:28, 35:36] = 2 ** 63 + 4                                 # z = Z - 1 face
    s[22, 20, 17] = 13                                                 # one voxel, its n = 12 box clear of every face
    s[18:21, 20, 17] = 12                                              # two pieces with a gap of three (closed from n = 2 on),
    s[18:21, 24:27, 17] = 12                                           # two voxels from id 13 along x: contested background
    s[24:26, 20:22, 17:19] = 14
    s[20:24, 14:18, 16:19] = 15                                        # a frame around a hole
    s[21:23, 15:17, 16:19] = 0
    s[0, 0, 0] = s[43, 39, 35] = 77                                    # two corners: the box is the whole volume
    s[(rng.random(s.shape) < 0.003) & (s == 0)] = 77
    return s


def main():
    rng = np.random.default_rng(17)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        bp = compile_block_processing(tmp)
        detect_seg_boundaries = lift_function(os.path.join(REF, 'extraction', 'find_object_properties.py'),
                                              'detect_seg_boundaries', {'np': np})
        closing = lift_closing_loop(os.path.join(REF, 'extraction', 'cs_extraction_steps.py'))
        names = []
        for name, p, shape, st in STENCIL_CASES:
            raw = pool_volume(rng, shape, p)
            seg = raw.astype(np.uint32)
            edges = np.asarray(detect_seg_boundaries(seg))
            cs = np.asarray(bp.process_block_nonzero(edges.astype(np.uint32), seg, st))
            out[f'st_{name}_raw'], out[f'st_{name}_stencil'] = raw, np.array(st, np.int32)
            out[f'st_{name}_edges'], out[f'st_{name}_cs'] = edges.astype(np.uint8), cs.astype(np.uint64)
            names.append(name)
        out['stencil_cases'] = np.array(names)

        sites = site_volume(rng)
        out['cl_in'] = sites
        out['close_nk'] = np.array(CLOSE_NK, np.int32)
        for n, k in CLOSE_NK:
            contacts = sites.copy()
            env = dict(np=np, scipy=scipy, contacts=contacts, bb_dc=bboxes_ascending(sites), n_closings=n, cs_dilation=k)
            exec(closing, env)
            out[f'cl_{n}_{k}_out'] = contacts
    path = os.path.join(HERE, 'g17_cs_edges.npz')
    save_npz(path, out)
    print('wrote', path, os.path.getsize(path), 'bytes')


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member date, so that the file regenerates byte for byte."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


if __name__ == '__main__':
    main()
