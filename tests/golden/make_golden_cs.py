"""Golden vectors for the first contact-site steps, produced by the REFERENCE'S OWN code:
``process_block_nonzero`` / ``kernel`` of /root/reference/syconn/extraction/block_processing_C.pyx (:21-75) is cythonized and
compiled into a temporary directory at generation time, ``detect_seg_boundaries`` is lifted by AST from
/root/reference/syconn/extraction/find_object_properties.py (:424-455, numba decorator stripped: numba is absent), and the
closing loop of ``_contact_site_extraction_thread`` (/root/reference/syconn/extraction/cs_extraction_steps.py:437-461, the
``for ix in bb_dc.keys()`` statement) is lifted by AST and executed with scipy.  ``find_object_properties_C`` does not compile
here: its bounding boxes come from a numpy stand-in that yields ids in ascending order (the order this build specifies, DESIGN.md
section 7).  Nothing compiled and no reference text is stored: inputs and outputs only.

    python tests/golden/make_golden_cs.py      ->  tests/golden/g15_contact_sites.npz
"""
import ast
import os
import sys
import tempfile

import numpy as np
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/syconn'


def compile_block_processing(tmp):
    from Cython.Build import cythonize
    from setuptools import Extension
    from setuptools.dist import Distribution
    src = os.path.join(tmp, 'block_processing_C.pyx')
    with open(src, 'w') as f:
        f.write(open(os.path.join(REF, 'extraction', 'block_processing_C.pyx')).read())
    ext = cythonize([Extension('block_processing_C', [src], language='c++', include_dirs=[np.get_include()])], quiet=True,
                    language_level=3)
    d = Distribution({'ext_modules': ext})
    cmd = d.get_command_obj('build_ext')
    cmd.build_lib, cmd.build_temp = tmp, os.path.join(tmp, 'build')
    d.run_command('build_ext')
    sys.path.insert(0, tmp)
    import block_processing_C
    return block_processing_C


def lift_function(path, name, ns):
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            node.decorator_list = []
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, 'exec'), ns)
            return ns[name]
    raise KeyError(name)


def lift_closing_loop(path):
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name == '_contact_site_extraction_thread':
            for sub in ast.walk(node):
                if isinstance(sub, ast.For) and ast.unparse(sub.iter) == 'bb_dc.keys()':
                    return compile(ast.Module(body=[sub], type_ignores=[]), path, 'exec')
    raise KeyError('closing loop')


def bboxes_ascending(vol):
    """find_object_properties(vol)[1] stand-in: id -> [[min], [max + 1]] in ascending id order.  The keys are np.uint64: with
    Python-int keys (what Cython returns) NumPy >= 2 raises OverflowError in ``res[proc_mask] * ix`` for ids >= 2^63 (pairs of
    cell ids >= 2^31), where NumPy 1's value-based casting gave the uint64 product."""
    ids, inv = np.unique(vol.ravel(), return_inverse=True)
    out = {}
    for k, sl in enumerate(scipy.ndimage.find_objects(inv.reshape(vol.shape) + 1)):
        if ids[k] == 0 or sl is None:
            continue
        out[ids[k]] = [[s.start for s in sl], [s.stop for s in sl]]
    return out


def voronoi(shape, n, rng, ids):
    pts = np.stack([rng.integers(0, s, n) for s in shape], 1)
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).reshape(-1, 1, 3)
    near = np.argmin(((g - pts[None]) ** 2).sum(-1), 1)
    return np.asarray(ids, np.uint64)[near].reshape(shape)


def main():
    rng = np.random.default_rng(15)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        bp = compile_block_processing(tmp)
        ns = {'np': np}
        detect_seg_boundaries = lift_function(os.path.join(REF, 'extraction', 'find_object_properties.py'),
                                              'detect_seg_boundaries', ns)
        closing = lift_closing_loop(os.path.join(REF, 'extraction', 'cs_extraction_steps.py'))

        # ---- stencil cases: raw uint64 ids are truncated to uint32 as the worker does (load_seg(...).astype(np.uint32))
        big = [2 ** 31 + 5, 2 ** 32 + 7, 2 ** 32, 2 ** 33 + 2 ** 31 + 11, 2 ** 32 - 1]
        raw_vor = voronoi((40, 36, 22), 14, rng, [3, 7, 12, 40, 41, 90, 91, 500, 1000] + big)
        raw_vor[:, :, :2] = 0                                          # background slab
        hand = np.zeros((3, 3, 3), np.uint64)
        flat = hand.reshape(-1)
        pos = [p for p in range(27) if p != 13]
        flat[pos[:9]], flat[pos[9:18]], flat[13] = 9, 7, 5           # centre 5: 9 x id 9, 9 x id 7 -> 0x5_00000007
        salt = rng.integers(1, 2 ** 32, (26, 26, 14), dtype=np.uint64)
        salt[rng.random(salt.shape) < 0.1] = 0
        few = rng.integers(0, 5, (16, 16, 10)).astype(np.uint64)      # many tied counts
        cases = [('vor13', raw_vor, (13, 13, 7)), ('vor7', raw_vor, (7, 7, 3)), ('vor3', raw_vor, (3, 3, 3)),
                 ('hand', hand, (3, 3, 3)), ('salt13', salt, (13, 13, 7)), ('salt3', salt[:12, :12, :8], (3, 3, 3)),
                 ('few7', few, (7, 7, 3)), ('few3', few, (3, 3, 3))]
        names = []
        for name, raw, st in cases:
            seg = raw.astype(np.uint32)
            edges = np.asarray(detect_seg_boundaries(seg))
            cs = np.asarray(bp.process_block_nonzero(edges.astype(np.uint32), seg, st))
            out[f'st_{name}_raw'], out[f'st_{name}_stencil'] = raw, np.array(st, np.int32)
            out[f'st_{name}_edges'], out[f'st_{name}_cs'] = edges.astype(np.uint8), cs.astype(np.uint64)
            names.append(name)
        out['stencil_cases'] = np.array(names)
        assert int(out['st_hand_cs'][0, 0, 0]) == 0x5_00000007

        # ---- closing cases
        sites = np.zeros((30, 26, 18), np.uint64)
        sites[0:3, 4:9, 2:5] = 11                                      # touches the x = 0 face
        sites[5:7, 4:9, 2:5] = 2 ** 63 + 4                             # 2 voxels from id 11: contested voxels (unsigned order)
        sites[27:30, 20:26, 14:18] = (5 << 32) | 9                     # corner of the volume
        sites[12:20, 10, 8] = 3                                        # thin line, its box overlaps the next site's
        sites[14:18, 13, 8:11] = 2
        sites[rng.random(sites.shape) < 0.004] = 77                    # one site scattered over the volume (box = all)
        close_cases = [('sites62', sites, 6, 2), ('sites30', sites, 3, 0), ('vor62', out['st_vor13_cs'], 6, 2),
                       ('vor30', out['st_vor13_cs'], 3, 0), ('vor7_31', out['st_vor7_cs'], 3, 1)]
        names = []
        for name, c0, n, k in close_cases:
            contacts = c0.copy()
            env = dict(np=np, scipy=scipy, contacts=contacts, bb_dc=bboxes_ascending(c0), n_closings=n, cs_dilation=k)
            exec(closing, env)
            out[f'cl_{name}_in'], out[f'cl_{name}_nk'] = c0, np.array([n, k], np.int32)
            out[f'cl_{name}_out'] = contacts
            names.append(name)
        out['close_cases'] = np.array(names)
    path = os.path.join(HERE, 'g15_contact_sites.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
