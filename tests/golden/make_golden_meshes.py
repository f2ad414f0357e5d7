"""Golden vectors for the meshes, produced by the REFERENCE'S OWN ``find_meshes``, ``merge_meshes``, ``merge_meshes_incl_norm`` and
``mesh_area_calc`` (/root/reference/syconn/proc/meshes.py:937-994, :453-519, :1113-1124), lifted by AST at generation time and run
unchanged over scipy's ``zoom`` and numpy.  zmesh and skimage are absent: ``Mesher`` and ``mesh_surface_area`` of tests/_mesh_ref.py
stand in for them (the unsimplified surface in the contract's order; 0.5 * sum |cross| in float64).  The ``mesh_bb`` / ``mesh_area`` of
step 2 are the statements of proc/sd_proc.py:957-975 restated over the lifted functions.  Nothing compiled and no reference text is
stored: inputs and outputs only, as flat arrays.

    python tests/golden/make_golden_meshes.py      ->  tests/golden/g25_meshes.npz

``vol`` (24, 10, 9) uint64 is cut into three chunks of 8 voxels along x at ``origin + (8 c, 0, 0)``; ``scaling``; two runs r: ``a`` with ds
(2, 2, 1), ``b`` with ds (1, 1, 1), both pad = 1.  Per run and chunk c: ``{r}{c}_ids``, ``_ind`` / ``_ind_begin`` (flat indices of all ids, offsets
per id), ``_vert`` / ``_vert_begin`` (flat vertices).  Per run the merge over the chunks in chunk order: ``{r}_ids``, ``_ind`` / ``_ind_begin``,
``_vert`` / ``_vert_begin`` (merge_meshes_incl_norm; merge_meshes gave the same arrays, asserted here), ``_area`` (mesh_area_calc), ``_bb``.
The property table ``p_ids`` / ``p_sizes`` / ``p_boxes`` / ``p_box_begin`` with ``p_min_obj_vx`` / ``p_mesh_min_obj_vx`` and per run the stored
``{r}_props_nvert`` / ``_props_ntri`` / ``_props_bb`` (float64) / ``_props_area``."""
import os
import sys

import numpy as np
from scipy.ndimage import zoom

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _mesh_ref as R  # noqa: E402
from make_golden_cs import lift_function  # noqa: E402

REF = '/root/reference/syconn'
U = np.uint64
PROPS = dict(normals=False, simplification_factor=50, max_simplification_error=40)


def toy_volume(rng):
    v = np.zeros((24, 10, 9), U)
    v[2:14, 2:8, 1:7] = 5                                   # through the face between chunks 0 and 1
    v[4:7, 3:6, 2:5] = 0                                    # with a cavity
    v[15:23, 1:5, 2:8] = 7                                  # through the face between chunks 1 and 2
    v[17:22, 6:9, 1:4] = U(2 ** 40 + 3)                     # scipy's zoom takes labels through float64: ids stay below 2^53 here
    v[3, 9, 8] = 9                                          # one voxel at odd coordinates: gone after ds (2, 2, 1)
    noise = rng.random(v.shape) < 0.04
    v[noise & (v == 0)] = 11
    v[0:3, 0:2, :] = 13                                     # on the faces of the volume: the pad replicates it
    return v


def flat(meshes):
    ids = np.array(sorted(meshes), U)
    ind = [np.asarray(meshes[i][0]) for i in ids]
    vert = [np.asarray(meshes[i][1]) for i in ids]
    begin = lambda parts: np.concatenate(([0], np.cumsum([len(p) for p in parts]))).astype(np.int64)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    for i in ids:
        assert meshes[i][0].dtype == np.uint32 and meshes[i][1].dtype == np.float32 and meshes[i][2].shape == (0,)
    return ids, cat(ind, np.uint32), begin(ind), cat(vert, np.float32), begin(vert)


def main():
    ns = {'np': np, 'zoom': zoom, 'Mesher': R.Mesher, 'mesh_surface_area': R.mesh_surface_area, 'global_params': None}
    exec('from typing import *', ns)
    path = f'{REF}/proc/meshes.py'
    find_meshes, merge_meshes = lift_function(path, 'find_meshes', ns), lift_function(path, 'merge_meshes', ns)
    merge_incl_norm, mesh_area_calc = lift_function(path, 'merge_meshes_incl_norm', ns), lift_function(path, 'mesh_area_calc', ns)
    rng = np.random.default_rng(2501)
    vol = toy_volume(rng)
    origin, scaling = np.array([16, 8, 24], np.int64), np.array([10., 10., 20.])
    out = dict(vol=vol, origin=origin, scaling=scaling, a_ds=np.array([2, 2, 1]), b_ds=np.array([1, 1, 1]))
    # the property table: sizes over the volume, one box per chunk that holds the id (min | max + 1, dataset coordinates)
    ids = np.unique(vol)
    ids = ids[ids != 0]
    boxes, box_begin = [], [0]
    for i in ids:
        for c in range(3):
            q = np.argwhere(vol[8 * c:8 * c + 8] == i)
            if len(q):
                boxes.append([q.min(0) + origin + (8 * c, 0, 0), q.max(0) + 1 + origin + (8 * c, 0, 0)])
        box_begin.append(len(boxes))
    sizes = np.array([(vol == i).sum() for i in ids], np.int64)
    min_obj_vx, mesh_min_obj_vx = 2, 20
    out.update(p_ids=ids, p_sizes=sizes, p_boxes=np.array(boxes, np.int64), p_box_begin=np.array(box_begin, np.int64),
               p_min_obj_vx=np.int64(min_obj_vx), p_mesh_min_obj_vx=np.int64(mesh_min_obj_vx))
    for r in 'ab':
        per_chunk = []
        for c in range(3):
            chunk = np.ascontiguousarray(vol[8 * c:8 * c + 8])
            m = find_meshes(chunk, origin + (8 * c, 0, 0), pad=1, ds=out[f'{r}_ds'], scaling=scaling, meshing_props=PROPS)
            assert set(m) == set(np.unique(chunk)) - {0}
            per_chunk.append(m)
            for k, v in zip(('ids', 'ind', 'ind_begin', 'vert', 'vert_begin'), flat(m)):
                out[f'{r}{c}_{k}'] = v
        merged, areas, bbs, props = {}, [], [], dict(nvert=[], ntri=[], bb=[], area=[])
        for k, i in enumerate(ids):
            parts = [m[i] for m in per_chunk if i in m]
            mesh = merge_incl_norm([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts])
            plain = merge_meshes([p[0] for p in parts], [p[1] for p in parts])
            assert np.array_equal(plain[0], mesh[0]) and np.array_equal(plain[1], mesh[1]) and mesh[0].dtype == np.uint32
            merged[i] = mesh
            verts = mesh[1].reshape(-1, 3)
            areas.append(mesh_area_calc(mesh) if len(verts) else 0.)
            bbs.append([np.min(verts, axis=0), np.max(verts, axis=0)] if len(verts) else np.zeros((2, 3), np.float32))
            # step 2 (sd_proc.py:951-975): an object below the thresholds has no cached meshes
            small = sizes[k] < mesh_min_obj_vx or sizes[k] < min_obj_vx
            parts = [] if small else parts
            mesh = merge_incl_norm([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts])
            verts = mesh[1].reshape(-1, 3)
            bb = np.array(boxes[box_begin[k]:box_begin[k + 1]])
            bounding_box = np.array([bb[:, 0].min(axis=0), bb[:, 1].max(axis=0)])
            if len(verts) > 0:
                props['bb'].append(np.array([np.min(verts, axis=0), np.max(verts, axis=0)], np.float64))
                props['area'].append(mesh_area_calc(mesh))
            else:
                props['bb'].append(bounding_box * scaling)
                props['area'].append(0)
            props['nvert'].append(len(verts))
            props['ntri'].append(len(mesh[0]) // 3)
        for k, v in zip(('ids', 'ind', 'ind_begin', 'vert', 'vert_begin'), flat(merged)):
            out[f'{r}_{k}'] = v
        out[f'{r}_area'], out[f'{r}_bb'] = np.array(areas, np.float64), np.array(bbs, np.float32)
        out.update({f'{r}_props_nvert': np.array(props['nvert'], np.int64), f'{r}_props_ntri': np.array(props['ntri'], np.int64),
                    f'{r}_props_bb': np.array(props['bb'], np.float64), f'{r}_props_area': np.array(props['area'], np.float64)})
    # the cases
    assert len(out['a0_ids']) and 9 in out['a0_ids'] and out['a0_vert_begin'][list(out['a0_ids']).index(9) + 1] == out['a0_vert_begin'][list(out['a0_ids']).index(9)]
    assert out['b0_vert_begin'][list(out['b0_ids']).index(9) + 1] - out['b0_vert_begin'][list(out['b0_ids']).index(9)] > 0
    assert 5 in out['b0_ids'] and 5 in out['b1_ids'] and 7 in out['b1_ids'] and 7 in out['b2_ids'] and U(2 ** 40 + 3) in out['b2_ids']
    assert (out['b_props_nvert'] == 0).any() and (out['b_props_nvert'] > 0).any()
    path = os.path.join(HERE, 'g25_meshes.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
