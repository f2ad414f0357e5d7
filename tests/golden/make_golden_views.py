"""Golden vectors for the view half, produced by the REFERENCE'S OWN code where it can run without OpenGL: ``MeshObject.__init__`` and
``transform_external_coords`` (/root/reference/syconn/proc/meshes.py:69-165), ``get_bounding_box`` (:363-381), ``calc_rot_matrices_helper``,
``get_rotmatrix_from_points`` and ``_calc_pca_components`` (:269-329), ``flag_empty_spaces`` (:332-360), ``id2rgba_array_contiguous`` /
``id2rgb_array_contiguous`` / ``rgba2id_array`` (handler/multiviews.py), ``semseg2mesh_counter`` (reps/super_segmentation_helper.py:
1527-1551) and ``colorcode_vertices`` (reps/rep_helper.py:281-340) are lifted by AST at generation time and run unchanged.  Stand-ins:
numba's ``@jit`` is dropped, ``in_bounding_box`` (a Cython extension) is restated, ``np.bool`` is ``bool``, cKDTree's ``n_jobs`` is
``workers``.  The arithmetic of ``semseg2mesh`` between the view loading and the storage (:1603-1645) is typed out here over the lifted
counter.  Nothing compiled and no reference text is stored: inputs and outputs only.

    python tests/golden/make_golden_views.py      ->  tests/golden/g27_views.npz

``m_``: the bent tube (``verts`` float32 nm, ``tris``), 40 locations ``coords``, ``comp_window``; MeshObject's ``center`` / ``max_dist`` /
``vn`` (normalised vertices) / ``cn`` (transform_external_coords), ``edge`` (the query box edge), ``rot`` (40, 16), ``empty``.
``r_``: point clouds ``verts`` (normalised already) around ``coords``, ``edge``, the reference's ``rot``, ``empty`` and ``n_in`` (inliers
per location), ``gap_ok`` (every eigenvalue gap >= 0.05 of the largest eigenvalue).  ``i_``: ``n`` ids through id2rgba -> rgba2id
(``ids``) and the background ``bg``.  ``v_``: ``index`` / ``labels`` pixels, ``n_verts``, ``verts``, ``bg``, ``bg_l``, the uint8 ``table``, ``vertex_labels``,
``k0`` and ``k1`` (semseg2mesh's result for k = 0 and k = 1)."""
import os
import sys
from collections import Counter

import numpy as np
import scipy.spatial

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _views_ref as R  # noqa: E402
from make_golden_cs import lift_function  # noqa: E402
from make_golden_syn_props import lift_method  # noqa: E402
from make_golden_syn_ssv import lift_patched  # noqa: E402

REF = '/root/reference/syconn'


def in_bounding_box(coords, bounding_box):
    """extraction/in_bounding_boxC.pyx: differences in the arrays' precision, the half edge a C float, strict on both sides."""
    coords = np.asarray(coords)
    bb = np.asarray(bounding_box, dtype=coords.dtype)
    edge = (bb[1] / 2).astype(np.float32)
    d = coords - bb[0]
    return ((d > -edge) & (d < edge)).all(1)


def namespace():
    if not hasattr(np, 'bool'):
        np.bool = bool
    ns = {'np': np, 'in_bounding_box': in_bounding_box, 'spatial': scipy.spatial, 'Counter': Counter,
          'start_multiprocess_imap': lambda f, params, **kw: [f(p) for p in params]}
    exec('from typing import *', ns)
    p = f'{REF}/proc/meshes.py'
    for name in ('get_bounding_box', '_calc_pca_components', 'get_rotmatrix_from_points', 'calc_rot_matrices_helper', 'flag_empty_spaces'):
        lift_function(p, name, ns)
    init, tec = lift_method(p, 'MeshObject', '__init__', ns), lift_method(p, 'MeshObject', 'transform_external_coords', ns)
    ns['MeshObject'] = type('MeshObject', (), {'__init__': init, 'transform_external_coords': tec,
                                                'vert_resh': property(lambda self: np.array(self.vertices).reshape(-1, 3))})
    p = f'{REF}/handler/multiviews.py'
    for name in ('id2rgb_array_contiguous', 'id2rgba_array_contiguous', 'rgba2id_array'):
        lift_function(p, name, ns)
    lift_function(f'{REF}/reps/super_segmentation_helper.py', 'semseg2mesh_counter', ns)
    lift_patched(f'{REF}/reps/rep_helper.py', 'colorcode_vertices', ns, 'n_jobs=nb_cpus', 'workers=1')
    return ns


def tube(ns, rng):
    verts, tris = R.bent_tube()
    pick = rng.choice(len(verts), 40, replace=False)
    coords = (verts[pick].astype(np.float64) + rng.normal(0, 150, (40, 3))).astype(np.float32)
    coords[-1] = verts.mean(0) + 60000                                             # far away: no inlier, a zero matrix
    comp_window = 8000.0
    mo = ns['MeshObject']('raw', tris.reshape(-1), verts.reshape(-1).copy())
    cn = mo.transform_external_coords(coords)
    edge = comp_window / mo.max_dist                                               # render_sso_coords :262
    rot = ns['calc_rot_matrices_helper']((cn, mo.vert_resh, edge))
    empty = ns['flag_empty_spaces'](cn, mo.vert_resh, edge)
    assert mo.vertices.dtype == np.float32 and cn.dtype == np.float32 and empty[-1] and not empty[:-1].any() and not rot[-1].any()
    assert np.array_equal(mo.vert_resh, R.normalise(verts, mo.center, mo.max_dist)) and np.array_equal(cn, R.normalise(coords, mo.center, mo.max_dist))
    return dict(m_verts=verts, m_tris=tris, m_coords=coords, m_comp_window=np.float64(comp_window), m_center=mo.center, m_max_dist=mo.max_dist,
                m_vn=mo.vert_resh, m_cn=cn, m_edge=np.float32(edge), m_rot=rot, m_empty=empty)


def clouds(ns, rng):
    edge = np.float32(0.25)
    h = np.float32(edge / 2)
    verts, coords = [], []
    def add(c, pts):
        coords.append(np.asarray(c, np.float32))
        verts.append(np.asarray(pts, np.float32).reshape(-1, 3))
    for k in range(48):
        c = np.array([(k % 6) - 2.5, ((k // 6) % 4) - 1.5, (k // 24) - 0.5]) * 0.5 + rng.normal(0, 0.01, 3)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        sd = np.array([0.05, 0.028, 0.012]) * rng.uniform(0.8, 1.2)
        add(c, c + (rng.normal(size=(int(rng.integers(40, 400)), 3)) * sd) @ q.T)
    add([5, 5, 5], np.zeros((0, 3)))                                               # 0 inliers
    add([6, 5, 5], [[6.01, 5, 5], [5.99, 5.01, 5]])                                # 2 inliers: zeros
    add([7, 5, 5], [[7.05, 5, 5], [6.98, 5.03, 5], [7.0, 4.99, 5.02]])             # 3 inliers
    c = np.array([8, 5, 5], np.float32)                                            # points exactly on the faces are outside
    face = [c + [h, 0, 0], c - [0, h, 0], c + [0, 0, h]]
    add(c, face + list(c + (rng.normal(size=(60, 3)) * [0.04, 0.02, 0.01])))
    coords, verts = np.stack(coords), np.concatenate(verts)
    for f in face:
        assert not in_bounding_box(np.asarray([f], np.float32), np.array([c, [edge] * 3], np.float32))[0]
    rot = ns['calc_rot_matrices_helper']((coords, verts, edge))
    empty = ns['flag_empty_spaces'](coords, verts, edge)
    n_in = np.array([in_bounding_box(verts, np.array([cc, [edge] * 3], np.float32)).sum() for cc in coords])
    gap_ok = np.zeros(len(coords), bool)
    for n, cc in enumerate(coords):
        pts = verts[in_bounding_box(verts, np.array([cc, [edge] * 3], np.float32))].astype(np.float64)
        if len(pts) > 2:
            ev = np.sort(np.linalg.eigvalsh(np.cov(pts, rowvar=False)))[::-1]
            gap_ok[n] = min(ev[0] - ev[1], ev[1] - ev[2]) >= 0.05 * ev[0]
    assert n_in[48:52].tolist()[:3] == [0, 2, 3] and n_in[51] == 60 and gap_ok[:48].sum() >= 40 and empty.tolist() == (n_in == 0).tolist()
    assert not rot[48].any() and not rot[49].any() and rot[50].any()
    return dict(r_verts=verts, r_coords=coords, r_edge=edge, r_rot=rot, r_empty=empty, r_n_in=n_in, r_gap_ok=gap_ok)


def ids(ns):
    n = 70000                                                                      # past 256^2: three colour bytes in use
    rgba = ns['id2rgba_array_contiguous'](np.arange(n))
    back = ns['rgba2id_array'](rgba.astype(np.int64))                          # the bytes as int64: NumPy >= 2 refuses uint8 * 256
    bg = ns['rgba2id_array'](np.full((1, 4), 255, np.int64))
    assert np.array_equal(back, np.arange(n)) and int(bg[0]) == R.BG_INDEX
    return dict(i_n=np.int64(n), i_ids=back, i_bg=bg)


def vote(ns, rng):
    n_verts, bg_l = 300, 4
    verts = rng.uniform(0, 1000, (n_verts, 3)).astype(np.float32)
    bg = np.uint32(R.BG_INDEX)
    idx, lab = [], []
    def hits(v, l, n):
        idx.extend([v] * n); lab.extend([l] * n)
    hits(0, 1, 255)                                                                # 255 hits: the count 255
    hits(1, 1, 256)                                                                # 256 hits wrap to 0: unpredicted
    hits(2, 2, 257)                                                                # 257 hits: the count 1 ...
    hits(2, 3, 2)                                                                  # ... which loses against 2
    hits(3, 2, 5); hits(3, 1, 5)                                                   # a tie: the first label
    hits(4, bg_l, 3)                                                               # a vertex that is background by its label
    for v in range(10, 200):
        for l in rng.integers(0, bg_l, int(rng.integers(1, 4))):
            hits(v, int(l), int(rng.integers(1, 9)))
    hits(int(bg), bg_l, 500)                                                       # background pixels
    order = rng.permutation(len(idx))
    idx, lab = np.array(idx, np.uint32)[order], np.array(lab, np.uint8)[order]
    # semseg2mesh :1603-1645
    i_views, semseg_views = idx.flatten(), lab.flatten()
    background_id = np.max(i_views)
    background_l = np.max(semseg_views)
    unpredicted_l = background_l + 1
    count_arr = np.zeros((n_verts, background_l + 1), dtype=np.uint8)
    with np.errstate(over='ignore'):
        count_arr = ns['semseg2mesh_counter'](i_views, semseg_views, background_id, count_arr)
    vertex_labels = np.argmax(count_arr, axis=1).astype(np.uint8)
    mask = np.sum(count_arr, axis=1) == 0
    vertex_labels[mask] = unpredicted_l
    k0 = vertex_labels
    predicted_vertices = verts[vertex_labels != unpredicted_l]
    predictions = vertex_labels[vertex_labels != unpredicted_l]
    predicted_vertices = predicted_vertices[predictions != background_l]
    predictions = predictions[predictions != background_l]
    k1 = ns['colorcode_vertices'](verts, predicted_vertices, predictions, k=1, return_color=False, nb_cpus=1)
    assert background_id == bg and background_l == bg_l and count_arr[0, 1] == 255 and count_arr[1, 1] == 0 and count_arr[2, 2] == 1
    assert k0[:5].tolist() == [1, 5, 3, 1, 4] and (k0[200:] == 5).all() and not np.isin(k1, (4, 5)).any()
    mine, table = R.vote(idx, lab, int(bg), n_verts, bg_l + 1, int(unpredicted_l))
    assert np.array_equal(mine, k0) and np.array_equal(table, count_arr)
    return dict(v_index=idx, v_labels=lab, v_n_verts=np.int64(n_verts), v_verts=verts, v_bg=bg, v_bg_l=np.int64(bg_l), v_table=count_arr,
                v_vertex_labels=vertex_labels, v_k0=k0, v_k1=np.asarray(k1, np.int32))


def main():
    rng = np.random.default_rng(2701)
    ns = namespace()
    out = {}
    out.update(tube(ns, rng))
    out.update(clouds(ns, rng))
    out.update(ids(ns))
    out.update(vote(ns, rng))
    path = os.path.join(HERE, 'g27_views.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
