"""Surface meshes of labelled objects on the device: ``find_meshes`` of the reference (/root/reference/syconn/proc/meshes.py:937-994)
for all labels of a chunk in one pass, the merge of per-chunk meshes and the ``mesh_bb`` / ``mesh_area`` of step 2 of
``map_subcell_extract_props`` (proc/sd_proc.py:951-975), over ``sd_mesh_count`` / ``sd_mesh_build`` / ``sd_mesh_merge``.

What differs from the reference, which meshes with ``zmesh.Mesher`` (marching cubes, then a simplifier):
* the surface is the UNSIMPLIFIED marching-cubes surface: ``simplification_factor`` and ``max_simplification_error`` of
  ``meshing_props`` are accepted and ignored;
* no normals: ``meshing_props['normals'] = True`` raises ``NotImplementedError``;
* the triangle table is derived from a stated rule (tools/gen_mc_table.py), vertex and triangle order are fixed (include/syconn_dense.h);
* voxel i sits at coordinate i; whether zmesh uses the same half-voxel convention has not been checked (one constant in sd_mesh.hip).
Everything around the mesher is the reference's arithmetic: scipy's ``zoom(chunk, 1 / ds, order=0)`` and numpy's edge pad as source-index
tables (no zoomed or padded copy exists), the offset, the clamp of negative coordinates to 0, the float32 cast, ``merge_meshes`` /
``merge_meshes_incl_norm``, the size thresholds and the ``mesh_bb`` / ``mesh_area`` fallbacks.  The ids of a chunk are found on the host
(``np.unique``, as the reference does) unless the caller passes them.  No CPU fallback: without the library or a device the calls raise."""
from typing import Dict, List, Optional, Sequence

import numpy as np

from ..extraction.spinehead import zoom_source_table


# ---------------------------------------------------------------------------------------------------------------------------------
# numpy drop-ins of the reference's helpers
def get_bounding_box(coordinates: np.ndarray):
    """Center of the coordinates and the largest distance to it along any axis (proc/meshes.py:363-381)."""
    if coordinates.ndim == 2 and coordinates.shape[1] == 3:
        coord_resh = coordinates
    else:
        coord_resh = coordinates.reshape(len(coordinates) // 3, 3)
    mean = np.mean(coord_resh, axis=0)
    max_dist = np.max(np.abs(coord_resh - mean))
    return mean, max_dist


def _merge(ind_lst, vert_lst, nb_simplices):
    all_vert = np.concatenate(vert_lst)
    vert_offset = np.cumsum([0, ] + [len(verts) // nb_simplices for verts in vert_lst]).astype(np.uint64)
    ind_ixs = np.cumsum([0, ] + [len(inds) for inds in ind_lst])
    all_ind = np.concatenate(ind_lst)
    for i in range(0, len(vert_lst)):
        all_ind[ind_ixs[i]:ind_ixs[i + 1]] += vert_offset[i]
    return all_ind, all_vert


def merge_meshes(ind_lst, vert_lst, nb_simplices=3):
    """Several meshes as one: flat indices shifted by the vertices before them (proc/meshes.py:453-480).  No mesh: three empty arrays."""
    assert len(vert_lst) == len(ind_lst), "Length of indices list differs from vertices list."
    if len(vert_lst) == 0:
        return [np.zeros((0,), dtype=np.uint64), np.zeros((0,)), np.zeros((0,))]
    return _merge(ind_lst, vert_lst, nb_simplices)


def merge_meshes_incl_norm(ind_lst, vert_lst, norm_lst, nb_simplices=3):
    """``merge_meshes`` with the concatenated normals as third entry (proc/meshes.py:483-519)."""
    assert len(vert_lst) == len(ind_lst), "Length of indices list differs from vertices list."
    if len(vert_lst) == 0:
        return [np.zeros((0,), dtype=np.uint64), np.zeros((0,)), np.zeros((0,))]
    all_norm = np.zeros((0,)) if len(norm_lst) == 0 else np.concatenate(norm_lst)
    all_ind, all_vert = _merge(ind_lst, vert_lst, nb_simplices)
    return [all_ind, all_vert, all_norm]


def mesh_area_calc(mesh) -> float:
    """Area in um^2 of ``mesh = [indices, vertices, ...]`` (proc/meshes.py:1113-1124): ``0.5 * sum |cross|`` in float64, divided by 1e6."""
    p = np.asarray(mesh[1], np.float64).reshape(-1, 3)[np.asarray(mesh[0]).reshape(-1, 3).astype(np.int64)]
    a, b = p[:, 0] - p[:, 1], p[:, 0] - p[:, 2]
    return np.sqrt((np.cross(a, b) ** 2).sum(axis=1)).sum() / 2. / 1e6


# ---------------------------------------------------------------------------------------------------------------------------------
# view normalisation and view rotations (proc/meshes.py:69-175, :236-360)
class MeshObject(object):
    """The normalisation members of the reference's ``MeshObject`` (proc/meshes.py:69-175): flat float32 ``vertices`` centred on
    ``center`` and divided by ``max_dist`` (both float32), flat uint64 ``indices``, ``vert_resh``, ``transform_external_coords``,
    ``retransform_external_coords``, ``bounding_box``, ``vertices_scaled``.  Normals, colours and the PCA members are not built."""

    def __init__(self, object_type, indices, vertices, normals=None, color=None, bounding_box=None):
        self.object_type = object_type
        vertices, indices = np.asarray(vertices), np.asarray(indices)
        if vertices.ndim == 2 and vertices.shape[1] == 3:
            self.vertices = vertices.flatten()
        else:
            self.vertices = np.array(vertices, dtype=np.float32)
        if indices.ndim == 2 and indices.shape[1] == 3:
            self.indices = indices.flatten().astype(np.uint64)
        else:
            self.indices = np.array(indices, dtype=np.uint64)
        if len(self.vertices) == 0:
            self.center, self.max_dist = 0, 1
            return
        if bounding_box is None:
            self.center, self.max_dist = get_bounding_box(self.vertices)
        else:
            self.center, self.max_dist = bounding_box[0], bounding_box[1]
        self.center = np.asarray(self.center).astype(np.float32)
        self.max_dist = np.asarray(self.max_dist).astype(np.float32)
        vert_resh = np.array(self.vertices).reshape((len(self.vertices) // 3, 3))
        vert_resh -= np.array(self.center, dtype=self.vertices.dtype)
        vert_resh = vert_resh / np.array(self.max_dist)
        self.vertices = vert_resh.reshape(len(self.vertices))

    @property
    def vert_resh(self):
        return np.array(self.vertices).reshape(-1, 3)

    def transform_external_coords(self, coords):
        if len(coords) == 0:
            return coords
        coords = np.array(coords, dtype=np.float32)
        coords = coords - self.center
        coords /= self.max_dist
        return coords

    def retransform_external_coords(self, coords):
        coords = np.array(coords, dtype=np.float32)
        coords *= self.max_dist
        coords += self.center
        return coords.astype(np.int32)

    @property
    def bounding_box(self):
        return [self.center, self.max_dist]

    @property
    def vertices_scaled(self):
        return (self.vert_resh * self.max_dist + self.center).flatten()


def _scalar_edge(name, edge_length):
    if not np.isscalar(edge_length):
        edge_length = np.min(edge_length)                                          # the reference warns and takes the smallest
    edge_length = np.float32(edge_length)
    if not np.isfinite(edge_length) or edge_length < 0:
        raise ValueError(f'{name}: edge_length must be a finite, non-negative number')
    return edge_length


def rot_vertex_stride(n_vertices: int) -> int:
    """``vertices[::8]`` above 1e5 vertices (proc/meshes.py:258-259)."""
    return 8 if n_vertices > 1e5 else 1


def calc_rot_matrices_device(verts_d, coords_d, center, max_dist, edge_length, dev, stride=None, flag_only=False):
    """``sd_views_rotations`` / ``sd_views_flag_empty`` over device tensors: raw float32 vertices and locations with the normalisation
    (`center`, `max_dist`) the kernels apply to both; `edge_length` in normalised units -> float64 (N, 16) on the device, or the
    uint8 "no inlier" flags."""
    import ctypes as C
    from .. import _dev as D
    n_verts, n = int(verts_d.shape[0]), int(coords_d.shape[0])
    stride = rot_vertex_stride(n_verts) if stride is None else int(stride)
    c3 = (C.c_float * 3)(*[float(v) for v in np.asarray(center, np.float32).reshape(3)])
    cnt = D.counters(dev)
    tmp = D.scratch('sd_views_rotations_temp_bytes', dev, n_verts, stride)
    head = (verts_d if n_verts else None, n_verts, stride, coords_d, n, c3, float(max_dist), float(edge_length))
    if flag_only:
        out = D.empty(n, D.u8, dev)
        D.call('sd_views_flag_empty', dev, *head, out, cnt, tmp, tmp.numel())
    else:
        out = D.empty((n, 16), D.f64, dev)
        D.call('sd_views_rotations', dev, *head, out, None, cnt, tmp, tmp.numel())
    return out[:n]


def _rot_inputs(name, coords, vertices, edge_length, device):
    from .. import _dev as D
    edge_length = _scalar_edge(name, edge_length)
    coords = np.array(coords, dtype=np.float32).reshape(-1, 3)
    vertices = np.asarray(vertices).reshape(-1, 3).astype(np.float32)
    if not (np.isfinite(coords).all() and np.isfinite(vertices).all()):
        raise ValueError(f'{name}: coordinates and vertices must be finite')
    dev = D.device(device)
    return D.up(vertices, dev), D.up(coords, dev), edge_length, dev


def calc_rot_matrices(coords: np.ndarray, vertices: np.ndarray, edge_length, nb_cpus: int = 1, device=None) -> np.ndarray:
    """Drop-in of the reference's ``calc_rot_matrices`` (proc/meshes.py:236-329): per location the flat (Fortran order) 4 x 4 matrix
    whose rows are the principal axes of the vertices inside the box of `edge_length` around it, 16 zeros for <= 2 inliers; every 8th
    vertex above 1e5.  `coords` and `vertices` are normalised already.  The sign of a row is this build's (the component of largest
    magnitude is positive; ``np.linalg.eig`` leaves it to LAPACK)."""
    from .. import _dev as D
    verts_d, coords_d, edge_length, dev = _rot_inputs('calc_rot_matrices', coords, vertices, edge_length, device)
    if coords_d.shape[0] == 0:
        return np.zeros((0, 16))
    return D.down(calc_rot_matrices_device(verts_d, coords_d, np.zeros(3, np.float32), 1.0, edge_length, dev))


def flag_empty_spaces(coords: np.ndarray, vertices: np.ndarray, edge_length, device=None) -> np.ndarray:
    """Drop-in of the reference's ``flag_empty_spaces`` (proc/meshes.py:332-360): True where no vertex lies inside the box; every 8th
    vertex above 1e6."""
    from .. import _dev as D
    verts_d, coords_d, edge_length, dev = _rot_inputs('flag_empty_spaces', coords, vertices, edge_length, device)
    if coords_d.shape[0] == 0:
        return np.zeros(0, bool)
    stride = 8 if verts_d.shape[0] > 1e6 else 1
    return D.down(calc_rot_matrices_device(verts_d, coords_d, np.zeros(3, np.float32), 1.0, edge_length, dev, stride, True)).astype(bool)


# ---------------------------------------------------------------------------------------------------------------------------------
class MeshTable:
    """Meshes of the objects of one label volume kind, plain numpy, a CSR by object: ``ids`` uint64 ascending, ``vert_begin`` /
    ``tri_begin`` uint64 (n + 1), ``vertices`` float32 (v, 3) in nm, ``indices`` uint32 (t, 3) local to the object, ``mesh_bb`` float32
    (n, 2, 3) (zeros without vertices; float64 where ``mesh_props`` has filled in scaled voxel boxes), ``mesh_area`` float64 (n) in um^2."""

    def __init__(self, ids, vert_begin, tri_begin, vertices, indices, mesh_bb, mesh_area):
        self.ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        self.vert_begin = np.ascontiguousarray(vert_begin, np.uint64).reshape(-1)
        self.tri_begin = np.ascontiguousarray(tri_begin, np.uint64).reshape(-1)
        self.vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        self.indices = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
        self.mesh_bb = np.ascontiguousarray(mesh_bb, np.float64 if np.asarray(mesh_bb).dtype == np.float64 else np.float32).reshape(-1, 2, 3)
        self.mesh_area = np.ascontiguousarray(mesh_area, np.float64).reshape(-1)
        n = len(self.ids)
        if not (len(self.vert_begin) == len(self.tri_begin) == n + 1 and len(self.mesh_bb) == len(self.mesh_area) == n):
            raise ValueError(f'MeshTable: {n} ids do not match the offsets or the per-object arrays')
        if int(self.vert_begin[-1]) != len(self.vertices) or int(self.tri_begin[-1]) != len(self.indices):
            raise ValueError('MeshTable: the offsets do not end at the number of vertices / triangles')

    def __len__(self):
        return len(self.ids)

    @classmethod
    def empty(cls):
        z = np.zeros(1, np.uint64)
        return cls(np.zeros(0, np.uint64), z, z, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), np.zeros((0, 2, 3), np.float32), np.zeros(0))

    def as_dict(self) -> Dict[int, List[np.ndarray]]:
        """id -> [indices flat uint32, vertices flat float32, empty float32 normals]: the reference's dictionary."""
        vb, tb = self.vert_begin.astype(np.int64), self.tri_begin.astype(np.int64)
        return {int(i): [self.indices[tb[k]:tb[k + 1]].reshape(-1), self.vertices[vb[k]:vb[k + 1]].reshape(-1), np.zeros((0,), np.float32)]
                for k, i in enumerate(self.ids)}

    def mesh_of(self, obj_id):
        """``[indices flat uint32, vertices flat float32, empty float32 normals]`` of one object, the form ``sso.mesh`` and
        ``sso.load_mesh`` have and the view functions of ``proc/rendering.py`` take; empty arrays for an id the table does not hold."""
        k = int(np.searchsorted(self.ids, np.uint64(obj_id)))
        if k >= len(self.ids) or self.ids[k] != np.uint64(obj_id):
            return [np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(0, np.float32)]
        vb, tb = self.vert_begin.astype(np.int64), self.tri_begin.astype(np.int64)
        return [self.indices[tb[k]:tb[k + 1]].reshape(-1), self.vertices[vb[k]:vb[k + 1]].reshape(-1), np.zeros(0, np.float32)]

    def vertices_of(self, ids):
        """``(vertices, vert_begin)`` of the objects `ids` in their order, as ``OrganelleTable`` / ``CellTable`` take them: float32 (w, 3)
        and int64 (len(ids) + 1).  An id the table does not hold has no vertices."""
        ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        if len(self.ids) == 0 or len(ids) == 0:
            return np.zeros((0, 3), np.float32), np.zeros(len(ids) + 1, np.int64)
        row = np.minimum(np.searchsorted(self.ids, ids), len(self.ids) - 1)
        vb = self.vert_begin.astype(np.int64)
        n = np.where(self.ids[row] == ids, vb[row + 1] - vb[row], 0)
        begin = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
        take = np.repeat(vb[row] - begin[:-1], n) + np.arange(begin[-1])
        return self.vertices[take], begin

    @staticmethod
    def merge(tables: Sequence['MeshTable'], device=None) -> 'MeshTable':
        """One table of all objects of `tables`: the pieces of an object one after another in the order of the list, indices shifted
        by the vertices before them, seam vertices kept twice (``merge_meshes_incl_norm`` per object, proc/sd_proc.py:957-964); ``mesh_bb``
        and ``mesh_area`` of the merged meshes.  One stable sort by id, one scan and one gather on the device."""
        from .. import _dev as D
        tables = [t for t in tables if len(t)]
        dev = D.device(device)
        if not tables:
            return MeshTable.empty()
        ids = np.concatenate([t.ids for t in tables])
        v0 = np.cumsum([0] + [len(t.vertices) for t in tables]).astype(np.uint64)
        t0 = np.cumsum([0] + [len(t.indices) for t in tables]).astype(np.uint64)
        vb = np.concatenate([t.vert_begin[:-1] + v0[k] for k, t in enumerate(tables)] + [v0[-1:]])
        tb = np.concatenate([t.tri_begin[:-1] + t0[k] for k, t in enumerate(tables)] + [t0[-1:]])
        verts, tris = np.concatenate([t.vertices for t in tables]), np.concatenate([t.indices for t in tables])
        P, NV, NT = len(ids), len(verts), len(tris)
        o_ids, o_vb, o_tb = D.empty(P, D.i64, dev), D.empty(P + 1, D.i64, dev), D.empty(P + 1, D.i64, dev)
        o_v, o_t = D.empty((NV, 3), torch_f32(), dev), D.empty((NT, 3), D.i32, dev)
        o_bb, o_area = D.empty((P, 6), torch_f32(), dev), D.empty(P, D.f64, dev)
        cnt = D.counters(dev)
        tmp = D.scratch('sd_mesh_merge_temp_bytes', dev, P)
        D.call('sd_mesh_merge', dev, D.up(ids, dev), D.up(vb, dev), D.up(tb, dev), P, D.up(verts, dev) if NV else None, NV,
               D.up(tris, dev) if NT else None, NT, o_ids, o_vb, o_tb, o_v, o_t, o_bb, o_area, cnt, tmp, tmp.numel())
        c = D.down(cnt)
        if c[7]:
            raise ValueError('MeshTable.merge: an offset table does not ascend from 0 to its total')
        n = int(c[0])
        return MeshTable(D.down(o_ids, n, np.uint64), D.down(o_vb, n + 1, np.uint64), D.down(o_tb, n + 1, np.uint64), D.down(o_v, NV),
                         D.down(o_t, NT, np.uint32), D.down(o_bb, n).reshape(n, 2, 3), D.down(o_area, n))


def torch_f32():
    import torch
    return torch.float32


# ---------------------------------------------------------------------------------------------------------------------------------
def _source_tables(shape, pad: int, ds):
    """Per axis the int32 source index of every sample of ``np.pad(zoom(chunk, 1 / ds, order=0), 1, mode='edge')`` (pad > 0) or of the
    zoomed chunk."""
    out = []
    for k in range(3):
        t = zoom_source_table(shape[k], ds[k]) if ds is not None else np.arange(shape[k], dtype=np.int32)
        if pad > 0:
            t = np.concatenate((t[:1], t, t[-1:]))
        out.append(np.ascontiguousarray(t, np.int32))
    return out


def _check_args(chunk_shape, offset, pad, ds, scaling, meshing_props):
    from .. import global_params
    if len(chunk_shape) != 3 or min(chunk_shape) < 1:
        raise ValueError(f'find_meshes: chunk must be a non-empty 3D array, got shape {tuple(chunk_shape)}')
    if pad not in (0, 1):
        raise ValueError(f'find_meshes: pad must be 0 or 1 (the reference pads by 1 for any pad > 0 but shifts the offset by pad), got {pad}')
    offset = np.asarray(offset, np.float64).reshape(-1)
    if offset.shape != (3,):
        raise ValueError('find_meshes: offset must have three entries')
    scaling = np.array(global_params.config['scaling'] if scaling is None else scaling, np.float64).reshape(-1)
    if scaling.shape != (3,) or not (scaling > 0).all():
        raise ValueError('find_meshes: scaling must be three positive numbers')
    if ds is not None:
        ds = np.array(ds, np.float64).reshape(-1)
        if ds.shape != (3,) or not (ds > 0).all():
            raise ValueError('find_meshes: ds must be three positive numbers')
    if meshing_props is None:
        meshing_props = global_params.config['meshes']['meshing_props']
    unknown = set(meshing_props) - {'normals', 'simplification_factor', 'max_simplification_error'}
    if unknown:
        raise ValueError(f'find_meshes: unknown meshing_props {sorted(unknown)}')
    if meshing_props.get('normals', False):
        raise NotImplementedError('find_meshes: normals are not built')
    return offset, scaling, ds


def find_meshes_table(chunk, offset, pad: int = 0, ds=None, scaling=None, meshing_props: Optional[dict] = None, device=None, ids=None) -> MeshTable:
    """The meshes of all non-zero labels of `chunk` ((x, y, z) integer labels, numpy or a device tensor of 8-byte integers) as a
    ``MeshTable``, vertices in nm: the reference's ``find_meshes`` (see the module docstring for what differs).  `offset` in voxels;
    `pad` 0 or 1; `ds` the downsampling per axis; `scaling` the voxel size (default: the configuration's).  `ids` (ascending, without
    0) may name the objects where the caller knows them; an id that loses all its voxels in the zoom keeps an empty entry."""
    import torch
    from .. import _dev as D
    offset, scaling, ds = _check_args(tuple(chunk.shape), offset, pad, ds, scaling, meshing_props)
    dev = D.device(device)
    if isinstance(chunk, torch.Tensor):
        if chunk.dtype != torch.int64:
            raise ValueError('find_meshes: a device chunk must hold 8-byte labels (int64 bits of uint64)')
        vol = chunk.to(dev).contiguous()
        if ids is None:
            ids = np.unique(D.down(torch.unique(vol), view=np.uint64))
    else:
        host = np.ascontiguousarray(chunk)
        if host.dtype.kind not in 'iub':
            raise ValueError(f'find_meshes: integer labels expected, got {host.dtype}')
        host = host.astype(np.uint64, copy=False)
        if ids is None:
            ids = np.unique(host)
        vol = D.up(host, dev)
    ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
    ids = ids[ids != 0]
    X, Y, Z = (int(v) for v in vol.shape)
    tabs = _source_tables((X, Y, Z), pad, ds)
    NX, NY, NZ = (len(t) for t in tabs)
    s_ds = scaling * ds if ds is not None else scaling
    off = offset * scaling - (pad * s_ds if pad > 0 else 0.0)
    n = len(ids)
    if n == 0:
        return MeshTable.empty()
    tx, ty, tz = (D.up(t, dev) for t in tabs)
    ids_dev = D.up(ids, dev)
    cnt = D.counters(dev)
    D.call('sd_mesh_count', dev, vol, X, Y, Z, tx, ty, tz, NX, NY, NZ, ids_dev, n, cnt)
    c = D.down(cnt)
    _check_counts('sd_mesh_count', c)
    nv, nt = int(c[0]), int(c[1])
    vb, tb = D.empty(n + 1, D.i64, dev), D.empty(n + 1, D.i64, dev)
    verts, tris = D.empty((nv, 3), torch.float32, dev), D.empty((nt, 3), D.i32, dev)
    bb, area = D.empty((n, 6), torch.float32, dev), D.empty(n, D.f64, dev)
    tmp = D.scratch('sd_mesh_build_temp_bytes', dev, NX, NY, NZ, nv, nt)
    D.call('sd_mesh_build', dev, vol, X, Y, Z, tx, ty, tz, NX, NY, NZ, ids_dev, n, D.f64x3(s_ds), D.f64x3(off), nv, nt, vb, tb, verts, tris, bb,
           area, cnt, tmp, tmp.numel())
    c = D.down(cnt)
    _check_counts('sd_mesh_build', c)
    if c[2] or c[5]:
        raise RuntimeError('sd_mesh_build: the counted capacities did not hold the mesh (internal error)')
    return MeshTable(ids, D.down(vb, n + 1, np.uint64), D.down(tb, n + 1, np.uint64), D.down(verts, nv), D.down(tris, nt, np.uint32),
                     D.down(bb, n).reshape(n, 2, 3), D.down(area, n))


def _check_counts(who, c):
    if c[7]:
        raise ValueError(f'{who}: a source table entry is out of range or the ids do not ascend strictly')
    if c[6]:
        raise ValueError(f'{who}: the chunk holds a label that is not in ids')


def find_meshes(chunk, offset, pad: int = 0, ds=None, scaling=None, meshing_props: Optional[dict] = None, device=None) -> Dict[int, List[np.ndarray]]:
    """Drop-in of the reference's ``find_meshes``: id -> [indices flat uint32, vertices flat float32 in nm, empty float32 normals] for
    every non-zero label of `chunk`, ids without a surface after the zoom included (empty arrays)."""
    return find_meshes_table(chunk, offset, pad, ds, scaling, meshing_props, device).as_dict()


def mesh_props(table: MeshTable, prop_table, scaling, min_obj_vx: int, mesh_min_obj_vx: int) -> MeshTable:
    """The meshes and attributes step 2 stores per object of `prop_table` (a ``PropTable``; proc/sd_proc.py:951-975): an object with
    ``size < mesh_min_obj_vx or size < min_obj_vx``, or without vertices, gets an empty mesh, ``mesh_bb = bounding_box * scaling`` and
    area 0; every other object its mesh of `table`, the minimum / maximum of its vertices and its area.  -> a ``MeshTable`` over
    ``prop_table.ids``."""
    scaling = np.asarray(scaling, np.float64)
    ids = np.ascontiguousarray(prop_table.ids, np.uint64)
    n = len(ids)
    row = np.searchsorted(table.ids, ids)
    known = row < len(table)
    known[known] = table.ids[row[known]] == ids[known]
    row = np.where(known, row, 0)
    vb, tb = table.vert_begin.astype(np.int64), table.tri_begin.astype(np.int64)
    sizes = np.asarray(prop_table.sizes, np.int64)
    nv = np.where(known, vb[row + 1] - vb[row], 0) if len(table) else np.zeros(n, np.int64)
    keep = known & ~((sizes < mesh_min_obj_vx) | (sizes < min_obj_vx)) & (nv > 0)
    nv = np.where(keep, nv, 0)
    ntri = np.where(keep, tb[row + 1] - tb[row], 0) if len(table) else np.zeros(n, np.int64)
    bb, area = np.zeros((n, 2, 3), np.float64), np.zeros(n, np.float64)
    box_begin = np.asarray(prop_table.box_begin, np.int64)
    verts, tris = [], []
    for k in range(n):
        if keep[k]:
            r = row[k]
            bb[k], area[k] = table.mesh_bb[r], table.mesh_area[r]
            verts.append(table.vertices[vb[r]:vb[r + 1]])
            tris.append(table.indices[tb[r]:tb[r + 1]])
        else:
            boxes = np.asarray(prop_table.boxes[box_begin[k]:box_begin[k + 1]])
            bb[k] = np.array([boxes[:, 0].min(axis=0), boxes[:, 1].max(axis=0)]) * scaling
    begin = lambda c: np.concatenate(([0], np.cumsum(c))).astype(np.uint64)
    return MeshTable(ids, begin(nv), begin(ntri), np.concatenate(verts) if verts else np.zeros((0, 3), np.float32),
                     np.concatenate(tris) if tris else np.zeros((0, 3), np.uint32), bb, area)
