"""Rendering locations of all objects of a vertex table in one device call: ``SegmentationObject.sample_locations`` of the reference
(reps/segmentation.py:700-732) without the storage, over ``sd_locations_voxel`` (``generate_rendering_locs``,
handler/multiviews.py:339-355, the default) and ``sd_locations_surface`` (``surface_samples``, reps/rep_helper.py:376-417, the legacy
rule).  The reference runs one open3d call, or one cKDTree and one ``histogramdd``, per supervoxel
(batchjob_sample_location_caching.py); here the objects are segments of one vertex array, as ``MeshTable.vert_begin`` lays them out.
DESIGN.md section 7 states both rules and what differs (the order of the voxel rule's locations, ties of the nearest vertex).  Not built:
the location storages (``locations.pkl``, the ``sample_locations`` attribute).  No CPU fallback."""
from typing import Dict

import numpy as np

from .. import global_params
from .meshes import MeshTable


class LocationTable:
    """Locations of the objects of a table, a CSR by object: ``ids`` uint64, ``loc_begin`` uint64 (n + 1), ``locations`` float32 (m, 3)
    in nm; numpy, or device tensors (``loc_begin`` then int64) when the call that made it kept them there."""

    def __init__(self, ids, loc_begin, locations):
        self.ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        self.on_device = not isinstance(locations, np.ndarray)
        if self.on_device:
            self.loc_begin, self.locations = loc_begin, locations
        else:
            self.loc_begin = np.ascontiguousarray(loc_begin, np.uint64).reshape(-1)
            self.locations = np.ascontiguousarray(locations).reshape(-1, 3)
        if len(self.loc_begin) != len(self.ids) + 1 or int(self.loc_begin[-1]) != len(self.locations):
            raise ValueError(f'LocationTable: {len(self.ids)} ids do not match the offsets, or the offsets the locations')

    def __len__(self):
        return len(self.ids)

    def host(self) -> 'LocationTable':
        if not self.on_device:
            return self
        return LocationTable(self.ids, self.loc_begin.cpu().numpy().astype(np.uint64), self.locations.cpu().numpy())

    def as_dict(self) -> Dict[int, np.ndarray]:
        """id -> (k, 3) locations: what ``sample_locations`` returns per object."""
        t = self.host()
        lb = t.loc_begin.astype(np.int64)
        return {int(i): t.locations[lb[k]:lb[k + 1]] for k, i in enumerate(t.ids)}

    def locations_of(self, ids):
        """``(locations, loc_begin)`` of the objects `ids` in their order: (w, 3) and int64 (len(ids) + 1).  An id the table does not
        hold has no locations."""
        t = self.host()
        ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        if len(t.ids) == 0 or len(ids) == 0:
            return np.zeros((0, 3), t.locations.dtype), np.zeros(len(ids) + 1, np.int64)
        order = np.argsort(t.ids, kind='stable')
        row = order[np.minimum(np.searchsorted(t.ids[order], ids), len(t.ids) - 1)]
        lb = t.loc_begin.astype(np.int64)
        n = np.where(t.ids[row] == ids, lb[row + 1] - lb[row], 0)
        begin = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
        take = np.repeat(lb[row] - begin[:-1], n) + np.arange(begin[-1])
        return t.locations[take], begin


def check_ds(who, ds_factor) -> float:
    if not np.isscalar(ds_factor) or not np.isfinite(ds_factor) or not ds_factor > 0:
        raise ValueError(f'{who}: ds_factor must be one positive, finite length in nm, got {ds_factor!r}')
    return float(ds_factor)


def check_surface_args(who, bin_sizes, r):
    bs = np.array(bin_sizes, dtype=np.float32).reshape(-1)
    if bs.shape != (3,) or not np.isfinite(bs).all() or not (bs > 0).all():
        raise ValueError(f'{who}: bin_sizes must be three positive, finite lengths, got {bin_sizes!r}')
    if not np.isscalar(r) or not np.isfinite(r) or r < 0:
        raise ValueError(f'{who}: r must be one finite radius >= 0, got {r!r}')
    return bs, float(r)


def check_finite(who, verts):
    if isinstance(verts, np.ndarray) and not np.isfinite(verts).all():
        raise ValueError(f'{who}: a vertex is NaN or infinite')


def locations_device(who, verts_d, begin_d, n_obj: int, dev, ds=None, bin_sizes=None, r=None):
    """The sizing and the emitting call of one rule over device tensors: `verts_d` float32 or float64 (v, 3), `begin_d` int64 bits of
    uint64 (n_obj + 1).  -> (loc_begin int64 (n_obj + 1), locations (m, 3): float64 for the voxel rule (`ds`), float32 for the surface
    rule (`bin_sizes`, `r`)), both on the device."""
    import ctypes as C
    import torch
    from .. import _dev as D
    n_verts = int(verts_d.shape[0])
    if n_verts >= 2 ** 31 or n_obj >= 2 ** 31:
        raise ValueError(f'{who}: vertices and objects < 2^31 per call')
    voxel = ds is not None
    f32 = verts_d.dtype == torch.float32
    loc_begin, cnt = D.empty(n_obj + 1, D.i64, dev), D.counters(dev)
    if voxel:
        name, head = 'sd_locations_voxel', (verts_d if n_verts else None, int(f32), begin_d, n_obj, n_verts, float(ds), loc_begin)
    else:
        name, head = 'sd_locations_surface', (verts_d if n_verts else None, begin_d, n_obj, n_verts, (C.c_float * 3)(*[float(b) for b in bin_sizes]),
                                              float(r), loc_begin)
    tmp = D.scratch(name + '_temp_bytes', dev, n_verts, n_obj)
    D.call(name, dev, *head, None, 0, cnt, tmp, tmp.numel())
    c = D.down(cnt)
    if c[7]:
        raise ValueError(f'{who}: the vertex offsets do not ascend from 0 to the number of vertices')
    if c[5]:
        raise ValueError(f'{who}: a vertex is NaN or infinite')
    if c[4]:
        from .. import _lib as L
        raise ValueError(f'{who}: an object spans more than {L.SD_LOCATIONS_MAX_CELLS} voxels / bins along an axis')
    n = int(c[0])
    loc = D.empty((n, 3), D.f64 if voxel else torch.float32, dev)
    if n:
        D.call(name, dev, *head, loc, n, cnt, tmp, tmp.numel())
        c = D.down(cnt)
        if c[1] or int(c[0]) != n:
            raise RuntimeError(f'{name}: the counted capacity did not hold the locations (internal error)')
    return loc_begin, loc[:n]


def one_object(who, verts, dev, **rule):
    """The locations of one vertex array (numpy) as a host array."""
    from .. import _dev as D
    v = np.ascontiguousarray(verts).reshape(-1, 3)
    begin = D.up(np.array([0, len(v)], np.uint64), dev)
    _, loc = locations_device(who, D.up(v, dev), begin, 1, dev, **rule)
    return D.down(loc)


def _table_parts(meshes):
    if isinstance(meshes, MeshTable):
        return meshes.ids, meshes.vert_begin, meshes.vertices
    if not isinstance(meshes, (tuple, list)) or len(meshes) != 3:
        raise ValueError('sample_locations_table: meshes must be a MeshTable or (ids, vert_begin, vertices)')
    return meshes


def sample_locations_table(meshes, ds_factor=None, use_new_renderings_locs=None, rep_coords=None, scaling=None, device=None,
                           return_device: bool = False) -> LocationTable:
    """``sample_locations`` of every object of `meshes` -- a ``MeshTable`` or ``(ids, vert_begin, vertices)``, the vertices numpy or a
    device tensor (v, 3) -- as a ``LocationTable`` of float32 locations.  `ds_factor` None means 2000; the default rule is the
    configuration's ``views.use_new_renderings_locs``: the voxel rule, else ``surface_samples(verts, [ds_factor] * 3, r=ds_factor / 2)``
    (reps/segmentation.py:721-726).  An object without vertices gets the single location ``np.array([rep_coord], np.float32) * scaling``
    (`rep_coords` (n, 3), `scaling` (3,) or (n, 3)); without them it raises.  With `return_device` offsets and locations stay on the
    device."""
    import torch
    ids, vert_begin, vertices = _table_parts(meshes)
    ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
    n_obj = len(ids)
    vb = np.ascontiguousarray(vert_begin.cpu().numpy() if isinstance(vert_begin, torch.Tensor) else vert_begin).astype(np.uint64).reshape(-1)
    if len(vb) != n_obj + 1:
        raise ValueError(f'sample_locations_table: {n_obj} ids need {n_obj + 1} vertex offsets, got {len(vb)}')
    ds = check_ds('sample_locations_table', 2000 if ds_factor is None else ds_factor)
    if use_new_renderings_locs is None:
        use_new_renderings_locs = global_params.config['views']['use_new_renderings_locs']
    n_verts = int(vertices.shape[0]) if len(vertices.shape) == 2 else int(np.prod(vertices.shape)) // 3
    if n_obj and (vb[0] != 0 or int(vb[-1]) != n_verts or (np.diff(vb.astype(np.int64)) < 0).any()):
        raise ValueError('sample_locations_table: the vertex offsets do not ascend from 0 to the number of vertices')
    empty = vb[1:] == vb[:-1]
    fallback = None
    if empty.any():
        if rep_coords is None or scaling is None:
            raise ValueError('sample_locations_table: an object has no vertices; its location needs rep_coords and scaling')
        rc = np.array(rep_coords, dtype=np.float32).reshape(-1, 3)
        if len(rc) != n_obj:
            raise ValueError(f'sample_locations_table: {len(rc)} rep_coords for {n_obj} objects')
        sc = np.broadcast_to(np.asarray(scaling), (n_obj, 3))
        fallback = (rc[empty] * sc[empty]).astype(np.float32)                    # np.array([rep_coord], np.float32) * scaling
    if not isinstance(vertices, torch.Tensor):
        vertices = np.ascontiguousarray(vertices).reshape(-1, 3)
        if not use_new_renderings_locs and vertices.dtype != np.float32:
            raise NotImplementedError('sample_locations_table: the legacy rule takes float32 vertices only')
        if vertices.dtype not in (np.float32, np.float64):
            vertices = vertices.astype(np.float64)
        check_finite('sample_locations_table', vertices)
    elif vertices.dtype not in (torch.float32, torch.float64) or (not use_new_renderings_locs and vertices.dtype != torch.float32):
        raise NotImplementedError('sample_locations_table: device vertices must be float32 (the voxel rule also takes float64)')
    from .. import _dev as D
    dev = D.device(device)
    if n_obj == 0:
        return LocationTable(ids, np.zeros(1, np.uint64), np.zeros((0, 3), np.float32))
    verts_d = vertices.to(dev).reshape(-1, 3).contiguous() if isinstance(vertices, torch.Tensor) else D.up(vertices, dev)
    rule = dict(ds=ds) if use_new_renderings_locs else dict(bin_sizes=[ds] * 3, r=ds / 2)
    loc_begin, loc = locations_device('sample_locations_table', verts_d, D.up(vb, dev), n_obj, dev, **rule)
    loc = loc.to(torch.float32)                                                  # .astype(np.float32)
    if fallback is not None:
        # one row more for every object without vertices: the rows of the others move back by the empty objects in front of them
        e = D.up(empty, dev).to(torch.int64)
        per = loc_begin[1:] - loc_begin[:-1]
        shift = torch.cumsum(e, 0) - e
        owner = torch.repeat_interleave(torch.arange(n_obj, device=dev), per)
        new_begin = torch.zeros(n_obj + 1, dtype=torch.int64, device=dev)
        new_begin[1:] = torch.cumsum(per + e, 0)
        out = torch.empty((int(loc.shape[0]) + len(fallback), 3), dtype=torch.float32, device=dev)
        out[torch.arange(loc.shape[0], device=dev) + shift[owner]] = loc
        out[new_begin[:-1][e.bool()]] = D.up(fallback, dev)
        loc_begin, loc = new_begin, out
    if return_device:
        return LocationTable(ids, loc_begin, loc)
    return LocationTable(ids, D.down(loc_begin, view=np.uint64), D.down(loc))
