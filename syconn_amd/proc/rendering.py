"""Multi-view depth and index images of cell and organelle meshes on the device: ``render_mesh_coords``, ``render_sso_coords`` and
``render_sso_coords_index_views`` of the reference (proc/rendering.py:95-114, :204-297, :300-396) over ``sd_views_index`` /
``sd_views_candidates`` / ``sd_views_render`` / ``sd_views_render_index``, and the table form ``render_views_table`` that keeps meshes,
indices and views on the device.

The reference renders with OpenGL (proc/rendering_egl.py); this is a compute rasteriser with a rule of its own:
the GL implementation's float32 pipeline, sub-pixel precision, depth quantisation and tie rule are unknown, so views agree with the
reference's in geometry, not bit for bit.  Everything around the raster is the reference's arithmetic: ``MeshObject``'s float32
normalisation, the edge lengths, the view angles, the 8-bit depth, ``gaussian_filter(., .7)`` on the uint8 image, the all-zero rule,
255 for missing meshes and skipped locations, ``rgba2id_array``'s background.  Not built (``NotImplementedError`` where a flag asks for
them): ``clahe``, ``wire_frame``, point rendering, lighting, ``draw_scale``, label views, the view storages.  No CPU fallback."""
from typing import Iterable, Optional, Sequence

import numpy as np

from .. import global_params
from .meshes import calc_rot_matrices_device, get_bounding_box

BG_INDEX = 2 ** 32 - 2


def gauss_weights(sigma: float = 0.7, truncate: float = 4.0) -> np.ndarray:
    """The weights of ``scipy.ndimage.gaussian_filter(img, sigma)`` by scipy's own expression."""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def view_angles(nb_views: int) -> np.ndarray:
    """Degrees of the rotation about x of every view (rendering_egl.py:559-563)."""
    if nb_views == 2:
        return np.array([(-1) ** (m + 1) * 25 for m in range(nb_views)], np.float64)
    return np.array([360. / nb_views * m for m in range(nb_views)], np.float64)


def _check_window(ws, nb_views, comp_window):
    from .. import _lib as L
    ws = tuple(int(v) for v in ws)
    if len(ws) != 2 or min(ws) < 1 or max(ws) > 8192:
        raise ValueError(f'views: ws must be two extents (x, y) in [1, 8192], got {ws}')
    if not 1 <= int(nb_views) <= L.SD_VIEWS_MAX_VIEWS:
        raise ValueError(f'views: nb_views must be in [1, {L.SD_VIEWS_MAX_VIEWS}], got {nb_views}')
    if not np.isscalar(comp_window) or not np.isfinite(comp_window) or comp_window <= 0:
        raise ValueError(f'views: comp_window must be one positive length in nm, got {comp_window!r}')
    return ws, int(nb_views), float(comp_window)


def _not_built(**flags):
    for name, value in flags.items():
        if value:
            raise NotImplementedError(f'views: {name} is not built')


class ViewMesh:
    """One mesh on the device, as the raster takes it: raw float32 vertices, uint32 triangles, ``MeshObject``'s center and max_dist, and
    the triangle grid (built on first use)."""

    def __init__(self, indices, vertices, bounding_box=None, device=None):
        import torch
        from .. import _dev as D
        self.dev = D.device(device)
        if isinstance(vertices, torch.Tensor):
            self.verts = vertices.to(self.dev, torch.float32).reshape(-1, 3).contiguous()
            host_v = None
        else:
            host_v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
            self.verts = D.up(host_v, self.dev)
        if isinstance(indices, torch.Tensor):
            self.tris = indices.to(self.dev).reshape(-1, 3).to(torch.int32).contiguous()
        else:
            ind = np.asarray(indices).reshape(-1, 3)
            if len(ind) and (ind.min() < 0 or ind.max() >= 2 ** 32):
                raise ValueError('views: a triangle index does not fit 32 bits')
            self.tris = D.up(ind.astype(np.uint32), self.dev)
        self.n_verts, self.n_tris = int(self.verts.shape[0]), int(self.tris.shape[0])
        if self.n_verts == 0:
            self.center, self.max_dist = np.zeros(3, np.float32), np.float32(1)
        elif bounding_box is not None:
            self.center, self.max_dist = np.asarray(bounding_box[0], np.float32).reshape(3), np.float32(bounding_box[1])
        else:
            if host_v is None:
                host_v = D.down(self.verts)
            center, max_dist = get_bounding_box(host_v.reshape(-1))               # MeshObject.__init__ (proc/meshes.py:88-94)
            self.center, self.max_dist = center.astype(np.float32), np.float32(max_dist)
        if not np.isfinite(self.center).all() or not (np.isfinite(self.max_dist) and self.max_dist > 0):
            raise ValueError('views: the mesh has no finite center and positive max_dist')
        self._index = None

    @property
    def center3(self):
        import ctypes as C
        return (C.c_float * 3)(*[float(v) for v in self.center])

    @property
    def index(self):
        from .. import _dev as D
        from .. import _lib as L
        if self._index is None:
            lib = L.load()
            ix = D.empty(int(lib.sd_views_index_bytes(self.n_tris)), D.u8, self.dev)
            cnt = D.counters(self.dev)
            tmp = D.scratch('sd_views_index_temp_bytes', self.dev, self.n_tris)
            D.call('sd_views_index', self.dev, self.verts if self.n_verts else None, self.n_verts, self.tris if self.n_tris else None, self.n_tris,
                   self.center3, float(self.max_dist), ix, ix.numel(), cnt, tmp, tmp.numel())
            if D.down(cnt)[3]:
                raise IndexError('views: a triangle names a vertex the mesh does not have')
            self._index = ix
        return self._index

    def edge_lengths(self, comp_window: float) -> np.ndarray:
        return np.array([comp_window, comp_window / 2, comp_window], np.float64) / np.float64(self.max_dist)


def _coords_device(coords, dev):
    import torch
    from .. import _dev as D
    if isinstance(coords, torch.Tensor):
        return coords.to(dev, torch.float32).reshape(-1, 3).contiguous()
    c = np.array(coords, dtype=np.float32).reshape(-1, 3)
    if not np.isfinite(c).all():
        raise ValueError('views: a rendering location is not finite')
    return D.up(c, dev)


def _rot_device(rot_mat, n, dev):
    import torch
    from .. import _dev as D
    if isinstance(rot_mat, torch.Tensor):
        r = rot_mat.to(dev, torch.float64).reshape(-1, 16).contiguous()
    else:
        r = np.ascontiguousarray(rot_mat, np.float64).reshape(-1, 16)
        if not np.isfinite(r).all():
            raise ValueError('views: a rotation matrix is not finite')
        r = D.up(r, dev)
    if r.shape[0] != n:
        raise ValueError(f'views: {r.shape[0]} rotation matrices for {n} locations')
    return r


def render_mesh_device(mesh: ViewMesh, coords_d, rot_d, ws, nb_views: int, comp_window: float, index_views: bool = False, out=None,
                       max_views_per_call: int = 8192):
    """Views of one mesh at the locations `coords_d` (device float32 (N, 3), raw nm) with the matrices `rot_d` (device float64 (N, 16)):
    a device tensor uint8 (N, nb_views, H, W), or int32 bits of uint32 for index views; written into `out` where given.  The locations
    go through the device in pieces of at most `max_views_per_call` views, which bounds the candidate lists."""
    import ctypes as C
    import torch
    from .. import _dev as D
    (W, H), dev, N = ws, mesh.dev, int(coords_d.shape[0])
    if out is None:
        out = torch.empty((N, nb_views, H, W), dtype=torch.int32 if index_views else torch.uint8, device=dev)
    if N == 0:
        return out
    if mesh.n_verts == 0 or mesh.n_tris == 0:
        out.fill_(-2 if index_views else 255)
        return out
    f64n = lambda v: (C.c_double * len(v))(*[float(x) for x in v])
    ang = np.deg2rad(view_angles(nb_views))
    E, cos_v, sin_v, w7 = f64n(mesh.edge_lengths(comp_window)), f64n(np.cos(ang)), f64n(np.sin(ang)), f64n(gauss_weights())
    step = max(1, int(max_views_per_call) // nb_views)
    cnt = D.counters(dev)
    for a in range(0, N, step):
        n = min(step, N - a)
        c_d = coords_d[a:a + n]
        begin = D.empty(n + 1, D.i64, dev)
        tmp = D.scratch('sd_views_candidates_temp_bytes', dev, n)
        args = (mesh.index, mesh.n_tris, c_d, n, mesh.center3, float(mesh.max_dist), E, begin)
        D.call('sd_views_candidates', dev, *args, None, 0, cnt, tmp, tmp.numel())
        c = D.down(cnt)
        if c[6]:
            raise ValueError('views: 2^31 candidate triangles or more in one call; lower max_views_per_call')
        n_cand = int(c[0])
        cand = D.empty(n_cand, D.i32, dev)
        if n_cand:
            D.call('sd_views_candidates', dev, *args, cand, n_cand, cnt, tmp, tmp.numel())
            c = D.down(cnt)
            if c[1] or int(c[0]) != n_cand:
                raise RuntimeError('sd_views_candidates: the counted capacity did not hold the candidates (internal error)')
        rtmp = D.scratch('sd_views_render_temp_bytes', dev, n, nb_views)
        view = out[a:a + n]
        head = (mesh.verts, mesh.n_verts, mesh.tris, mesh.n_tris, mesh.index, c_d, n, rot_d[a:a + n], mesh.center3, float(mesh.max_dist), E, cos_v, sin_v,
                nb_views, W, H)
        tail = (begin, cand if n_cand else None, n_cand, view, view.numel(), cnt, rtmp, rtmp.numel())
        if index_views:
            D.call('sd_views_render_index', dev, *head, *tail)
        else:
            D.call('sd_views_render', dev, *head, w7, *tail)
        if D.down(cnt)[3]:
            raise IndexError('views: a triangle names a vertex the mesh does not have')
    return out


def render_views_table(meshes: Sequence, coords, rot_mat=None, ws=None, nb_views: Optional[int] = None, comp_window: Optional[float] = None,
                       index_views: bool = False, max_views_per_call: int = 8192, device=None, return_device: bool = False):
    """Views of several meshes of one cell at the same locations, one channel per mesh: ``(views, rot_mat)`` with views uint8
    (N, len(meshes), nb_views, H, W) -- uint32 for `index_views` -- and rot_mat float64 (N, 16).  `meshes`: ``ViewMesh`` objects,
    ``(indices, vertices)`` pairs or None / empty meshes (a channel of 255).  The first mesh gives the rotations unless `rot_mat` is
    passed; meshes, their indices and, with `return_device`, views and matrices stay on the device.  One default view is 32 KiB, so
    10^4 locations x 2 views x 4 channels are 2.6 GB: `max_views_per_call` bounds what one launch set works on, the output is the caller's
    to bound by the number of locations."""
    import torch
    from .. import _dev as D
    cfg = global_params.config['views']['view_properties']
    ws, nb_views, comp_window = _check_window(cfg['ws'] if ws is None else ws, cfg['nb_views'] if nb_views is None else nb_views,
                                              cfg['comp_window'] if comp_window is None else comp_window)
    dev = D.device(device)
    vms = []
    for m in meshes:
        if m is None or isinstance(m, ViewMesh):
            vms.append(m)
        else:
            vms.append(ViewMesh(m[0], m[1], device=dev) if len(m[1]) else None)
    coords_d = _coords_device(coords, dev)
    N = int(coords_d.shape[0])
    if rot_mat is None:
        first = vms[0] if vms else None
        if first is None or first.n_verts == 0:
            rot_d = torch.zeros((N, 16), dtype=torch.float64, device=dev)
        else:
            rot_d = calc_rot_matrices_device(first.verts, coords_d, first.center, first.max_dist, np.float32(comp_window / first.max_dist), dev)
    else:
        rot_d = _rot_device(rot_mat, N, dev)
    out = torch.empty((N, len(vms), nb_views, ws[1], ws[0]), dtype=torch.int32 if index_views else torch.uint8, device=dev)
    for k, vm in enumerate(vms):
        if vm is None:
            out[:, k] = -2 if index_views else 255
            continue
        # a channel is a strided slice of the output: render into a contiguous piece and place it
        out[:, k] = render_mesh_device(vm, coords_d, rot_d, ws, nb_views, comp_window, index_views, None, max_views_per_call)
    if return_device:
        return out, rot_d
    return D.down(out, view=np.uint32 if index_views else None), D.down(rot_d)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's functions
def render_mesh_coords(coords: np.ndarray, ind: np.ndarray, vert: np.ndarray, clahe: bool = False, verbose: bool = False, ws=None,
                       rot_matrices=None, views_key: str = 'raw', return_rot_matrices: bool = False, depth_map: bool = True,
                       smooth_shade: bool = True, wire_frame: bool = False, nb_views: Optional[int] = None, triangulation: bool = True,
                       comp_window: float = 8e3, device=None):
    """Depth views uint8 (N, nb_views, ws[1], ws[0]) of the mesh at `coords` (proc/rendering.py:95-114 with rendering_egl.py:611-681)."""
    _not_built(clahe=clahe, wire_frame=wire_frame, color_rendering=not depth_map, point_rendering=not triangulation)
    views, rot = render_views_table([(ind, vert)], coords, rot_matrices, ws, nb_views, comp_window, device=device)
    return (views[:, 0], rot) if return_rot_matrices else views[:, 0]


def _subcell_objects(add_cellobjects):
    view_cfg = global_params.config['views']
    if add_cellobjects is None or add_cellobjects is True:
        add_cellobjects = list(view_cfg['subcell_objects'])
        if view_cfg['use_onthefly_views'] and 'sj' in add_cellobjects:
            add_cellobjects[add_cellobjects.index('sj')] = 'syn_ssv'
    return add_cellobjects


def render_sso_coords(sso, coords: np.ndarray, add_cellobjects: Optional[Iterable[str]] = None, verbose: bool = False, clahe: bool = False,
                      ws=None, cellobjects_only: bool = False, wire_frame: bool = False, nb_views: Optional[int] = None,
                      comp_window: Optional[float] = None, rot_mat: Optional[np.ndarray] = None, return_rot_mat: bool = False, device=None,
                      return_device: bool = False):
    """Views of a cell at `coords`: uint8 (N, channels, nb_views, ws[1], ws[0]), the cell's mesh first (left out with
    `cellobjects_only`), then one channel per entry of `add_cellobjects`; a missing or empty mesh gives 255.  `sso` is anything with
    ``.mesh`` and ``.load_mesh(name)`` (``[indices, vertices, ...]``).  proc/rendering.py:204-297.  With `return_device` the views (and
    matrices) stay on the device as tensors (the view network reads them there)."""
    _not_built(clahe=clahe, wire_frame=wire_frame)
    add_cellobjects = _subcell_objects(add_cellobjects)
    names = list(add_cellobjects) if add_cellobjects is not False else []
    if cellobjects_only and not names:
        raise ValueError('render_sso_coords: add_cellobjects must hold at least one entry when rendering cell objects only')
    mesh = sso.mesh
    pair = lambda m: (m[0], m[1]) if len(m[1]) else None
    from .. import _dev as D
    dev = D.device(device)
    cell = pair(mesh)
    cell_vm = ViewMesh(cell[0], cell[1], device=dev) if cell is not None else None
    coords_d = _coords_device(coords, dev)
    N = int(coords_d.shape[0])
    if rot_mat is None and cell_vm is not None and N:
        ws_, nb_, cw_ = _window_defaults(ws, nb_views, comp_window)
        rot_mat = calc_rot_matrices_device(cell_vm.verts, coords_d, cell_vm.center, cell_vm.max_dist, np.float32(cw_ / cell_vm.max_dist), dev)
    elif rot_mat is None:
        rot_mat = np.zeros((N, 16))
    meshes = ([] if cellobjects_only else [cell_vm]) + [pair(sso.load_mesh(name)) for name in names]
    views, rot = render_views_table(meshes, coords_d, rot_mat, ws, nb_views, comp_window, device=dev, return_device=return_device)
    return (views, rot) if return_rot_mat else views


def _window_defaults(ws, nb_views, comp_window):
    cfg = global_params.config['views']['view_properties']
    return _check_window(cfg['ws'] if ws is None else ws, cfg['nb_views'] if nb_views is None else nb_views,
                         cfg['comp_window'] if comp_window is None else comp_window)


def render_sso_coords_index_views(sso, coords: np.ndarray, verbose: bool = False, ws=None, rot_mat: Optional[np.ndarray] = None,
                                  nb_views: Optional[int] = None, comp_window: Optional[float] = None, return_rot_matrices: bool = False,
                                  device=None):
    """Index views of the cell's mesh: uint32 (N, 1, nb_views, ws[1], ws[0]), per pixel the last vertex of the nearest triangle (the
    provoking vertex of flat shading), 2^32 - 2 where nothing is drawn.  proc/rendering.py:300-396."""
    ind, vert = sso.mesh[0], sso.mesh[1]
    meshes = [(ind, vert)] if len(vert) else [None]
    views, rot = render_views_table(meshes, coords, rot_mat, ws, nb_views, comp_window, index_views=True, device=device)
    return (views, rot) if return_rot_matrices else views


def render_sampled_views(sso, ds_factor=None, index_views: bool = False, return_locations: bool = False, **render_kw):
    """Views of a cell at its own rendering locations: ``sample_locations_sso`` of the cell's supervoxels (``sso.svs``), concatenated,
    into ``render_sso_coords`` -- ``render_sso_coords_index_views`` with `index_views` --, whose keyword arguments `render_kw` are; with
    `return_locations` ``(views, locations)``.  Locations and views are computed on the device; the locations cross the host between
    the two."""
    from ..reps.super_segmentation_helper import sample_locations_sso
    parts = sample_locations_sso(sso, ds_factor, device=render_kw.get('device'))
    locs = np.concatenate(parts) if parts else np.zeros((0, 3), np.float32)
    views = (render_sso_coords_index_views if index_views else render_sso_coords)(sso, locs, **render_kw)
    return (views, locs) if return_locations else views
