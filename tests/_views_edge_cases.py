"""Raster inputs placed on the structure edges of csrc/sd_views.hip: the tiled all-zero rule, the 2^22 bound and the depth cut-off hit
exactly, the 64-sample threshold between lane and wave drawing, large triangles and depth ties across the tile seams, more candidates
than a block has threads, windows narrower than the filter, 2 and 16 views.  tests/test_views_edges_cpu.py pins with the restatement
(tests/_views_ref.py) that every input sits where it claims; tests/test_gpu_views_edges.py runs the device against the restatement.
Unless a case says otherwise: identity rotation, centre 0, max_dist 1, comp_window 2 (E = [2, 1, 2]), one view at angle 0."""
import numpy as np

import _views_ref as R

TILED_WS = (257, 129)                                                              # 2 x 2 depth tiles and 3 x 2 index tiles
DEPTH_TILE, INDEX_TILE, HALO = (250, 122), (128, 128), 3                           # render() of sd_views.hip
NARROW_MAX = 64                                                                    # a pixel box of more samples is drawn by the whole wave
TINY_WS = ((1, 1), (2, 1), (1, 3), (3, 2), (5, 1), (7, 3), (3, 7))
TINY_NAMES = ('near_plane', 'far_plane', 'pixel_centres')
ZF4 = (0.2, 0.6, 0.4, 0.7)                                                         # a depth per vertex of a quad


def P(X, Y, Zf=0.5, W=32, H=16):
    return (R.px_x(X, W), R.px_y(Y, H), R.z_of(Zf))


def quad(x0, y0, x1, y1, Zf=0.5, W=32, H=16):
    z = [Zf] * 4 if np.isscalar(Zf) else list(Zf)
    return [P(x0, y0, z[0], W, H), P(x1, y0, z[1], W, H), P(x1, y1, z[2], W, H), P(x0, y1, z[3], W, H)]


class Case:
    """One mesh with the call it is rendered by; the restatement's views are computed once per mode and never changed."""

    def __init__(self, v, t, ws=R.EDGE_WS, coords=((0.0, 0.0, 0.0),), rot=None, nb_views=1, cos_sin=None):
        self.v, self.t, self.ws, self.nb_views = np.array(v, np.float32).reshape(-1, 3), np.array(t, np.uint32).reshape(-1, 3), ws, nb_views
        self.coords = np.array(coords, np.float32).reshape(-1, 3)
        self.rot = np.tile(R.IDENTITY, (len(self.coords), 1)) if rot is None else np.array(rot, np.float64).reshape(-1, 16)
        self.cos_sin = R.view_cos_sin(nb_views) if cos_sin is None else cos_sin
        self.E = R.edge_lengths(R.EDGE_CW, 1.0)
        self._ref = {}

    def ref(self, index):
        """-> (views [N, nb_views, H, W], dropped) of the restatement."""
        if index not in self._ref:
            out, dropped = R.render(self.v, self.t, self.coords, self.rot, self.E, self.nb_views, self.ws, index=index, cos_sin=self.cos_sin)
            out.setflags(write=False)
            self._ref[index] = (out, dropped)
        return self._ref[index]

    def raw(self, loc=0, view=0):
        """-> (depth bytes before the filter, winning triangle or -1, dropped) of one view."""
        D, t, dropped = R.raster_view(self.v, self.t, self.coords[loc], self.rot[loc], self.E, self.cos_sin[0][view], self.cos_sin[1][view], *self.ws)
        return np.where(D < R.D_ONE, D >> 16, 255).astype(np.uint8), t, dropped

    def pixel_boxes(self):
        """Samples in every triangle's pixel box by the rule of tri_setup (location 0, view 0, identity), before any clamp to the window."""
        W, H = self.ws
        p = self.v.astype(np.float64) - self.coords[0].astype(np.float64)
        snap = lambda a: np.floor(a * 256.0 + 0.5).astype(np.int64)
        xs, ys = snap((p[:, 0] / self.E[0] + 0.5) * W)[self.t.astype(np.int64)], snap((p[:, 1] / self.E[1] + 0.5) * H)[self.t.astype(np.int64)]
        nx = ((xs.max(1) - 128) >> 8) - ((xs.min(1) + 127) >> 8) + 1
        ny = ((ys.max(1) - 128) >> 8) - ((ys.min(1) + 127) >> 8) + 1
        return nx * ny


# ---- 1. the tiled all-zero rule -----------------------------------------------------------------------------------------------------------
W2, H2 = TILED_WS
SHIFT_LEFT = (R.px_x(-4.0, W2) + 1.0, 0.0, 0.0)                                     # a location 4 pixels to the left: the gap of corner_nonzero leaves the window


def _corner_mesh():
    return quad(-4, -4, 253.25, 133, 0.0, W2, H2) + quad(-4, -4, 261, 125.25, 0.0, W2, H2), [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7)]


def zero_rule_cases():
    c = {}
    c['all_zero'] = Case(quad(-4, -4, W2 + 4, H2 + 4, 0.0, W2, H2), [(0, 1, 2), (0, 2, 3)], TILED_WS)
    c['corner_nonzero'] = Case(*_corner_mesh(), TILED_WS)
    # one call: a view that is all zero, one whose only non-zero bytes lie in the last tile, a skipped location -- once with one view
    # and once with two views at angle 0, where (location, view) is not the location
    rot = np.stack([R.IDENTITY, R.IDENTITY, np.zeros(16)])
    coords = (SHIFT_LEFT, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    c['three_locations'] = Case(*_corner_mesh(), TILED_WS, coords, rot)
    c['three_locations_two_views'] = Case(*_corner_mesh(), TILED_WS, coords, rot, 2, (np.ones(2), np.zeros(2)))
    return c


# ---- 2. the bounds, exactly ---------------------------------------------------------------------------------------------------------------
def _bound_mesh(x_far):
    return quad(4, 4, 10, 10) + [(-1.0, -0.5, 0.0), (x_far, 0.0, 0.0), (-1.0, 0.5, 0.0)], [(0, 1, 2), (4, 5, 6), (0, 2, 3)]


def bound_cases():
    c = {}
    c['at_bound'] = Case(*_bound_mesh(R.px_x(16384.0)))                             # xs = 2^22
    c['below_bound'] = Case(*_bound_mesh(R.px_x(16384.0 - 1.0 / 256)))              # xs = 2^22 - 1
    c['at_bound_tiled'] = Case(*_bound_mesh(R.px_x(16384.0)), TILED_WS, ((0.0, 0.0, 0.0), (0.125, 0.0625, 0.0)), None, 3)
    c['last_depth'] = Case(quad(4, 4, 10, 10, 1.0 - 2.0 ** -23), [(0, 1, 2), (0, 2, 3)])       # D = 2^24 - 2
    c['past_last_depth'] = Case(quad(4, 4, 10, 10, 1.0 - 2.0 ** -24), [(0, 1, 2), (0, 2, 3)])  # D = 2^24 - 1
    return c


# ---- 3. lane or wave ----------------------------------------------------------------------------------------------------------------------
def split_cases():
    c = {}
    c['box_64'] = Case(quad(4.25, 3.25, 12.25, 11.25, ZF4), [(0, 1, 2), (0, 2, 3)])
    c['box_65'] = Case(quad(4.25, 3.25, 17.25, 8.25, ZF4), [(0, 1, 2), (0, 2, 3)])
    return c


# ---- 4. seams under large triangles -------------------------------------------------------------------------------------------------------
SEAM_QUAD, SEAM_STEP = (122.5, 62.5, 262.5, 132.5), 2                              # the diagonal has slope 1 / 2, runs through pixel centres and leaves the window
SEAM_COLS, SEAM_ROWS = (DEPTH_TILE[0], INDEX_TILE[0]), (DEPTH_TILE[1], INDEX_TILE[1])


def seam_cases():
    q = quad(*SEAM_QUAD, ZF4, W2, H2)
    c = {}
    c['shared_edge'] = Case(q, [(0, 1, 2), (0, 2, 3)], TILED_WS)
    c['shared_edge_flipped'] = Case(q, [(0, 2, 1), (0, 2, 3)], TILED_WS)
    c['coplanar'] = Case(q + q, [(0, 1, 2), (4, 5, 6), (4, 6, 7), (0, 2, 3)], TILED_WS)
    return c


# ---- 5. more candidates than a block has threads ------------------------------------------------------------------------------------------
LATTICE_K = 48
LATTICE_WS = ((32, 16), (128, 64))                                                 # 256-thread blocks; a region above 4096 pixels: 1024 threads


def lattice_mesh():
    k = LATTICE_K
    gx, gy = np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing='ij')
    x, y = gx * 0.05 - 1.2, gy * 0.05 - 1.2
    sheets = [0.35 * np.sin(3 * x + 1) * np.cos(2 * y), 0.3 * np.cos(2.5 * x) * np.sin(3.5 * y + 0.5) + 0.05]
    verts = np.concatenate([np.stack([x, y, z], -1).reshape(-1, 3) for z in sheets]).astype(np.float32)
    a = (gx[:-1, :-1] * (k + 1) + gy[:-1, :-1]).reshape(-1)
    one = np.concatenate([np.stack([a, a + k + 1, a + k + 2], 1), np.stack([a, a + k + 2, a + 1], 1)])
    return verts, np.concatenate([one, one + (k + 1) ** 2]).astype(np.uint32)


_lattice = {}


def lattice_case(ws):
    if ws not in _lattice:
        _lattice[ws] = Case(*lattice_mesh(), ws, ((0.0, 0.0, 0.0), (0.31, -0.17, 0.05)), None, 2)
    return _lattice[ws]


# ---- 6. windows narrower than the filter --------------------------------------------------------------------------------------------------
_tiny = {}


def tiny_case(name, ws):
    if (name, ws) not in _tiny:
        _tiny[name, ws] = Case(*R.edge_cases()[name], ws)
    return _tiny[name, ws]


# ---- 7. view counts -----------------------------------------------------------------------------------------------------------------------
_tube = {}


def tube_ref(gold, nb_views, index, n_loc=2, ws=(32, 16)):
    key = (nb_views, index, n_loc, ws)
    if key not in _tube:
        g = gold
        out, dropped = R.render(g['m_vn'], g['m_tris'], g['m_cn'][:n_loc], g['m_rot'][:n_loc], R.edge_lengths(float(g['m_comp_window']), g['m_max_dist']),
                                nb_views, ws, index=index)
        out.setflags(write=False)
        _tube[key] = (out, dropped)
    return _tube[key]


_cases = {}


def cases(group):
    """The cases of 'zero_rule', 'bound', 'split' or 'seam', built once."""
    if group not in _cases:
        _cases[group] = {'zero_rule': zero_rule_cases, 'bound': bound_cases, 'split': split_cases, 'seam': seam_cases}[group]()
    return _cases[group]


NAMES = {'zero_rule': ('all_zero', 'corner_nonzero', 'three_locations', 'three_locations_two_views'),
         'bound': ('at_bound', 'below_bound', 'at_bound_tiled', 'last_depth', 'past_last_depth'),
         'split': ('box_64', 'box_65'), 'seam': ('shared_edge', 'shared_edge_flipped', 'coplanar')}
