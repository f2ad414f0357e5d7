"""The view raster rule, the view rotations and the pixel -> vertex vote of csrc/sd_views.hip restated in numpy (DESIGN.md section 7 states
the rule in words; where the two differ this file is the normative one).  Every float64 product and sum below is one numpy operation, so
it is rounded on its own, as the kernels' are (contraction off); float32 quotients are numpy's, which are correctly rounded."""
import numpy as np

BG_INDEX = 2 ** 32 - 2
SNAP_LIM = 1 << 22
D_ONE = 1 << 24


def gauss_weights(sigma=0.7, truncate=4.0):
    """The 7 weights of ``scipy.ndimage.gaussian_filter(img, .7)``, by scipy's own expression (``_gaussian_kernel1d``)."""
    radius = int(truncate * float(sigma) + 0.5)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / sigma2 * x ** 2)
    return phi / phi.sum()


def view_angles(nb_views):
    """Degrees of the rotation about x of every view (rendering_egl.py:657-660)."""
    if nb_views == 2:
        return np.array([(-1) ** (m + 1) * 25 for m in range(nb_views)], np.float64)
    return np.array([360. / nb_views * m for m in range(nb_views)], np.float64)


def view_cos_sin(nb_views):
    a = np.deg2rad(view_angles(nb_views))
    return np.cos(a), np.sin(a)


def normalise(v, center, max_dist):
    v = np.asarray(v, np.float32).reshape(-1, 3)
    d = (v - np.asarray(center, np.float32)).astype(np.float32)
    return (d / np.float32(max_dist)).astype(np.float32)


def edge_lengths(comp_window, max_dist):
    return np.array([comp_window, comp_window / 2, comp_window], np.float64) / np.float64(np.float32(max_dist))


def filter_axis(img, axis, w):
    """One pass of the filter along `axis`, truncated to uint8: scipy's symmetric correlate1d with mode 'reflect' (numpy's 'symmetric')."""
    a = np.moveaxis(np.asarray(img, np.uint8), axis, 0).astype(np.float64)
    n = a.shape[0]
    pad = np.pad(a, ((3, 3),) + ((0, 0),) * (a.ndim - 1), mode='symmetric')
    tmp = pad[3:3 + n] * w[3]
    for i in (-3, -2, -1):
        tmp = tmp + (pad[3 + i:3 + i + n] + pad[3 - i:3 - i + n]) * w[i + 3]
    return np.moveaxis(tmp.astype(np.uint8), 0, axis)


def depth_filter(img, w=None):
    """Rule 7 after the bytes: axis 0, then axis 1, then the all-zero rule."""
    w = gauss_weights() if w is None else w
    out = filter_axis(filter_axis(img, 0, w), 1, w)
    if out.sum() == 0:
        out = np.full_like(out, 255)
    return out


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _bias(dx, dy):
    return 0 if (dy > 0 or (dy == 0 and dx < 0)) else 1


def raster_view(vn, tris, cn, rot, E, cos_m, sin_m, W, H):
    """One view -> (D int64 [H, W] with D_ONE where nothing is drawn, t int64 [H, W] the winning triangle or -1, dropped triangles)."""
    vn = np.asarray(vn, np.float32).reshape(-1, 3).astype(np.float64)
    tris = np.asarray(tris).reshape(-1, 3).astype(np.int64)
    cn = np.asarray(cn, np.float32).astype(np.float64)
    M = np.asarray(rot, np.float64).reshape(4, 4, order='F')
    Dbuf = np.full((H, W), D_ONE, np.int64)
    tbuf = np.full((H, W), -1, np.int64)
    if len(tris) == 0 or not M.any() or not vn.any():
        return Dbuf, tbuf, 0
    p0, p1, p2 = vn[:, 0] - cn[0], vn[:, 1] - cn[1], vn[:, 2] - cn[2]
    q = [((M[i, 0] * p0) + M[i, 1] * p1) + M[i, 2] * p2 for i in range(3)]
    xe = q[0]
    ye = (cos_m * q[1]) - (sin_m * q[2])
    ze = (sin_m * q[1]) + (cos_m * q[2])
    X = (xe / E[0] + 0.5) * np.float64(W)
    Y = (ye / E[1] + 0.5) * np.float64(H)
    Zf = 0.5 - ze / E[2]
    snap = lambda v: np.clip(np.floor(v * 256.0 + 0.5), -2.0 ** 40, 2.0 ** 40).astype(np.int64)
    xs, ys = snap(X)[tris], snap(Y)[tris]
    zf = Zf[tris]
    c0 = np.maximum((xs.min(1) - 128 + 255) >> 8, 0)
    c1 = np.minimum((xs.max(1) - 128) >> 8, W - 1)
    r0 = np.maximum((ys.min(1) - 128 + 255) >> 8, 0)
    r1 = np.minimum((ys.max(1) - 128) >> 8, H - 1)
    keep = (c0 <= c1) & (r0 <= r1)
    big = ((np.abs(xs) >= SNAP_LIM) | (np.abs(ys) >= SNAP_LIM)).any(1)
    dropped = int((keep & big).sum())
    keep &= ~big
    for t in np.flatnonzero(keep):
        x, y, z = xs[t].tolist(), ys[t].tolist(), zf[t]
        area = _edge(x[0], y[0], x[1], y[1], x[2], y[2])
        if area == 0:
            continue
        k1, k2 = (1, 2) if area > 0 else (2, 1)
        area = abs(area)
        x, y = [x[0], x[k1], x[k2]], [y[0], y[k1], y[k2]]
        z0, dz1, dz2 = z[0], z[k1] - z[0], z[k2] - z[0]
        px = (256 * np.arange(c0[t], c1[t] + 1) + 128)[None, :]
        py = (256 * np.arange(r0[t], r1[t] + 1) + 128)[:, None]
        e01 = _edge(x[0], y[0], x[1], y[1], px, py)
        e12 = _edge(x[1], y[1], x[2], y[2], px, py)
        e20 = _edge(x[2], y[2], x[0], y[0], px, py)
        inside = (e01 >= _bias(x[1] - x[0], y[1] - y[0])) & (e12 >= _bias(x[2] - x[1], y[2] - y[1])) & (e20 >= _bias(x[0] - x[2], y[0] - y[2]))
        if not inside.any():
            continue
        Df = z0 + ((e20.astype(np.float64) * dz1) + (e01.astype(np.float64) * dz2)) / np.float64(area)
        Dd = np.floor(Df * 16777216.0)
        ok = inside & (Dd >= 0.0) & (Dd < 16777215.0)
        D = np.where(ok, Dd, D_ONE).astype(np.int64)
        sub_D, sub_t = Dbuf[r0[t]:r1[t] + 1, c0[t]:c1[t] + 1], tbuf[r0[t]:r1[t] + 1, c0[t]:c1[t] + 1]
        win = ok & (D < sub_D)                                                     # ascending t: the lower triangle keeps a tie
        sub_D[win] = D[win]
        sub_t[win] = t
    return Dbuf, tbuf, dropped


def render(vn, tris, cn, rot, E, nb_views, ws, index=False, cos_sin=None, dense=None):
    """-> (views [N, nb_views, H, W] uint8 depth or uint32 index, triangles dropped at the 2^22 bound).  `vn` / `cn` normalised float32."""
    W, H = int(ws[0]), int(ws[1])
    cn = np.asarray(cn, np.float32).reshape(-1, 3)
    rot = np.asarray(rot, np.float64).reshape(-1, 16)
    cos_v, sin_v = view_cos_sin(nb_views) if cos_sin is None else cos_sin
    tris = np.asarray(tris).reshape(-1, 3)
    out = np.zeros((len(cn), nb_views, H, W), np.uint32 if index else np.uint8)
    w = gauss_weights()
    dropped = 0
    one_view = raster_view_dense if (W * H <= 2048 if dense is None else dense) else raster_view
    for n in range(len(cn)):
        for m in range(nb_views):
            D, t, d = one_view(vn, tris, cn[n], rot[n], E, cos_v[m], sin_v[m], W, H)
            dropped += d
            if index:
                out[n, m] = np.where(t >= 0, tris[np.maximum(t, 0), 2] if len(tris) else 0, BG_INDEX).astype(np.uint32)
            else:
                out[n, m] = depth_filter(np.where(D < D_ONE, D >> 16, 255).astype(np.uint8), w)
    return out, dropped


# ---- rotations -------------------------------------------------------------------------------------------------------------------------
def in_bounding_box(vertices, c, edge_length):
    """extraction/in_bounding_boxC.pyx on float32 arrays: float32 differences, the half edge in float32, strict on both sides."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    h = np.float32(np.float32(edge_length) / np.float32(2))
    d = (v - np.asarray(c, np.float32)).astype(np.float32)
    return ((d > -h) & (d < h)).all(1)


def sign_rows(rows):
    """The component of largest magnitude of every row positive, lowest index on a tie."""
    rows = np.array(rows, np.float64)
    for r in rows:
        if r[np.argmax(np.abs(r))] < 0:
            r *= -1
    return rows


def rot_matrices(cn, vn, edge_length, stride=1):
    """-> ([N, 16] float64, empty [N] bool): float64 mean and covariance of the inliers, rows by descending eigenvalue, signed."""
    vn = np.asarray(vn, np.float32).reshape(-1, 3)[::stride]
    cn = np.asarray(cn, np.float32).reshape(-1, 3)
    out, empty = np.zeros((len(cn), 16)), np.zeros(len(cn), bool)
    for n, c in enumerate(cn):
        pts = vn[in_bounding_box(vn, c, edge_length)].astype(np.float64)
        empty[n] = len(pts) == 0
        if len(pts) <= 2:
            continue
        d = pts - pts.mean(0)
        cov = d.T @ d / (len(pts) - 1)
        evals, evecs = np.linalg.eigh(cov)
        rows = sign_rows(evecs[:, np.argsort(evals, kind='stable')[::-1]].T)
        m = np.zeros((4, 4))
        m[:3, :3] = rows
        m[3, 3] = 1
        out[n] = m.flatten('F')
    return out, empty


# ---- the vote --------------------------------------------------------------------------------------------------------------------------
def vote(index_arr, label_arr, background_id, n_verts, n_labels, unpredicted):
    """semseg2mesh_counter with its uint8 table, then argmax / the unpredicted rule -> (vertex labels uint8, table uint8)."""
    index_arr = np.asarray(index_arr).reshape(-1).astype(np.int64)
    label_arr = np.asarray(label_arr).reshape(-1).astype(np.int64)
    keep = index_arr != background_id
    if (index_arr[keep] >= n_verts).any():
        raise IndexError('a pixel names a vertex the mesh does not have')
    cnt = np.zeros((n_verts, n_labels), np.int64)
    np.add.at(cnt, (index_arr[keep], label_arr[keep]), 1)
    table = (cnt & 255).astype(np.uint8)
    labels = np.argmax(table, axis=1).astype(np.uint8) if n_verts else np.zeros(0, np.uint8)
    labels[table.sum(axis=1) == 0] = unpredicted
    return labels, table


# ---- test meshes -----------------------------------------------------------------------------------------------------------------------
def bent_tube(n_rings=64, n_side=16, radius=300.0, length=12000.0, bend=2500.0, offset=(20000.0, 31000.0, 9000.0)):
    """An analytic bent tube in nm: float32 vertices (n_rings * n_side, 3) and uint32 triangles (2 * n_side * (n_rings - 1), 3)."""
    s = np.linspace(0.0, 1.0, n_rings)
    centre = np.stack([length * s, bend * np.sin(np.pi * s), 0.4 * bend * np.sin(2 * np.pi * s)], 1)
    tang = np.gradient(centre, axis=0)
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    up = np.cross(tang, np.array([0.0, 0.0, 1.0]))
    up /= np.linalg.norm(up, axis=1, keepdims=True)
    side = np.cross(tang, up)
    phi = 2 * np.pi * np.arange(n_side) / n_side
    r = radius * (1.0 + 0.3 * np.sin(6 * np.pi * s))[:, None, None]
    verts = centre[:, None] + r * (np.cos(phi)[None, :, None] * up[:, None] + np.sin(phi)[None, :, None] * side[:, None])
    verts = (verts + np.asarray(offset)).reshape(-1, 3).astype(np.float32)
    tris = []
    for i in range(n_rings - 1):
        for j in range(n_side):
            a, b = i * n_side + j, i * n_side + (j + 1) % n_side
            tris += [(a, b, a + n_side), (b, b + n_side, a + n_side)]
    return verts, np.array(tris, np.uint32)


def raster_view_dense(vn, tris, cn, rot, E, cos_m, sin_m, W, H):
    """``raster_view`` with all triangles against all pixels at once (small windows); the same rule, written a second time."""
    vn = np.asarray(vn, np.float32).reshape(-1, 3).astype(np.float64)
    tris = np.asarray(tris).reshape(-1, 3).astype(np.int64)
    cn = np.asarray(cn, np.float32).astype(np.float64)
    M = np.asarray(rot, np.float64).reshape(4, 4, order='F')
    Dbuf, tbuf = np.full((H, W), D_ONE, np.int64), np.full((H, W), -1, np.int64)
    if len(tris) == 0 or not M.any() or not vn.any():
        return Dbuf, tbuf, 0
    p = [vn[:, a] - cn[a] for a in range(3)]
    q = [((M[i, 0] * p[0]) + M[i, 1] * p[1]) + M[i, 2] * p[2] for i in range(3)]
    ye, ze = (cos_m * q[1]) - (sin_m * q[2]), (sin_m * q[1]) + (cos_m * q[2])
    snap = lambda v: np.clip(np.floor(v * 256.0 + 0.5), -2.0 ** 40, 2.0 ** 40).astype(np.int64)
    xs, ys = snap((q[0] / E[0] + 0.5) * np.float64(W))[tris], snap((ye / E[1] + 0.5) * np.float64(H))[tris]
    zf = (0.5 - ze / E[2])[tris]
    hit = (np.maximum((xs.min(1) + 127) >> 8, 0) <= np.minimum((xs.max(1) - 128) >> 8, W - 1)) & \
          (np.maximum((ys.min(1) + 127) >> 8, 0) <= np.minimum((ys.max(1) - 128) >> 8, H - 1))
    big = ((np.abs(xs) >= SNAP_LIM) | (np.abs(ys) >= SNAP_LIM)).any(1)
    dropped = int((hit & big).sum())
    area = _edge(xs[:, 0], ys[:, 0], xs[:, 1], ys[:, 1], xs[:, 2], ys[:, 2])
    use = np.flatnonzero(hit & ~big & (area != 0))
    if len(use) == 0:
        return Dbuf, tbuf, dropped
    xs, ys, zf, area = xs[use], ys[use], zf[use], area[use]
    flip = area < 0
    order = np.where(flip[:, None], [0, 2, 1], [0, 1, 2])
    xs, ys, zf = np.take_along_axis(xs, order, 1), np.take_along_axis(ys, order, 1), np.take_along_axis(zf, order, 1)
    area = np.abs(area)
    px = (256 * np.arange(W) + 128)[None, None, :]
    py = (256 * np.arange(H) + 128)[None, :, None]
    col = lambda a, k: a[:, k][:, None, None]
    def edge(a, b):
        dx, dy = col(xs, b) - col(xs, a), col(ys, b) - col(ys, a)
        e = dx * (py - col(ys, a)) - dy * (px - col(xs, a))
        return e, np.where((dy > 0) | ((dy == 0) & (dx < 0)), 0, 1)
    (e01, b01), (e12, b12), (e20, b20) = edge(0, 1), edge(1, 2), edge(2, 0)
    inside = (e01 >= b01) & (e12 >= b12) & (e20 >= b20)
    Df = col(zf, 0) + ((e20.astype(np.float64) * (col(zf, 1) - col(zf, 0))) + (e01.astype(np.float64) * (col(zf, 2) - col(zf, 0)))) / area.astype(np.float64)[:, None, None]
    Dd = np.floor(Df * 16777216.0)
    ok = inside & (Dd >= 0.0) & (Dd < 16777215.0)
    D = np.where(ok, Dd, D_ONE).astype(np.int64)
    first = D.argmin(0)                                                            # the first minimum: the lowest triangle at equal depth
    Dbuf = np.take_along_axis(D, first[None], 0)[0]
    tbuf = np.where(Dbuf < D_ONE, use[first], -1)
    return Dbuf, tbuf, dropped


# ---- rule edges: identity matrix, center 0, max_dist 1, comp_window 2 (E = [2, 1, 2]), one view (angle 0), ws (32, 16) ---------------------
EDGE_WS, EDGE_CW = (32, 16), 2.0
IDENTITY = np.eye(4).flatten('F')


def px_x(X, W=32):
    """The normalised x whose window coordinate is X (exact for multiples of 1/2 at W = 32)."""
    return X / W * 2.0 - 1.0


def px_y(Y, H=16):
    return Y / H - 0.5


def z_of(Zf):
    return (0.5 - Zf) * 2.0


def edge_cases():
    """name -> (vertices float32, triangles uint32)."""
    P = lambda X, Y, Zf=0.5: (px_x(X), px_y(Y), z_of(Zf))
    quad = lambda x0, y0, x1, y1, Zf=0.5: [P(x0, y0, Zf), P(x1, y0, Zf), P(x1, y1, Zf), P(x0, y1, Zf)]
    cases = {}
    cases['pixel_centres'] = (quad(4.5, 3.5, 12.5, 10.5), [(0, 1, 2), (0, 2, 3)])
    cases['border'] = (quad(0, 0, 32, 16, 0.25), [(0, 1, 2), (0, 2, 3)])
    cases['shared_edge'] = (quad(4.5, 3.5, 12.5, 11.5), [(0, 1, 2), (0, 2, 3)])
    cases['shared_edge_flipped'] = (quad(4.5, 3.5, 12.5, 11.5), [(0, 2, 1), (0, 2, 3)])
    cases['coplanar'] = (quad(2, 2, 20, 12) + quad(2, 2, 20, 12), [(0, 1, 2), (4, 5, 6), (4, 6, 7), (0, 2, 3)])
    cases['near_plane'] = ([P(2, 2, -0.25), P(30, 2, 0.25), P(2, 14, 0.25)], [(0, 1, 2)])
    cases['far_plane'] = ([P(2, 2, 1.25), P(30, 2, 0.75), P(2, 14, 0.75)], [(0, 1, 2)])
    cases['d_zero'] = (quad(-4, -4, 40, 20, 0.0), [(0, 1, 2), (0, 2, 3)])
    cases['zero_area'] = (quad(3, 3, 9, 9) + [P(10, 10), P(14, 14), P(18, 18)], [(0, 0, 1), (4, 5, 6), (1, 1, 1), (0, 1, 2), (4, 6, 5)])
    far = [(40.0 + 0.01 * k, 40.0 + 0.02 * (k % 7), 0.1 * (k % 3)) for k in range(120)]
    cases['huge'] = ([(-2.0, -2.0, 0.0), (200.0, -2.0, 0.0), (-2.0, 200.0, 0.0)] + far, [(k + 3, k + 4, k + 5) for k in range(0, 117)] + [(0, 1, 2)])
    cases['beyond_bound'] = (quad(4, 4, 10, 10) + [(-1.0, -0.5, 0.0), (2000.0, 0.0, 0.0), (-1.0, 0.5, 0.0)], [(0, 1, 2), (4, 5, 6), (0, 2, 3)])
    return {k: (np.array(v, np.float32), np.array(t, np.uint32)) for k, (v, t) in cases.items()}
