"""numpy / scipy restatements for the glia view step (tests/test_glia_views_cpu.py, tests/test_gpu_glia_views.py,
tests/golden/make_golden_glia_views.py): the centre component of a plane by ``scipy.ndimage.label``, the float64 softmax, the partition
logic of ``predict_views``, and the seeded planes and views the tests share."""
import functools
import zlib

import numpy as np
from scipy import ndimage


# -- single_conn_comp_img (proc/image.py:125-144) ----------------------------------------------------------------------------------
def center_component(img: np.ndarray, background) -> np.ndarray:
    """One 2-D image: the pixels of the 4-connected component of ``img != background`` (``ndimage.label``'s default structure) that
    holds the centre pixel ``(H // 2, W // 2)`` keep their value, every other pixel becomes `background`; a background centre
    (label 0) empties the image."""
    img = np.asarray(img)
    assert img.ndim == 2
    labeled, _ = ndimage.label(img != background)
    lab = labeled[img.shape[0] // 2, img.shape[1] // 2]
    out = np.full_like(img, background)
    if lab != 0:
        keep = labeled == lab
        out[keep] = img[keep]
    return out


def center_component_planes(planes: np.ndarray, background) -> np.ndarray:
    planes = np.asarray(planes)
    flat = planes.reshape(-1, *planes.shape[-2:])
    return np.stack([center_component(p, background) for p in flat]).reshape(planes.shape) if len(flat) else planes.copy()


# -- the probabilities --------------------------------------------------------------------------------------------------------------
def softmax64(logits: np.ndarray) -> np.ndarray:
    """float32 logits (n, C) -> float32: exp(x - max) / sum in float64, rounded once."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True)) if len(x) else x
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32) if len(x) else x.astype(np.float32)


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Steps between two arrays of non-negative finite float32."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# -- predict_views (proc/sd_proc.py:1386-1427) ----------------------------------------------------------------------------------------
def predict_views(predict_proba, views, single_cc_only=False, background=1):
    """The partition logic: every plane of channel 0 filtered (for two views: the reference's ``data[i, 0, :1]`` and ``data[i, 0, 1:]``),
    one ``predict_proba`` call over the concatenation, the slices ``probas[part_views[i]:part_views[i + 1]]``.  -> (slices, part_views)."""
    views = [np.array(v, copy=True) for v in views]
    if single_cc_only:
        for v in views:
            v[:, 0] = center_component_planes(v[:, 0], background)
    part_views = np.cumsum([0] + [len(v) for v in views])
    probas = predict_proba(np.concatenate(views))
    return [probas[part_views[i]:part_views[i + 1]] for i in range(len(views))], part_views


def fake_proba(views: np.ndarray) -> np.ndarray:
    """The model of the partition golden: a function of every pixel of a sample that tells samples, channels and views apart, float32
    (n, 2), exact in float64 (integer sums far below 2^53) and rounded once."""
    v = np.asarray(views).astype(np.float64)
    n = v.shape[0]
    w = (np.arange(int(np.prod(v.shape[1:]))) % 251 + 1).astype(np.float64)
    s = v.reshape(n, -1) @ w
    return np.stack([s, s / 7.0 + 3.0], 1).astype(np.float32)


# -- planes -------------------------------------------------------------------------------------------------------------------------
def spiral(H: int, W: int, fg: int = 7, bg: int = 255) -> np.ndarray:
    """A one-pixel path that winds inwards from (0, 0), rings two pixels apart, extended until it covers the centre pixel."""
    img = np.full((H, W), bg, np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    top, left, bottom, right = 0, 0, H - 1, W - 1
    img[0, 0] = fg
    turns_without_move = 0
    while turns_without_move < 4:
        ny, nx = y + dy, x + dx
        if {(0, 1): nx <= right, (1, 0): ny <= bottom, (0, -1): nx >= left, (-1, 0): ny >= top}[(dy, dx)]:
            y, x = ny, nx
            img[y, x] = fg
            turns_without_move = 0
            continue
        # turn right and shrink the side just finished by two
        if (dy, dx) == (0, 1):
            top += 2
        elif (dy, dx) == (1, 0):
            right -= 2
        elif (dy, dx) == (0, -1):
            bottom -= 2
        else:
            left += 2
        dy, dx = dx, -dy
        turns_without_move += 1
    cy, cx = H // 2, W // 2
    if img[cy, cx] == bg:      # join the centre to the path's end by a straight run
        while y != cy:
            y += 1 if cy > y else -1
            img[y, x] = fg
        while x != cx:
            x += 1 if cx > x else -1
            img[y, x] = fg
    return img


def serpentine(H: int, W: int, fg: int = 9, bg: int = 255, vertical: bool = False) -> np.ndarray:
    """Full rows at even y joined alternately at the right and the left end: one path that crosses every word seam in both directions.
    `vertical`: full columns at even x instead, which a flood that fills runs along x climbs one pixel per round."""
    if vertical:
        return np.ascontiguousarray(serpentine(W, H, fg, bg).T)
    img = np.full((H, W), bg, np.uint8)
    img[0::2] = fg
    for k, y in enumerate(range(1, H - 1, 2)):
        img[y, W - 1 if k % 2 == 0 else 0] = fg
    cy, cx = H // 2, W // 2
    if img[cy, cx] == bg:
        img[cy, cx] = fg      # (an odd centre row: the pixel joins the rows above and below)
    return img


def row_end_pair(W: int, bg: int = 255) -> np.ndarray:
    """5 x W: a run that ends at x = W - 1 of row 2 (it holds the centre) and another that starts at x = 0 of row 3: neighbours in
    memory, not in the image."""
    img = np.full((5, W), bg, np.uint8)
    img[2, W // 2:] = 50
    img[3, :max(W // 2 - 1, 1)] = 60
    return img


def diagonal_pair(H: int = 7, W: int = 9, bg: int = 255) -> np.ndarray:
    """Two blocks that touch only diagonally at the centre pixel."""
    img = np.full((H, W), bg, np.uint8)
    cy, cx = H // 2, W // 2
    img[cy:, cx:] = 20
    img[:cy, :cx] = 30
    return img


@functools.lru_cache(maxsize=None)
def small_planes(H: int, W: int, bg: int):
    """Seeded planes of one size for both backgrounds: no foreground, all foreground, the centre on background, random densities, values
    that include the other background."""
    rng = np.random.default_rng(1000 * H + W + bg)
    other = 1 if bg == 255 else 255
    out = [np.full((H, W), bg, np.uint8), np.full((H, W), other, np.uint8)]
    hole = np.full((H, W), 33, np.uint8)
    hole[H // 2, W // 2] = bg
    out.append(hole)
    for dens in (0.3, 0.6, 0.9):
        p = rng.integers(0, 256, (H, W)).astype(np.uint8)
        p[p == bg] = other
        p[rng.random((H, W)) >= dens] = bg
        out.append(p)
        q = p.copy()
        q[H // 2, W // 2] = 77 if bg != 77 else 78      # the same plane with a foreground centre
        out.append(q)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def random_planes(n: int, H: int, W: int, bg: int, seed: int):
    """n planes, alternately at foreground densities 0.3 and 0.6, the centre always foreground."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 255, (n, H, W)).astype(np.uint8)
    p[p == bg] = 3
    dens = np.where(np.arange(n) % 2 == 0, 0.3, 0.6)[:, None, None]
    p[rng.random((n, H, W)) >= dens] = bg
    p[:, H // 2, W // 2] = 100
    return p


def golden_planes():
    """The dozen (plane, background) pairs that go through the reference's own ``single_conn_comp_img``."""
    return [(small_planes(17, 33, 255)[2], 255), (small_planes(17, 33, 255)[3], 255), (small_planes(17, 33, 255)[6], 255),
            (row_end_pair(32), 255), (row_end_pair(33), 255), (diagonal_pair(), 255), (spiral(16, 40), 255), (serpentine(9, 70), 255),
            (small_planes(3, 65, 1)[3], 1), (small_planes(3, 65, 1)[4], 1), (small_planes(17, 31, 1)[6], 1), (small_planes(2, 32, 1)[8], 1)]


# -- the partition golden ---------------------------------------------------------------------------------------------------------------
GOLDEN_COUNTS = (3, 0, 5)      # locations of the three supervoxels


def golden_views(C: int = 1, H: int = 12, W: int = 20, nb_views: int = 2, seed: int = 32):
    """Per supervoxel a uint8 array (n_i, C, nb_views, H, W): blobs on a background of 1 -- the value the reference's
    ``single_conn_comp_img`` call treats as background -- of which the one at the centre survives ``single_cc_only``."""
    rng = np.random.default_rng(seed + C)
    out = []
    for n in GOLDEN_COUNTS:
        v = np.ones((n, C, nb_views, H, W), np.uint8)
        for idx in np.ndindex(n, C, nb_views):
            v[idx][H // 2 - 2:H // 2 + 2, W // 2 - 3:W // 2 + 3] = rng.integers(2, 255, (4, 6))
            v[idx][0:3, 0:4] = rng.integers(2, 255, (3, 4))
            v[idx][H - 2:, W - 5:] = rng.integers(2, 255, (2, 5))
        out.append(v)
    return out


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return np.uint32(c)
