"""Label volumes for the skeletonisation tests: the smallest shapes that still exercise the structure of csrc/sd_skeletonize.hip.  T is the
exported tile edge; every case is (name, seg uint64 (X, Y, Z), parameters of _skeletonize_ref.skeletonize / proc.skeleton.trace_chunk).
`multi` marks the cases whose invalidation radius is small against the object, which must yield at least three rounds."""
import numpy as np

T = 16      # SD_SKELETONIZE_TILE (test_skeletonize_cpu.py checks it against the header)


def draw(seg, points, label, thick=0):
    """Voxels along the polyline through `points` (straight or exactly diagonal segments), thickened by `thick` in every direction."""
    for a, b in zip(points[:-1], points[1:]):
        a, b = np.array(a), np.array(b)
        n = int(np.abs(b - a).max())
        for k in range(n + 1):
            q = a + (b - a) * k // max(n, 1)
            lo, hi = np.maximum(q - thick, 0), q + thick + 1
            seg[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = label
    return seg


def tile_seams():
    """(T + 1, T + 2, 2T + 1): a tortuous tube that crosses the tile seams along x, y, z and on both diagonals, with two side branches."""
    seg = np.zeros((T + 1, T + 2, 2 * T + 1), np.uint64)
    draw(seg, [(1, 1, 1), (1, 1, 2 * T - 2), (T - 1, T - 1, 2 * T - 2), (T - 1, T - 1, T + 4), (T - 1, 2, T + 4), (T - 1, 2, 3), (4, T - 1, 3), (4, T - 1, T - 4),
               (T - 1, T - 1 - (T - 5), T - 4 + (T - 5))], 7, 0)
    draw(seg, [(1, 1, T), (8, 8, T)], 7, 0)
    draw(seg, [(T - 1, 8, T + 4), (T - 1 - 6, 8, T + 4 + 6)], 7, 0)
    seg[0:3, 0:3, 0:3] = 7
    return seg


def branch_y():
    seg = np.zeros((21, 21, 5), np.uint64)
    draw(seg, [(10, 10, 2), (10, 1, 2)], 3, 1)
    draw(seg, [(10, 10, 2), (2, 18, 2)], 3, 1)
    draw(seg, [(10, 10, 2), (18, 18, 2)], 3, 1)
    draw(seg, [(4, 5, 2), (16, 5, 2)], 3, 0)      # two twigs on the stem, mirror images like the arms
    return seg


def branch_cross():
    seg = np.zeros((23, 23, 5), np.uint64)
    draw(seg, [(11, 1, 2), (11, 21, 2)], 3, 1)
    draw(seg, [(1, 11, 2), (21, 11, 2)], 3, 1)
    return seg


def multi_label():
    """Two labels that touch only diagonally, two components of one label, a component below the dust threshold (5 voxels, threshold 6), a
    component on the array border."""
    seg = np.zeros((T + 3, 14, 12), np.uint64)
    draw(seg, [(1, 1, 1), (8, 1, 1), (8, 6, 1)], 5, 0)
    draw(seg, [(9, 7, 2), (9, 12, 2), (14, 12, 7)], 9, 0)      # (8, 6, 1) - (9, 7, 2): a corner contact of labels 5 and 9
    draw(seg, [(1, 5, 5), (1, 12, 5), (5, 12, 9)], 5, 0)       # the second component of label 5
    draw(seg, [(12, 2, 9), (16, 2, 9)], 4, 0)                  # dust
    draw(seg, [(T + 2, 0, 0), (T + 2, 13, 0), (T + 2, 13, 11)], 11, 0)      # on the border
    draw(seg, [(T + 2, 6, 0), (T - 4, 6, 0)], 11, 0)
    draw(seg, [(T + 2, 13, 5), (T - 3, 13, 5)], 11, 0)
    return seg


def small_tree():
    seg = np.zeros((12, 15, 9), np.uint64)
    draw(seg, [(1, 1, 1), (10, 10, 1), (10, 13, 7)], 2, 0)
    draw(seg, [(5, 5, 1), (5, 12, 7)], 2, 0)
    draw(seg, [(8, 8, 1), (2, 12, 4)], 2, 0)
    seg[4:7, 4:7, 0:3] = 2
    return seg


def minimal():
    seg = np.zeros((5, 6, 7), np.uint64)
    seg[1, 1, 1] = 4
    seg[3, 3, 3] = 6
    seg[3, 4, 4] = 6
    return seg


THIN = dict(dust_threshold=1, scale=1.0, const=1.0, pdrf_scale=100000.0, pdrf_exponent=4, max_paths=100)


def cases():
    out = [('tile_seams', tile_seams(), dict(THIN, w=(1, 1, 1)), True),
           ('branch_y', branch_y(), dict(THIN, w=(1, 1, 1)), True),
           ('branch_cross', branch_cross(), dict(THIN, w=(1, 1, 1)), True),
           ('multi_label', multi_label(), dict(THIN, w=(1, 1, 1), dust_threshold=6), True),
           ('minimal', minimal(), dict(THIN, w=(1, 1, 1)), False),
           ('max_paths_1', small_tree(), dict(THIN, w=(1, 1, 1), max_paths=1), False),
           ('reference_params', small_tree(), dict(THIN, w=(10, 10, 20), scale=2.0, const=500.0), False)]
    for w, e in (((1, 1, 1), 1), ((10, 10, 20), 4), ((9, 9, 20), 16), ((10, 10, 20), 1), ((9, 9, 20), 4), ((1, 1, 1), 16)):
        out.append((f'aniso_{w[0]}_{w[2]}_e{e}', small_tree(), dict(THIN, w=w, pdrf_exponent=e, scale=1.0, const=float(min(w))), True))
    return out
