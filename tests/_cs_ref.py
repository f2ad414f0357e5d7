"""numpy + scipy restatement of the contact-site steps the device computes (a test helper): boundary mask, partner stencil,
per-site closing + dilation with a selectable site order."""
import numpy as np
import scipy.ndimage


def seg_boundaries(seg):
    """Non-zero voxels with an in-array 6-neighbour of another value (0 included)."""
    b = np.zeros(seg.shape, bool)
    for ax in range(3):
        n = seg.shape[ax]
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, n - 1), slice(1, n)
        d = seg[tuple(lo)] != seg[tuple(hi)]
        b[tuple(lo)] |= d
        b[tuple(hi)] |= d
    return b & (seg != 0)


def _box_sum(m, st):
    """Valid-convolution window sums of a 0/1 array (integral image)."""
    c = np.zeros(tuple(s + 1 for s in m.shape), np.int32)
    c[1:, 1:, 1:] = m.astype(np.int32).cumsum(0).cumsum(1).cumsum(2)
    a, b, d = st
    X, Y, Z = m.shape[0] - a + 1, m.shape[1] - b + 1, m.shape[2] - d + 1
    s = lambda i, j, k: c[i:i + X, j:j + Y, k:k + Z]
    return (s(a, b, d) - s(0, b, d) - s(a, 0, d) - s(a, b, 0) + s(0, 0, d) + s(0, b, 0) + s(a, 0, 0) - s(0, 0, 0))


def contact_partners(edges, seg, st):
    """For flagged centres: the most frequent window id other than 0 and the centre (ties: smallest), packed with the centre."""
    seg = seg.astype(np.uint32)
    st = tuple(int(s) for s in st)
    out_shape = tuple(n - s + 1 for n, s in zip(seg.shape, st))
    h = [s // 2 for s in st]
    centre = seg[h[0]:h[0] + out_shape[0], h[1]:h[1] + out_shape[1], h[2]:h[2] + out_shape[2]]
    flag = edges[h[0]:h[0] + out_shape[0], h[1]:h[1] + out_shape[1], h[2]:h[2] + out_shape[2]] != 0
    best = np.zeros(out_shape, np.int32)
    key = np.zeros(out_shape, np.uint32)
    ids, inv = np.unique(seg.ravel(), return_inverse=True)
    lab = inv.reshape(seg.shape) + 1
    for k, sl in enumerate(scipy.ndimage.find_objects(lab)):
        u = ids[k]
        if u == 0 or sl is None:
            continue
        # outputs whose window meets the id's box
        o_lo = [max(s.start - st[a] + 1, 0) for a, s in enumerate(sl)]
        o_hi = [min(s.stop, out_shape[a]) for a, s in enumerate(sl)]
        if any(l >= hh for l, hh in zip(o_lo, o_hi)):
            continue
        sub = lab[o_lo[0]:o_hi[0] + st[0] - 1, o_lo[1]:o_hi[1] + st[1] - 1, o_lo[2]:o_hi[2] + st[2] - 1] == k + 1
        cnt = _box_sum(sub, st)
        osl = tuple(slice(l, hh) for l, hh in zip(o_lo, o_hi))
        cnt[centre[osl] == u] = 0
        upd = cnt > best[osl]                                          # ascending ids + strict '>': ties keep the smaller id
        best[osl][upd] = cnt[upd]
        key[osl][upd] = u
    c64, k64 = centre.astype(np.uint64), key.astype(np.uint64)
    lo, hi = np.minimum(c64, k64), np.maximum(c64, k64)
    res = (lo << np.uint64(32)) | hi
    res[(best == 0) | ~flag] = 0
    return res


def close_dilate(contacts, n, k, order='ascending'):
    """Per site (ascending or descending id order): closing^n then dilation^k of the site in its box; background voxels of the
    current volume inside the result take the id (the reference's loop, cs_extraction_steps.py:437-461)."""
    out = contacts.copy()
    ids, inv = np.unique(contacts.ravel(), return_inverse=True)
    slices = scipy.ndimage.find_objects(inv.reshape(contacts.shape) + 1)
    order_k = range(len(ids)) if order == 'ascending' else range(len(ids) - 1, -1, -1)
    for q in order_k:
        ix, sl = ids[q], slices[q]
        if ix == 0 or sl is None:
            continue
        lo = [max(s.start - n, 0) for s in sl]
        box = tuple(slice(l, s.stop + n) for l, s in zip(lo, sl))
        sub = out[box]
        m = sub == ix
        res = scipy.ndimage.binary_closing(m, iterations=n) if n > 0 else m
        if k > 0:
            res = scipy.ndimage.binary_dilation(res, iterations=k)
        sub[(m | (sub == 0)) & res] = ix
    return out
