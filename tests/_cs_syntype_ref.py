"""numpy + scipy restatement of the synapse statistics of contact sites and of the per-chunk worker (a test helper):
extract_cs_syntype, the sj morphology on binary masks, the syn-type masks and the worker body with its merges.  Builds on
``_cs_ref`` (boundaries, partner stencil, closing + dilation in ascending id order)."""
import os
import sys
from collections import defaultdict

import numpy as np
import scipy.ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cs_ref  # noqa: E402


def extract_cs_syntype(cs, syn, asym, sym, offset):
    """The five results of block_processing_C.pyx extract_cs_syntype, dict keys in ascending id order."""
    flat = cs.reshape(-1)
    lin = np.flatnonzero(flat)                                       # raster (x, y, z) scan order
    keys = flat[lin]
    coords = np.stack(np.unravel_index(lin, cs.shape), 1).astype(np.int64)
    sflag = syn.reshape(-1)[lin] != 0

    def props(k, c):
        ids, first, inv = np.unique(k, return_index=True, return_inverse=True)
        lo = np.full((len(ids), 3), np.iinfo(np.int64).max, np.int64)
        hi = np.zeros((len(ids), 3), np.int64)
        for a in range(3):
            np.minimum.at(lo[:, a], inv, c[:, a])
            np.maximum.at(hi[:, a], inv, c[:, a] + 1)
        size = np.bincount(inv, minlength=len(ids))
        il = ids.tolist()
        return (dict(zip(il, c[first].tolist())), dict(zip(il, np.stack([lo, hi], 1).tolist())), dict(zip(il, size.tolist())))

    cs_p = list(props(keys, coords))
    syn_p = list(props(keys[sflag], coords[sflag]))
    sk = keys[sflag]
    def counts(m):
        ids, n = np.unique(sk[m.reshape(-1)[lin][sflag] == 1], return_counts=True)
        return dict(zip(ids.tolist(), n.tolist()))
    vox = {}
    sc = coords[sflag] + np.asarray(offset, np.int64)
    order = np.argsort(sk, kind='stable')
    ids, start, n = np.unique(sk[order], return_index=True, return_counts=True)
    for k, s0, c in zip(ids.tolist(), start.tolist(), n.tolist()):
        vox[k] = sc[order[s0:s0 + c]].tolist()
    return cs_p, syn_p, counts(asym), counts(sym), vox


def count_subsequent_mops(mops):
    names, cnt = [], []
    for m in mops:
        if names and names[-1] == m:
            cnt[-1] += 1
        else:
            names.append(m)
            cnt.append(1)
    return names, cnt


def binary_morphology(mask, ops, structure):
    """apply_morphological_operations on a 0/1 mask: per merged run, the operation inside the foreground's box (zero pad of
    `n` for closing / dilation, then cropped back); erosion / opening replace the foreground, closing / dilation also fill
    background."""
    out = (np.asarray(mask) != 0).astype(np.uint8)
    for op, n in zip(*count_subsequent_mops(list(ops))):
        sl = scipy.ndimage.find_objects(out)
        if not sl or sl[0] is None:
            continue
        box = sl[0]
        sub = out[box]
        grow = op in ('binary_closing', 'binary_dilation')
        m = np.pad(sub, n) if grow else sub.copy()
        res = getattr(scipy.ndimage, op)(m, structure=structure, iterations=n)
        if grow:
            res = res[n:-n, n:-n, n:-n]
            sub[(sub == 1) | (sub == 0)] = res[(sub == 1) | (sub == 0)]
        else:
            sub[sub == 1] = res[sub == 1]
    return out


def aniso_struct(scaling):
    aniso = int(scaling[2] // scaling[0])
    st = np.zeros((5, 5, 3), bool)
    st[2, 2, :] = True
    for dx in range(-2, 3):
        for dy in range(-2, 3):
            if abs(dx) + abs(dy) <= aniso:
                st[2 + dx, 2 + dy, 1] = True
    return st


def merge_prop_dicts(into, chunk, offset):
    rc, bb, sz = chunk
    for k in rc:
        into[0][k] = (np.asarray(rc[k]) + offset).tolist()
    for k in bb:
        into[1][k].append((np.asarray(bb[k]) + offset).tolist())
    for k, n in sz.items():
        into[2][k] = into[2].get(k, 0) + n


def worker(chunks, kd, kd_sj, cfg, transf_func_sj_seg=None, kd_sym=None, kd_asym=None):
    """The worker body on host arrays.  `cfg`: dict with cs_filtersize, cs_dilation, sj_ops, scaling, sj_thresh, syntype,
    sym_label, asym_label, same_kd.  Returns (cs_props, syn_props, syn_voxels {str: int64 (n, 3)}, asym, sym, cores) with
    cores = [(offset, cs core (z, y, x), syn core (z, y, x))]."""
    fs = np.asarray(cfg['cs_filtersize'])
    so = fs // 2
    ov = int(max(so))
    struct = aniso_struct(cfg['scaling'])
    cs_props, syn_props = [{}, defaultdict(list), {}], [{}, defaultdict(list), {}]
    vox, tot_a, tot_s, cores = {}, {}, {}, []
    for ch in chunks:
        off = np.asarray(ch.coordinates) - ov
        size = 2 * ov + np.asarray(ch.size)
        data = kd.load_seg(size=size + 2 * so, offset=off - so, mag=1).astype(np.uint32).swapaxes(0, 2)
        edges = _cs_ref.seg_boundaries(data)
        contacts = _cs_ref.contact_partners(edges, data, fs)
        contacts = _cs_ref.close_dilate(contacts, ov, cfg['cs_dilation'])
        if transf_func_sj_seg is None:
            sj = (kd_sj.load_raw(size=size, offset=off, mag=1).swapaxes(0, 2) > 255 * cfg['sj_thresh']).astype('u1')
        else:
            sj = transf_func_sj_seg(kd_sj.load_seg(size=size, offset=off, mag=1).swapaxes(0, 2)).astype('u1', copy=False)
        if cfg['sj_ops']:
            sj = binary_morphology(sj, cfg['sj_ops'], struct)
        if cfg['syntype']:
            if not cfg['same_kd']:
                def one(k, lab):
                    if lab is None:
                        return (k.load_raw(size=size, offset=off, mag=1).swapaxes(0, 2) >= 123).astype('u1')
                    return (k.load_seg(size=size, offset=off, mag=1).swapaxes(0, 2) == lab).astype('u1')
                sym, asym = one(kd_sym, cfg['sym_label']), one(kd_asym, cfg['asym_label'])
            else:
                t = kd_sym.load_seg(size=size, offset=off, mag=1).swapaxes(0, 2)
                asym, sym = (t == cfg['asym_label']).astype('u1'), (t == cfg['sym_label']).astype('u1')
        else:
            sym = asym = np.zeros_like(sj)
        c = (slice(ov, -ov),) * 3
        cp, sp, a, s, v = extract_cs_syntype(contacts[c], sj[c], asym[c], sym[c], off + ov)
        syn_seg = np.where(sj != 0, contacts, 0)
        cores.append((off + ov, contacts[c].swapaxes(0, 2).copy(), syn_seg[c].swapaxes(0, 2).copy()))
        merge_prop_dicts(cs_props, cp, off + ov)
        merge_prop_dicts(syn_props, sp, off + ov)
        for k, x in v.items():
            vox.setdefault(str(k), []).extend(x)
        for tot, d in ((tot_a, a), (tot_s, s)):
            for k, n in d.items():
                tot[k] = tot.get(k, 0) + n
    return cs_props, syn_props, {k: np.asarray(x, np.int64) for k, x in vox.items()}, tot_a, tot_s, cores
