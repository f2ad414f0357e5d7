"""Drop-in for the Cython natives re-exported by /root/reference/syconn/extraction/find_object_properties.py:9-11
(implemented in find_object_properties_C.pyx): label-volume statistics of segmentation chunks, computed on the MI355X
by one streaming pass into device hash tables (``include/syconn_dense.h``: ``sd_segstats_*``).

Same call signatures and return structure as the reference (plain dicts with list values, as Cython converts the C++
maps): ids are Python ints, coordinates index the (x, y, z) array that was passed in.  Inputs may be numpy arrays
(uint32 / uint64, copied to the device) or torch tensors already on the device (int32 / int64 bit patterns or
torch.uint32 / torch.uint64).  There is no CPU fallback.
"""
import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _dev as D
from .. import _lib as L


def _to_device(vol, device) -> Tuple[torch.Tensor, int]:
    """-> (contiguous device tensor viewed as a signed integer type of the same width, SD_U32 | SD_U64)."""
    if isinstance(vol, np.ndarray):
        if vol.dtype not in (np.uint64, np.uint32):
            raise TypeError(f'label volumes must be uint32 or uint64, got {vol.dtype}')   # the fused type n_type of the .pyx
        t = D.up(vol, device)
    else:
        t = vol
        if t.dtype in (torch.uint64, torch.int64):
            t = t.view(torch.int64)
        elif t.dtype in (torch.uint32, torch.int32):
            t = t.view(torch.int32)
        else:
            raise TypeError(f'label volumes must be 32- or 64-bit integers, got {t.dtype}')
        t = t.to(device).contiguous()
    return t, (L.SD_U64 if t.dtype == torch.int64 else L.SD_U32)


def _pow2_at_least(n: int) -> int:
    return 1 << max(10, int(n - 1).bit_length())


class SegStats:
    """Result of one pass, still as dense arrays (ids ascending): ``cell`` / ``sub[i]`` = (ids, first, size, bbox) with
    bbox (n, 2, 3); ``pairs[i]`` = (subcell ids, cell ids, counts).  ``cap_obj`` / ``cap_pair``: the table capacities the pass
    ended with (larger than the ones it started with when a table overflowed and the pass was repeated)."""

    def __init__(self):
        self.shape = None
        self.cell = None
        self.sub: List[tuple] = []
        self.pairs: List[tuple] = []
        self.cap_obj = self.cap_pair = 0


class DeviceScan:
    """Hash tables of ``sd_segstats_scan`` kept on the device and reused from chunk to chunk (the scan initialises them itself).
    After ``scan``: ``tabs[0]`` = cell table (when a cell volume was given), ``tabs[k..]`` = subcell tables, ``ptabs[i]`` = pair table
    of subcell volume i; capacities grow (and stay grown) when a pass reports overflow."""

    def __init__(self, device=None, cap_obj: Optional[int] = None, cap_pair: Optional[int] = None):
        self.lib = L.load()
        self.device = D.device(device)
        self.cap_obj = _pow2_at_least(cap_obj) if cap_obj else 0
        self.cap_pair = _pow2_at_least(cap_pair) if cap_pair else 0
        self.tabs: List[torch.Tensor] = []
        self.ptabs: List[torch.Tensor] = []
        self.status = torch.zeros(2, dtype=torch.int32, device=self.device)
        self.shape = None
        self.has_cell = False
        self.n_sub = 0

    def _room(self, n_tabs: int, n_ptabs: int):
        ob, pb = self.lib.sd_objtable_bytes(self.cap_obj), self.lib.sd_pairtable_bytes(self.cap_pair)
        self.tabs = [t for t in self.tabs if t.numel() == ob][:n_tabs]
        self.ptabs = [t for t in self.ptabs if t.numel() == pb][:n_ptabs]
        while len(self.tabs) < n_tabs:
            self.tabs.append(torch.empty(ob, dtype=torch.uint8, device=self.device))
        while len(self.ptabs) < n_ptabs:
            self.ptabs.append(torch.empty(pb, dtype=torch.uint8, device=self.device))

    def scan(self, cell, subs: Sequence = (), want_props: bool = True, status_out: Optional[torch.Tensor] = None):
        """One streaming pass over `cell` (may be None) and the `subs` volumes, all of one (X, Y, Z) shape and dtype.
        `status_out` (int32[2] on the device): the pass writes its overflow flags there and this call does NOT wait for them -- the
        caller reads them later and repeats the work with larger tables (`cap_obj` / `cap_pair` are then the caller's business);
        without it the flags are awaited here and an overflowed pass is repeated with 4x the capacity."""
        device = self.device
        vols = [v for v in ([cell] if cell is not None else []) + list(subs)]
        if not vols:
            raise ValueError('no volume given')
        shape = tuple(int(s) for s in vols[0].shape)
        if len(shape) != 3:
            raise ValueError('label volumes must be 3D (x, y, z)')
        for v in vols:
            assert tuple(v.shape) == shape, 'Segmentation of cells and subcellular structures must have same shape.'
        dev = [_to_device(v, device) for v in vols]
        if len({d for _, d in dev}) != 1:
            raise TypeError('all label volumes of one call must share a dtype')
        dtype = dev[0][1]
        cell_t = dev[0][0] if cell is not None else None
        sub_ts = [t for t, _ in (dev[1:] if cell is not None else dev)]
        n_sub = len(sub_ts)
        nvox = shape[0] * shape[1] * shape[2]
        # capacity guess: label volumes hold far fewer objects than voxels; overflow is detected and the pass repeated
        if not self.cap_obj:
            self.cap_obj = _pow2_at_least(min(2 * nvox, max(1 << 16, nvox // 256)))
        if not self.cap_pair:
            self.cap_pair = self.cap_obj
        while True:
            self._room(1 + n_sub, n_sub if cell_t is not None else 0)
            tabs, ptabs = self.tabs, self.ptabs
            sub_ptrs = (C.c_void_p * max(n_sub, 1))(*[t.data_ptr() for t in sub_ts])
            sub_tabs = (C.c_void_p * max(n_sub, 1))(*[t.data_ptr() for t in tabs[1:]])
            pair_tabs = (C.c_void_p * max(n_sub, 1))(*[t.data_ptr() for t in ptabs])
            D.call('sd_segstats_scan', device, cell_t, sub_ptrs, n_sub, dtype, *shape, tabs[0] if cell_t is not None else None, sub_tabs,
                   self.cap_obj, pair_tabs, self.cap_pair, 1 if want_props else 0, self.status if status_out is None else status_out)
            if status_out is not None:
                break
            st = self.status.cpu().tolist()
            if not any(st):
                break
            if st[0]:
                if self.cap_obj >= 2 * nvox:
                    raise RuntimeError('sd_segstats_scan: object table overflow at maximum capacity')
                self.cap_obj *= 4
            if st[1]:
                self.cap_pair *= 4
        self.shape, self.has_cell, self.n_sub = shape, cell_t is not None, n_sub
        return self

    @property
    def cell_table(self):
        return self.tabs[0] if self.has_cell else None

    @property
    def sub_tables(self):
        return self.tabs[1:1 + self.n_sub]


def segstats(cell, subs: Sequence = (), want_props: bool = True, device=None, cap_obj: Optional[int] = None,
             cap_pair: Optional[int] = None) -> SegStats:
    """One streaming pass over `cell` (may be None) and the `subs` volumes, all of one (X, Y, Z) shape and dtype."""
    sc = DeviceScan(device, cap_obj, cap_pair).scan(cell, subs, want_props)
    device, cap_obj, cap_pair, tabs, ptabs = sc.device, sc.cap_obj, sc.cap_pair, sc.tabs, sc.ptabs
    shape, n_sub = sc.shape, sc.n_sub
    cell_t = True if sc.has_cell else None

    def objects(tab):
        n_max = cap_obj
        cnt = D.counters(device, 1)
        ids, first, size = (D.empty(n_max, D.i64, device) for _ in range(3))
        bb = D.empty((n_max, 6), D.i32, device)
        D.call('sd_segstats_compact_objects', device, tab, cap_obj, ids, first, size, bb, n_max, cnt)
        n = int(cnt.item())
        ids_h = D.down(ids, n, np.uint64)
        order = np.argsort(ids_h, kind='stable')
        return ids_h[order], D.down(first, n)[order], D.down(size, n)[order], D.down(bb, n).reshape(n, 2, 3)[order]

    def pairs(ptab, stab, ctab):
        n_max = cap_pair
        cnt = D.counters(device, 1)
        a, b, c = (D.empty(n_max, D.i64, device) for _ in range(3))
        D.call('sd_segstats_compact_pairs', device, ptab, cap_pair, stab, ctab, cap_obj, a, b, c, n_max, cnt)
        n = int(cnt.item())
        s_h, c_h, n_h = D.down(a, n, np.uint64), D.down(b, n, np.uint64), D.down(c, n)
        order = np.lexsort((c_h, s_h))
        return s_h[order], c_h[order], n_h[order]

    res = SegStats()
    res.shape = shape
    res.cap_obj, res.cap_pair = cap_obj, cap_pair
    if want_props:
        if cell_t is not None:
            res.cell = objects(tabs[0])
        res.sub = [objects(t) for t in tabs[1:1 + n_sub]]
    if cell_t is not None:
        res.pairs = [pairs(ptabs[i], tabs[1 + i], tabs[0]) for i in range(n_sub)]
    return res


def _prop_dicts(shape, ids, first, size, bb):
    rc = np.stack(np.unravel_index(first, shape), axis=1) if len(ids) else np.zeros((0, 3), np.int64)
    keys = ids.tolist()
    return dict(zip(keys, rc.tolist())), dict(zip(keys, bb.tolist())), dict(zip(keys, size.tolist()))


def _pair_dict(s, c, n) -> Dict[int, Dict[int, int]]:
    d: Dict[int, Dict[int, int]] = {}
    for sk, ck, cnt in zip(s.tolist(), c.tolist(), n.tolist()):
        d.setdefault(sk, {})[ck] = cnt
    return d


def find_object_properties(chunk):
    """find_object_properties_C.pyx:24-49: ``(rep_coords, bounding_box, sizes)`` of the non-zero ids of `chunk` (x,y,z):
    id -> first voxel in raster order, id -> [[min], [max + 1]], id -> voxel count."""
    r = segstats(chunk)
    return _prop_dicts(r.shape, *r.cell)


def map_subcell_extract_props(ch, subcell_chs):
    """find_object_properties_C.pyx:112-192: ``[rc, bb, size]`` of the cell segmentation, ``[[rc...], [bb...], [size...]]``
    per subcellular volume, and per subcellular volume ``subcell id -> cell id -> overlapping voxels``."""
    subs = [subcell_chs[i] for i in range(len(subcell_chs))]
    r = segstats(ch, subs)
    cell = list(_prop_dicts(r.shape, *r.cell))
    sub = [[], [], []]
    for s in r.sub:
        rc, bb, sz = _prop_dicts(r.shape, *s)
        sub[0].append(rc); sub[1].append(bb); sub[2].append(sz)
    return cell, sub, [_pair_dict(*p) for p in r.pairs]


def map_subcell_C(ch, subcell_chs):
    """find_object_properties_C.pyx:72-109: the overlap counts only."""
    subs = [subcell_chs[i] for i in range(len(subcell_chs))]
    r = segstats(ch, subs, want_props=False)
    return [_pair_dict(*p) for p in r.pairs]


# ---- contact sites (block_processing_C.pyx:21-75, find_object_properties.py:424-472 of the reference) -------------------------
def _u32_volume(arr, device) -> torch.Tensor:
    """uint32 (X, Y, Z) volume -> contiguous int32 device tensor (the same bits)."""
    if isinstance(arr, np.ndarray):
        if arr.dtype != np.uint32:
            raise TypeError(f'the cell segmentation must be uint32, got {arr.dtype}')
        t = D.up(arr, device)
    else:
        if arr.dtype not in (torch.uint32, torch.int32):
            raise TypeError(f'the cell segmentation must be a 32-bit integer tensor, got {arr.dtype}')
        t = arr.view(torch.int32).to(device).contiguous()
    if t.dim() != 3:
        raise ValueError('the segmentation must be 3D (x, y, z)')
    return t


def _mask_volume(arr, device) -> torch.Tensor:
    """any (X, Y, Z) array / tensor -> contiguous uint8 device tensor, 1 where non-zero."""
    t = torch.from_numpy(np.ascontiguousarray(arr)) if isinstance(arr, np.ndarray) else arr
    if t.dtype == torch.uint64:
        t = t.view(torch.int64)
    elif t.dtype == torch.uint32:
        t = t.view(torch.int32)
    return (t.to(device) != 0).to(torch.uint8).contiguous()


def detect_seg_boundaries(arr, return_device: bool = False, device=None):
    """find_object_properties.py:424-455: boolean mask of the non-zero voxels of `arr` (uint32, x, y, z) that have an in-array
    6-neighbour with another value (0 counts as another value).  ``return_device``: a uint8 device tensor instead."""
    dev = D.device(device)
    seg = _u32_volume(arr, dev)
    X, Y, Z = (int(s) for s in seg.shape)
    mask = torch.empty((X, Y, Z), dtype=torch.uint8, device=dev)
    D.call('sd_seg_boundaries', dev, seg, X, Y, Z, mask)
    return mask if return_device else mask.cpu().numpy().view(np.bool_)


def process_block_nonzero(edges, arr, stencil1=(7, 7, 3), return_device: bool = False, device=None):
    """block_processing_C.pyx:50-75: for every centre voxel with ``edges != 0`` the most frequent id of its `stencil1` window other
    than 0 and the centre id (ties: the smallest id), packed as ``(min << 32) | max`` with the centre id; valid convolution, uint64
    of shape ``arr.shape - stencil1 + 1``.  ``return_device``: an int64 device tensor holding the uint64 bits."""
    stencil = tuple(int(s) for s in stencil1)
    assert sum(s % 2 for s in stencil) == 3
    dev = D.device(device)
    seg = _u32_volume(arr, dev)
    e = _mask_volume(edges, dev)
    X, Y, Z = (int(s) for s in seg.shape)
    if tuple(e.shape) != (X, Y, Z):
        raise ValueError('edges and arr must have the same shape')
    out_shape = tuple(max(n - s + 1, 0) for n, s in zip((X, Y, Z), stencil))
    out = torch.zeros(out_shape, dtype=torch.int64, device=dev)
    ws = D.scratch('sd_contact_partners_workspace_bytes', dev)
    if out.numel():
        D.call('sd_contact_partners', dev, e, seg, X, Y, Z, *stencil, out, ws, ws.numel())
    return out if return_device else out.cpu().numpy().view(np.uint64)


def detect_cs(arr, stencil=None, return_device: bool = False, device=None):
    """find_object_properties.py:458-472: contact-site ids of a uint32 cell segmentation (uint64, valid convolution of the
    stencil; default ``config['cell_objects']['cs_filtersize']``)."""
    if stencil is None:
        from .. import global_params
        stencil = global_params.config['cell_objects']['cs_filtersize']
    dev = D.device(device)
    seg = _u32_volume(arr, dev)
    edges = detect_seg_boundaries(seg, return_device=True, device=dev)
    return process_block_nonzero(edges, seg, stencil, return_device=return_device, device=dev)


# ---- synapse statistics of contact sites (block_processing_C.pyx:78-158 extract_cs_syntype; find_object_properties.py:302-344) ----
def _u8_volume(arr, device) -> torch.Tensor:
    """uint8 / bool (X, Y, Z) array or tensor -> contiguous uint8 device tensor with the same values."""
    t = torch.from_numpy(np.ascontiguousarray(arr)) if isinstance(arr, np.ndarray) else arr
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype != torch.uint8:
        raise TypeError(f'syn / type masks must be uint8, got {t.dtype}')
    return t.to(device).contiguous()


class CsSyntype:
    """Result of ``cs_syntype`` as device tensors, sites in ascending id order.  ``rec`` int64 (n, SD_CST_COLS), the columns of
    ``sd_cs_syntype_records``; ``voxels`` int64 (n_syn, 3), the syn voxels of site i at rows ``rec[i, 23] : rec[i, 23] + rec[i, 14]``,
    in scan order, offset included."""

    def __init__(self, rec: torch.Tensor, voxels: torch.Tensor, cs_core=None, syn_core=None):
        self.rec, self.voxels, self.cs_core, self.syn_core = rec, voxels, cs_core, syn_core

    @property
    def ids(self) -> torch.Tensor:
        return self.rec[:, 0]

    def host(self):
        """(rec, voxels) as numpy arrays (column 0 of rec holds the uint64 ids' bits)."""
        return self.rec.cpu().numpy(), self.voxels.cpu().numpy()


def cs_syntype_dicts(rec: np.ndarray, voxels: np.ndarray):
    """Host records -> the return value of ``extract_cs_syntype`` (dicts in ascending id order)."""
    ids = rec[:, 0].view(np.uint64).tolist() if len(rec) else []
    def props(c0):
        return (dict(zip(ids, rec[:, c0:c0 + 3].tolist())), dict(zip(ids, rec[:, c0 + 4:c0 + 10].reshape(-1, 2, 3).tolist())),
                dict(zip(ids, rec[:, c0 + 3].tolist())))
    cs_rc, cs_bb, cs_sz = props(1)
    syn = rec[:, 14] > 0
    s_rc, s_bb, s_sz = props(11)
    keep = lambda d, m: {k: v for (k, v), f in zip(d.items(), m) if f}
    syn_m = syn.tolist()
    asym = {k: v for k, v in zip(ids, rec[:, 21].tolist()) if v}
    sym = {k: v for k, v in zip(ids, rec[:, 22].tolist()) if v}
    vox = {}
    if len(rec):
        for k, o, n in zip(ids, rec[:, 23].tolist(), rec[:, 14].tolist()):
            if n:
                vox[k] = voxels[o:o + n].tolist()
    return [cs_rc, cs_bb, cs_sz], [keep(s_rc, syn_m), keep(s_bb, syn_m), keep(s_sz, syn_m)], asym, sym, vox


class CsSyntypeScan:
    """The hash table of ``sd_cs_syntype_scan`` kept on the device from call to call; its capacity grows (and stays grown) when a
    pass reports overflow, as ``DeviceScan`` does."""

    def __init__(self, device=None, cap: Optional[int] = None):
        self.lib = L.load()
        self.device = D.device(device)
        self.cap = _pow2_at_least(cap) if cap else 0
        self.table = None
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.passes = 0                          # scan passes of the last call (> 1: the table overflowed)

    def run(self, cs, syn, asym, sym, offset=(0, 0, 0), origin=(0, 0, 0), extent=None, want_cores: bool = False) -> CsSyntype:
        """extract_cs_syntype on the window [origin, origin + extent) of the four (X, Y, Z) volumes (default: all of it);
        `offset` is added to the voxel lists only.  ``want_cores``: also the window's ids and its syn segmentation (the ids where
        syn != 0, else 0) as (nx, ny, nz) device tensors of the id type."""
        lib, dev = self.lib, self.device
        c, dtype = _to_device(cs, dev)
        if c.dim() != 3:
            raise ValueError('cs_seg must be 3D (x, y, z)')
        shape = tuple(int(s) for s in c.shape)
        m = [_u8_volume(v, dev) for v in (syn, asym, sym)]
        for v in m:
            if tuple(v.shape) != shape:
                raise ValueError('cs_seg, syn_mask, sym_mask and asym_mask must all have the same shape')
        org = tuple(int(v) for v in origin)
        ext = tuple(int(s) - o for s, o in zip(shape, org)) if extent is None else tuple(int(v) for v in extent)
        off = np.asarray(offset, dtype=np.int64).reshape(3)
        nvox = ext[0] * ext[1] * ext[2]
        if not self.cap:
            self.cap = _pow2_at_least(min(2 * max(nvox, 1), max(1 << 12, nvox // 256)))
        cores = [torch.empty(ext, dtype=c.dtype, device=dev) for _ in range(2)] if want_cores else [None, None]
        self.passes = 0
        while True:
            nb = lib.sd_cs_syntype_table_bytes(self.cap)
            if self.table is None or self.table.numel() != nb:
                self.table = torch.empty(nb, dtype=torch.uint8, device=dev)
            D.call('sd_cs_syntype_scan', dev, c, dtype, *m, *shape, *org, *ext, self.table, self.cap, *cores, self.status)
            self.passes += 1
            if not int(self.status.item()):
                break
            if self.cap >= 2 * max(nvox, 1):
                raise RuntimeError('sd_cs_syntype_scan: table overflow at maximum capacity')
            self.cap *= 4
        cap = self.cap
        cnt = D.counters(dev, 1)
        ids, slots = D.empty(cap, D.i64, dev), D.empty(cap, D.i32, dev)
        D.call('sd_cs_syntype_compact', dev, self.table, cap, ids, slots, cap, cnt)
        n = int(cnt.item())
        # ascending ids: the order is taken on the host from the n ids, as segstats does
        order = np.argsort(D.down(ids, n, np.uint64), kind='stable')
        slots_sorted = slots[:n][D.up(order, dev)].contiguous()
        rec = D.empty((n, L.SD_CST_COLS), D.i64, dev)
        n_syn = D.counters(dev, 1)
        D.call('sd_cs_syntype_records', dev, self.table, cap, slots_sorted if n else None, n, *ext, rec, n_syn)
        ns = int(n_syn.item())
        vox = D.empty((ns, 3), D.i64, dev)
        D.call('sd_cs_syntype_voxels', dev, c, dtype, m[0], *shape, *org, rec, n, ns, D.i64x3(off), vox, self.status)
        if ns and int(self.status.item()):
            raise RuntimeError('sd_cs_syntype_voxels: voxel counts disagree with the site records')
        return CsSyntype(rec[:n], vox[:ns], *cores)


def cs_syntype(cs_seg, syn_mask, asym_mask, sym_mask, offset=(0, 0, 0), device=None, cap: Optional[int] = None, **kw) -> CsSyntype:
    """Array form of ``extract_cs_syntype``: everything stays on the device (see ``CsSyntype``)."""
    return CsSyntypeScan(device, cap).run(cs_seg, syn_mask, asym_mask, sym_mask, offset, **kw)


def extract_cs_syntype(cs_seg, syn_mask, asym_mask, sym_mask, offset=(0, 0, 0), device=None):
    """block_processing_C.pyx:78-158: ``[rep_coords, bounding_box, sizes], [rep_coords_syn, bounding_box_syn, sizes_syn], cs_asym,
    cs_sym, voxels_syn`` of a uint32 / uint64 contact volume (x, y, z; 0 = background) and three uint8 masks of its shape.  Syn
    voxels are those with ``syn_mask != 0``; ``cs_asym`` / ``cs_sym`` count syn voxels whose type mask is exactly 1; a site appears in
    the syn, asym, sym and voxel dicts only when it has an entry there.  ``voxels_syn[id]`` lists the syn voxels in x, y, z scan
    order as ``[x + offset[0], y + offset[1], z + offset[2]]``; coordinates and boxes are local.  Dict keys are in ascending id
    order (the reference's follow its unordered_maps: DESIGN.md section 7)."""
    return cs_syntype_dicts(*cs_syntype(cs_seg, syn_mask, asym_mask, sym_mask, offset, device=device).host())


def merge_type_dicts(type_dicts: List[dict]):
    """find_object_properties.py:302-321: add the counts of every further dict into the first, in place."""
    tot_map = type_dicts[0]
    for el in type_dicts[1:]:
        for cs_id, cnt in el.items():
            if cs_id in tot_map:
                tot_map[cs_id] += cnt
            else:
                tot_map[cs_id] = cnt


def merge_voxel_dicts(voxel_dicts: List[dict], key_to_str: bool = False):
    """find_object_properties.py:324-344: append the voxel lists of every further dict to the first, in place (numpy arrays
    become lists on first insertion); ``key_to_str``: keys become ``str(id)`` (for ``np.savez``)."""
    tot_map = voxel_dicts[0]
    for el in voxel_dicts[1:]:
        for cs_id, vxs in el.items():
            if key_to_str:
                cs_id = str(cs_id)
            if cs_id in tot_map:
                tot_map[cs_id].extend(vxs)
            else:
                if isinstance(vxs, np.ndarray):
                    vxs = vxs.tolist()
                tot_map[cs_id] = vxs
