"""Contact-site extraction on the MI355X: the device form of the per-chunk steps of
/root/reference/syconn/extraction/cs_extraction_steps.py (``_contact_site_extraction_thread``, :317-495).

Here: the partner search (``find_object_properties.detect_cs``) and the closing + dilation of every contact site inside its own
box (:437-461, ``close_and_dilate_cs``).  Where several sites claim one background voxel the smallest id wins.
Further down: the sj / syn-type masks, the per-chunk worker (:317-495) and the dataset driver ``extract_contact_sites`` (:44-314)
with the merging half of its second step (``_write_props_to_syn_thread`` / ``_write_props_collect_helper``, :498-673): the records
of all chunks stay on the device and are merged once (``ContactSiteMerger``, ``csrc/sd_cs_merge.hip``).
There is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from .. import _dev as D
from .. import _lib as L
from ..proc.records import OBJECT_FIELDS, Records, segment_offsets
from .find_object_properties import segstats

# summed box volume (bytes per workspace plane) of one batch of sites; a single larger box gets a batch of its own
WS_BUDGET = 1 << 28


def _u64_volume(arr, device) -> torch.Tensor:
    if isinstance(arr, np.ndarray):
        if arr.dtype != np.uint64:
            raise TypeError(f'contact volumes must be uint64, got {arr.dtype}')
        t = D.up(arr, device)
    else:
        if arr.dtype not in (torch.uint64, torch.int64):
            raise TypeError(f'contact volumes must be 64-bit integer tensors, got {arr.dtype}')
        t = arr.view(torch.int64).to(device).contiguous()
    if t.dim() != 3:
        raise ValueError('the contact volume must be 3D (x, y, z)')
    return t


def site_boxes(shape, bb, n_closings: int):
    """The boxes the reference closes every site in (:439-446): ``[max(lo - n, 0), hi + n)``, the end clipped as slicing clips.
    bb (n, 2, 3) -> (origin (n, 3), extent (n, 3)) as int64."""
    lo = np.maximum(np.asarray(bb[:, 0], np.int64) - n_closings, 0)
    hi = np.minimum(np.asarray(bb[:, 1], np.int64) + n_closings, np.asarray(shape, np.int64))
    return lo, hi - lo


class SitePlan:
    """The batches of one close / dilate call: per batch the device table of sd_cs_close_dilate, its site count and box volume."""

    def __init__(self, shape, ids, batches, ws_bytes):
        self.shape, self.ids, self.batches, self.ws_bytes = shape, ids, batches, ws_bytes

    @property
    def box_voxels(self) -> int:
        return sum(tot for _, _, tot in self.batches)


def plan_sites(c0: torch.Tensor, n_closings: int, device, ws_budget: int = WS_BUDGET) -> SitePlan:
    """Site ids (ascending) and boxes of a device contact volume, packed into batches of at most `ws_budget` box voxels."""
    X, Y, Z = (int(s) for s in c0.shape)
    if not c0.numel():
        return SitePlan((X, Y, Z), np.zeros(0, np.uint64), [], 0)
    ids, _, _, bb = segstats(c0, device=device).cell                   # ascending ids (the order of this build)
    if len(ids) and ids[-1] == np.uint64(2 ** 64 - 1):
        raise ValueError('close_and_dilate_cs: id 2^64 - 1 is reserved (the unclaimed marker of sd_cs_close_dilate)')
    if not len(ids):
        return SitePlan((X, Y, Z), ids, [], 0)
    lo, ext = site_boxes((X, Y, Z), bb, n_closings)
    vol = np.prod(ext, axis=1)
    budget = max(int(ws_budget), int(vol.max()))
    ends = np.cumsum(vol)
    batches, start = [], 0
    while start < len(ids):
        base = ends[start - 1] if start else 0
        end = max(int(np.searchsorted(ends, base + budget, side='right')), start + 1)
        tab = np.empty((end - start, 8), np.int64)
        tab[:, 0] = ids[start:end].view(np.int64)
        tab[:, 1:4] = lo[start:end]
        tab[:, 4:7] = ext[start:end]
        tab[:, 7] = np.concatenate([[0], np.cumsum(vol[start:end])[:-1]])
        batches.append((D.up(tab, device), end - start, int(vol[start:end].sum())))
        start = end
    return SitePlan((X, Y, Z), ids, batches, 2 * max(tot for _, _, tot in batches))


def run_sites(c0: torch.Tensor, plan: SitePlan, n_closings: int, cs_dilation: int, out: torch.Tensor, ws: torch.Tensor):
    """The sd_cs_close_dilate launches of a plan (asynchronous on the current stream; `ws` >= plan.ws_bytes bytes)."""
    X, Y, Z = plan.shape
    if not plan.batches:
        D.call('sd_cs_close_dilate', c0.device, c0, X, Y, Z, None, 0, 0, n_closings, cs_dilation, L.SD_CS_FIRST | L.SD_CS_LAST, out, None, 0)
        return out
    for b, (tab_d, n_obj, tot) in enumerate(plan.batches):
        flags = (L.SD_CS_FIRST if b == 0 else 0) | (L.SD_CS_LAST if b == len(plan.batches) - 1 else 0)
        D.call('sd_cs_close_dilate', c0.device, c0, X, Y, Z, tab_d, n_obj, tot, n_closings, cs_dilation, flags, out, ws, ws.numel())
    return out


def close_and_dilate_cs(contacts, n_closings: int, cs_dilation: int, return_device: bool = False, device=None,
                        ws_budget: int = WS_BUDGET):
    """cs_extraction_steps.py:437-461 on a uint64 contact volume (x, y, z): every site `ix` is closed `n_closings` times and
    dilated `cs_dilation` times (6-connected cross, border 0) inside its box, and the background voxels of the input inside the
    result take `ix` -- the smallest claiming id where sites compete.  Returns a new uint64 volume (``return_device``: an int64
    device tensor with the uint64 bits).  The id 2^64 - 1 is reserved and raises ValueError (packed cell pairs never take it)."""
    n_closings, cs_dilation = int(n_closings), int(cs_dilation)
    if n_closings < 0 or cs_dilation < 0:
        raise ValueError('n_closings and cs_dilation must be >= 0')
    dev = D.device(device)
    c0 = _u64_volume(contacts, dev)
    plan = plan_sites(c0, n_closings, dev, ws_budget)
    out = torch.empty_like(c0)
    ws = D.empty(plan.ws_bytes, D.u8, dev)
    run_sites(c0, plan, n_closings, cs_dilation, out, ws)
    return out if return_device else out.cpu().numpy().view(np.uint64)


# ---- sj / syn-type masks and the per-chunk worker (cs_extraction_steps.py:317-495) ---------------------------------------------
def binary_morphology(mask, morph_ops, structure, threshold: float = 0.0, return_device: bool = False, device=None):
    """``apply_morphological_operations(mask, morph_ops, mop_kwargs=dict(structure=structure))`` (image.py:358-438, 485-519) on the
    0/1 mask ``mask > threshold`` of a uint8 (x, y, z) volume: runs of equal operations are merged, each run acts inside the
    bounding box of the current foreground (zero pad for closing / dilation), an empty mask stays empty.  -> uint8 0/1 volume."""
    from .object_extraction_steps import _MOPS, _count_subsequent_mops
    dev = D.device(device)
    t = torch.from_numpy(np.ascontiguousarray(mask)) if isinstance(mask, np.ndarray) else mask
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype != torch.uint8 or t.dim() != 3:
        raise TypeError('binary_morphology: expected a 3D uint8 (x, y, z) volume')
    t = t.to(dev).contiguous()
    ops = list(morph_ops)
    for m in ops:
        if m not in _MOPS:
            raise NotImplementedError(f"Only erosion or dilation allowed. Attempted to use morphological operation '{m}'.")
    names, counts = _count_subsequent_mops(ops) if ops else ([], [])
    st = np.ascontiguousarray(np.asarray(structure)).astype(np.uint8)
    X, Y, Z = (int(s) for s in t.shape)
    pmax = max([c for n, c in zip(names, counts) if n in ('binary_closing', 'binary_dilation')], default=0)
    ws = D.scratch('sd_objseg_workspace_bytes', dev, X, Y, Z, pmax)
    out = torch.empty((X, Y, Z), dtype=torch.uint8, device=dev)
    n = len(names)
    ops_a = (C.c_int32 * max(n, 1))(*[_MOPS[m] for m in names])
    it_a = (C.c_int32 * max(n, 1))(*counts)
    D.call('sd_binary_morphology', dev, t, X, Y, Z, float(threshold), ops_a, it_a, n, st.ctypes.data_as(C.c_void_p),
           *[int(s) for s in st.shape], out, ws, ws.numel())
    return out if return_device else out.cpu().numpy()


def syntype_masks(vol, label_a=None, label_b=None, device=None):
    """The syn-type masks of the worker (:411-430) from one loaded (x, y, z) volume, as uint8 device tensors: uint8 raw data ->
    ``vol >= 123``; uint64 labels -> ``(vol == label_a, vol == label_b)`` (the second only when `label_b` is given)."""
    dev = D.device(device)
    t = torch.from_numpy(np.ascontiguousarray(vol)) if isinstance(vol, np.ndarray) else vol
    if t.dtype == torch.uint8:
        dtype = L.SD_U8
    elif t.dtype in (torch.uint64, torch.int64):
        dtype, t = L.SD_U64, t.view(torch.int64)
        if label_a is None:
            raise ValueError('syntype_masks: label volumes need a label')
    else:
        raise TypeError(f'syntype_masks: expected uint8 raw data or uint64 labels, got {t.dtype}')
    t = t.to(dev).contiguous()
    a = torch.empty(t.shape, dtype=torch.uint8, device=dev)
    b = torch.empty(t.shape, dtype=torch.uint8, device=dev) if (dtype == L.SD_U64 and label_b is not None) else None
    lab = lambda v: int(np.uint64(0 if v is None else int(v) % 2 ** 64))
    D.call('sd_syntype_masks', dev, t, dtype, t.numel(), lab(label_a), lab(label_b), a, b)
    return (a, b) if b is not None else a


def _upload_xyz(arr_zyx: np.ndarray, dev) -> torch.Tensor:
    """A (z, y, x) array as KnossosDataset loads it -> contiguous (x, y, z) device tensor (the reference's ``.swapaxes(0, 2)``)."""
    return D.up(arr_zyx, dev).permute(2, 1, 0).contiguous()


def _check_worker_config(cfg):
    """The refusals of the worker, before any data is touched: identical sym / asym sources (:348-354) and a stencil without
    overlap (the reference's ``[overlap:-overlap]`` slices would be empty)."""
    if cfg.syntype_available and (cfg.sym_label == cfg.asym_label) and (cfg.kd_sym_path == cfg.kd_asym_path):
        raise ValueError('Both KnossosDatasets and labels for symmetric and '
                         'asymmetric synapses are identical. Either one '
                         'must differ.')
    cs_filtersize = np.array(cfg['cell_objects']['cs_filtersize'])
    overlap = int(max(cs_filtersize // 2))
    if overlap == 0:
        raise ValueError(f'cs_filtersize {cs_filtersize.tolist()}: max(cs_filtersize) // 2 == 0 leaves no overlap, and the '
                         f"worker's [overlap:-overlap] crops would be empty")
    return cs_filtersize, overlap


class _ChunkExtractor:
    """Steps 1-5 of the worker body (:374-480) for one chunk at a time: loads, partner stencil, closing + dilation, sj and syn-type
    masks, and the statistics pass over the chunk core.  Everything between the loads and the result stays on the device.  Shared
    by ``_contact_site_extraction_thread`` and ``extract_contact_sites``."""

    def __init__(self, knossos_path, transf_func_sj_seg=None, device=None):
        from .. import global_params
        from ..handler import basics
        from .find_object_properties import CsSyntypeScan
        from .object_extraction_steps import get_aniso_struct
        cfg = self.cfg = global_params.config
        self.transf_func_sj_seg = transf_func_sj_seg
        morph_ops = cfg['cell_objects']['extract_morph_op']
        self.struct = get_aniso_struct(np.array(cfg['scaling']))
        self.cs_filtersize, self.overlap = _check_worker_config(cfg)
        self.syntype = cfg.syntype_available
        self.sym_label, self.asym_label = cfg.sym_label, cfg.asym_label
        self.same_kd = self.syntype and cfg.kd_asym_path == cfg.kd_sym_path
        if self.same_kd:
            assert self.asym_label is not None, 'Label of asymmetric synapses is not set.'
            assert self.sym_label is not None, 'Label of symmetric synapses is not set.'
        self.kd_sj = basics.kd_factory(cfg.kd_sj_path)
        self.kd_sym = basics.kd_factory(cfg.kd_sym_path) if self.syntype else None
        self.kd_asym = basics.kd_factory(cfg.kd_asym_path) if self.syntype else None
        self.kd = basics.kd_factory(knossos_path)
        self.cs_dilation = int(cfg['cell_objects']['cs_dilation'])
        self.stencil_offset = self.cs_filtersize // 2
        self.sj_ops = list(morph_ops['sj']) if 'sj' in morph_ops else []
        self.dev = D.device(device)
        self.scan = CsSyntypeScan(self.dev)

    def run(self, chunk):
        """-> (``CsSyntype`` of the chunk core with both core volumes, the core's (x, y, z) origin in the dataset)."""
        from .find_object_properties import detect_cs
        cfg, dev, overlap, stencil_offset = self.cfg, self.dev, self.overlap, self.stencil_offset
        kd, kd_sj, kd_sym, kd_asym = self.kd, self.kd_sj, self.kd_sym, self.kd_asym
        offset = np.array(chunk.coordinates - overlap)
        size = 2 * overlap + np.array(chunk.size)
        # 1. cell segmentation with the stencil's halo, truncated to uint32 (:374-376)
        seg64 = _upload_xyz(kd.load_seg(size=size + 2 * stencil_offset, offset=offset - stencil_offset, mag=1), dev)
        seg = (seg64 & 0xFFFFFFFF).to(torch.int32)
        del seg64
        # 2. partner stencil (valid convolution: `contacts` has the shape `size`), 3. closing + dilation of every site (:437-461)
        c0 = detect_cs(seg, stencil=self.cs_filtersize, return_device=True, device=dev)
        del seg
        plan = plan_sites(c0, overlap, dev)
        contacts = torch.empty_like(c0)
        ws = D.empty(plan.ws_bytes, D.u8, dev)
        run_sites(c0, plan, overlap, self.cs_dilation, contacts, ws)
        del c0, ws
        # 4. sj mask (:392-408) and syn-type masks (:411-433)
        if self.transf_func_sj_seg is None:
            sj_in = _upload_xyz(kd_sj.load_raw(size=size, offset=offset, mag=1), dev)
            thr = 255 * cfg['cell_objects']['probathresholds']['sj']
            sj_d = binary_morphology(sj_in, self.sj_ops, self.struct, threshold=thr, return_device=True, device=dev)
        else:
            sj_h = np.asarray(self.transf_func_sj_seg(kd_sj.load_seg(size=size, offset=offset, mag=1).swapaxes(0, 2))).astype('u1', copy=False)
            if self.sj_ops and np.any(sj_h > 1):
                raise ValueError('transf_func_sj_seg returned values other than 0 and 1 while sj morphology is configured: the '
                                 'reference would apply it per label; this build takes binary sj masks only (DESIGN.md section 7)')
            sj_d = D.up(sj_h, dev)
            if self.sj_ops:
                sj_d = binary_morphology(sj_d, self.sj_ops, self.struct, threshold=0, return_device=True, device=dev)
        if self.syntype:
            if not self.same_kd:
                def one(kd_t, label):
                    if label is None:
                        return syntype_masks(_upload_xyz(kd_t.load_raw(size=size, offset=offset, mag=1), dev), device=dev)
                    return syntype_masks(_upload_xyz(kd_t.load_seg(size=size, offset=offset, mag=1), dev), label, device=dev)
                sym_d, asym_d = one(kd_sym, self.sym_label), one(kd_asym, self.asym_label)
            else:
                asym_d, sym_d = syntype_masks(_upload_xyz(kd_sym.load_seg(size=size, offset=offset, mag=1), dev), self.asym_label,
                                              self.sym_label, device=dev)
        else:
            sym_d = torch.zeros_like(sj_d)
            asym_d = sym_d
        # 5. statistics, voxel lists and the two core volumes in one pass over the core (:464-480)
        core = tuple(int(s) - 2 * overlap for s in size)
        res = self.scan.run(contacts, sj_d, asym_d, sym_d, offset=offset + overlap, origin=(overlap,) * 3, extent=core, want_cores=True)
        return res, offset + overlap


def _contact_site_extraction_thread(args):
    """cs_extraction_steps.py:317-495: contact sites and synapses of the chunks `args[0]`.  `args` = (chunks, knossos_path of the
    cell segmentation, worker_nr, dir_props, transf_func_sj_seg).  Writes ``cs_props_{w}.pkl``, ``syn_props_{w}.pkl``,
    ``syn_voxels_{w}.npz``, ``tot_asym_cnt_{w}.pkl`` and ``tot_sym_cnt_{w}.pkl`` into ``{dir_props}/{w}/`` and the chunk cores
    into ``{wd}/knossosdatasets/cs_seg/`` and ``syn_seg/`` (initialised by the caller).  Per chunk everything between the loads
    and the two core volumes runs on the device (``_ChunkExtractor``); the host does the KnossosDataset I/O and the dict merges.
    Returns ``(worker_nr, dict(cs=[ids], syn=[ids]))``; dict keys are in ascending id order per chunk."""
    import os
    from collections import defaultdict
    from .. import global_params
    from ..handler import basics
    from ..proc.sd_proc import merge_prop_dicts
    from .find_object_properties import cs_syntype_dicts, merge_type_dicts, merge_voxel_dicts

    chunks, knossos_path, worker_nr, dir_props, transf_func_sj_seg = args[:5]
    worker_dir_props = f"{dir_props}/{worker_nr}/"
    os.makedirs(worker_dir_props, exist_ok=True)
    cfg = global_params.config
    body = _ChunkExtractor(knossos_path, transf_func_sj_seg)
    kd_cs = basics.kd_factory(f"{cfg.working_dir}/knossosdatasets/cs_seg/")
    kd_syn = basics.kd_factory(f"{cfg.working_dir}/knossosdatasets/syn_seg/")

    cs_props = [{}, defaultdict(list), {}]
    syn_props = [{}, defaultdict(list), {}]
    syn_voxels = {}
    tot_sym_cnt = {}
    tot_asym_cnt = {}
    for chunk in chunks:
        res, core_offset = body.run(chunk)
        # 6. to the host: the two cores (z, y, x) and the compact site arrays
        cs_core = res.cs_core.permute(2, 1, 0).contiguous().cpu().numpy().view(np.uint64)
        syn_core = res.syn_core.permute(2, 1, 0).contiguous().cpu().numpy().view(np.uint64)
        curr_cs_p, curr_syn_p, asym_cnt, sym_cnt, curr_syn_vx = cs_syntype_dicts(*res.host())
        del res
        kd_cs.save_seg(offset=core_offset, mags=[1, ], data=cs_core, data_mag=1)
        kd_syn.save_seg(offset=core_offset, mags=[1, ], data=syn_core, data_mag=1)
        merge_prop_dicts([cs_props, curr_cs_p], offset=core_offset)
        merge_prop_dicts([syn_props, curr_syn_p], offset=core_offset)
        merge_voxel_dicts([syn_voxels, curr_syn_vx], key_to_str=True)
        merge_type_dicts([tot_asym_cnt, asym_cnt])
        merge_type_dicts([tot_sym_cnt, sym_cnt])
        del curr_cs_p, curr_syn_p, asym_cnt, sym_cnt
    basics.write_obj2pkl(f'{worker_dir_props}/cs_props_{worker_nr}.pkl', cs_props)
    basics.write_obj2pkl(f'{worker_dir_props}/syn_props_{worker_nr}.pkl', syn_props)
    np.savez(f'{worker_dir_props}/syn_voxels_{worker_nr}.npz', **syn_voxels)
    basics.write_obj2pkl(f'{worker_dir_props}/tot_asym_cnt_{worker_nr}.pkl', tot_asym_cnt)
    basics.write_obj2pkl(f'{worker_dir_props}/tot_sym_cnt_{worker_nr}.pkl', tot_sym_cnt)
    return worker_nr, dict(cs=list(cs_props[0].keys()), syn=list(syn_props[0].keys()))


# ---- the dataset driver (cs_extraction_steps.py:44-314) and the merging half of its second step (:498-673) --------------------
def storage_keys(ids, n_folders_fs: int):
    """The storage bucket of every id as ``rep_helper.subfold_from_ix_new(ix, n_folders_fs)`` names it (rep_helper.py:143-163).
    The reference divides by the float ``1e3``: the bucket is ``int(ix // 1e3 % n_folders)`` in float64 arithmetic, which for
    contact-site ids (packed uint32 pairs, mostly > 2^53) differs from the integer result and is reproduced as such."""
    assert n_folders_fs % 10 == 0
    order = int(np.log10(n_folders_fs))
    ix = (np.asarray(ids, dtype=np.uint64).astype(np.float64) // 1e3 % n_folders_fs).astype(np.int64)
    out = []
    for v in ix.tolist():
        id_str = '{num:0{w}d}'.format(num=v, w=order)
        out.append('/' + ''.join('%s/' % id_str[i:i + 2] for i in range(0, order, 2)))
    return out


class CsTable:
    """Merged contact sites that passed ``min_obj_vx['cs']`` (plain numpy): ``ids`` ascending (uint64), ``sizes`` (int64),
    ``rep_coords`` (n, 3) int32 = the last chunk's, ``bounding_boxes`` (n, 2, 3) int32 = the union box, ``boxes`` (m, 2, 3) int32 =
    every (chunk, id) box in id-major / chunk-minor order, ``box_begin`` (n + 1) offsets into ``boxes``."""

    def __init__(self, ids, sizes, rep_coords, bounding_boxes, boxes, box_begin):
        self.ids, self.sizes, self.rep_coords, self.bounding_boxes = ids, sizes, rep_coords, bounding_boxes
        self.boxes, self.box_begin = boxes, box_begin

    def __len__(self):
        return len(self.ids)

    def storage_keys(self, n_folders_fs: int):
        return storage_keys(self.ids, n_folders_fs)

    def as_dict(self) -> dict:
        """id -> what ``_write_props_to_syn_thread`` stores for a ``cs`` object (:581-590): ``rep_coord`` (int32), ``bounding_box``,
        ``size`` and ``boxes``, the (k, 2, 3) box list it hands to ``VoxelStorageDyn``."""
        b = self.box_begin.tolist()
        return {k: dict(rep_coord=self.rep_coords[i], bounding_box=self.bounding_boxes[i], size=s, boxes=self.boxes[b[i]:b[i + 1]])
                for i, (k, s) in enumerate(zip(self.ids.tolist(), self.sizes.tolist()))}


class SynTable(CsTable):
    """Merged synapses whose cs object was kept and that passed ``min_obj_vx['syn']``: the columns of ``CsTable`` and ``asym`` /
    ``sym`` (summed voxel counts), ``asym_prop`` / ``sym_prop`` (count / size, float64), ``cs_size``, ``voxels`` (v, 3) uint32 = the
    voxel lists of all ids (id-major, chunks in chunk order, scan order inside a chunk), ``vox_begin`` (n + 1) offsets into it."""

    def __init__(self, ids, sizes, rep_coords, bounding_boxes, boxes, box_begin, asym, sym, cs_size, voxels, vox_begin):
        super().__init__(ids, sizes, rep_coords, bounding_boxes, boxes, box_begin)
        self.asym, self.sym, self.cs_size, self.voxels, self.vox_begin = asym, sym, cs_size, voxels, vox_begin
        # Python's int / int is the correctly rounded quotient; so is float64 division of two exactly represented integers
        self.asym_prop = asym / sizes if len(ids) else np.zeros(0, np.float64)
        self.sym_prop = sym / sizes if len(ids) else np.zeros(0, np.float64)

    def as_dict(self) -> dict:
        """id -> what ``_write_props_to_syn_thread`` stores for a ``syn`` object (:595-622): the entries of a cs object (boxes as
        int64, the reference concatenates lists there), ``sym_prop``, ``asym_prop``, ``cs_id``, ``cs_size`` and ``voxels``
        (uint32, the voxel cache)."""
        b, v = self.box_begin.tolist(), self.vox_begin.tolist()
        bb64, boxes64 = self.bounding_boxes.astype(np.int64), self.boxes.astype(np.int64)
        rows = zip(self.ids.tolist(), self.sizes.tolist(), self.sym_prop.tolist(), self.asym_prop.tolist(), self.cs_size.tolist())
        return {k: dict(rep_coord=self.rep_coords[i], bounding_box=bb64[i], size=s, boxes=boxes64[b[i]:b[i + 1]], sym_prop=sp,
                        asym_prop=ap, cs_id=k, cs_size=cz, voxels=self.voxels[v[i]:v[i + 1]])
                for i, (k, s, sp, ap, cz) in enumerate(rows)}


class ContactSiteMerger:
    """The counterpart of ``proc.sd_proc.ChunkMerger`` for contact sites: the records of every chunk (``CsSyntype``, device) are
    appended to growable device arrays by ``sd_cs_merge_append`` and merged once per dataset by ``sd_cs_merge_objects`` /
    ``sd_cs_merge_synapses``.  The scan that produces a chunk's result has told the host its site and voxel counts already, so the
    arrays are sized from them and ``add_chunk`` neither waits for the device nor copies anything to the host."""

    def __init__(self, min_obj_vx: dict, device, capacity: int = 1 << 14, vox_capacity: int = 1 << 18):
        self.device = torch.device(device)
        self.min_cs, self.min_syn = int(min_obj_vx['cs']), int(min_obj_vx['syn'])
        syn = OBJECT_FIELDS + [('asym', 'int64', 1), ('sym', 'int64', 1), ('vpos', 'int64', 1)]
        self.cursors = D.counters(self.device, 3)
        self.cs = Records(self.device, OBJECT_FIELDS, capacity, self.cursors[0:1])
        self.syn = Records(self.device, syn, capacity, self.cursors[1:2])
        self.vox = Records(self.device, [('rows', 'int32', 3)], vox_capacity, self.cursors[2:3])
        self.n_cs = self.n_vox = 0          # appended so far (the syn records are at most n_cs)
        self.n_chunks = 0
        self.n_cs_all = self.n_syn_all = 0  # ids before the size filter (set by finish: the reference's log line counts these)

    def add_chunk(self, result, origin):
        """`result`: the ``CsSyntype`` of one chunk core whose (x, y, z) origin in the dataset is `origin` (its voxel rows carry
        the origin already, its records do not)."""
        n, n_vox = int(result.rec.shape[0]), int(result.voxels.shape[0])
        self.cs.room_for(self.n_cs, n)
        self.syn.room_for(self.n_cs, n)
        self.vox.room_for(self.n_vox, n_vox)
        ox, oy, oz = (int(v) for v in origin)
        D.call('sd_cs_merge_append', self.device, result.rec if n else None, n, result.voxels if n_vox else None, n_vox, ox, oy, oz,
               *self.cs.ptrs(), self.cs.capacity, *self.syn.ptrs(), self.syn.capacity, *self.vox.ptrs(), self.vox.capacity, self.cursors)
        self.n_cs += n
        self.n_vox += n_vox
        self.n_chunks += 1

    def finish(self):
        """-> (``CsTable``, ``SynTable``).  One merge of each kind on the device, then the download of the compacted tables."""
        dev = self.device
        n_cs, n_syn, n_vox = (int(v) for v in D.down(self.cursors))
        if n_cs > self.cs.capacity or n_syn > self.syn.capacity or n_vox > self.vox.capacity:
            raise RuntimeError(f'sd_cs_merge_append: record arrays overran ({n_cs}/{self.cs.capacity} cs, {n_syn}/{self.syn.capacity} '
                               f'syn, {n_vox}/{self.vox.capacity} voxel rows)')
        tmp = D.scratch('sd_cs_merge_temp_bytes', dev, max(n_cs, n_syn, 1))

        def common(n):
            return [D.empty(n, D.i64, dev), D.empty(n, D.i64, dev), D.empty((n, 3), D.i32, dev), D.empty((n, 6), D.i32, dev),
                    D.empty(n, D.i32, dev), D.empty((n, 6), D.i32, dev)]
        c_out, c_cnt = common(n_cs), D.counters(dev, 4)
        a = self.cs.arrays
        D.call('sd_cs_merge_objects', dev, a['ids'], a['sizes'], a['rc'], a['bb'], n_cs, self.min_cs, *c_out, c_cnt, tmp, tmp.numel())
        u_cs, b_cs, _, self.n_cs_all = (int(v) for v in D.down(c_cnt))
        s_out, s_cnt = common(n_syn), D.counters(dev, 4)
        s_more = [D.empty(n_syn, D.i64, dev), D.empty(n_syn, D.i64, dev), D.empty(n_syn, D.i64, dev), D.empty(n_syn, D.i32, dev),
                  D.empty((n_vox, 3), D.i32, dev)]
        a = self.syn.arrays
        D.call('sd_cs_merge_synapses', dev, *[a[k] for k in ('ids', 'sizes', 'rc', 'bb', 'asym', 'sym', 'vpos')], n_syn, self.vox.arrays['rows'],
               n_vox, c_out[0], c_out[1], u_cs, self.min_syn, *s_out, *s_more, s_cnt, tmp, tmp.numel())
        u_syn, b_syn, v_syn, self.n_syn_all = (int(v) for v in D.down(s_cnt))

        def table(out, u, b):
            ids, tot, rc, ubox, beg, boxes = out
            return [D.down(ids, u, np.uint64), D.down(tot, u), D.down(rc, u), D.down(ubox, u).reshape(u, 2, 3),
                    D.down(boxes, b).reshape(b, 2, 3), segment_offsets(beg, u, b)]
        cs_t = CsTable(*table(c_out, u_cs, b_cs))
        asym, sym, cs_size, vbeg, vout = s_more
        syn_t = SynTable(*table(s_out, u_syn, b_syn), D.down(asym, u_syn), D.down(sym, u_syn), D.down(cs_size, u_syn),
                         D.down(vout, v_syn, np.uint32), segment_offsets(vbeg, u_syn, v_syn))
        return cs_t, syn_t


class _CoreWriter:
    """Takes the two core volumes of a chunk off the device on a side stream into page-locked buffers (two sets, guarded by
    events) and writes them into the cs_seg / syn_seg KnossosDatasets on a writer thread, while the device works on the next
    chunk -- as ``parallel.py`` does for its strips."""

    def __init__(self, device, kd_cs, kd_syn):
        import queue
        import threading
        self.device, self.kd_cs, self.kd_syn = device, kd_cs, kd_syn
        self.side = torch.cuda.Stream(device=device)
        self.bufs = [None, None]
        self.free = [threading.Event(), threading.Event()]
        for e in self.free:
            e.set()
        self.jobs = queue.Queue()
        self.error = None
        self.k = 0
        self.busy_s = 0.0                 # time the writer thread spent in save_seg (for the probe)
        self.thread = threading.Thread(target=self._work, daemon=True)
        self.thread.start()

    def _work(self):
        import time
        while True:
            job = self.jobs.get()
            if job is None:
                return
            slot, done, offset, shape = job
            try:
                if self.error is None:
                    done.synchronize()
                    t0 = time.perf_counter()
                    n = int(np.prod(shape))
                    for kd, buf in zip((self.kd_cs, self.kd_syn), self.bufs[slot]):
                        kd.save_seg(offset=offset, mags=[1, ], data=buf.numpy()[:n].view(np.uint64).reshape(shape), data_mag=1)
                    self.busy_s += time.perf_counter() - t0
            except BaseException as e:          # re-raised by close()
                self.error = e
            finally:
                self.free[slot].set()

    def submit(self, result, offset):
        """Queue the cores of `result` ((x, y, z) device tensors) for ``save_seg(offset=offset)`` as (z, y, x) volumes."""
        slot = self.k % 2
        self.k += 1
        self.free[slot].wait()
        if self.error is not None:
            self.close()
        self.free[slot].clear()
        zyx = [t.permute(2, 1, 0).contiguous() for t in (result.cs_core, result.syn_core)]
        n = zyx[0].numel()
        if self.bufs[slot] is None or self.bufs[slot][0].numel() < n:
            self.bufs[slot] = [torch.empty(n, dtype=torch.int64).pin_memory() for _ in range(2)]
        ready = torch.cuda.current_stream(self.device).record_event()
        with torch.cuda.stream(self.side):
            self.side.wait_event(ready)
            for buf, t in zip(self.bufs[slot], zyx):
                buf[:n].copy_(t.reshape(-1), non_blocking=True)
                t.record_stream(self.side)
            done = torch.cuda.Event()
            done.record(self.side)
        self.jobs.put((slot, done, np.asarray(offset), tuple(zyx[0].shape)))

    def close(self):
        self.jobs.put(None)
        self.thread.join()
        if self.error is not None:
            raise self.error


def job_major_order(chunk_list, max_n_jobs: int):
    """The order in which the reference's two-level merge sees the chunks: dealt to jobs round-robin (``chunkify``), merged inside a
    job in chunk order and across jobs in job order."""
    from ..handler.basics import chunkify
    return [c for job in chunkify(list(chunk_list), max_n_jobs) for c in job]


def extract_contact_sites(chunk_size=None, log=None, max_n_jobs=None, cube_of_interest_bb=None, n_folders_fs: int = 1000,
                          cube_shape=None, overwrite: bool = False, transf_func_sj_seg=None, *, as_tables: bool = False, device=None):
    """cs_extraction_steps.py:44-314 with the merging half of its second step (:498-673): contact sites and synapses of the cell
    segmentation ``config.kd_seg_path`` over a regular chunk grid.  Writes the ``cs_seg`` / ``syn_seg`` KnossosDatasets under
    ``{wd}/knossosdatasets/`` and returns ``(cs, syn)``: per id what ``_write_props_to_syn_thread`` puts into its storages
    (``CsTable.as_dict`` / ``SynTable.as_dict``), or the tables themselves with ``as_tables=True``.

    The chunks run on one device in the job-major order of the reference's in-process mode (``job_major_order``), their records
    stay on the device (``ContactSiteMerger``) and are merged once; no worker files are written.  Not built:
    the ``AttributeDict`` / ``VoxelStorageDyn`` storages and ``storage_targets_cs.pkl`` (``storage_keys`` names every id's bucket),
    ``dataset_analysis``, the batch-job dispatch and multi-GPU distribution.  `n_folders_fs` is accepted for the signature."""
    import logging
    import os
    import shutil
    from .. import global_params
    from ..handler import basics
    from ..knossos import ChunkDataset, KnossosDataset
    from .object_extraction_wrapper import calculate_chunk_numbers_for_box
    cfg = global_params.config
    kd = basics.kd_factory(cfg.kd_seg_path)
    if cube_of_interest_bb is None:
        cube_of_interest_bb = [np.zeros(3, dtype=np.int32), kd.boundary]
    if cube_shape is None:
        cube_shape = (256, 256, 256)
    if chunk_size is None:
        chunk_size = (512, 512, 512)
    if np.any(np.array(chunk_size) % np.array(cube_shape)):
        raise ValueError('Chunk size must be divisible by cube shape.')
    if max_n_jobs is None:
        max_n_jobs = cfg.ncore_total * 8
    size = np.asarray(cube_of_interest_bb[1]) - np.asarray(cube_of_interest_bb[0]) + 1
    offset = np.asarray(cube_of_interest_bb[0])
    _check_worker_config(cfg)
    wd = cfg.working_dir
    sd_paths = [f'{wd}/syn_0', f'{wd}/cs_0']            # SegmentationDataset(obj_type, version=0).path
    if any(os.path.exists(p) for p in sd_paths):
        if not overwrite:
            raise FileExistsError('Overwrite was set to False, but SegmentationDataset "syn" or "cs" already exists.')
        for p in sd_paths:
            shutil.rmtree(p, ignore_errors=True)
    cset = ChunkDataset()
    cset.initialize(kd, kd.boundary, chunk_size, cfg.temp_path + '/chunkdatasets/cs/', box_coords=[0, 0, 0], fit_box_size=True)
    if log is None:
        log = logging.getLogger('syconn_amd.extraction')
    chunk_list, _ = calculate_chunk_numbers_for_box(cset, offset, size)
    kds = []
    for ot in ['cs', 'syn']:
        path_kd = f'{wd}/knossosdatasets/{ot}_seg/'
        if os.path.isdir(path_kd):
            log.debug('Found existing KD at {}. Removing it now.'.format(path_kd))
            shutil.rmtree(path_kd)
        target_kd = KnossosDataset()
        target_kd._cube_shape = tuple(int(c) for c in cube_shape)
        scale = np.array(cfg['scaling'])
        target_kd.initialize_without_conf(path_kd, kd.boundary, scale, kd.experiment_name, mags=[1, ], create_pyk_conf=True,
                                          create_knossos_conf=False)
        kds.append(target_kd)
    order = job_major_order(chunk_list, max_n_jobs)
    body = _ChunkExtractor(cfg.kd_seg_path, transf_func_sj_seg, device)
    with torch.cuda.device(body.dev):
        merger = ContactSiteMerger(cfg['cell_objects']['min_obj_vx'], body.dev)
        writer = _CoreWriter(body.dev, *kds)
        try:
            for k in order:
                res, core_offset = body.run(cset.chunk_dict[k])
                merger.add_chunk(res, core_offset)
                writer.submit(res, core_offset)
                del res
        finally:
            writer.close()
        cs_t, syn_t = merger.finish()
    log.info(f'Finished extraction of initial contact sites (#objects: {merger.n_cs_all}) and synapses'
             f' (#objects: {merger.n_syn_all}).')
    if merger.n_syn_all == 0:
        log.critical('WARNING: Did not find any synapses during extraction step.')
    if as_tables:
        return cs_t, syn_t
    return cs_t.as_dict(), syn_t.as_dict()
