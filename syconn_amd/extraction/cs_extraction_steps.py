"""Contact-site extraction on the MI355X: the device form of the per-chunk steps of
/root/reference/syconn/extraction/cs_extraction_steps.py (``_contact_site_extraction_thread``, :317-495).

Here: the partner search (``find_object_properties.detect_cs``) and the closing + dilation of every contact site inside its own
box (:437-461, ``close_and_dilate_cs``).  Where several sites claim one background voxel the smallest id wins.
There is no CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from .find_object_properties import _cs_device, segstats

# summed box volume (bytes per workspace plane) of one batch of sites; a single larger box gets a batch of its own
WS_BUDGET = 1 << 28


def _u64_volume(arr, device) -> torch.Tensor:
    if isinstance(arr, np.ndarray):
        if arr.dtype != np.uint64:
            raise TypeError(f'contact volumes must be uint64, got {arr.dtype}')
        t = torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to(device)
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
        batches.append((torch.from_numpy(tab).to(device), end - start, int(vol[start:end].sum())))
        start = end
    return SitePlan((X, Y, Z), ids, batches, 2 * max(tot for _, _, tot in batches))


def run_sites(c0: torch.Tensor, plan: SitePlan, n_closings: int, cs_dilation: int, out: torch.Tensor, ws: torch.Tensor):
    """The sd_cs_close_dilate launches of a plan (asynchronous on the current stream; `ws` >= plan.ws_bytes bytes)."""
    lib = L.load()
    X, Y, Z = plan.shape
    stream = torch.cuda.current_stream(c0.device).cuda_stream
    if not plan.batches:
        L.check(lib.sd_cs_close_dilate(c0.data_ptr(), X, Y, Z, None, 0, 0, n_closings, cs_dilation,
                                       L.SD_CS_FIRST | L.SD_CS_LAST, out.data_ptr(), None, 0, stream), 'sd_cs_close_dilate')
        return out
    for b, (tab_d, n_obj, tot) in enumerate(plan.batches):
        flags = (L.SD_CS_FIRST if b == 0 else 0) | (L.SD_CS_LAST if b == len(plan.batches) - 1 else 0)
        L.check(lib.sd_cs_close_dilate(c0.data_ptr(), X, Y, Z, tab_d.data_ptr(), n_obj, tot, n_closings, cs_dilation, flags,
                                       out.data_ptr(), ws.data_ptr(), ws.numel(), stream), 'sd_cs_close_dilate')
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
    dev = _cs_device(device)
    c0 = _u64_volume(contacts, dev)
    plan = plan_sites(c0, n_closings, dev, ws_budget)
    out = torch.empty_like(c0)
    ws = torch.empty(max(plan.ws_bytes, 1), dtype=torch.uint8, device=dev)
    run_sites(c0, plan, n_closings, cs_dilation, out, ws)
    return out if return_device else out.cpu().numpy().view(np.uint64)


# ---- sj / syn-type masks and the per-chunk worker (cs_extraction_steps.py:317-495) ---------------------------------------------
def binary_morphology(mask, morph_ops, structure, threshold: float = 0.0, return_device: bool = False, device=None):
    """``apply_morphological_operations(mask, morph_ops, mop_kwargs=dict(structure=structure))`` (image.py:358-438, 485-519) on the
    0/1 mask ``mask > threshold`` of a uint8 (x, y, z) volume: runs of equal operations are merged, each run acts inside the
    bounding box of the current foreground (zero pad for closing / dilation), an empty mask stays empty.  -> uint8 0/1 volume."""
    from .object_extraction_steps import _MOPS, _count_subsequent_mops
    lib = L.load()
    dev = _cs_device(device)
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
    ws_bytes = lib.sd_objseg_workspace_bytes(X, Y, Z, pmax)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty((X, Y, Z), dtype=torch.uint8, device=dev)
    n = len(names)
    ops_a = (C.c_int32 * max(n, 1))(*[_MOPS[m] for m in names])
    it_a = (C.c_int32 * max(n, 1))(*counts)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L.check(lib.sd_binary_morphology(t.data_ptr(), X, Y, Z, float(threshold), ops_a, it_a, n, st.ctypes.data_as(C.c_void_p),
                                     *[int(s) for s in st.shape], out.data_ptr(), ws.data_ptr(), ws_bytes, stream),
            'sd_binary_morphology')
    return out if return_device else out.cpu().numpy()


def syntype_masks(vol, label_a=None, label_b=None, device=None):
    """The syn-type masks of the worker (:411-430) from one loaded (x, y, z) volume, as uint8 device tensors: uint8 raw data ->
    ``vol >= 123``; uint64 labels -> ``(vol == label_a, vol == label_b)`` (the second only when `label_b` is given)."""
    lib = L.load()
    dev = _cs_device(device)
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
    stream = torch.cuda.current_stream(dev).cuda_stream
    lab = lambda v: int(np.uint64(0 if v is None else int(v) % 2 ** 64))
    L.check(lib.sd_syntype_masks(t.data_ptr(), dtype, t.numel(), lab(label_a), lab(label_b), a.data_ptr(),
                                 b.data_ptr() if b is not None else None, stream), 'sd_syntype_masks')
    return (a, b) if b is not None else a


def _upload_xyz(arr_zyx: np.ndarray, dev) -> torch.Tensor:
    """A (z, y, x) array as KnossosDataset loads it -> contiguous (x, y, z) device tensor (the reference's ``.swapaxes(0, 2)``)."""
    a = np.ascontiguousarray(arr_zyx)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(dev).permute(2, 1, 0).contiguous()


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


def _contact_site_extraction_thread(args):
    """cs_extraction_steps.py:317-495: contact sites and synapses of the chunks `args[0]`.  `args` = (chunks, knossos_path of the
    cell segmentation, worker_nr, dir_props, transf_func_sj_seg).  Writes ``cs_props_{w}.pkl``, ``syn_props_{w}.pkl``,
    ``syn_voxels_{w}.npz``, ``tot_asym_cnt_{w}.pkl`` and ``tot_sym_cnt_{w}.pkl`` into ``{dir_props}/{w}/`` and the chunk cores
    into ``{wd}/knossosdatasets/cs_seg/`` and ``syn_seg/`` (initialised by the caller).  Per chunk everything between the loads
    and the two core volumes runs on the device; the host does the KnossosDataset I/O and the dict merges.  Returns
    ``(worker_nr, dict(cs=[ids], syn=[ids]))``; dict keys are in ascending id order per chunk."""
    import os
    from collections import defaultdict
    from .. import global_params
    from ..handler import basics
    from ..proc.sd_proc import merge_prop_dicts
    from .find_object_properties import CsSyntypeScan, cs_syntype_dicts, detect_cs, merge_type_dicts, merge_voxel_dicts
    from .object_extraction_steps import get_aniso_struct

    chunks, knossos_path, worker_nr, dir_props, transf_func_sj_seg = args[:5]
    worker_dir_props = f"{dir_props}/{worker_nr}/"
    os.makedirs(worker_dir_props, exist_ok=True)
    cfg = global_params.config
    morph_ops = cfg['cell_objects']['extract_morph_op']
    scaling = np.array(cfg['scaling'])
    struct = get_aniso_struct(scaling)
    cs_filtersize, overlap = _check_worker_config(cfg)
    syntype = cfg.syntype_available
    sym_label, asym_label = cfg.sym_label, cfg.asym_label
    same_kd = syntype and cfg.kd_asym_path == cfg.kd_sym_path
    if same_kd:
        assert asym_label is not None, 'Label of asymmetric synapses is not set.'
        assert sym_label is not None, 'Label of symmetric synapses is not set.'

    kd_cs = basics.kd_factory(f"{cfg.working_dir}/knossosdatasets/cs_seg/")
    kd_syn = basics.kd_factory(f"{cfg.working_dir}/knossosdatasets/syn_seg/")
    kd_sj = basics.kd_factory(cfg.kd_sj_path)
    kd_sym = basics.kd_factory(cfg.kd_sym_path) if syntype else None
    kd_asym = basics.kd_factory(cfg.kd_asym_path) if syntype else None
    kd = basics.kd_factory(knossos_path)

    cs_props = [{}, defaultdict(list), {}]
    syn_props = [{}, defaultdict(list), {}]
    syn_voxels = {}
    tot_sym_cnt = {}
    tot_asym_cnt = {}
    cs_dilation = int(cfg['cell_objects']['cs_dilation'])
    stencil_offset = cs_filtersize // 2
    sj_ops = list(morph_ops['sj']) if 'sj' in morph_ops else []
    dev = _cs_device()
    scan = CsSyntypeScan(dev)
    for chunk in chunks:
        offset = np.array(chunk.coordinates - overlap)
        size = 2 * overlap + np.array(chunk.size)
        # 1. cell segmentation with the stencil's halo, truncated to uint32 (:374-376)
        seg64 = _upload_xyz(kd.load_seg(size=size + 2 * stencil_offset, offset=offset - stencil_offset, mag=1), dev)
        seg = (seg64 & 0xFFFFFFFF).to(torch.int32)
        del seg64
        # 2. partner stencil (valid convolution: `contacts` has the shape `size`), 3. closing + dilation of every site (:437-461)
        c0 = detect_cs(seg, stencil=cs_filtersize, return_device=True, device=dev)
        del seg
        plan = plan_sites(c0, overlap, dev)
        contacts = torch.empty_like(c0)
        ws = torch.empty(max(plan.ws_bytes, 1), dtype=torch.uint8, device=dev)
        run_sites(c0, plan, overlap, cs_dilation, contacts, ws)
        del c0, ws
        # 4. sj mask (:392-408) and syn-type masks (:411-433)
        if transf_func_sj_seg is None:
            sj_in = _upload_xyz(kd_sj.load_raw(size=size, offset=offset, mag=1), dev)
            thr = 255 * cfg['cell_objects']['probathresholds']['sj']
            sj_d = binary_morphology(sj_in, sj_ops, struct, threshold=thr, return_device=True, device=dev)
        else:
            sj_h = np.asarray(transf_func_sj_seg(kd_sj.load_seg(size=size, offset=offset, mag=1).swapaxes(0, 2))).astype('u1', copy=False)
            if sj_ops and np.any(sj_h > 1):
                raise ValueError('transf_func_sj_seg returned values other than 0 and 1 while sj morphology is configured: the '
                                 'reference would apply it per label; this build takes binary sj masks only (DESIGN.md section 7)')
            sj_d = torch.from_numpy(np.ascontiguousarray(sj_h)).to(dev)
            if sj_ops:
                sj_d = binary_morphology(sj_d, sj_ops, struct, threshold=0, return_device=True, device=dev)
        if syntype:
            if not same_kd:
                def one(kd_t, label):
                    if label is None:
                        return syntype_masks(_upload_xyz(kd_t.load_raw(size=size, offset=offset, mag=1), dev), device=dev)
                    return syntype_masks(_upload_xyz(kd_t.load_seg(size=size, offset=offset, mag=1), dev), label, device=dev)
                sym_d, asym_d = one(kd_sym, sym_label), one(kd_asym, asym_label)
            else:
                asym_d, sym_d = syntype_masks(_upload_xyz(kd_sym.load_seg(size=size, offset=offset, mag=1), dev), asym_label,
                                              sym_label, device=dev)
        else:
            sym_d = torch.zeros_like(sj_d)
            asym_d = sym_d
        # 5. statistics, voxel lists and the two core volumes in one pass over the core (:464-480)
        core = tuple(int(s) - 2 * overlap for s in size)
        res = scan.run(contacts, sj_d, asym_d, sym_d, offset=offset + overlap, origin=(overlap,) * 3, extent=core, want_cores=True)
        # 6. to the host: the two cores (z, y, x) and the compact site arrays
        cs_core = res.cs_core.permute(2, 1, 0).contiguous().cpu().numpy().view(np.uint64)
        syn_core = res.syn_core.permute(2, 1, 0).contiguous().cpu().numpy().view(np.uint64)
        curr_cs_p, curr_syn_p, asym_cnt, sym_cnt, curr_syn_vx = cs_syntype_dicts(*res.host())
        del contacts, sj_d, sym_d, asym_d, res
        kd_cs.save_seg(offset=offset + overlap, mags=[1, ], data=cs_core, data_mag=1)
        kd_syn.save_seg(offset=offset + overlap, mags=[1, ], data=syn_core, data_mag=1)
        merge_prop_dicts([cs_props, curr_cs_p], offset=offset + overlap)
        merge_prop_dicts([syn_props, curr_syn_p], offset=offset + overlap)
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
