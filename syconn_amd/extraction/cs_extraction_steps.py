"""Contact-site extraction on the MI355X: the device form of the per-chunk steps of
/root/reference/syconn/extraction/cs_extraction_steps.py (``_contact_site_extraction_thread``, :317-495).

Here: the partner search (``find_object_properties.detect_cs``) and the closing + dilation of every contact site inside its own
box (:437-461, ``close_and_dilate_cs``).  Where several sites claim one background voxel the smallest id wins.
There is no CPU fallback.
"""
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
