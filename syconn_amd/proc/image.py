"""``single_conn_comp_img`` of the reference (proc/image.py:125-144) over ``sd_views_center_component``: the connected component at the
centre of a view, for one image or -- ``center_component_planes`` -- for a batch of planes that stays on the device.  No CPU fallback."""
import numpy as np


def _background_u8(who, background) -> int:
    if isinstance(background, bool) or not np.isscalar(background) or not np.isfinite(background) or int(background) != background \
            or not 0 <= int(background) <= 255:
        raise ValueError(f'{who}: background must be an integer in [0, 255], got {background!r}')
    return int(background)


def center_component_planes(planes, background=1, out=None):
    """`planes`: uint8 device tensor (..., H, W), contiguous.  -> the same shape with, per plane, everything but the 4-connected
    component of ``pixel != background`` that holds the centre pixel ``(H // 2, W // 2)`` set to `background`.  ``out=planes`` filters in
    place.  A plane whose two bit masks do not fit the LDS of one workgroup is a ``ValueError`` before anything is launched."""
    import torch
    from .. import _dev as D
    who = 'center_component_planes'
    bg = _background_u8(who, background)
    if not isinstance(planes, torch.Tensor) or not planes.is_cuda or planes.dtype != torch.uint8 or planes.dim() < 2 or not planes.is_contiguous():
        raise ValueError(f'{who}: planes must be a contiguous uint8 device tensor (..., H, W)')
    if out is None:
        out = torch.empty_like(planes)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != planes.device or out.shape != planes.shape or not out.is_contiguous():
        raise ValueError(f'{who}: out must be a contiguous uint8 tensor of the shape and device of planes')
    H, W = int(planes.shape[-2]), int(planes.shape[-1])
    if H < 1 or W < 1:
        raise ValueError(f'{who}: empty planes')
    n = planes.numel() // (H * W)
    with torch.cuda.device(planes.device):
        D.call('sd_views_center_component', planes.device, planes if n else None, n, H, W, bg, out if n else None)
    return out


def single_conn_comp_img(img, background=1.0, device=None):
    """Drop-in of ``single_conn_comp_img`` (proc/image.py:125-144): the connected component of ``img != background`` at the centre of one
    image of any shape that squeezes to 2-D; everything else becomes `background`.  4-connectivity (``scipy.ndimage.label``'s default);
    the centre is the integer ``(H // 2, W // 2)`` -- the reference indexes with ``np.array(shape) / 2``, a float index that the numpy
    of its time truncated and current numpy refuses --; a background centre empties the image (the reference's ``labeled == 0``
    branch).  `img` is uint8, or float32 that is exactly uint8-valued (returned as float32); anything else raises
    ``NotImplementedError``.  `background` defaults to 1 as in the reference: a leftover of float views in [0, 1] -- the renderer's
    background is 255, and ``predict_views`` passes its own."""
    import torch
    from .. import _dev as D
    img = np.asarray(img)
    orig_shape = img.shape
    sq = np.squeeze(img)
    if sq.ndim != 2:
        raise ValueError(f'single_conn_comp_img: the image must squeeze to 2-D, got shape {orig_shape}')
    bg = _background_u8('single_conn_comp_img', background)
    if sq.dtype == np.uint8:
        u8 = sq
    elif sq.dtype == np.float32:
        u8 = sq.astype(np.uint8) if np.isfinite(sq).all() and sq.min(initial=0) >= 0 and sq.max(initial=0) <= 255 else None
        if u8 is None or not np.array_equal(u8.astype(np.float32), sq):
            raise NotImplementedError('single_conn_comp_img: float32 images must hold uint8 values exactly')
    else:
        raise NotImplementedError(f'single_conn_comp_img: images must be uint8 or uint8-valued float32, got {sq.dtype}')
    dev = D.device(device)
    res = center_component_planes(D.up(u8, dev), bg).cpu().numpy()
    return res.astype(img.dtype, copy=False).reshape(orig_shape)
