"""Drop-in for ``syconn.handler.multiviews.generate_rendering_locs`` (handler/multiviews.py:339-355) on the device.  The reference calls
open3d's ``PointCloud.voxel_down_sample``; this is that algorithm as open3d publishes it (tests/_locations_ref.py),
with the locations in ascending order of their voxel instead of the order of open3d's hash map.  No CPU fallback."""
import numpy as np


def generate_rendering_locs(verts: np.ndarray, ds_factor: float, device=None) -> np.ndarray:
    """One location per occupied voxel of edge `ds_factor` (the mean of its vertices): float64 (N, 3).  `verts` (n, 3) of any real
    dtype; float32 is read as it is, everything else as float64.  ``ValueError`` for ``ds_factor <= 0``, a vertex that is NaN or
    infinite, and an extent of more voxels per axis than ``SD_LOCATIONS_MAX_CELLS``."""
    from ..proc.locations import check_ds, check_finite, one_object
    ds = check_ds('generate_rendering_locs', ds_factor)
    v = np.asarray(verts)
    if v.dtype != np.float32:
        v = v.astype(np.float64)
    v = v.reshape(-1, 3)
    check_finite('generate_rendering_locs', v)
    from .. import _dev as D
    dev = D.device(device)
    if len(v) == 0:
        return np.zeros((0, 3), np.float64)
    return one_object('generate_rendering_locs', v, dev, ds=ds)
