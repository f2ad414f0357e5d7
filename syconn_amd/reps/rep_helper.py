"""Drop-in for ``syconn.reps.rep_helper.surface_samples`` (reps/rep_helper.py:376-417) on the device: the legacy rule of the rendering
locations (``views.use_new_renderings_locs: False``).  DESIGN.md section 7 states the rule; tests/golden/g28_locations.npz pins it to
the reference's own function.  No CPU fallback."""
from typing import Tuple

import numpy as np


def surface_samples(coords: np.ndarray, bin_sizes: Tuple[int, int, int] = (2000, 2000, 2000), max_nb_samples: int = 5000, r: int = 1000,
                    device=None) -> np.ndarray:
    """At the centre of every occupied histogram bin the nearest coordinate, and around it the mean of all coordinates within `r`:
    float32 (N, 3).  `coords` float32 (n, 3), n >= 1 (another dtype: ``NotImplementedError``).  `max_nb_samples` is accepted and has no
    effect, as in the reference, where the number of samples never exceeds it and the threshold branch is dead."""
    from ..proc.locations import check_finite, check_surface_args, one_object
    bs, r = check_surface_args('surface_samples', bin_sizes, r)
    v = np.asarray(coords)
    if v.dtype != np.float32:
        raise NotImplementedError(f'surface_samples: float32 coordinates only, got {v.dtype}')
    v = v.reshape(-1, 3)
    if len(v) == 0:
        raise ValueError('surface_samples: no coordinates')
    check_finite('surface_samples', v)
    from .. import _dev as D
    return one_object('surface_samples', v, D.device(device), bin_sizes=bs, r=r)
