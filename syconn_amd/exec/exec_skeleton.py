"""The skeleton attributes that follow the dense predictions, for all cells of a table at once.  ``predict_myelin``'s docstring
(/root/reference/syconn/exec/exec_dense_prediction.py:25-39) names the two steps: ``map_myelin2coords(ssv.skeleton["nodes"], mag=4)``
and ``majorityvote_skeleton_property(ssv, "myelin")``."""
import numpy as np

from .. import global_params
from ..reps.super_segmentation_helper import map_myelin2coords, skeleton_majority_vote


def map_myelin_global(cells, edges, edge_begin, max_dist=None, scaling=None, mag: int = 4, device=None, **map_kwargs) -> dict:
    """``map_myelin2coords`` over the skeleton nodes of every cell of a ``CellTable`` and the sliding-window vote of the result along
    the skeletons (`edges` (e, 2): node indices inside the cell, `edge_begin` (cells + 1)).  `max_dist` defaults to
    ``config['compartments']['dist_axoness_averaging']``, `scaling` to ``config['scaling']``.  -> ``{'myelin': uint8,
    'myelin_avg{max_dist}': uint8}``, ready for ``CellTable.node_attrs``."""
    cfg = global_params.config
    max_dist = cfg['compartments']['dist_axoness_averaging'] if max_dist is None else max_dist
    scaling = cfg['scaling'] if scaling is None else scaling
    myelin = map_myelin2coords(cells.nodes, mag=mag, **map_kwargs)
    avg = skeleton_majority_vote(cells.nodes, cells.node_begin, edges, edge_begin, myelin, np.asarray(scaling), max_dist, device)
    return {'myelin': myelin, 'myelin_avg%d' % max_dist: avg}
