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


def run_kimimaro_skeletonization(seg, scaling=None, map_myelin: bool = False, cube_size=None, cube_of_interest_bb=None, ds=None, sv_ids=None,
                                 ssv_ids=None, dust_threshold=1000, teasar_params=None, device=None, **myelin_kwargs):
    """``run_kimimaro_skeletonization`` (/root/reference/syconn/exec/exec_skeleton.py:115-198) as a table over the chunks of a label
    volume in memory (`seg` (X, Y, Z), voxel 0 at its origin): ``kimimaro_skelgen`` per cube of `cube_size` mag-1 voxels (default 1024 x
    1024 x 512, the whole box if that is smaller) inside `cube_of_interest_bb` (default: the volume; a cube that reaches beyond it reads
    zeros), `ds` defaulting to ``scaling[2] // scaling``, then ``kimimaro_mergeskels`` per cell.  -> ``SkeletonTable``; with `map_myelin`
    also the ``map_myelin_global`` columns of its nodes (`myelin_kwargs` go there).  No storages, no batch jobs."""
    from types import SimpleNamespace
    from ..proc.skeleton import SkeletonTable, kimimaro_mergeskels, kimimaro_skelgen
    seg = np.asarray(seg)
    scaling = np.asarray(global_params.config['scaling'] if scaling is None else scaling)
    if ds is None:
        ds = scaling[2] // scaling
        if not (ds > 0).all():
            raise ValueError('run_kimimaro_skeletonization: scaling[2] // scaling must be positive')
    bb = np.array([[0, 0, 0], seg.shape] if cube_of_interest_bb is None else cube_of_interest_bb, dtype=np.int64)
    if bb.shape != (2, 3) or (bb[1] <= bb[0]).any() or (bb[0] < 0).any():
        raise ValueError('run_kimimaro_skeletonization: cube_of_interest_bb is (lower, upper) in mag-1 voxels')
    size = bb[1] - bb[0]
    cube = np.array([1024, 1024, 512] if cube_size is None else cube_size, dtype=np.int64)
    if (cube > size).all():
        cube = size
    inside = seg[:bb[1][0], :bb[1][1], :bb[1][2]]
    pieces = {}
    for ox in range(bb[0][0], bb[1][0], cube[0]):
        for oy in range(bb[0][1], bb[1][1], cube[1]):
            for oz in range(bb[0][2], bb[1][2], cube[2]):
                part = kimimaro_skelgen(inside, cube, (ox, oy, oz), ds=ds, dust_threshold=dust_threshold, scaling=scaling, sv_ids=sv_ids, ssv_ids=ssv_ids,
                                        teasar_params=teasar_params, device=device)
                for cell, skel in part.items():
                    pieces.setdefault(cell, []).append(skel)
    table = SkeletonTable.from_skeletons({cell: kimimaro_mergeskels(p) for cell, p in pieces.items()})
    if not map_myelin:
        return table
    cols = table.to_cell_columns(scaling)
    cells = SimpleNamespace(nodes=cols['nodes'], node_begin=cols['node_begin'])
    return table, map_myelin_global(cells, cols['edges'], cols['edge_begin'], scaling=scaling, device=device, **myelin_kwargs)


def run_skeleton_generation(seg, cube_of_interest_bb=None, map_myelin: bool = False, **kwargs):
    """``run_skeleton_generation`` (/root/reference/syconn/exec/exec_skeleton.py:27-44): the volume-based path (``use_kimimaro``, the
    reference's default); the mesh-based fallback is not built."""
    if not global_params.config['use_kimimaro']:
        raise NotImplementedError('run_skeleton_generation: the mesh-based fallback (create_sso_skeleton_fast) is not built')
    return run_kimimaro_skeletonization(seg, map_myelin=map_myelin, cube_of_interest_bb=cube_of_interest_bb, **kwargs)
