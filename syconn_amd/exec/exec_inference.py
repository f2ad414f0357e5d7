"""Astrocyte splitting between ``run_create_rag`` and ``run_create_neuron_ssd``: ``run_astrocyte_splitting`` of /root/reference/syconn/
exec/exec_inference.py (:341-380) over the tables of ``exec_init``.  The reference reads the pruned graph from an edge-list file, splits
cell by cell in batch jobs and writes the neuron graph to a file; here the pruned graph is the ``SvGraphComponents`` of
``run_create_rag`` and the result's ``neuron_edges`` go straight into ``run_create_neuron_ssd(edges=...)``.  The glia probabilities come
from ``run_astrocyte_prediction`` (the reference's ``run_astrocyte_rendering`` and ``run_astrocyte_prediction``, :290-338, in one: the
views of every supervoxel are rendered, predicted and classified on the device and never stored), so that ``run_create_rag ->
run_astrocyte_prediction -> run_astrocyte_splitting -> run_create_neuron_ssd`` runs without an outside input.  Not built: view
storages, batch jobs, files, the point models."""
import numpy as np

from .. import global_params
from ..proc import glia_splitting, graphs


class AstrocyteSplitting:
    """``split`` (``GliaSplit``), ``svs`` (``collect_glia_sv``: astrocyte_svs / neuron_svs / pruned_svs), ``graph`` (``AstrocyteSvGraph``),
    ``glia`` (the class per table row) and ``glia_proba`` (the mean per table row, None where classes were given); ``neuron_edges`` is
    ``graph.neuron_edges``."""

    def __init__(self, split, svs, graph, glia, glia_proba):
        self.split, self.svs, self.graph, self.glia, self.glia_proba = split, svs, graph, glia, glia_proba
        self.neuron_edges = graph.neuron_edges


def _boxes_nm(sv_props, mesh_bb, scaling):
    """mesh_bb per table row: given (a ``MeshTable`` of ``mesh_props`` or an (n, 2, 3) array), or ``bounding_box * scaling`` for supervoxels
    without a mesh (reps/segmentation.py:604-617)."""
    n = len(sv_props.ids)
    if mesh_bb is not None:
        bb = np.asarray(mesh_bb.mesh_bb if hasattr(mesh_bb, 'mesh_bb') else mesh_bb)
        if bb.size != 6 * n:
            raise ValueError(f'run_astrocyte_splitting: mesh_bb must have the shape ({n}, 2, 3), got {bb.shape}')
        return bb.reshape(n, 2, 3)
    box_begin = np.asarray(sv_props.box_begin, np.int64)
    boxes = np.asarray(sv_props.boxes, np.int64).reshape(-1, 2, 3)
    if n and (np.diff(box_begin) < 1).any():
        raise ValueError('run_astrocyte_splitting: a supervoxel without a bounding box')
    lo = np.minimum.reduceat(boxes[:, 0], box_begin[:-1]) if n else np.zeros((0, 3), np.int64)
    hi = np.maximum.reduceat(boxes[:, 1], box_begin[:-1]) if n else np.zeros((0, 3), np.int64)
    return np.stack([lo, hi], 1) * scaling


def run_astrocyte_splitting(components, sv_props, mesh_bb=None, glia_probas=None, view_begin=None, glia=None, thresh=None,
                            use_point_models=None, scaling=None, min_cc_size=None, device=None) -> AstrocyteSplitting:
    """``run_astrocyte_splitting`` (:341-380).  `components`: the ``SvGraphComponents`` of ``run_create_rag`` (its ``edges`` are the graph,
    its ``sv_ids`` the nodes, its ``node_size`` the size of every supervoxel's original cell); `sv_props`: the cell ``PropTable``.  Boxes:
    `mesh_bb` (the ``MeshTable`` of ``mesh_props`` over `sv_props`, or an (n, 2, 3) array in nm), without it ``bounding_box * scaling``.
    The glia class per table row: `glia`, or ``glia_pred(glia_probas, view_begin, thresh, use_point_models)``.  `min_cc_size` (default
    ``config['min_cc_size_ssv']``) is both the threshold of ``remove_glia_nodes`` and the ``min_ssv_size`` of
    ``write_astrocyte_svgraph`` (:378)."""
    what = 'run_astrocyte_splitting'
    if (glia is None) == (glia_probas is None):
        raise ValueError(f'{what}: pass either glia or glia_probas (with view_begin)')
    if glia_probas is not None and view_begin is None:
        raise ValueError(f'{what}: glia_probas needs view_begin')
    scaling = np.asarray(global_params.config['scaling'] if scaling is None else scaling, dtype=np.float64)
    if min_cc_size is None:
        min_cc_size = global_params.config['min_cc_size_ssv']
    ids = np.ascontiguousarray(np.asarray(sv_props.ids).reshape(-1), dtype=np.uint64)
    boxes = _boxes_nm(sv_props, mesh_bb, scaling)
    proba = None
    if glia is None:
        if len(np.asarray(view_begin).reshape(-1)) != len(ids) + 1:
            raise ValueError(f'{what}: view_begin must have one entry per supervoxel and one more')
        glia, proba = graphs.glia_pred(glia_probas, view_begin, thresh, use_point_models, device)
    # the size of the original cell per table row: +inf for supervoxels outside the graph (they are no nodes)
    cell_size = np.full(len(ids), np.inf)
    row = np.searchsorted(ids, components.node_ids)
    ok = row < len(ids)
    ok[ok] = ids[row[ok]] == components.node_ids[ok]
    cell_size[row[ok]] = components.node_size[ok]
    split = glia_splitting.run_glia_splitting(components.edges, ids, boxes, glia, min_cc_size, components.sv_ids, cell_size, min_cc_size,
                                              sv_props.sizes, device)
    return AstrocyteSplitting(split, glia_splitting.collect_glia_sv(split, ids), glia_splitting.write_astrocyte_svgraph(split, scaling),
                              np.asarray(glia), proba)


def run_astrocyte_prediction(cells, model=None, thresh=None, **kw):
    """``run_astrocyte_rendering`` (exec/exec_render.py:206) and ``run_astrocyte_prediction`` (exec/exec_inference.py:290-338) in one:
    views are never stored, so rendering is no step of its own.  `cells`: the connected components of the pruned supervoxel graph as
    objects with ``.mesh`` and ``.svs``; -> the ``GliaTable`` of ``predict_glia_table`` (whose keyword arguments `kw` are), with the
    views on the device from the rasteriser to the class.  ``table.glia_probas[:, 1]`` and ``table.view_begin`` go into
    ``run_astrocyte_splitting``.  `model` defaults to ``get_glia_model_e3()``, `thresh` to ``config['glia']['glia_thresh']``.  The
    reference spreads the cells over batch jobs and storages; neither layer is built, nor is the point-model path."""
    from ..handler.prediction import get_glia_model_e3
    from ..reps.super_segmentation_helper import predict_glia_table
    if global_params.config['use_point_models']:
        raise NotImplementedError('run_astrocyte_prediction: the point models are not built')
    model = get_glia_model_e3() if model is None else model
    return predict_glia_table(cells, model, thresh=thresh, **kw)


def run_celltype_prediction(cells, model=None, views=None, ids=None, nb_views_model=None, use_syntype=None, bs: int = 40, **vote_kw):
    """exec/exec_inference.py:113-144 as a table form: the cell types of `cells` (objects with ``load_views()`` and ``syn_props``, or
    `views` per cell) with one pass over the view network -> ``CellTypeTable``.  The reference spreads the cells over batch jobs that
    each call ``predict_celltype_multiview``; the dataset and job layers are not built.  `model` defaults to
    ``get_celltype_model_e3()``, `nb_views_model` to ``config['celltypes']['nb_views_model']``, `use_syntype` to
    ``config.syntype_available`` (as ``predict_sso_celltype`` decides it)."""
    from ..handler.prediction import get_celltype_model_e3
    from ..reps.super_segmentation_helper import predict_celltypes_table
    if global_params.config['use_point_models']:
        raise NotImplementedError('run_celltype_prediction: the point models are not built')
    model = get_celltype_model_e3() if model is None else model
    nb = global_params.config['celltypes']['nb_views_model'] if nb_views_model is None else nb_views_model
    syn = bool(global_params.config.syntype_available) if use_syntype is None else use_syntype
    return predict_celltypes_table(cells, model, views=views, nb_views_model=nb, use_syntype=syn, bs=bs, ids=ids, **vote_kw)


def run_morphology_embedding(cells, model=None, views=None, locations=None, ids=None, bs=None):
    """exec/exec_inference.py:29-66 as a table form: the local morphology embeddings of `cells` (objects with ``skeleton``,
    ``scaling``, and rendered views in ``view_dict['tmp_views']`` with their rendering locations, or `views` and `locations` per cell)
    with one pass over the representation network and one nearest-location call -> ``MorphologyTable``.  The reference spreads the
    cells over batch jobs that each call ``predict_views_embedding``; the dataset and job layers and the point-model branch
    (``infere_cell_morphology_ssd``) are not built.  `model` defaults to ``get_tripletnet_model_e3()``."""
    from ..handler.prediction import get_tripletnet_model_e3
    from ..reps.super_segmentation_helper import embed_cells_table
    if global_params.config['use_point_models']:
        raise NotImplementedError('run_morphology_embedding: the point models are not built')
    model = get_tripletnet_model_e3() if model is None else model
    return embed_cells_table(cells, model, views=views, locations=locations, bs=bs, ids=ids)


def run_semsegaxoness_prediction(cells, model=None, view_props=None, map_properties=None, pred_key=None, max_dist=None, bs: int = 5, device=None):
    """exec/exec_inference.py:147-186 over cells in memory, each handled as ``semsegaxoness_predictor`` does
    (reps/super_segmentation_object.py:3468-3494): ``semseg_of_sso_nocache`` with ``config['compartments']['view_properties_semsegax']``
    (updated by `view_props`), then ``semsegaxoness2skel`` with ``map_properties_semsegax``, the views' ``semseg_key`` and
    ``dist_axoness_averaging``.  -> the ids of the cells that raised a ``RuntimeError`` (the reference's "missing" list).  The dataset,
    job and point-model layers are not built.  `model` defaults to ``get_semseg_axon_model()``; bs = 5 as in the batch job script."""
    import logging
    from ..handler.prediction import get_semseg_axon_model
    from ..reps.super_segmentation_helper import semseg_of_sso_nocache
    from ..reps.super_segmentation_object import semsegaxoness2skel
    if global_params.config['use_point_models']:
        raise NotImplementedError('run_semsegaxoness_prediction: the point models are not built')
    comp = global_params.config['compartments']
    props = dict(comp['view_properties_semsegax'])
    props.update(view_props or {})
    map_properties = dict(comp['map_properties_semsegax'] if map_properties is None else map_properties)
    pred_key = props['semseg_key'] if pred_key is None else pred_key
    max_dist = comp['dist_axoness_averaging'] if max_dist is None else max_dist
    model = get_semseg_axon_model() if model is None else model
    missing = []
    for sso in cells:
        try:
            semseg_of_sso_nocache(sso, model, bs=bs, device=device, **props)
            semsegaxoness2skel(sso, map_properties, pred_key, max_dist)
        except RuntimeError as e:
            missing.append(sso.id)
            logging.getLogger('syconn_amd.reps').error('Error during sem. seg. prediction of SSV {}. {}'.format(sso.id, repr(e)))
    return missing


def run_semsegspiness_prediction(cells, model=None, view_props=None, kwargs_semseg2mesh=None, kwargs_semsegforcoords=None, device=None):
    """exec/exec_inference.py:189-214 over cells in memory, each handled as ``semsegspiness_predictor`` does (:3560-3597):
    ``semseg_of_sso_nocache`` with ``config['views']['view_properties']`` (updated by `view_props`) and
    ``config['spines']['semseg2mesh_spines']``, then the vertex labels at the skeleton nodes (``semseg_for_coords`` with
    ``semseg2coords_spines``) into ``sso.skeleton[semseg_key]`` and ``sso.save_skeleton()``.  -> the ids of the cells that raised a
    ``RuntimeError``.  `model` defaults to ``get_semseg_spiness_model()``."""
    import logging
    from ..handler.prediction import get_semseg_spiness_model
    from ..reps.super_segmentation_helper import semseg_of_sso_nocache
    from ..reps.super_segmentation_object import semseg_for_coords
    props = dict(global_params.config['views']['view_properties'])
    props.update(view_props or {})
    s2m = dict(global_params.config['spines']['semseg2mesh_spines'] if kwargs_semseg2mesh is None else kwargs_semseg2mesh)
    s2c = dict(global_params.config['spines']['semseg2coords_spines'] if kwargs_semsegforcoords is None else kwargs_semsegforcoords)
    model = get_semseg_spiness_model() if model is None else model
    missing = []
    for sso in cells:
        try:
            semseg_of_sso_nocache(sso, model, device=device, **props, **s2m)
            sso.load_skeleton()
            if sso.skeleton is None or len(sso.skeleton['nodes']) == 0:
                logging.getLogger('syconn_amd.reps').warning(f'Skeleton of SSV {sso.id} has zero nodes.')
                node_preds = np.zeros((0,), dtype=np.int32)
            else:
                node_preds = semseg_for_coords(sso, sso.skeleton['nodes'], s2m['semseg_key'], device=device, **s2c)
            sso.skeleton[s2m['semseg_key']] = node_preds
            sso.save_skeleton()
        except RuntimeError as e:
            missing.append(sso.id)
            logging.getLogger('syconn_amd.reps').error('Error during sem. seg. prediction of SSV {}. {}'.format(sso.id, repr(e)))
    return missing
