"""Drop-in for ``semsegaxoness2skel`` of ``syconn.reps.super_segmentation_object`` (/root/reference/syconn/reps/
super_segmentation_object.py:3497-3557) and its table form over a ``CellTable``.  The three steps -- the vertex predictions at the
skeleton nodes (``semseg_for_coords``, :2190-2240), the sliding-window vote (``majorityvote_skeleton_property``) and the compartment
vote (``majority_vote_compartments``) -- run on the device for all cells of a call: one ``segmented_knn`` call, one
``skeleton_majority_vote`` call, one ``skeleton_compartment_majority`` call.  No CPU fallback.
"""
import logging

import numpy as np

from .. import _lib as L
from .super_segmentation_helper import skeleton_compartment_majority, skeleton_majority_vote

log_reps = logging.getLogger('syconn_amd.reps')


def _recover_boutons(node_preds, smoothed):
    """Bouton predictions (3: en-passant, 4: terminal) come back where the smoothed label is axon (:3545-3546, :3554-3555)."""
    smoothed[(node_preds == 3) & (smoothed == 1)] = 3
    smoothed[(node_preds == 4) & (smoothed == 1)] = 4
    return smoothed


def _smooth(node_preds, nodes, node_begin, edges, edge_begin, scaling, max_dist, device):
    """Node predictions -> (merged int32 labels, their sliding-window vote, the compartment vote as float64), :3531-3556."""
    nodes_ax_den_so = np.array(node_preds, dtype=np.int32)
    nodes_ax_den_so[nodes_ax_den_so == 3] = 1
    nodes_ax_den_so[nodes_ax_den_so == 4] = 1
    avg = _recover_boutons(node_preds, skeleton_majority_vote(nodes, node_begin, edges, edge_begin, nodes_ax_den_so, scaling, max_dist, device))
    comp = np.zeros(len(avg))
    comp[:] = skeleton_compartment_majority(node_begin, edges, edge_begin, avg, device=device)
    return nodes_ax_den_so, avg, _recover_boutons(node_preds, comp)


def semsegaxoness2skel_table(cells, edges, edge_begin, map_properties: dict, pred_key: str, max_dist, scaling, device=None) -> dict:
    """``semsegaxoness2skel`` for all cells of a ``CellTable`` (``cs_processing_steps.CellTable``: vertices, ``vertex_labels[pred_key]``
    and the skeleton nodes) plus their skeleton edges (`edges` (e, 2): node indices inside the cell, `edge_begin` (cells + 1)).
    `map_properties`: ``k`` (<= 64), ``ds_vertices``, optionally ``ignore_labels``.  -> the node attributes ``pred_key`` (int32),
    ``"{pred_key}_avg{max_dist}"`` (int32) and ``"{pred_key}_avg{max_dist}_comp_maj"`` (float64) for all nodes of the table.  The
    nodes of a cell without mesh vertices get zeros in all three (the reference's branch for such a cell, :3520-3525)."""
    from ..extraction.cs_processing_steps import CellTable, _check_positive_int, segmented_knn, spine_vertices
    if not isinstance(cells, CellTable):
        raise TypeError('cells must be a CellTable')
    k, ds_vertices = map_properties['k'], map_properties['ds_vertices']
    _check_positive_int(k=k, ds_vertices=ds_vertices)
    if int(k) > L.SD_SYN_PROPS_MAX_K:
        raise ValueError(f'k = {k}: at most {L.SD_SYN_PROPS_MAX_K} neighbours per query')
    scaling = np.asarray(scaling)
    n_nodes, n_vert = np.diff(cells.node_begin), np.diff(cells.vert_begin)
    used = (n_nodes > 0) & (n_vert > 0)
    node_preds = np.zeros(len(cells.nodes), np.int32)
    if used.any():
        verts, lab, begin = spine_vertices(cells, used, pred_key, int(ds_vertices), map_properties.get('ignore_labels'))
        empty = np.flatnonzero(used & (np.diff(begin) == 0))
        if len(empty):
            raise ValueError(f'every mesh vertex of cell {int(cells.ids[empty[0]])} carries an ignored label: no vertex to vote')
        cell_of = np.repeat(np.arange(len(cells)), n_nodes)
        q = np.flatnonzero(used[cell_of])
        q_xyz = np.asarray(cells.nodes[q] * scaling, np.float64)                # np.array(coords) * self.scaling (:2219)
        node_preds[q] = segmented_knn(verts, begin, lab, cell_of[q], q_xyz, int(k), device)
    merged, avg, comp = _smooth(node_preds, cells.nodes, cells.node_begin, edges, edge_begin, scaling, max_dist, device)
    return {pred_key: merged, "{}_avg{}".format(pred_key, max_dist): avg, "{}_avg{}_comp_maj".format(pred_key, max_dist): comp}


def semsegaxoness2skel(sso, map_properties: dict, pred_key: str, max_dist: int):
    """Drop-in for ``semsegaxoness2skel`` (:3497-3557): populates ``sso.skeleton[pred_key]``, ``"{}_avg{}".format(pred_key, max_dist)``
    and ``"{}_avg{}_comp_maj".format(pred_key, max_dist)`` and calls ``sso.save_skeleton()``.  Reads of a (duck-typed) ``sso``:
    ``skeleton`` / ``load_skeleton``, ``mesh[1]``, ``label_dict('vertex')[pred_key]``, ``scaling``, ``id``."""
    from ..extraction.cs_processing_steps import CellTable
    if sso.skeleton is None:
        sso.load_skeleton()
    if sso.skeleton is None:
        log_reps.warning(f"Skeleton of {sso} hdoes not exist.")
        return
    if len(sso.skeleton["nodes"]) == 0 or len(sso.mesh[1]) == 0:
        log_reps.warning(f"Skeleton of {sso} has zero nodes or no mesh vertices.")
        sso.skeleton["{}_avg{}".format(pred_key, max_dist)] = np.zeros((len(sso.skeleton['nodes']), 1))
        sso.skeleton["{}_avg{}_comp_maj".format(pred_key, max_dist)] = np.zeros((len(sso.skeleton['nodes']), 1))
        sso.save_skeleton()
        return
    nodes = np.asarray(sso.skeleton['nodes']).reshape(-1, 3)
    edges = np.array(sso.skeleton['edges'], dtype=np.int64).reshape(-1, 2)
    verts = np.asarray(sso.mesh[1]).reshape(-1, 3)
    cells = CellTable([sso.id], verts, [0, len(verts)], {pred_key: sso.label_dict('vertex')[pred_key]}, nodes, [0, len(nodes)], {})
    res = semsegaxoness2skel_table(cells, edges, [0, len(edges)], map_properties, pred_key, max_dist, sso.scaling)
    for key, val in res.items():
        sso.skeleton[key] = val
    sso.save_skeleton()


# -- cell types (the methods of the reference's SuperSegmentationObject, as functions of the cell object) ------------------------------
def predict_celltype_multiview(sso, model, pred_key_appendix: str = '', model_tnet=None, view_props=None, onthefly_views: bool = False,
                               overwrite: bool = True, model_props=None, verbose: bool = False, save_to_attr_dict: bool = True, **kw):
    """reps/super_segmentation_object.py:3125-3165: ``celltype_cnn_e3``, ``_probas`` and ``_certainty`` of `sso` from `model` (a
    ``handler.prediction.ViewModel``), from the stored views (``sso.load_views()``, or ``views=`` in `kw`) or, with `onthefly_views`,
    from views rendered with the view properties of the config (updated by `view_props`).  With `model_tnet` (a
    ``handler.prediction.EmbeddingModel``) the morphology embedding follows, as there (:3160-3165): ``view_embedding_of_sso_nocache``
    on the view properties without ``use_syntype``, with ``overwrite=True``.  Any other `model_tnet` object -- an arbitrary torch
    module is not built -- is a NotImplementedError before anything runs."""
    from .. import global_params
    from ..handler.prediction import EmbeddingModel
    from . import super_segmentation_helper as ssh
    if model_tnet is not None and not isinstance(model_tnet, EmbeddingModel):
        raise NotImplementedError('predict_celltype_multiview: the morphology embedding (view_embedding_of_sso_nocache) is built for '
                                  'handler.prediction.EmbeddingModel only, not for an arbitrary module')
    model_props = dict(model_props or {})
    props = dict(global_params.config['views']['view_properties'])
    props.update(view_props or {})
    if not onthefly_views:
        out = ssh.predict_sso_celltype(sso, model, pred_key_appendix=pred_key_appendix, save_to_attr_dict=save_to_attr_dict,
                                       overwrite=overwrite, **model_props, **kw)
    else:
        out = ssh.celltype_of_sso_nocache(sso, model, pred_key_appendix=pred_key_appendix, save_to_attr_dict=save_to_attr_dict,
                                          overwrite=overwrite, verbose=verbose, **props, **model_props, **kw)
    if model_tnet is not None:
        emb_props = {k: v for k, v in props.items() if k != 'use_syntype'}
        ssh.view_embedding_of_sso_nocache(sso, model_tnet, pred_key_appendix=pred_key_appendix, overwrite=True, device=kw.get('device'), **emb_props)
    return out


def predict_views_embedding(sso, model, pred_key_appendix: str = '', view_key=None):
    """reps/super_segmentation_object.py:3032-3079, the cached-views form of ``view_embedding_of_sso_nocache``: the views of
    ``sso.load_views(view_key=view_key)`` (n_loc, C, nb_views, H, W), uint8, host or device, through `model` (a
    ``handler.prediction.EmbeddingModel``), and every skeleton node gets the latent of the rendering location
    ``sso.skeleton['view_ixs']``, which is computed from ``sso.sample_locations()`` and written when absent, as there.  Stores and
    returns ``sso.skeleton['latent_morph' + pred_key_appendix]``, float32 (n_nodes, z_dim)."""
    from . import super_segmentation_helper as ssh
    views = sso.load_views(view_key=view_key)
    if hasattr(sso, 'load_skeleton'):
        sso.load_skeleton()
    locs = ssh._cell_locations(sso) if 'view_ixs' not in sso.skeleton else np.zeros((len(views), 3), np.float32)
    return ssh._embed_to_skeleton(sso, model, views, locs, 'latent_morph' + pred_key_appendix, 'view_ixs')


def predict_views_gliaSV(sso, model, pred_key_appendix: str = '', verbose: bool = False, single_cc_only: bool = False):
    """reps/super_segmentation_object.py:2842-2859: the glia probabilities of the supervoxels ``sso.svs`` from their stored views
    (``sv.load_views(woglia=False, raw_only=True)``) through ``predict_sos_views``, into ``sv.attr_dict['glia_probas' +
    pred_key_appendix]``.  A cell of version ``'tmp'`` is not written to (as there); its probabilities are returned, one row per
    location in the order of ``predict_sos_views`` -- the reference drops them."""
    from ..proc.sd_proc import predict_sos_views
    pred_key = "glia_probas" + pred_key_appendix
    return predict_sos_views(model, sso.svs, pred_key, nb_cpus=getattr(sso, 'nb_cpus', 1), verbose=verbose, woglia=False, raw_only=True,
                             single_cc_only=single_cc_only, return_proba=getattr(sso, 'version', None) == 'tmp')


def certainty_celltype(sso, pred_key=None) -> float:
    """reps/super_segmentation_object.py:3193-3220: the stored certainty, else the entropy certainty of the stored logits."""
    from ..handler.prediction import certainty_estimate
    pred_key = 'celltype_cnn_e3' if pred_key is None else pred_key
    cert = sso.attr_dict.get(pred_key + '_certainty')
    if cert is not None:
        return cert
    return certainty_estimate(sso.attr_dict[pred_key + '_probas'], is_logit=True)


# -- compartment labels (predict_semseg, :2022-2120) -------------------------------------------------------------------------------------
def predict_semseg(sso, m, semseg_key: str, nb_views=None, verbose: bool = False, raw_view_key=None, save: bool = False, ws=None,
                   comp_window=None, add_cellobjects=True, bs: int = 10, views=None):
    """reps/super_segmentation_object.py:2072-2093, the non-default branch (`nb_views`, `raw_view_key` or `views` given): the pixel
    labels of the raw views `views` (n_loc, C, nb_views, H, W), host or device -- rendered here at ``sso._sample_locations`` with `ws`
    and `comp_window` if not passed -- through ``predict_views_semseg``; returned, and kept in ``sso.view_dict[semseg_key]`` when the
    cell caches views.  The default branch (views stored per supervoxel) and `save` need the view storage, which is not built."""
    from . import super_segmentation_helper as ssh
    if nb_views is None and raw_view_key is None and views is None:
        raise NotImplementedError('predict_semseg: the per-supervoxel view storage is not built; pass nb_views (and views, or ws and comp_window)')
    if save:
        raise NotImplementedError('predict_semseg: the view storage is not built (save=True)')
    if views is None:
        from .. import global_params
        from ..proc.rendering import render_sso_coords
        if nb_views is None:
            nb_views = global_params.config['views']['view_properties']['nb_views']
        locs = getattr(sso, '_sample_locations', None)
        if locs is None:
            raise ValueError('predict_semseg: no views and no rendering locations (sso._sample_locations)')
        locs = np.concatenate(locs) if isinstance(locs, (list, tuple)) else np.asarray(locs)
        views = render_sso_coords(sso, locs, ws=ws, comp_window=comp_window, nb_views=nb_views, verbose=verbose, add_cellobjects=add_cellobjects,
                                  return_device=True)
    labeled_views = ssh.predict_views_semseg(views, m, verbose=verbose, batch_size=bs)
    if nb_views is not None:
        assert labeled_views.shape[2] == nb_views, "Predictions have wrong shape."
    if getattr(sso, 'view_caching', False) and hasattr(sso, 'view_dict'):
        sso.view_dict[semseg_key] = labeled_views
    return labeled_views


def semseg_for_coords(sso, coords, semseg_key: str, k: int = 5, ds_vertices: int = 20, ignore_labels=None, device=None) -> np.ndarray:
    """reps/super_segmentation_object.py:2190-2240 for one cell: the majority label of the `k` nearest mesh vertices (every
    `ds_vertices`-th one, without `ignore_labels`) of every coordinate (voxels; scaled by ``sso.scaling``), int32.  Zeros without
    vertices or coordinates, as there."""
    from ..extraction.cs_processing_steps import CellTable, _check_positive_int, segmented_knn, spine_vertices
    coords = np.asarray(coords).reshape(-1, 3)
    verts = np.asarray(sso.mesh[1]).reshape(-1, 3)
    if len(coords) == 0 or len(verts) == 0:
        return np.zeros(len(coords), np.int32)
    _check_positive_int(k=k, ds_vertices=ds_vertices)
    if int(k) > L.SD_SYN_PROPS_MAX_K:
        raise ValueError(f'k = {k}: at most {L.SD_SYN_PROPS_MAX_K} neighbours per query')
    cells = CellTable([sso.id], verts, [0, len(verts)], {semseg_key: sso.label_dict('vertex')[semseg_key]}, coords, [0, len(coords)], {})
    v, lab, begin = spine_vertices(cells, np.array([True]), semseg_key, int(ds_vertices), ignore_labels)
    if begin[-1] == 0:
        raise ValueError(f'every mesh vertex of cell {sso.id} carries an ignored label: no vertex to vote')
    q_xyz = np.asarray(coords * np.asarray(sso.scaling), np.float64)
    return segmented_knn(v, begin, lab, np.zeros(len(coords), np.int64), q_xyz, int(k), device).astype(np.int32)
