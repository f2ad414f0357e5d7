"""Cells from the supervoxel graph: ``run_create_rag`` and ``run_create_neuron_ssd`` of /root/reference/syconn/exec/exec_init.py
(:299-367, :32-123) over the tables ``map_subcell_extract_props(as_tables=True)`` returns.  The reference reads edge-list files into
networkx and writes ``SuperSegmentationDataset`` storages; here edges arrive as an ``(e, 2)`` uint64 array and everything stays in
memory.  Between the two runs ``exec_inference.run_astrocyte_splitting`` turns the pruned graph into the neuron graph.  Not built: the
files, the storages and their numpy caches, the per-cell ``edgelist`` files, meshes."""
from typing import Dict, Optional, Sequence

import numpy as np

from .. import global_params
from ..proc import graphs, ssd_proc


def _scaling(scaling):
    return np.asarray(global_params.config['scaling'] if scaling is None else scaling, dtype=np.float64)


def run_create_rag(edges, sv_props, scaling=None, min_cc_size=None, device=None) -> graphs.SvGraphComponents:
    """``run_create_rag`` (:299-367): node 0 is removed, every supervoxel of `sv_props` (the cell ``PropTable``) without an edge becomes a
    component of its own, components whose bounding box diagonal is ``<= min_cc_size`` nm (default ``config['min_cc_size_ssv']``) are
    dropped.  The result holds the pruned graph (``edges``), the agglomeration lists (``ssv_ids`` / ``sv_begin`` / ``sv_ids``) and
    ``total_size`` in voxels."""
    if min_cc_size is None:
        min_cc_size = global_params.config['min_cc_size_ssv']
    return graphs.svgraph_components(edges, sv_props, _scaling(scaling), min_cc_size, strict=True, device=device)


class CellAssembly:
    """What ``run_create_neuron_ssd`` returns: ``cells`` (``CellLists``), ``props`` (``CellProps``: size, bounding_box, rep_coord per cell),
    ``mappings`` (object type -> ``CellMapping``) and, where the cells came from a graph, ``components`` (``SvGraphComponents``)."""

    def __init__(self, cells, props, mappings, components=None):
        self.cells, self.props, self.mappings, self.components = cells, props, mappings, components

    def organelle_cells(self, obj_type: str) -> np.ndarray:
        """The ``cells`` column of the ``OrganelleTable`` of `obj_type`."""
        return ssd_proc.organelle_cells(self.mappings[obj_type])

    def ssv_lookup(self):
        return ssd_proc.ssv_lookup(self.cells)


def run_create_neuron_ssd(sv_props, organelle_props: Dict[str, object], organelle_maps: Dict[str, object], edges=None, cell_lists=None,
                          apply_ssv_size_threshold: bool = False, scaling=None, min_cc_size=None, obj_types: Optional[Sequence[str]] = None,
                          allow_missing: bool = False, device=None) -> CellAssembly:
    """``run_create_neuron_ssd`` (:32-123) over ``(sv_props, organelle_props, organelle_maps)`` =
    ``map_subcell_extract_props(..., as_tables=True)``.  The cells are the components of `edges` (with `apply_ssv_size_threshold`
    those with a diagonal ``< min_cc_size`` are dropped, :75; without it none is) or, as in the reference's agglomeration-list branch
    (:82-87), `cell_lists` = ``(sv_begin, sv_ids)`` or a ``CellLists``.  Then the cell properties and, for `obj_types` (default
    ``config['process_cell_organelles']``), ``apply_mapping_decisions``."""
    if (edges is None) == (cell_lists is None):
        raise ValueError('run_create_neuron_ssd: pass either edges or cell_lists')
    comps = None
    if edges is not None:
        thresh = -np.inf
        if apply_ssv_size_threshold:
            thresh = global_params.config['min_cc_size_ssv'] if min_cc_size is None else min_cc_size
        comps = graphs.svgraph_components(edges, sv_props, _scaling(scaling), thresh, strict=False, device=device)
        cells = ssd_proc.CellLists(comps.ssv_ids, comps.sv_begin, comps.sv_ids)
    else:
        cells = cell_lists if isinstance(cell_lists, ssd_proc.CellLists) else ssd_proc.CellLists.from_lists(*cell_lists)
    if obj_types is None:
        obj_types = global_params.config['process_cell_organelles']
    props = ssd_proc.cell_properties(cells, sv_props, allow_missing=allow_missing, device=device)
    mappings = ssd_proc.apply_mapping_decisions(cells, organelle_maps, organelle_props, obj_types, device=device)
    return CellAssembly(cells, props, mappings, comps)
