"""Thin forms of the synapse steps of ``syconn.exec.exec_syns`` on tables in memory (no storages, no batch jobs)."""
import numpy as np

from ..extraction.cs_processing_steps import CellTable, calculate_spinehead_volume


def run_spinehead_volume_calc(cells: CellTable, sv_begin, sv_ids, syn_ssv, syn_ids, seg, **kwargs) -> CellTable:
    """``run_spinehead_volume_calc`` (/root/reference/syconn/exec/exec_syns.py: ``extract_spinehead_volume_mesh`` for every cell, stored in
    its attribute dict): the spine head volumes of all cells of the table for the synapses of a ``SynSsvTable`` (``rep_coords``,
    ``neuron_partners``), set as ``cells.spinehead_vol`` -- what ``collect_properties_from_ssv_partners`` then looks up.  Returns `cells`."""
    n = len(syn_ssv)
    syn_ids = np.arange(n, dtype=np.uint64) if syn_ids is None else syn_ids
    sb, ids, vols = calculate_spinehead_volume(cells, sv_begin, sv_ids, syn_ids, syn_ssv.rep_coords, syn_ssv.neuron_partners, seg, **kwargs)
    cells.spinehead_vol = (sb, ids, vols.astype(np.float32))
    return cells
