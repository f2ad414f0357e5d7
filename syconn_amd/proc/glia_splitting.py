"""Astrocyte splitting over tables: ``run_glia_splitting``, ``collect_glia_sv`` and ``write_astrocyte_svgraph`` of /root/reference/syconn/
proc/glia_splitting.py (:26-161).  The reference splits cell by cell in batch jobs (``SuperSegmentationObject.gliasplit`` ->
``split_glia_graph`` -> ``remove_glia_nodes``), keeps the lists in per-cell attribute dictionaries and writes ``.npy`` arrays, edge-list
files and KNOSSOS merge lists; here all cells are split in one device call (``proc.graphs.split_glia_table``) and everything stays in
memory.  Not built: the files, the ``gliaremoval`` storages, ``gliasplit2mesh``."""
import numpy as np

from .. import global_params
from . import graphs


def run_glia_splitting(edges, sv_ids, boxes_nm, glia, min_cc_size=None, nodes=None, cell_size=None, min_cell_size=None, sv_sizes=None,
                       device=None) -> graphs.GliaSplit:
    """``run_glia_splitting`` (:26-34): every cell of the graph `edges` (+ `nodes` without an edge) is split into neuron and glia
    components.  The arguments are those of ``split_glia_table``; `cell_size` / `min_cell_size` are the size filter that
    ``write_astrocyte_svgraph`` applies to the ORIGINAL cells (:125-127, :147-149), given here because the split graphs come from the
    same call."""
    return graphs.split_glia_table(edges, sv_ids, boxes_nm, glia, min_cc_size, nodes, cell_size, min_cell_size, sv_sizes, device)


def collect_glia_sv(split: graphs.GliaSplit, table_ids) -> dict:
    """``collect_glia_sv`` (:37-63): ``astrocyte_svs`` = the supervoxels of the glia components of all cells, ``pruned_svs`` = the table
    ids that are not in the graph (``missing_ids``: sorted out by the size filter of ``run_create_rag``), ``neuron_svs`` = the remaining
    table ids; all uint64 ascending."""
    ids = np.ascontiguousarray(np.asarray(table_ids).reshape(-1), dtype=np.uint64)
    astro = split.node_ids[split.node_class == 1]
    pruned = np.setdiff1d(ids, split.node_ids)
    neuron = np.setdiff1d(ids, np.union1d(astro, pruned))
    return dict(astrocyte_svs=astro, neuron_svs=neuron, pruned_svs=pruned)


class AstrocyteSvGraph:
    """What ``write_astrocyte_svgraph`` writes, in memory: ``neuron_edges`` / ``astrocyte_edges`` (the two edge lists, input order),
    ``neuron`` / ``astrocyte`` (``GliaComponents``: the two agglomeration lists), ``n_neuron_ccs`` / ``n_neuron_svs`` / ``n_astrocyte_ccs`` /
    ``n_astrocyte_svs`` (the numbers it logs), ``total_size`` (voxels of the astrocyte supervoxels) and ``total_size_cmm`` (mm^3)."""

    def __init__(self, **columns):
        self.__dict__.update(columns)


def write_astrocyte_svgraph(split: graphs.GliaSplit, scaling=None) -> AstrocyteSvGraph:
    """``write_astrocyte_svgraph`` (:77-161) from a split that was made with `cell_size` / `min_cell_size` (its ``min_ssv_size``) and
    `sv_sizes`: the neuron graph is the input graph without the astrocyte supervoxels, the astrocyte graph its complement, both without
    the supervoxels of cells below the size.  A neuron supervoxel whose neighbours all became glia is in ``neuron`` and, without a self
    loop, in no edge of ``neuron_edges``, as in the reference's list and edge-list files."""
    scaling = np.asarray(global_params.config['scaling'] if scaling is None else scaling, dtype=np.float64)
    total = int(split.astrocyte_size)
    return AstrocyteSvGraph(neuron_edges=split.neuron_edges, astrocyte_edges=split.astrocyte_edges, neuron=split.neuron, astrocyte=split.glia,
                            n_neuron_ccs=len(split.neuron), n_neuron_svs=len(split.neuron.sv_ids), n_astrocyte_ccs=len(split.glia),
                            n_astrocyte_svs=len(split.glia.sv_ids), total_size=total, total_size_cmm=np.prod(scaling) * total / 1e18)
