"""Cell properties, organelle -> cell mapping and cell -> synapse lists over tables in memory: what /root/reference/syconn/proc/
ssd_proc.py does per ``SuperSegmentationObject`` in Python -- ``_aggregate_segmentation_object_mappings_thread`` (:55-91, a ``Counter``
per cell over the per-supervoxel overlap ratios of proc/sd_proc.py:1063-1084), ``_apply_mapping_decisions_thread`` (:126-238) and
``map_synssv_objects_thread`` (:315-342) -- with the cell attributes of reps/super_segmentation_object.py (:713-727, :1148-1168).
Every step is one device call (``sd_cell_props``, ``sd_cell_mapping``, ``sd_cell_synapses``); no CPU fallback, no storage layer.

Deviations.  The reference's per-cell mapping lists are in the insertion order of nested dictionaries; here they ascend by organelle
id (the sums do not depend on it).  ``_apply_mapping_decisions_thread`` reads the three thresholds of the FIRST object type and uses
them for every later one (its ``if lower_ratio is None`` is never true again); here every type gets its own thresholds, which equals
the reference called with one type at a time.  Cells given as explicit lists are reordered to ascend by cell id (the smallest
supervoxel id of the list, :87); the order inside a list is kept, and it decides the bits of the ratio sums."""
from typing import Dict, Optional, Sequence

import numpy as np

from .. import _dev as D
from .graphs import SvTable, _u64


class CellLists:
    """The cells as CSR, plain numpy: ``ssv_ids`` uint64 strictly ascending, ``sv_begin`` int64 (n + 1), ``sv_ids`` uint64: cell c owns
    ``sv_ids[sv_begin[c]:sv_begin[c + 1]]``.  ``svgraph_components`` yields the lists ascending; ``from_lists`` keeps the caller's
    order inside a cell."""

    def __init__(self, ssv_ids, sv_begin, sv_ids):
        self.ssv_ids = _u64('CellLists: ssv_ids', ssv_ids)
        self.sv_ids = _u64('CellLists: sv_ids', sv_ids)
        self.sv_begin = np.ascontiguousarray(np.asarray(sv_begin).reshape(-1), dtype=np.int64)
        n = len(self.ssv_ids)
        if len(self.sv_begin) != n + 1 or self.sv_begin[0] != 0 or self.sv_begin[-1] != len(self.sv_ids) or np.any(np.diff(self.sv_begin) < 0):
            raise ValueError(f'CellLists: sv_begin must hold {n + 1} ascending offsets from 0 to {len(self.sv_ids)}')
        if np.any(np.diff(self.sv_begin) == 0):
            raise ValueError(f'CellLists: cell {int(self.ssv_ids[np.flatnonzero(np.diff(self.sv_begin) == 0)[0]])} is empty')
        if (self.sv_ids == 0).any():
            raise ValueError('CellLists: supervoxel id 0 in a cell')
        srt = np.sort(self.sv_ids)
        dup = np.flatnonzero(srt[1:] == srt[:-1])
        if len(dup):
            raise ValueError(f'CellLists: supervoxel {int(srt[dup[0]])} is in two cells (or twice in one)')
        if n > 1 and not (self.ssv_ids[1:] > self.ssv_ids[:-1]).all():
            raise ValueError('CellLists: ssv_ids must ascend strictly')

    def __len__(self):
        return len(self.ssv_ids)

    @classmethod
    def from_lists(cls, sv_begin, sv_ids):
        """Cells as explicit supervoxel lists (the agglomeration-list branch, exec_init.py:82-87): the cell id is the smallest id of its
        list, the order inside a list is the caller's."""
        sv_ids = _u64('CellLists.from_lists: sv_ids', sv_ids)
        b = np.asarray(sv_begin, dtype=np.int64).reshape(-1)
        if len(b) < 1 or b[0] != 0 or b[-1] != len(sv_ids) or np.any(np.diff(b) < 0):
            raise ValueError(f'CellLists.from_lists: sv_begin must hold ascending offsets from 0 to {len(sv_ids)}')
        n_sv = np.diff(b)
        if np.any(n_sv == 0):
            raise ValueError(f'CellLists.from_lists: list {int(np.flatnonzero(n_sv == 0)[0])} is empty')
        if len(n_sv) == 0:
            return cls(np.zeros(0, np.uint64), b, sv_ids)
        ssv = np.minimum.reduceat(sv_ids, b[:-1])
        order = np.argsort(ssv, kind='stable')
        new_b = np.concatenate(([0], np.cumsum(n_sv[order])))
        src = np.repeat(b[:-1][order] - new_b[:-1], n_sv[order]) + np.arange(len(sv_ids))
        return cls(ssv[order], new_b, sv_ids[src])

    def mapping_dict(self) -> dict:
        """cell id -> its supervoxel ids (``ssd.mapping_dict``)."""
        return dict(zip(self.ssv_ids.tolist(), np.split(self.sv_ids, self.sv_begin[1:-1]))) if len(self) else {}


def ssv_lookup(cells: CellLists):
    """``(sv_ids, ssv_ids)``: the cell of every supervoxel, the pair ``combine_and_split_syn`` / ``filter_relevant_syn`` take."""
    return cells.sv_ids.copy(), np.repeat(cells.ssv_ids, np.diff(cells.sv_begin))


class CellProps:
    """``size`` int64 (n), ``bounding_box`` int32 (n, 2, 3), ``rep_coord`` int32 (n, 3) of the cells of a ``CellLists``."""

    def __init__(self, size, bounding_box, rep_coord):
        self.size, self.bounding_box, self.rep_coord = size, bounding_box, rep_coord


def cell_properties(cells: CellLists, sv_props, allow_missing: bool = False, device=None) -> CellProps:
    """Per cell ``size`` = the sum of its supervoxels' sizes (``calculate_size``, :1148-1152), ``bounding_box`` = min of the lower and
    max of the upper corners (``calculate_bounding_box``, :1154-1168), ``rep_coord`` = that of the first supervoxel in the cell's
    order (:713-727).  A supervoxel that is not in `sv_props` (a ``PropTable``) raises ``ValueError`` unless `allow_missing`: then it
    contributes nothing, and a cell without any known supervoxel gets size 0 and the zero box."""
    dev = D.device(device)
    tab = sv_props if isinstance(sv_props, SvTable) else SvTable(sv_props, dev)
    n = len(cells)
    size, box, rep = D.empty(n, D.i64, dev), D.empty((n, 6), D.i32, dev), D.empty((n, 3), D.i32, dev)
    counts_d = D.counters(dev)
    sb, sv = D.up(cells.sv_begin, dev), D.up(cells.sv_ids, dev)
    D.call('sd_cell_props', dev, sb, sv, n, len(cells.sv_ids), tab.ids, tab.sizes, tab.rep, tab.box_begin, tab.boxes, tab.n, tab.n_boxes, size, box,
           rep, counts_d)
    counts = D.down(counts_d)
    if int(counts[7]):
        raise ValueError('cell_properties: the cell lists or the supervoxel table are inconsistent')
    if int(counts[0]) and not allow_missing:
        raise ValueError(f'cell_properties: {int(counts[0])} supervoxels are not in the table, e.g. {int(counts.view(np.uint64)[5])}')
    return CellProps(D.down(size, n), D.down(box, n).reshape(n, 2, 3), D.down(rep, n))


class CellMapping:
    """One organelle kind mapped to the cells.  Pairs (cell, organelle) ascend by cell row, then organelle id: ``cell_begin`` int64
    (n_cells + 1) into ``ids`` uint64 / ``ratios`` float64 / ``accepted`` bool; ``acc_begin`` into ``acc_ids`` = the accepted organelles
    per cell; per organelle of the table (``org_ids``) ``org_n_cells`` = accepting cells and ``org_first_cell`` = the id of the first one
    (0: none).  ``n_records`` = overlap records that were used."""

    def __init__(self, **columns):
        self.__dict__.update(columns)

    def as_dicts(self):
        """Per cell ``(mapping ids, mapping ratios, accepted ids)`` as lists: ``mapping_{obj}_ids``, ``mapping_{obj}_ratios``, ``{obj}``."""
        cb, ab = self.cell_begin.tolist(), self.acc_begin.tolist()
        ids, ratios, acc = self.ids.tolist(), self.ratios.tolist(), self.acc_ids.tolist()
        return {c: (ids[cb[i]:cb[i + 1]], ratios[cb[i]:cb[i + 1]], acc[ab[i]:ab[i + 1]]) for i, c in enumerate(self.ssv_ids.tolist())}


def mapping_thresholds(obj_type: str, config=None):
    """``(lower ratio, upper ratio, size threshold)`` of `obj_type` from ``config['cell_objects']`` with the reference's errors
    (ssd_proc.py:151-172): a missing lower ratio or size threshold raises ``ValueError``, a missing upper ratio is 1."""
    if config is None:
        from .. import global_params
        config = global_params.config
    cell_objects_dc = config['cell_objects']
    try:
        lower_ratio = cell_objects_dc["lower_mapping_ratios"][obj_type]
    except KeyError:
        raise ValueError("Lower ratio undefined.")
    try:
        upper_ratio = cell_objects_dc["upper_mapping_ratios"][obj_type]
    except KeyError:
        upper_ratio = 1.
    try:
        sizethreshold = cell_objects_dc["sizethresholds"][obj_type]
    except KeyError:
        raise ValueError("Size threshold undefined.")
    return float(lower_ratio), float(upper_ratio), float(sizethreshold)


def map_organelle(cells: CellLists, map_table, organelle_props, lower_ratio: float, upper_ratio: float, sizethreshold: float, device=None) -> CellMapping:
    """``sd_cell_mapping`` for one organelle kind: `map_table` a ``MapTable`` (organelle id, supervoxel id, voxels), `organelle_props` its
    ``PropTable`` (ids ascending, sizes).  See ``CellMapping``."""
    what = 'map_organelle'
    dev = D.device(device)
    sub, sv = _u64(f'{what}: organelle ids of the records', map_table.sub_ids), _u64(f'{what}: supervoxel ids of the records', map_table.cell_ids)
    cnt = np.ascontiguousarray(np.asarray(map_table.counts).reshape(-1), dtype=np.int64)
    org_ids = _u64(f'{what}: organelle ids', organelle_props.ids)
    org_sizes = np.ascontiguousarray(np.asarray(organelle_props.sizes).reshape(-1), dtype=np.int64)
    if not (len(sub) == len(sv) == len(cnt)) or len(org_ids) != len(org_sizes):
        raise ValueError(f'{what}: columns of unequal length')
    if len(org_ids) > 1 and not (org_ids[1:] > org_ids[:-1]).all():
        raise ValueError(f'{what}: organelle ids must ascend strictly')
    if len(org_sizes) and org_sizes.min() <= 0:
        raise ValueError(f'{what}: organelle sizes must be positive')
    for name, v in (('lower_ratio', lower_ratio), ('upper_ratio', upper_ratio), ('sizethreshold', sizethreshold)):
        if np.isnan(float(v)):
            raise ValueError(f'{what}: {name} is NaN')
    r, o, n, s = len(sub), len(org_ids), len(cells), len(cells.sv_ids)
    cell_begin, pair_org, acc_begin, acc_org = (D.empty(k, D.i64, dev) for k in (n + 1, r, n + 1, r))
    ratio, accepted = D.empty(r, D.f64, dev), D.empty(r, D.u8, dev)
    org_n, org_first = D.empty(o, D.i32, dev), D.empty(o, D.i32, dev)
    counts_d = D.counters(dev)
    tmp = D.scratch('sd_cell_mapping_temp_bytes', dev, r, s)
    d = [D.up(a, dev) for a in (sub, sv, cnt, org_ids, org_sizes, cells.sv_begin, cells.sv_ids)]
    D.call('sd_cell_mapping', dev, d[0], d[1], d[2], r, d[3], d[4], o, d[5], d[6], n, s, float(lower_ratio), float(upper_ratio), float(sizethreshold),
           cell_begin, pair_org, ratio, accepted, acc_begin, acc_org, org_n, org_first, counts_d, tmp, tmp.numel())
    counts = D.down(counts_d)
    if int(counts[6]):
        raise ValueError(f'{what}: a supervoxel is in two cells, or 0 is in one')
    if int(counts[7]):
        raise ValueError(f'{what}: the cell lists or the organelle table are inconsistent')
    n_pairs, n_acc = int(counts[1]), int(counts[2])
    first = D.down(org_first, o, np.uint32)
    first_id = np.zeros(o, np.uint64)
    has = first != 0xffffffff
    first_id[has] = cells.ssv_ids[first[has]]
    return CellMapping(ssv_ids=cells.ssv_ids, org_ids=org_ids, cell_begin=D.down(cell_begin, n + 1), ids=D.down(pair_org, n_pairs, np.uint64),
                       ratios=D.down(ratio, n_pairs), accepted=D.down(accepted, n_pairs).astype(bool), acc_begin=D.down(acc_begin, n + 1),
                       acc_ids=D.down(acc_org, n_acc, np.uint64), org_n_cells=D.down(org_n, o, np.uint32).astype(np.int64),
                       org_first_cell=first_id, n_records=int(counts[0]))


def aggregate_segmentation_object_mappings(cells: CellLists, map_tables: dict, organelle_props: dict, obj_types: Optional[Sequence[str]] = None,
                                           device=None) -> Dict[str, CellMapping]:
    """``aggregate_segmentation_object_mappings`` (:28-91) over tables: per object type the summed overlap ratios of every (cell,
    organelle) pair -- ``mapping_{obj}_ids`` / ``mapping_{obj}_ratios`` of every cell.  No decision is made: nothing is accepted."""
    obj_types = list(map_tables) if obj_types is None else list(obj_types)
    return {k: map_organelle(cells, map_tables[k], organelle_props[k], np.inf, 1., np.inf, device) for k in obj_types}


def apply_mapping_decisions(cells: CellLists, map_tables: dict, organelle_props: dict, obj_types: Optional[Sequence[str]] = None, config=None,
                            device=None) -> Dict[str, CellMapping]:
    """``apply_mapping_decisions`` (:94-279) over tables: the summed ratios and, with the thresholds of ``config['cell_objects']``, the
    organelles every cell accepts (``ratio > lower``, ``ratio <= upper`` unless ``upper >= 1``, ``size > sizethreshold``)."""
    obj_types = list(map_tables) if obj_types is None else list(obj_types)
    thresholds = {k: mapping_thresholds(k, config) for k in obj_types}
    return {k: map_organelle(cells, map_tables[k], organelle_props[k], *thresholds[k], device=device) for k in obj_types}


def organelle_cells(mapping: CellMapping) -> np.ndarray:
    """The ``cells`` column of an ``OrganelleTable``: per organelle of the table the cell that accepted it, 0 = none.  Raises
    ``ValueError`` where two cells accepted one organelle (possible for lower ratios below 0.5, e.g. ``sj`` with 0.1)."""
    twice = np.flatnonzero(mapping.org_n_cells > 1)
    if len(twice):
        raise ValueError(f'organelle_cells: {len(twice)} organelles are accepted by more than one cell, e.g. {int(mapping.org_ids[twice[0]])}')
    return mapping.org_first_cell.copy()


class CellSynapses:
    """``syn_begin`` int64 (n_cells + 1) into ``syn_ids`` uint64: the ``syn_ssv`` attribute of every cell."""

    def __init__(self, syn_begin, syn_ids):
        self.syn_begin, self.syn_ids = syn_begin, syn_ids


def map_synssv_objects(cells: CellLists, neuron_partners, syn_prob, syn_ids, syn_threshold=None, device=None) -> CellSynapses:
    """``map_synssv_objects_thread`` (:315-342) without the meshes: of the synapses with ``syn_prob > syn_threshold`` every cell lists
    those with it in slot 0 of `neuron_partners`, in row order, then those with it in slot 1 (a synapse of a cell with itself
    appears twice).  The comparison is numpy's, in the dtype of `syn_prob`, as in the reference."""
    what = 'map_synssv_objects'
    if syn_threshold is None:
        from .. import global_params
        syn_threshold = global_params.config['cell_objects']['thresh_synssv_proba']
    partners = _u64(f'{what}: neuron_partners', neuron_partners, cols=2)
    ids = _u64(f'{what}: syn_ids', syn_ids)
    prob = np.asarray(syn_prob).reshape(-1)
    if not (len(partners) == len(ids) == len(prob)):
        raise ValueError(f'{what}: {len(partners)} partner rows, {len(ids)} ids, {len(prob)} probabilities')
    keep = np.ascontiguousarray(prob > syn_threshold, dtype=np.uint8)
    dev = D.device(device)
    n, n_cells = len(ids), len(cells)
    begin, out = D.empty(n_cells + 1, D.i64, dev), D.empty(2 * n, D.i64, dev)
    counts_d = D.counters(dev)
    tmp = D.scratch('sd_cell_synapses_temp_bytes', dev, n)
    d = [D.up(a, dev) for a in (partners, keep, ids, cells.ssv_ids)]
    D.call('sd_cell_synapses', dev, d[0], d[1], d[2], n, d[3], n_cells, begin, out, counts_d, tmp, tmp.numel())
    counts = D.down(counts_d)
    if int(counts[7]):
        raise ValueError(f'{what}: the cell ids do not ascend')
    return CellSynapses(D.down(begin), D.down(out, int(counts[0]), np.uint64))
