"""Synapse agglomeration on the MI355X: the device form of ``combine_and_split_syn`` of
/root/reference/syconn/extraction/cs_processing_steps.py (:239-602), the call that follows ``extract_contact_sites`` in the reference's
``exec_syns.py`` (:111-116) and turns the supervoxel-level ``syn`` fragments into the cell-level synapses (``syn_ssv``).

``filter_relevant_syn`` (numpy, :260-317) groups the fragments by cell pair; ``connected_cluster`` is the array form of
``connected_cluster_kdtree`` (:552-602) for one group; ``combine_and_split_syn`` runs all groups of a ``SynTable`` through one set of
launches (``csrc/sd_syn_ssv.hip``: components, then per-component statistics) and finishes on the host with the reference's own
arithmetic on a few values per synapse (:458-509).  Where this departs from the reference -- no ``dist_inter_object`` prefilter, a
lower bound on the gap, all voxels for ``rep_coord``, no meshes, storages or ids -- is written down in DESIGN.md section 7.
There is no CPU fallback for the device parts.

``map_objects_from_synssv_partners`` (:811-1093), the call after it, maps the mitochondria and vesicle clouds of the two partner cells
to every ``syn_ssv`` row (``csrc/sd_synssv_map.hip``) and ``synssv_o_features`` (:1404-1431) lays out the classifier's feature rows.
"""
import numpy as np

from .. import _lib as L

# the 32 offsets of the reference's first stage (``query_pairs(r=2)`` on voxel coordinates, :581): dx^2 + dy^2 + dz^2 <= 4
_R2_OFFSETS = np.array([(x, y, z) for x in range(-2, 3) for y in range(-2, 3) for z in range(-2, 3) if 0 < x * x + y * y + z * z <= 4])


def min_gap_nm(scaling) -> float:
    """The longest scaled length of the first-stage offsets.  A gap above it makes the reference's same-fragment edges (voxel
    distance <= 2) a subset of its gap edges, so that one edge rule describes the partition."""
    s = np.asarray(scaling, np.float64)
    return float(np.sqrt(((_R2_OFFSETS * s) ** 2).sum(1)).max())


def _check_gap(cs_gap_nm, scaling):
    s = np.asarray(scaling, np.float64).reshape(-1)
    if s.shape != (3,) or not np.all(s > 0):
        raise ValueError(f'scaling must be three positive voxel sizes, got {scaling}')
    gap = float(cs_gap_nm)
    if not gap > min_gap_nm(s):
        raise ValueError(f'cs_gap_nm = {gap} must exceed {min_gap_nm(s)} nm, the longest scaled offset within two voxels at scaling '
                         f'{s.tolist()}: below it the reference joins voxels of one fragment that the gap would not')
    return gap, s


def _check_scaling32(scaling):
    """Three positive voxel sizes as the float32 that ``SegmentationDataset.scaling`` / ``SuperSegmentationObject.scaling`` hold
    (segmentation.py:1747), widened to float64 as numpy widens them in a product.  (``_check_gap`` is a different rule on purpose:
    it evaluates ``min_gap_nm`` and the binning cell on the float64 values the caller gives.)"""
    scale = np.asarray(scaling, np.float32).reshape(-1).astype(np.float64)
    if scale.shape != (3,) or not np.all(scale > 0):
        raise ValueError(f'scaling must be three positive voxel sizes, got {scaling}')
    return scale


def _check_positive_int(**named):
    for name, v in named.items():
        if isinstance(v, bool) or int(v) != v or int(v) < 1:
            raise ValueError(f'{name} must be an integer >= 1, got {v!r}')


def choose_cell(scaling, cs_gap_nm):
    """The binning cell (voxels per axis) of the component search: per axis the largest extent whose share of the scaled diagonal is
    gap / sqrt(3), shrunk until ``||(c - 1) * scaling||`` (float64) is strictly below the gap -- all voxels of a group inside one cell
    are then connected without a test.  The largest such cell keeps the neighbourhood a wave has to walk smallest."""
    gap, s = _check_gap(cs_gap_nm, scaling)
    c = np.maximum(np.floor(gap / (np.sqrt(3.0) * s)).astype(np.int64), 0) + 1
    while not np.sqrt((((c - 1) * s) ** 2).sum()) < gap:
        a = int(np.argmax((c - 1) * s))
        c[a] -= 1
    return c


def _mapping_arrays(sv_ids, ssv_ids):
    if ssv_ids is None:                                    # a dict sv -> ssv
        items = sorted(dict(sv_ids).items())
        sv = np.array([k for k, _ in items], np.uint64)
        ssv = np.array([v for _, v in items], np.int64)
    else:
        sv, ssv = np.asarray(sv_ids).astype(np.uint64), np.asarray(ssv_ids).astype(np.int64)
        if sv.shape != ssv.shape or sv.ndim != 1:
            raise ValueError('sv_ids and ssv_ids must be two 1D arrays of equal length')
        order = np.argsort(sv, kind='stable')
        sv, ssv = sv[order], ssv[order]
    if len(sv) > 1 and np.any(sv[1:] == sv[:-1]):
        raise ValueError('a supervoxel id occurs twice in the sv -> ssv mapping')
    return sv, ssv


def filter_relevant_syn(syn_ids, sv_ids, ssv_ids=None):
    """``filter_relevant_syn`` (:260-317) for ``syn`` objects, on arrays: the partner supervoxels of every id are decoded as
    ``cs_id_to_partner_ids_vec`` does (``id >> 32``, the rest), a supervoxel above the largest mapped id becomes 0, every supervoxel is
    mapped to its cell (unmapped: 0), rows whose two cells are both > 0 and differ are kept and keyed by ``(max << 32) + min``.
    The sv -> ssv mapping is two arrays, or a dict as `sv_ids`.

    -> ``(enc_keys, group_begin, syn_rows)``: the keys in order of first appearance (uint64), offsets (groups + 1) into `syn_rows`,
    and the rows of `syn_ids` group by group, in input order inside a group -- the reference's ``defaultdict(list)`` as arrays."""
    ids = np.asarray(syn_ids).astype(np.uint64).reshape(-1)
    sv_map, ssv_map = _mapping_arrays(sv_ids, ssv_ids)
    hi = ids >> np.uint64(32)
    sv = np.stack([hi, ids - (hi << np.uint64(32))], 1)
    if len(sv_map):
        sv[sv > sv_map[-1]] = 0
        at = np.minimum(np.searchsorted(sv_map, sv), len(sv_map) - 1)
        mapped = np.where(sv_map[at] == sv, ssv_map[at], 0)
    else:
        mapped = np.zeros(sv.shape, np.int64)
    rows = np.flatnonzero(np.all(mapped > 0, axis=1) & (mapped[:, 0] != mapped[:, 1]))
    pairs = mapped[rows].astype(np.uint64)
    enc = (pairs.max(1) << np.uint64(32)) + pairs.min(1) if len(rows) else np.zeros(0, np.uint64)
    uniq, first, inv = np.unique(enc, return_index=True, return_inverse=True)
    rank_of_uniq = np.empty(len(uniq), np.int64)
    appearance = np.argsort(first, kind='stable')
    rank_of_uniq[appearance] = np.arange(len(uniq))
    rank = rank_of_uniq[inv.reshape(-1)]
    order = np.argsort(rank, kind='stable')
    group_begin = np.concatenate(([0], np.cumsum(np.bincount(rank, minlength=len(uniq))))).astype(np.int64)
    return uniq[appearance], group_begin, rows[order].astype(np.int64)


class SynSsvTable:
    """Cell-level synapses that passed ``min_obj_vx['syn_ssv']`` (plain numpy), in the reference's processing order: groups (cell pairs)
    in first-appearance order, the components of a group in ascending order of their smallest flat voxel index.

    ``neuron_partners`` (n, 2) uint64 = (larger, smaller) cell id; ``sizes`` int64; ``rep_coords`` (n, 3) int32; ``bounding_boxes``
    (n, 2, 3) int32 = [min, max] inclusive; ``voxels`` (v, 3) uint32 / ``vox_begin`` (n + 1), ascending flat index inside a row;
    ``cs_ids`` uint64 / ``cs_begin`` (n + 1) = the fragment ids the reference aggregates (its ``synix_list`` indexing unless
    ``reference_indexing=False``); ``frag_ids`` / ``frag_counts`` / ``frag_begin`` = the fragments that really contribute and their exact
    voxel counts, whatever the indexing; ``sym_prop``, ``asym_prop``, ``syn_type_sym_ratio`` float64, ``syn_sign`` int64;
    ``ordinal`` int64 = the row's count among ALL components of the run before the size filter (dropped components consume an id
    in the reference), ``group`` / ``group_ordinal`` = the row's group and its count inside that group."""

    COLUMNS = ('neuron_partners', 'sizes', 'rep_coords', 'bounding_boxes', 'voxels', 'vox_begin', 'cs_ids', 'cs_begin', 'frag_ids',
               'frag_counts', 'frag_begin', 'sym_prop', 'asym_prop', 'syn_type_sym_ratio', 'syn_sign', 'ordinal', 'group', 'group_ordinal')

    def __init__(self, **columns):
        for name in self.COLUMNS:
            setattr(self, name, columns[name])
        self.n_components = int(columns.get('n_components', len(self.sizes)))     # before the size filter

    def __len__(self):
        return len(self.sizes)

    def as_dict(self) -> list:
        """One attribute dict per row with the keys ``_combine_and_split_syn_thread`` stores (:470-513) except the mesh entries:
        ``neuron_partners``, ``rep_coord`` (int32), ``bounding_box`` (uint32, as ``np.min`` / ``np.max`` of the voxel cache), ``size``,
        ``cs_ids`` (list), ``sym_prop``, ``asym_prop``, ``syn_type_sym_ratio``, ``syn_sign``; and ``voxels``, what it puts into the voxel
        storage."""
        c, v = self.cs_begin.tolist(), self.vox_begin.tolist()
        bb = self.bounding_boxes.astype(np.uint32)
        out = []
        for i in range(len(self)):
            ratio = self.syn_type_sym_ratio[i]
            out.append(dict(neuron_partners=self.neuron_partners[i], rep_coord=self.rep_coords[i], bounding_box=bb[i],
                            size=int(self.sizes[i]), cs_ids=self.cs_ids[c[i]:c[i + 1]].tolist(), sym_prop=self.sym_prop[i],
                            asym_prop=self.asym_prop[i], syn_type_sym_ratio=-1 if ratio == -1 else ratio,
                            syn_sign=int(self.syn_sign[i]), voxels=self.voxels[v[i]:v[i + 1]]))
        return out


def build_syn_ssv_table(enc_keys, group_frag_begin, frag_ids, frag_sym_prop, frag_asym_prop, comp_group, comp_sizes, comp_bbox, comp_rep_vox,
                        pair_comp, pair_frag, pair_cnt, voxels, scaling, min_obj_vx: int, sym_thresh: float, reference_indexing: bool = True):
    """The host edge (:458-509), numpy only: from the per-component statistics of ALL components (in processing order: `comp_group`,
    `comp_sizes`, `comp_bbox` (k, 2, 3), `comp_rep_vox` (k, 3) = the voxel nearest the centre of mass), the voxel count of every
    (component, fragment) that occurs (`pair_comp` ascending, `pair_frag` = fragment number over all groups, ascending inside a
    component) and the voxel rows of the kept components, to the ``SynSsvTable``.  The fragments' attributes come group by group
    (`group_frag_begin` offsets into `frag_ids` / `frag_sym_prop` / `frag_asym_prop`).

    The weights ``cnt / np.sum(cnt)``, ``np.sum(w * props)``, the ratio and the sign are the reference's expressions.  With
    `reference_indexing` fragment j of a group is looked up as ``max(j - 1, 0)``, as the reference's ``synix_list`` has it (:434-440):
    fragments 0 and 1 share fragment 0's attributes and fold their counts, the last fragment's attributes are never read."""
    enc_keys = np.asarray(enc_keys, np.uint64)
    gfb = np.asarray(group_frag_begin, np.int64)
    frag_ids = np.asarray(frag_ids, np.uint64)
    frag_sym_prop, frag_asym_prop = np.asarray(frag_sym_prop, np.float64), np.asarray(frag_asym_prop, np.float64)
    comp_group, comp_sizes = np.asarray(comp_group, np.int64), np.asarray(comp_sizes, np.int64)
    pair_comp, pair_frag, pair_cnt = np.asarray(pair_comp, np.int64), np.asarray(pair_frag, np.int64), np.asarray(pair_cnt, np.int64)
    scaling = np.asarray(scaling, np.float32)               # SegmentationDataset.scaling is float32 (segmentation.py:1747)
    K = len(comp_sizes)
    keep = comp_sizes >= int(min_obj_vx)                    # :462 ``np.sum(cnt) < min_obj_vx -> continue``
    rows = np.flatnonzero(keep)
    n = len(rows)
    row_of_comp = np.full(K, -1, np.int64)
    row_of_comp[rows] = np.arange(n)
    first_of_group = np.concatenate(([0], np.cumsum(np.bincount(comp_group, minlength=len(enc_keys)))))[:-1] if K else np.zeros(0, np.int64)
    # the pairs of the kept rows
    pk = keep[pair_comp] if len(pair_comp) else np.zeros(0, bool)
    p_row, p_frag, p_cnt = row_of_comp[pair_comp[pk]], pair_frag[pk], pair_cnt[pk]
    frag_begin = np.concatenate(([0], np.cumsum(np.bincount(p_row, minlength=n)))).astype(np.int64)
    # the index the reference reads the attributes at
    j = p_frag - gfb[comp_group[rows]][p_row] if n else np.zeros(0, np.int64)
    ix = np.maximum(j - 1, 0) if reference_indexing else j
    head = np.ones(len(ix), bool)
    if len(ix) > 1:
        head[1:] = (p_row[1:] != p_row[:-1]) | (ix[1:] != ix[:-1])
    starts = np.flatnonzero(head)
    a_row, a_ix = p_row[starts], (ix + gfb[comp_group[rows]][p_row])[starts] if n else np.zeros(0, np.int64)
    a_cnt = np.add.reduceat(p_cnt, starts) if len(starts) else np.zeros(0, np.int64)       # np.unique(..., return_counts=True)
    cs_begin = np.concatenate(([0], np.cumsum(np.bincount(a_row, minlength=n)))).astype(np.int64)
    sym, asym = np.zeros(n, np.float64), np.zeros(n, np.float64)
    m = np.diff(cs_begin)
    one = np.flatnonzero(m == 1)                             # a single entry: weight cnt / cnt = 1.0, the sum of one product is itself
    sym[one], asym[one] = frag_sym_prop[a_ix[cs_begin[one]]], frag_asym_prop[a_ix[cs_begin[one]]]
    for r in np.flatnonzero(m != 1).tolist():
        sl = slice(cs_begin[r], cs_begin[r + 1])
        this_syn_ids_cnt = a_cnt[sl]
        this_agg_syn_weights = this_syn_ids_cnt / np.sum(this_syn_ids_cnt)
        sym[r] = np.sum(this_agg_syn_weights * np.array(frag_sym_prop[a_ix[sl]].tolist()))
        asym[r] = np.sum(this_agg_syn_weights * np.array(frag_asym_prop[a_ix[sl]].tolist()))
    zero = sym + asym == 0
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(zero, -1.0, sym / (asym + sym))
    sign = np.where(ratio > sym_thresh, -1, 1).astype(np.int64)
    rep_vox = np.asarray(comp_rep_vox)[rows].astype(np.uint32).reshape(n, 3)
    rep = (rep_vox * scaling // scaling).astype(np.int32)    # :472 on the chosen voxel
    hi = enc_keys[comp_group[rows]] >> np.uint64(32)
    partners = np.stack([hi, enc_keys[comp_group[rows]] - (hi << np.uint64(32))], 1) if n else np.zeros((0, 2), np.uint64)
    sizes = comp_sizes[rows]
    return SynSsvTable(neuron_partners=partners, sizes=sizes, rep_coords=rep, bounding_boxes=np.asarray(comp_bbox, np.int32).reshape(K, 2, 3)[rows],
                       voxels=np.asarray(voxels, np.uint32).reshape(-1, 3), vox_begin=np.concatenate(([0], np.cumsum(sizes))).astype(np.int64),
                       cs_ids=frag_ids[a_ix], cs_begin=cs_begin, frag_ids=frag_ids[p_frag], frag_counts=p_cnt, frag_begin=frag_begin,
                       sym_prop=sym, asym_prop=asym, syn_type_sym_ratio=ratio, syn_sign=sign, ordinal=rows.astype(np.int64),
                       group=comp_group[rows], group_ordinal=rows - first_of_group[comp_group[rows]] if n else np.zeros(0, np.int64),
                       n_components=K)


# ---- the device part ------------------------------------------------------------------------------------------------------------------
class _Agglomerator:
    """The launches of ``csrc/sd_syn_ssv.hip`` over one flat voxel array: `vox` (N, 3) int32 in the reference's flat order, `vox_frag` (N)
    the fragment number of every voxel (ascending), `frag_group` (F) the group of every fragment.  The voxel rows are uploaded once."""

    def __init__(self, vox, vox_frag, frag_group, n_group, scaling, cs_gap_nm, device=None):
        from .. import _dev as D
        self.gap, self.scale = _check_gap(cs_gap_nm, scaling)
        self.lib, self.dev = L.load(), D.device(device)
        vox = np.ascontiguousarray(vox, dtype=np.int32).reshape(-1, 3)
        self.n, self.n_frag, self.n_group = len(vox), len(frag_group), int(n_group)
        self.cell = choose_cell(self.scale, self.gap)
        self.counts = np.zeros(8, np.int64)
        if not self.n:
            return
        if self.n >= 2 ** 31:
            raise ValueError('combine_and_split_syn: fewer than 2^31 voxel rows per call')
        vox_frag = np.ascontiguousarray(vox_frag, dtype=np.uint32)
        frag_group = np.ascontiguousarray(frag_group, dtype=np.uint32)
        vgroup = frag_group[vox_frag]
        gstart = np.flatnonzero(np.concatenate(([True], vgroup[1:] != vgroup[:-1])))
        if len(gstart) != self.n_group or np.any(np.diff(vgroup.astype(np.int64)) < 0):
            raise ValueError('combine_and_split_syn: the voxels must come group by group, every group non-empty')
        lo, hi = np.minimum.reduceat(vox, gstart, axis=0), np.maximum.reduceat(vox, gstart, axis=0)
        n_cells = ((hi.astype(np.int64) - lo) // self.cell).max(0) + 1
        self.bits = np.array([int(v - 1).bit_length() for v in n_cells.tolist()], np.int32)
        if int(self.bits.sum()) + int(self.n_group - 1).bit_length() > 63:
            raise ValueError(f'combine_and_split_syn: {self.n_group} groups spanning up to {n_cells.tolist()} cells do not fit a 63-bit key')
        self.vox_d, self.frag_d, self.fgroup_d, self.origin_d = (D.up(a, self.dev) for a in (vox, vox_frag, frag_group, lo))
        self.tmp = D.scratch('sd_syn_ssv_temp_bytes', self.dev, self.n)
        self.labels_d = D.empty(self.n, D.i32, self.dev)
        self.counts_d = D.counters(self.dev)
        self._scale_c, self._cell_c, self._bits_c = D.f64x3(self.scale), D.i32x3(self.cell), D.i32x3(self.bits)

    def components(self, stages: int = 7):
        """Launch the stages (bit 0 cells, bit 1 link, bit 2 number) on the current stream; asynchronous."""
        if not self.n:
            return
        import torch
        # written out, not through _dev.call: the first stage's device span starts with this call's host time (profiles/hostcall_ab_probe.json)
        L.check(self.lib.sd_syn_ssv_components(self.vox_d.data_ptr(), self.frag_d.data_ptr(), self.fgroup_d.data_ptr(), self.origin_d.data_ptr(),
                                               self.n, self.n_frag, self.n_group, self._scale_c, self.gap, self._cell_c, self._bits_c,
                                               int(stages), self.labels_d.data_ptr(), self.counts_d.data_ptr(), self.tmp.data_ptr(),
                                               self.tmp.numel(), torch.cuda.current_stream(self.dev).cuda_stream), 'sd_syn_ssv_components')

    def read_counts(self):
        """-> counts of ``sd_syn_ssv_components`` on the host (waits for the device)."""
        if self.n:
            self.counts = self.counts_d.cpu().numpy()
            if self.counts[7]:
                raise RuntimeError('sd_syn_ssv_components: a voxel row was outside its group box or fragment table')
        return self.counts

    def labels(self) -> np.ndarray:
        return self.labels_d.cpu().numpy() if self.n else np.zeros(0, np.int32)

    def stats(self, min_obj_vx: int):
        """Per-component statistics of all `n_comp` components and the voxel rows of the kept ones (waits for the device).
        -> dict of numpy arrays for ``build_syn_ssv_table``."""
        from .. import _dev as D
        dev, n = self.dev, self.n
        K = int(self.counts[0])
        if not n:
            z = np.zeros(0, np.int64)
            return dict(comp_sizes=z, comp_bbox=np.zeros((0, 2, 3), np.int32), comp_rep_flat=z, pair_comp=z, pair_frag=z, pair_cnt=z,
                        voxels=np.zeros((0, 3), np.uint32))
        new = lambda m: D.empty(m, D.i32, dev)
        comp_begin, bbox, rep = new(K + 1), new((K, 6)), new(K)
        p_comp, p_frag, p_begin, vout = new(n + 1), new(n + 1), new(n + 1), new((n, 3))
        cnt = D.counters(dev, 4)
        D.call('sd_syn_ssv_stats', dev, self.vox_d, self.frag_d, self.labels_d, n, K, self._scale_c, int(min_obj_vx), comp_begin, bbox, rep,
               p_comp, p_frag, p_begin, vout, cnt, self.tmp, self.tmp.numel())
        P, n_kept, _, bad = (int(v) for v in D.down(cnt))
        if bad:
            raise RuntimeError('sd_syn_ssv_stats: a component label was out of range')
        u = lambda t, m=None: D.down(t, m, np.uint32).astype(np.int64)
        begin = u(comp_begin)
        pb = u(p_begin, P + 1)
        return dict(comp_sizes=np.diff(begin), comp_bbox=D.down(bbox).reshape(K, 2, 3), comp_rep_flat=u(rep), pair_comp=u(p_comp, P),
                    pair_frag=u(p_frag, P), pair_cnt=np.diff(pb), voxels=D.down(vout, n_kept, np.uint32))


def _flatten(voxel_lists):
    lists = [np.asarray(v).reshape(-1, 3) for v in voxel_lists]
    vox = np.concatenate(lists).astype(np.int64) if lists else np.zeros((0, 3), np.int64)
    if len(vox) and (vox.min() < -2 ** 31 or vox.max() >= 2 ** 31):
        raise ValueError('voxel coordinates must fit int32')
    return vox.astype(np.int32), np.repeat(np.arange(len(lists), dtype=np.uint32), [len(v) for v in lists])


def connected_cluster(voxel_lists, cs_gap_nm, scaling, device=None) -> np.ndarray:
    """The array form of ``connected_cluster_kdtree(voxel_lists, dist_intra_object=cs_gap_nm, dist_inter_object=20000, scale=scaling)``
    (:552-602) for one group: `voxel_lists` = one (n_i, 3) voxel array per fragment.  -> int32 component number of every voxel of
    ``np.concatenate(voxel_lists)``; components are numbered in ascending order of their smallest flat index, the order of the
    reference's list of sets.  Two voxels are joined when their scaled distance is strictly below `cs_gap_nm`; there is no
    ``dist_inter_object`` prefilter.  Raises ValueError for a gap that does not exceed ``min_gap_nm(scaling)``."""
    _check_gap(cs_gap_nm, scaling)
    vox, vfrag = _flatten(voxel_lists)
    if not len(vox):
        return np.zeros(0, np.int32)
    agg = _Agglomerator(vox, vfrag, np.zeros(len(voxel_lists), np.uint32), 1, scaling, cs_gap_nm, device)
    agg.components()
    agg.read_counts()
    return agg.labels()


def combine_and_split_syn(syn_table, sv_ids, ssv_ids=None, scaling=None, cs_gap_nm=None, min_obj_vx=None, sym_thresh=None,
                          reference_indexing: bool = True, device=None, return_stats: bool = False):
    """``combine_and_split_syn`` (:320-387) with its worker ``_combine_and_split_syn_thread`` (:390-549) on the ``SynTable`` that
    ``extract_contact_sites(as_tables=True)`` returns: the fragments are grouped by cell pair (``filter_relevant_syn``; `sv_ids` /
    `ssv_ids` = the supervoxel -> cell mapping as two arrays, or a dict as `sv_ids`), the voxels of every pair are split into
    components closer than `cs_gap_nm` (all pairs in one set of launches), and every component with at least
    ``min_obj_vx['syn_ssv']`` voxels becomes a row of the returned ``SynSsvTable``.  `scaling` falls back to ``config['scaling']``,
    `cs_gap_nm`, `min_obj_vx` (a dict or a number) and `sym_thresh` to ``config['cell_objects']``.  ``reference_indexing=False`` looks
    every fragment's attributes up at its own index instead of the reference's ``max(j - 1, 0)``.

    Not built: meshes (``mesh_bb``, ``mesh_area``), the storages, the id assignment (``ordinal`` is what it
    needs) and the batch jobs."""
    from .. import global_params
    cfg = global_params.config
    if scaling is None:
        scaling = cfg['scaling']
    cobj = cfg['cell_objects']
    cs_gap_nm = cobj['cs_gap_nm'] if cs_gap_nm is None else cs_gap_nm
    min_obj_vx = cobj['min_obj_vx'] if min_obj_vx is None else min_obj_vx
    min_vx = int(min_obj_vx['syn_ssv'] if isinstance(min_obj_vx, dict) else min_obj_vx)
    sym_thresh = cobj['sym_thresh'] if sym_thresh is None else sym_thresh
    gap, scale = _check_gap(cs_gap_nm, scaling)
    enc_keys, group_begin, syn_rows = filter_relevant_syn(syn_table.ids, sv_ids, ssv_ids)
    vb = np.asarray(syn_table.vox_begin, np.int64)
    run_start, run_len = vb[:-1][syn_rows], np.diff(vb)[syn_rows]
    if np.any(np.add.reduceat(run_len, group_begin[:-1]) == 0) if len(enc_keys) else False:
        raise ValueError('Voxels not available for syn-objects of a cell pair.')                     # :444-447
    begin = np.concatenate(([0], np.cumsum(run_len)))
    src = np.repeat(run_start - begin[:-1], run_len) + np.arange(begin[-1])
    vox = np.asarray(syn_table.voxels).reshape(-1, 3)[src]
    if len(vox) and int(vox.max()) >= 2 ** 31:
        raise ValueError('voxel coordinates must fit int32')
    vox_frag = np.repeat(np.arange(len(syn_rows), dtype=np.uint32), run_len)
    frag_group = np.repeat(np.arange(len(enc_keys), dtype=np.uint32), np.diff(group_begin))
    agg = _Agglomerator(vox.astype(np.int32), vox_frag, frag_group, len(enc_keys), scale, gap, device)
    agg.components()
    counts = agg.read_counts()
    st = agg.stats(min_vx)
    # the group of every component is the group of any of its voxels: take the representative
    comp_group = frag_group[vox_frag[st['comp_rep_flat']]].astype(np.int64) if agg.n else np.zeros(0, np.int64)
    table = build_syn_ssv_table(enc_keys, group_begin, np.asarray(syn_table.ids)[syn_rows], np.asarray(syn_table.sym_prop)[syn_rows],
                                np.asarray(syn_table.asym_prop)[syn_rows], comp_group, st['comp_sizes'], st['comp_bbox'],
                                vox[st['comp_rep_flat']] if agg.n else np.zeros((0, 3), np.uint32), st['pair_comp'], st['pair_frag'],
                                st['pair_cnt'], st['voxels'], scale, min_vx, float(sym_thresh), reference_indexing)
    if return_stats:
        return table, dict(counts=counts, cell=agg.cell, n_vox=agg.n, n_groups=len(enc_keys))
    return table


# ---- organelles of the partner cells, mapped to the cell-level synapses -----------------------------------------------------------------
# ``map_objects_from_synssv_partners`` of the reference (extraction/cs_processing_steps.py:811-1093), the call that follows
# ``combine_and_split_syn`` in ``exec_syns.run_syn_generation``, and the classifier's feature rows (``synssv_o_features``, :1404-1431).
# A *side* is (synapse row i, partner slot p) = 2 i + p; slot 0 is ``neuron_partners[i, 0]``, the larger cell id.
class OrganelleTable:
    """Objects of one organelle type (``mi``, ``vc``, ...), plain numpy: ``ids`` uint64 (m); ``cells`` uint64 (m) = the cell every
    object is assigned to (the reference's ``ssv_o.mi_ids`` / ``vc_ids`` read the other way round), 0 = none; ``sizes`` int64 (m) in
    voxels; ``rep_coords`` int32 (m, 3) in voxels; ``vertices`` float32 (W, 3) in nm = the mesh vertices of all objects
    (``mesh[1].reshape(-1, 3)``), object by object; ``vert_begin`` int64 (m + 1) = their offsets.  Shapes and offsets are checked."""

    def __init__(self, ids, cells, sizes, rep_coords, vertices, vert_begin):
        self.ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        m = len(self.ids)
        self.cells = np.ascontiguousarray(cells, dtype=np.uint64).reshape(-1)
        self.sizes = np.ascontiguousarray(sizes, dtype=np.int64).reshape(-1)
        self.rep_coords = np.ascontiguousarray(rep_coords, dtype=np.int32).reshape(-1, 3)
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        self.vert_begin = np.ascontiguousarray(vert_begin, dtype=np.int64).reshape(-1)
        if not (len(self.cells) == len(self.sizes) == len(self.rep_coords) == m):
            raise ValueError(f'OrganelleTable: {m} ids but {len(self.cells)} cells, {len(self.sizes)} sizes, {len(self.rep_coords)} rep_coords')
        _check_offsets('OrganelleTable: vert_begin', self.vert_begin, m, len(self.vertices))

    def __len__(self):
        return len(self.ids)


def _check_offsets(what, begin, n_rows, n_items):
    if len(begin) != n_rows + 1 or begin[0] != 0 or begin[-1] != n_items or np.any(np.diff(begin) < 0):
        raise ValueError(f'{what} must hold {n_rows + 1} ascending offsets from 0 to {n_items}')


class PairList:
    """The (side, organelle) pairs of one organelle type: ``side_begin`` int64 (2 n + 1) offsets of the sides, ``pair_obj`` int64 =
    organelle row (ascending inside a side), ``pair_close`` int64 = sampled vertices with a sampled synapse voxel strictly inside the
    radius, ``pair_len`` int64 = sampled vertices, ``pair_min_d2`` float64 = the smallest squared distance below the squared radius
    (inf if none)."""

    def __init__(self, side_begin, pair_obj, pair_close, pair_len, pair_min_d2):
        self.side_begin = np.asarray(side_begin, np.int64)
        self.pair_obj, self.pair_close = np.asarray(pair_obj, np.int64), np.asarray(pair_close, np.int64)
        self.pair_len, self.pair_min_d2 = np.asarray(pair_len, np.int64), np.asarray(pair_min_d2, np.float64)
        P = len(self.pair_obj)
        _check_offsets('PairList: side_begin', self.side_begin, len(self.side_begin) - 1, P)
        if not (len(self.pair_close) == len(self.pair_len) == len(self.pair_min_d2) == P) or len(self.side_begin) % 2 != 1:
            raise ValueError('PairList: columns of unequal length')

    @classmethod
    def empty(cls, n_syn):
        z = np.zeros(0, np.int64)
        return cls(np.zeros(2 * n_syn + 1, np.int64), z, z, z, np.zeros(0, np.float64))


class SynSsvMapping:
    """What ``map_objects_from_synssv_partners`` stores per synapse and partner: for every organelle type t ``n_{t}_objs`` and
    ``n_{t}_vxs`` int32 (n, 2) and ``min_dst_{t}_nm`` float32 (n, 2) (attributes; column p = partner slot p), and ``pairs[t]``, the
    ``PairList`` they were made from."""

    def __init__(self, n_syn, columns, pairs):
        self.n_syn, self.types, self.pairs = int(n_syn), tuple(columns), dict(pairs)
        for t, (n_objs, n_vxs, min_dst) in columns.items():
            setattr(self, f'n_{t}_objs', n_objs)
            setattr(self, f'n_{t}_vxs', n_vxs)
            setattr(self, f'min_dst_{t}_nm', min_dst)

    def __len__(self):
        return self.n_syn

    def as_dicts(self) -> list:
        """One dict per synapse with the keys ``_objects_from_cell_to_syn_dict`` (:1085-1090) adds to its attribute dict."""
        out = [dict() for _ in range(self.n_syn)]
        for t in self.types:
            cols = ((f'n_{t}_objs', getattr(self, f'n_{t}_objs')), (f'n_{t}_vxs', getattr(self, f'n_{t}_vxs')),
                    (f'min_dst_{t}_nm', getattr(self, f'min_dst_{t}_nm')))
            for i, d in enumerate(out):
                for p in (0, 1):
                    for name, col in cols:
                        d[f'{name}_{p}'] = col[i, p]
        return out


def build_synssv_mapping(n_syn: int, organelles: dict, pairs: dict) -> SynSsvMapping:
    """The host edge (:1040-1052 and :929-934), numpy only: from the pair list of every type (`pairs`: type -> ``PairList``) and the
    organelles' sizes and ids to the three columns per type.  Per side, over its pairs in list order: ``close_frac = close / len``,
    ``n_obj_vxs = np.array([close_frac * size, ...])``, ``n_objects = np.sum(n_obj_vxs > 0)``, ``n_vxs = np.sum(n_obj_vxs)`` stored
    into int32 (truncated), ``min_dist = sqrt(min d^2)`` if below 1e12 else 1e12, stored into float32.  A pair without vertices and
    an ``n_vxs`` of 2^31 or more raise ValueError (the reference fails on the first and is undefined on the second)."""
    columns = {}
    for t, pl in pairs.items():
        table = organelles[t]
        if len(pl.side_begin) != 2 * n_syn + 1:
            raise ValueError(f'{t}: side_begin holds {len(pl.side_begin)} offsets for {n_syn} synapses')
        n_objs, n_vxs = np.zeros(2 * n_syn, np.int32), np.zeros(2 * n_syn, np.int32)
        min_dst = np.full(2 * n_syn, 1e12, np.float32)
        if len(pl.pair_obj):
            if pl.pair_obj.min() < 0 or pl.pair_obj.max() >= len(table):
                raise ValueError(f'{t}: an organelle row of the pair list is outside the table')
            if np.any(pl.pair_len <= 0):
                o = int(pl.pair_obj[np.flatnonzero(pl.pair_len <= 0)[0]])
                raise ValueError(f'{t} object {int(table.ids[o])} (row {o}) is a candidate but has no mesh vertices')
            close_frac = pl.pair_close / pl.pair_len
            x = close_frac * table.sizes[pl.pair_obj]
            m = np.diff(pl.side_begin)
            sides = np.flatnonzero(m)
            total = np.zeros(len(sides), np.float64)
            single = m[sides] == 1                               # the sum of one term is the term
            total[single] = x[pl.side_begin[sides[single]]]
            for k in np.flatnonzero(~single).tolist():
                n_obj_vxs = x[pl.side_begin[sides[k]]:pl.side_begin[sides[k] + 1]]
                total[k] = np.sum(n_obj_vxs)
            if np.any(total >= 2.0 ** 31) or np.any(total <= -2.0 ** 31 - 1):
                s = int(sides[np.flatnonzero((total >= 2.0 ** 31) | (total <= -2.0 ** 31 - 1))[0]])
                raise ValueError(f'{t}: n_vxs of synapse {s // 2}, partner {s % 2} does not fit int32')
            n_vxs[sides] = total                                 # float64 into int32: truncated toward zero
            n_objs[sides] = np.add.reduceat((x > 0).astype(np.int64), pl.side_begin[sides])
            best = np.minimum.reduceat(pl.pair_min_d2, pl.side_begin[sides])
            dist = np.sqrt(best)
            min_dst[sides] = np.where(dist < 1e12, dist, 1e12)
        columns[t] = (n_objs.reshape(n_syn, 2), n_vxs.reshape(n_syn, 2), min_dst.reshape(n_syn, 2))
    return SynSsvMapping(n_syn, columns, pairs)


def synssv_o_featurenames() -> list:
    """:1427-1431."""
    return ['size_vx', 'mesh_area_um2', 'n_mi_objs_neuron1', 'n_mi_vxs_neuron1', 'min_dst_mi_nm_neuron1', 'n_vc_objs_neuron1',
            'n_vc_vxs_neuron1', 'min_dst_vc_nm_neuron1', 'n_mi_objs_neuron2', 'n_mi_vxs_neuron2', 'min_dst_mi_nm_neuron2',
            'n_vc_objs_neuron2', 'n_vc_vxs_neuron2', 'min_dst_vc_nm_neuron2']


def synssv_o_features(syn_ssv, mapping: SynSsvMapping, mesh_area) -> np.ndarray:
    """``synssv_o_features`` (:1404-1424) for every row of `syn_ssv`: float64 (n, 14) in the order of ``synssv_o_featurenames``.
    `mesh_area` (n) is an input, this package builds no meshes.  Needs the types ``mi`` and ``vc``."""
    missing = [t for t in ('mi', 'vc') if t not in mapping.types]
    if missing:
        raise ValueError(f'synssv_o_features needs the organelle types mi and vc, the mapping lacks {missing}')
    n = len(syn_ssv)
    area = np.asarray(mesh_area, np.float64).reshape(-1)
    if len(mapping) != n or len(area) != n:
        raise ValueError(f'{n} synapses, {len(mapping)} mapped rows, {len(area)} mesh areas')
    cols = [np.asarray(syn_ssv.sizes, np.float64), area]
    for p in (0, 1):
        for t in ('mi', 'vc'):
            cols += [getattr(mapping, f'n_{t}_objs')[:, p], getattr(mapping, f'n_{t}_vxs')[:, p], getattr(mapping, f'min_dst_{t}_nm')[:, p]]
    return np.stack([np.asarray(c, np.float64) for c in cols], 1) if n else np.zeros((0, 14), np.float64)


MAP_COUNT_NAMES = ('pairs', 'work_items', 'vertices_rejected', 'tiles_skipped', 'tiles_staged', 'point_tests')


class _ObjectMapper:
    """The launches of ``csrc/sd_synssv_map.hip`` over one ``SynSsvTable``: the voxel runs are uploaded once, their sampled, sorted
    and tiled form (``prepare``) serves every organelle type."""

    def __init__(self, syn_ssv, scale, sample_fact, device=None):
        from .. import _dev as D
        self.lib, self.dev = L.load(), D.device(device)
        self.scale, self.f = np.asarray(scale, np.float64), int(sample_fact)
        self.n = n = len(syn_ssv)
        partners = np.ascontiguousarray(syn_ssv.neuron_partners, dtype=np.uint64).reshape(n, 2)
        rep = np.ascontiguousarray(syn_ssv.rep_coords, dtype=np.int32).reshape(n, 3)
        vox = np.ascontiguousarray(syn_ssv.voxels, dtype=np.uint32).reshape(-1, 3)
        vb = np.ascontiguousarray(syn_ssv.vox_begin, dtype=np.int64).reshape(-1)
        _check_offsets('syn_ssv.vox_begin', vb, n, len(vox))
        svb = np.concatenate(([0], np.cumsum(-(-np.diff(vb) // self.f)))).astype(np.int64)
        self.n_vox, self.n_sv = len(vox), int(svb[-1])
        if 2 * n >= 2 ** 31 or self.n_sv >= 2 ** 31:
            raise ValueError('map_objects_from_synssv_partners: fewer than 2^30 synapses and 2^31 sampled voxels per call')
        self.cell_d, self.rep_d = D.up(partners.reshape(-1), self.dev), D.up(rep, self.dev)
        self.vox_d, self.vb_d, self.svb_d = D.up(vox, self.dev), D.up(vb, self.dev), D.up(svb, self.dev)
        self._scale_c = D.f64x3(self.scale)
        self.pair_tmp = D.scratch('sd_synssv_map_pairs_temp_bytes', self.dev, 2 * n)
        self.tmp, self.tmp_pairs, self.prepared = None, 0, False
        self.vox_counts_d = D.counters(self.dev)

    def candidates(self, table: OrganelleTable, max_rep_dist_nm: float, stage: int = 3):
        """The pair list of one type (both calls of ``sd_synssv_map_pairs``; waits for the count in between).  -> dict."""
        from .. import _dev as D
        n = self.n
        keep = np.flatnonzero(table.cells != 0)
        order = keep[np.argsort(table.cells[keep], kind='stable')]
        c = dict(table=table, m=len(order), P=0, side_begin=np.zeros(2 * n + 1, np.int64), pair_obj=np.zeros(0, np.int64))
        if not len(order):
            return c
        if len(table) >= 2 ** 31:
            raise ValueError('map_objects_from_synssv_partners: fewer than 2^31 organelles of one type per call')
        c['cell_d'], c['row_d'] = D.up(table.cells[order], self.dev), D.up(order.astype(np.uint32), self.dev)
        c['rep_d'] = D.up(table.rep_coords[order], self.dev)
        c['begin_d'] = D.empty(2 * n + 1, D.i32, self.dev)
        c['counts_d'] = D.counters(self.dev)
        c['D'] = float(max_rep_dist_nm)
        self.pairs_call(c, None)
        c['P'] = P = int(c['counts_d'][0].item())
        if P >= 2 ** 31:
            raise ValueError('map_objects_from_synssv_partners: fewer than 2^31 (side, organelle) pairs per type and call')
        c['side_begin'] = D.down(c['begin_d'], view=np.uint32).astype(np.int64)
        if P:
            c['obj_d'] = D.empty(P, D.i32, self.dev)
            self.pairs_call(c, c['obj_d'])
            c['pair_obj'] = D.down(c['obj_d'], view=np.uint32).astype(np.int64)
        return c

    def pairs_call(self, c, obj_d):
        from .. import _dev as D
        D.call('sd_synssv_map_pairs', self.dev, self.cell_d, self.rep_d, 2 * self.n, c['cell_d'], c['row_d'], c['rep_d'], c['m'], self._scale_c,
               c['D'], c['begin_d'], obj_d, 0 if obj_d is None else obj_d.numel(), c['counts_d'], self.pair_tmp, self.pair_tmp.numel())

    def reserve(self, n_pairs: int):
        """Scratch of the query for up to `n_pairs` pairs; a new allocation loses the prepared voxels."""
        if self.tmp is None or n_pairs > self.tmp_pairs:
            from .. import _dev as D
            self.tmp_pairs = int(n_pairs)
            self.tmp = D.scratch('sd_synssv_map_query_temp_bytes', self.dev, self.n, self.n_sv, self.tmp_pairs)
            self.prepared = False

    def _query_call(self, stages, R, c=None, out=None, counts_d=None, n_items=0):
        from .. import _dev as D
        z = lambda k: c[k] if c is not None else None
        t = c['table'] if c is not None else None
        D.call('sd_synssv_map_query', self.dev, self.vox_d, self.vb_d, self.svb_d, self.n, self.n_vox, self.n_sv, z('vert_d'), z('vtb_d'),
               len(t) if t is not None else 0, len(t.vertices) if t is not None else 0, z('begin_d'), z('obj_d'), c['P'] if c is not None else 0,
               self.tmp_pairs, self.f, self._scale_c, float(R), int(stages), int(n_items), *(out or (None,) * 3), counts_d, self.tmp,
               self.tmp.numel())

    def prepare(self):
        """Stage 1: the sampled voxels of all synapses, sorted and tiled, into the scratch (asynchronous)."""
        if self.tmp is None:
            self.reserve(1)
        self._query_call(1, 0.0, counts_d=self.vox_counts_d)
        self.prepared = True

    def query(self, c, max_vert_dist_nm: float):
        """Stage 2 for the pair list `c` of ``candidates`` (waits for the device).  -> (``PairList``, counts as a dict)."""
        from .. import _dev as D
        P, table = c['P'], c['table']
        if not P:
            return PairList.empty(self.n), dict.fromkeys(MAP_COUNT_NAMES, 0)
        n_vert = -(-np.diff(table.vert_begin) // self.f)
        plen = n_vert[c['pair_obj']]
        if np.any(plen == 0):
            o = int(c['pair_obj'][np.flatnonzero(plen == 0)[0]])
            raise ValueError(f'object {int(table.ids[o])} (row {o}) is a candidate but has no mesh vertices')
        if int(plen.max()) >= 2 ** 32:
            raise ValueError('map_objects_from_synssv_partners: fewer than 2^32 sampled vertices per organelle')
        n_items = int((-(-plen // L.SD_SYNSSV_MAP_ITEM)).sum())
        if n_items >= 2 ** 32:
            raise ValueError('map_objects_from_synssv_partners: fewer than 2^32 work items per type and call')
        self.reserve(P)
        if not self.prepared:
            self.prepare()
        if 'vert_d' not in c:
            c['vert_d'], c['vtb_d'] = D.up(table.vertices, self.dev), D.up(table.vert_begin, self.dev)
        out = (D.empty(P, D.i32, self.dev), D.empty(P, D.i32, self.dev), D.empty(P, D.i64, self.dev))
        counts_d = D.counters(self.dev)
        self._query_call(2, max_vert_dist_nm, c, out, counts_d, n_items)
        counts = D.down(counts_d)
        if counts[7] or int(D.down(self.vox_counts_d)[7]):
            raise RuntimeError('sd_synssv_map_query: an offset or an organelle row was out of range')
        u = lambda t: D.down(t, view=np.uint32).astype(np.int64)
        pl = PairList(c['side_begin'], c['pair_obj'], u(out[0]), u(out[1]), D.down(out[2], view=np.float64))
        if not np.array_equal(pl.pair_len, plen) or int(counts[1]) != n_items:
            raise RuntimeError('sd_synssv_map_query: the sampled vertex counts of the device differ from the host\'s')
        return pl, dict(zip(MAP_COUNT_NAMES, (int(v) for v in counts[:6])))


def map_objects_from_synssv_partners(syn_ssv, organelles: dict, scaling=None, max_vert_dist_nm=None, max_rep_coord_dist_nm=None,
                                     sample_fact: int = 2, device=None, return_stats: bool = False):
    """``map_objects_from_synssv_partners`` (:811-886) with its workers ``_map_objects_from_synssv_partners_thread`` (:888-1009),
    ``_map_objects_from_synssv`` (:1012-1052) and ``_objects_from_cell_to_syn_dict`` (:1055-1093) on the ``SynSsvTable`` that
    ``combine_and_split_syn`` returns (its ``neuron_partners``, ``rep_coords``, ``voxels`` and ``vox_begin``) and one
    ``OrganelleTable`` per type (`organelles`: type name -> table).  For every synapse, partner and type: the organelles of the
    partner cell whose representative coordinate is within `max_rep_coord_dist_nm` of the synapse's are candidates; of every
    candidate, every `sample_fact`-th mesh vertex is tested against every `sample_fact`-th voxel of the synapse (strictly inside
    `max_vert_dist_nm`: a dict by type, or a number).  `scaling` falls back to ``config['scaling']``, the distances to
    ``config['cell_objects']``.  -> ``SynSsvMapping`` (and with `return_stats` a dict with the device's counters per type).

    Not built: the meshes (vertices are an input), the ``cache_syn.pkl`` files, storages, batch jobs and the
    classifier.  No CPU fallback."""
    from .. import global_params
    cfg = global_params.config
    if scaling is None:
        scaling = cfg['scaling']
    cobj = cfg['cell_objects']
    max_vert_dist_nm = cobj['max_vert_dist_nm'] if max_vert_dist_nm is None else max_vert_dist_nm
    D = float(cobj['max_rep_coord_dist_nm'] if max_rep_coord_dist_nm is None else max_rep_coord_dist_nm)
    _check_positive_int(sample_fact=sample_fact)
    scale = _check_scaling32(scaling)
    radius = {}
    for t, table in organelles.items():
        if not isinstance(table, OrganelleTable):
            raise TypeError(f'organelles[{t!r}] must be an OrganelleTable')
        if isinstance(max_vert_dist_nm, dict):
            if t not in max_vert_dist_nm:
                raise ValueError(f'max_vert_dist_nm has no entry for {t!r}')
            radius[t] = float(max_vert_dist_nm[t])
        else:
            radius[t] = float(max_vert_dist_nm)
        if not (radius[t] >= 0 and np.isfinite(radius[t])):
            raise ValueError(f'max_vert_dist_nm[{t!r}] = {radius[t]}')
    if not (D >= 0 and np.isfinite(D)):
        raise ValueError(f'max_rep_coord_dist_nm = {D}')
    n = len(syn_ssv)
    _check_offsets('syn_ssv.vox_begin', np.asarray(syn_ssv.vox_begin, np.int64).reshape(-1), n, len(np.asarray(syn_ssv.voxels).reshape(-1, 3)))
    pairs = {t: PairList.empty(n) for t in organelles}
    stats = {t: dict.fromkeys(MAP_COUNT_NAMES, 0) for t in organelles}
    todo = [t for t, table in organelles.items() if n and np.any(table.cells != 0)]
    if todo:
        mapper = _ObjectMapper(syn_ssv, scale, sample_fact, device)
        cands = {t: mapper.candidates(organelles[t], D) for t in todo}
        mapper.reserve(max(c['P'] for c in cands.values()))
        for t in todo:
            try:
                pairs[t], stats[t] = mapper.query(cands[t], radius[t])
            except ValueError as e:
                raise ValueError(f'{t}: {e}') from None
    mapping = build_synssv_mapping(n, organelles, pairs)
    if return_stats:
        return mapping, stats
    return mapping


# -- classify_synssv_objects, collect_properties_from_ssv_partners, export_matrix (csrc/sd_syn_props.hip) ---------------------------------
class PackedForest:
    """A fitted random forest as flat arrays, the form ``sd_syn_props_forest`` walks: per node ``feature`` int32, ``threshold``
    float64, ``left`` / ``right`` int32 (rows of these arrays, -1 at a leaf, a child's row above its parent's), ``proba`` float64
    (nodes, classes) = the class fractions of the node, and ``tree_begin`` int32 (trees + 1).  ``n_features`` is the row length."""

    def __init__(self, feature, threshold, left, right, proba, tree_begin, n_features):
        self.feature = np.ascontiguousarray(feature, dtype=np.int32).reshape(-1)
        self.threshold = np.ascontiguousarray(threshold, dtype=np.float64).reshape(-1)
        self.left = np.ascontiguousarray(left, dtype=np.int32).reshape(-1)
        self.right = np.ascontiguousarray(right, dtype=np.int32).reshape(-1)
        self.proba = np.ascontiguousarray(proba, dtype=np.float64)
        self.tree_begin = np.ascontiguousarray(tree_begin, dtype=np.int32).reshape(-1)
        self.n_features = int(n_features)
        n = len(self.feature)
        if self.proba.ndim != 2 or not (len(self.threshold) == len(self.left) == len(self.right) == len(self.proba) == n):
            raise ValueError('PackedForest: the node arrays differ in length')
        tb = self.tree_begin
        if len(tb) < 2 or tb[0] != 0 or tb[-1] != n or np.any(np.diff(tb) < 1):
            raise ValueError(f'PackedForest: tree_begin must ascend from 0 to {n} nodes with at least one node per tree')
        if self.n_features < 1 or self.proba.shape[1] < 1:
            raise ValueError('PackedForest: at least one feature and one class')
        leaf = self.left < 0
        if np.any((self.right < 0) != leaf):
            raise ValueError('PackedForest: a node with one child')
        inner = np.flatnonzero(~leaf)
        tree = np.searchsorted(tb, inner, side='right') - 1
        for child in (self.left[inner], self.right[inner]):
            if np.any(child <= inner) or np.any(child >= tb[tree + 1]):
                raise ValueError('PackedForest: a child must lie above its parent and inside its tree')
        if len(inner) and (self.feature[inner].min() < 0 or self.feature[inner].max() >= self.n_features):
            raise ValueError('PackedForest: a feature index outside the row')
        if np.isnan(self.threshold[inner]).any() or not np.isfinite(self.proba).all():
            raise ValueError('PackedForest: NaN threshold or non-finite class fraction')

    @property
    def n_trees(self):
        return len(self.tree_begin) - 1

    @property
    def n_classes(self):
        return self.proba.shape[1]

    @classmethod
    def from_sklearn(cls, rfc):
        """From a fitted ``RandomForestClassifier`` (anything with ``estimators_[i].tree_`` and one output).  The class fractions are
        ``tree_.value`` where its rows sum to one already (sklearn >= 1.3 returns them as they are), else ``value / value.sum()``
        (what older versions compute per prediction)."""
        feature, threshold, left, right, proba, begin = [], [], [], [], [], [0]
        n_features = None
        for est in rfc.estimators_:
            t = est.tree_
            value = np.asarray(t.value, np.float64)
            if value.ndim != 3 or value.shape[1] != 1:
                raise ValueError('PackedForest.from_sklearn: one output per tree')
            value = value[:, 0, :]
            total = value.sum(1, keepdims=True)
            counts = np.abs(total - 1.0) > 1e-9
            value = np.where(counts, value / np.where(total == 0, 1.0, total), value)
            off = begin[-1]
            lc, rc = np.asarray(t.children_left, np.int64), np.asarray(t.children_right, np.int64)
            feature.append(np.where(lc < 0, 0, np.asarray(t.feature)))
            threshold.append(np.where(lc < 0, 0.0, np.asarray(t.threshold, np.float64)))
            left.append(np.where(lc < 0, -1, lc + off))
            right.append(np.where(rc < 0, -1, rc + off))
            proba.append(value)
            begin.append(off + len(lc))
            nf = int(getattr(t, 'n_features', getattr(est, 'n_features_in_', 0)))
            n_features = nf if n_features is None else n_features
            if nf != n_features:
                raise ValueError('PackedForest.from_sklearn: trees over rows of different length')
        if not feature:
            raise ValueError('PackedForest.from_sklearn: no trees')
        if len({p.shape[1] for p in proba}) != 1:
            raise ValueError('PackedForest.from_sklearn: trees with different numbers of classes')
        return cls(np.concatenate(feature), np.concatenate(threshold), np.concatenate(left), np.concatenate(right), np.concatenate(proba),
                   begin, n_features)

    _FIELDS = ('feature', 'threshold', 'left', 'right', 'proba', 'tree_begin')

    def save(self, path):
        np.savez_compressed(path, n_features=np.int64(self.n_features), **{k: getattr(self, k) for k in self._FIELDS})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(*(z[k] for k in cls._FIELDS), int(z['n_features']))

    def check_rows(self, features) -> np.ndarray:
        """The rows as float64 (n, n_features); NaN and values that are not finite as float32 raise ValueError (sklearn refuses them)."""
        x = np.ascontiguousarray(features, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != self.n_features:
            raise ValueError(f'the forest was fitted on rows of {self.n_features} features, got an array of shape {x.shape}')
        with np.errstate(over='ignore'):
            if not np.isfinite(x.astype(np.float32)).all():
                raise ValueError('features hold NaN or a value that is not finite as float32')
        return x

    def predict_proba(self, features, device=None) -> np.ndarray:
        """float64 (n, classes) on the device: ``RandomForestClassifier.predict_proba`` with ``n_jobs=1``, bit for bit."""
        from .. import _dev as D
        x = self.check_rows(features)
        out = np.zeros((len(x), self.n_classes), np.float64)
        if not len(x):
            return out
        if len(x) >= 2 ** 31:
            raise ValueError('PackedForest.predict_proba: fewer than 2^31 rows per call')
        dev = D.device(device)
        arrs = [D.up(a, dev) for a in (x, self.feature, self.threshold, self.left, self.right, self.proba, self.tree_begin)]
        out_d = D.empty(out.shape, D.f64, dev)
        counts_d = D.counters(dev)
        D.call('sd_syn_props_forest', dev, arrs[0], len(x), self.n_features, *arrs[1:], self.n_trees, len(self.feature), self.n_classes, out_d,
               counts_d)
        out = D.down(out_d)
        if int(D.down(counts_d)[7]):
            raise RuntimeError('sd_syn_props_forest: a node or a feature index was out of range')
        return out


def classify_synssv_objects(features, forest, device=None) -> np.ndarray:
    """``classify_synssv_objects`` (:1096-1161) on the rows of ``synssv_o_features``: ``syn_prob`` float64 (n) = column 1 of the forest's
    class probabilities, what ``rfc.predict_proba([feats])[0][1]`` gives row by row.  `forest`: a ``PackedForest`` or a fitted sklearn
    forest.  No CPU fallback."""
    if not isinstance(forest, PackedForest):
        forest = PackedForest.from_sklearn(forest)
    if forest.n_classes < 2:
        raise ValueError('classify_synssv_objects: the forest knows one class only, there is no column 1')
    return np.ascontiguousarray(forest.predict_proba(features, device)[:, 1])


class CellTable:
    """What ``collect_properties_from_ssv_partners`` reads of the cells, plain numpy.  Per cell: ``ids`` uint64 (unique), ``celltypes``
    int32 (default -1: no ``celltype_cnn_e3``); the mesh: ``vertices`` float32 (v, 3) in nm with ``vert_begin`` (cells + 1) and
    ``vertex_labels[key]`` int32 (v), e.g. ``'spiness'``; the skeleton: ``nodes`` (m, 3) in voxels (kept as float64) with ``node_begin``
    (cells + 1) and ``node_attrs[key]``: an integer array (m) such as ``'axoness_avg10000'``, or float32 (m, e) for ``'latent_morph'``;
    ``node_attr_present[key]`` bool (cells): False where the skeleton of a cell lacks the key (default: present everywhere);
    ``spinehead_vol`` = (``sh_begin`` (cells + 1), syn_ssv ids uint64, volumes float32): the entries of every cell's ``spinehead_vol``
    dict, or None."""

    def __init__(self, ids, vertices, vert_begin, vertex_labels, nodes, node_begin, node_attrs, celltypes=None, node_attr_present=None,
                 spinehead_vol=None):
        self.ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        n = len(self.ids)
        if len(np.unique(self.ids)) != n:
            raise ValueError('CellTable: a cell id occurs twice')
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        self.vert_begin = np.ascontiguousarray(vert_begin, dtype=np.int64).reshape(-1)
        _check_offsets('CellTable: vert_begin', self.vert_begin, n, len(self.vertices))
        self.nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1, 3)
        self.node_begin = np.ascontiguousarray(node_begin, dtype=np.int64).reshape(-1)
        _check_offsets('CellTable: node_begin', self.node_begin, n, len(self.nodes))
        if not (np.isfinite(self.vertices).all() and np.isfinite(self.nodes).all()):
            raise ValueError('CellTable: a vertex or node coordinate is not finite')
        self.celltypes = np.full(n, -1, np.int32) if celltypes is None else np.ascontiguousarray(celltypes, dtype=np.int32).reshape(-1)
        if len(self.celltypes) != n:
            raise ValueError(f'CellTable: {n} cells, {len(self.celltypes)} celltypes')
        self.vertex_labels = {}
        for key, lab in dict(vertex_labels).items():
            lab = np.asarray(lab)
            lab = lab.squeeze(1) if lab.ndim == 2 else lab
            if lab.shape != (len(self.vertices),):
                raise ValueError('Size of vertices and their labels does not match!')
            self.vertex_labels[key] = np.ascontiguousarray(lab, dtype=np.int32)
        self.node_attrs, self.node_attr_present = {}, {}
        for key, a in dict(node_attrs).items():
            a = np.asarray(a)
            if key == 'latent_morph':
                a = np.ascontiguousarray(a, dtype=np.float32)
                a = a.reshape(len(self.nodes), -1) if a.ndim != 2 else a
            else:
                a = np.ascontiguousarray(a.reshape(-1), dtype=np.int32)
            if len(a) != len(self.nodes):
                raise ValueError(f'CellTable: node attribute {key!r} holds {len(a)} rows for {len(self.nodes)} nodes')
            self.node_attrs[key] = a
            present = np.ones(n, bool) if node_attr_present is None or key not in node_attr_present else \
                np.ascontiguousarray(node_attr_present[key], dtype=bool).reshape(-1)
            if len(present) != n:
                raise ValueError(f'CellTable: node_attr_present[{key!r}] must hold one flag per cell')
            self.node_attr_present[key] = present
        self.spinehead_vol = None
        if spinehead_vol is not None:
            sb, sid, vol = spinehead_vol
            sb, sid = np.ascontiguousarray(sb, dtype=np.int64).reshape(-1), np.ascontiguousarray(sid, dtype=np.uint64).reshape(-1)
            vol = np.ascontiguousarray(vol, dtype=np.float32).reshape(-1)
            _check_offsets('CellTable: spinehead_vol offsets', sb, n, len(sid))
            if len(vol) != len(sid):
                raise ValueError('CellTable: spinehead_vol ids and volumes differ in length')
            self.spinehead_vol = (sb, sid, vol)

    def __len__(self):
        return len(self.ids)

    @classmethod
    def from_cells(cls, cells):
        """From one dict per cell: ``id``, and optionally ``celltype``, ``vertices``, ``vertex_labels`` {key: array}, ``nodes``,
        ``node_attrs`` {key: array} (a key may be missing in some cells), ``spinehead_vol`` {syn_ssv id: volume}."""
        cells = list(cells)
        verts = [np.asarray(c.get('vertices', np.zeros((0, 3))), np.float32).reshape(-1, 3) for c in cells]
        nodes = [np.asarray(c.get('nodes', np.zeros((0, 3))), np.float64).reshape(-1, 3) for c in cells]
        vkeys = sorted({k for c in cells for k in c.get('vertex_labels', {})})
        nkeys = sorted({k for c in cells for k in c.get('node_attrs', {})})
        vlab = {}
        for k in vkeys:
            for c, v in zip(cells, verts):
                if len(v) and k not in c.get('vertex_labels', {}):
                    raise ValueError(f'CellTable: cell {c["id"]} has vertices but no {k!r} labels')
            vlab[k] = np.concatenate([np.asarray(c.get('vertex_labels', {}).get(k, np.zeros(0)), np.int64).reshape(-1) for c in cells])
        nattr, present = {}, {}
        for k in nkeys:
            parts = [np.asarray(c['node_attrs'][k]) for c in cells if k in c.get('node_attrs', {})]
            tail = parts[0].shape[1:] if k == 'latent_morph' else ()
            fill = [np.asarray(c['node_attrs'][k]).reshape((len(m),) + tail) if k in c.get('node_attrs', {}) else
                    np.zeros((len(m),) + tail, parts[0].dtype) for c, m in zip(cells, nodes)]
            nattr[k] = np.concatenate(fill)
            present[k] = np.array([k in c.get('node_attrs', {}) for c in cells], bool)
        sh = None
        if any('spinehead_vol' in c for c in cells):
            items = [sorted(c.get('spinehead_vol', {}).items()) for c in cells]
            sh = (np.concatenate(([0], np.cumsum([len(i) for i in items]))), np.array([k for i in items for k, _ in i], np.uint64),
                  np.array([v for i in items for _, v in i], np.float32))
        offs = lambda parts: np.concatenate(([0], np.cumsum([len(p) for p in parts])))
        return cls([c['id'] for c in cells], np.concatenate(verts) if verts else np.zeros((0, 3)), offs(verts), vlab,
                   np.concatenate(nodes) if nodes else np.zeros((0, 3)), offs(nodes), nattr, [c.get('celltype', -1) for c in cells], present, sh)


class SynSsvProperties:
    """What ``collect_properties_from_ssv_partners`` stores per synapse; column p = partner slot p: ``partner_axoness``,
    ``partner_spiness``, ``partner_celltypes`` int32 (n, 2), ``partner_spineheadvol`` float32 (n, 2), ``latent_morph`` float32
    (n, 2, e), ``syn_sign`` int64 (n)."""

    COLUMNS = ('partner_axoness', 'partner_spiness', 'partner_celltypes', 'partner_spineheadvol', 'latent_morph', 'syn_sign')

    def __init__(self, **columns):
        for name in self.COLUMNS:
            setattr(self, name, columns[name])

    def __len__(self):
        return len(self.syn_sign)

    def as_dicts(self) -> list:
        """One dict per synapse with the keys ``_from_cell_to_syn_dict`` (:222-227) adds to its attribute dict: two-element lists,
        and ``syn_sign``."""
        return [dict(partner_axoness=[self.partner_axoness[i, 0], self.partner_axoness[i, 1]],
                     partner_spiness=[self.partner_spiness[i, 0], self.partner_spiness[i, 1]],
                     partner_celltypes=[self.partner_celltypes[i, 0], self.partner_celltypes[i, 1]],
                     partner_spineheadvol=[self.partner_spineheadvol[i, 0], self.partner_spineheadvol[i, 1]],
                     syn_sign=int(self.syn_sign[i]), latent_morph=[self.latent_morph[i, 0], self.latent_morph[i, 1]]) for i in range(len(self))]


def segmented_knn(points, begin, labels, q_cell, q_xyz, k: int, device=None, return_neighbours: bool = False, return_counts: bool = False):
    """``sd_syn_props_knn``: for every query (`q_cell` = row of its cell, `q_xyz` float64 nm) the vote over the ``min(k, points of the
    cell)`` points of cell c = ``points[begin[c]:begin[c + 1]]`` (float32 or float64, (v, 3)) with the smallest (d^2, row), d^2 =
    ((dx dx) + dy dy) + dz dz in float64: the label (`labels` int32 per point; None: the row of the point) with the highest count, on
    equal counts the one that occurs first in that order; -1 for a cell without points.  With `return_neighbours` also the rows
    (n_q, k) int32, padded with -1, and d^2 (n_q, k) float64, padded with inf; with `return_counts` the device's counters."""
    from .. import _dev as D
    pts = np.asarray(points)
    pts = np.ascontiguousarray(pts, dtype=np.float32 if pts.dtype == np.float32 else np.float64).reshape(-1, 3)
    begin = np.ascontiguousarray(begin, dtype=np.int64).reshape(-1)
    n_cells = len(begin) - 1
    if n_cells < 0:
        raise ValueError('segmented_knn: begin must hold cells + 1 offsets')
    _check_offsets('segmented_knn: begin', begin, n_cells, len(pts))
    q_cell = np.ascontiguousarray(q_cell, dtype=np.int64).reshape(-1)
    q_xyz = np.ascontiguousarray(q_xyz, dtype=np.float64).reshape(-1, 3)
    n_q = len(q_cell)
    if isinstance(k, bool) or int(k) != k:
        raise ValueError(f'k must be an integer, got {k!r}')
    k = int(k)
    if len(q_xyz) != n_q:
        raise ValueError(f'segmented_knn: {n_q} query cells, {len(q_xyz)} coordinates')
    if n_q and (q_cell.min() < 0 or q_cell.max() >= n_cells):
        raise ValueError('segmented_knn: a query names a cell row outside the table')
    if not (np.isfinite(pts).all() and np.isfinite(q_xyz).all()):
        raise ValueError('segmented_knn: a coordinate is not finite')
    if labels is not None:
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        if len(labels) != len(pts):
            raise ValueError('Size of vertices and their labels does not match!')
    dev = D.device(device)
    pts_d, begin_d, lab_d = D.up(pts, dev), D.up(begin, dev), None if labels is None else D.up(labels, dev)
    qc_d, qx_d = D.up(q_cell.astype(np.uint32), dev), D.up(q_xyz, dev)
    kk = max(1, min(k, L.SD_SYN_PROPS_MAX_K))
    vote_d = D.empty(n_q, D.i32, dev)
    idx_d = D.empty((n_q, kk), D.i32, dev) if return_neighbours else None
    d2_d = D.empty((n_q, kk), D.f64, dev) if return_neighbours else None
    counts_d = D.counters(dev)
    tmp = D.scratch('sd_syn_props_knn_temp_bytes', dev, len(pts), n_cells)
    D.call('sd_syn_props_knn', dev, pts_d, int(pts.dtype == np.float32), begin_d, n_cells, len(pts), lab_d, qc_d, qx_d, n_q, k, 3, vote_d, idx_d,
           d2_d, counts_d, tmp, tmp.numel())
    counts = D.down(counts_d)
    if int(counts[7]):
        raise RuntimeError('sd_syn_props_knn: an offset, a cell row or a point row was out of range')
    out = [D.down(vote_d)[:n_q]]
    if return_neighbours:
        out += [D.down(idx_d)[:n_q], D.down(d2_d)[:n_q]]
    if return_counts:
        out.append(dict(tiles_visited=int(counts[0]), tiles_skipped=int(counts[1])))
    return out[0] if len(out) == 1 else tuple(out)


def _cell_rows(cells: CellTable, ids):
    """-> (row of every id in the table, found mask); a missing id gets some row of the table (none if the table is empty)."""
    if not len(cells):
        return np.zeros(len(ids), np.int64), np.zeros(len(ids), bool)
    order = np.argsort(cells.ids, kind='stable')
    row = order[np.minimum(np.searchsorted(cells.ids[order], ids), len(cells) - 1)]
    return row, cells.ids[row] == ids


def _nearest_nodes(cells: CellTable, used, rows, q_xyz, scale, device):
    """The skeleton node nearest to every query (`rows`: its cell, flagged in `used`; ``attr_for_coords``'s k = 1 tree over
    ``nodes * scaling``) as a row of ``cells.nodes``.  Only the nodes of the used cells go to the device."""
    n_nodes = np.diff(cells.node_begin)
    begin = np.concatenate(([0], np.cumsum(np.where(used, n_nodes, 0)))).astype(np.int64)
    node_keep = np.repeat(used, n_nodes)
    nearest = segmented_knn(cells.nodes[node_keep] * scale, begin, None, rows, q_xyz, 1, device)
    return np.flatnonzero(node_keep)[nearest]               # kept node j is node flatnonzero(node_keep)[j] of the table


def spine_vertices(cells: CellTable, used, semseg_key: str, ds_vertices: int, ignore_labels):
    """The vertices ``semseg_for_coords`` (super_segmentation_object.py:2219-2237) hands to the tree, for the cells flagged in `used`:
    every ``ds``-th vertex of a cell (``ds = max(1, ds_vertices // 10)`` below 5e6 vertices), without the ignored labels.
    -> (vertices float32, labels int32, begin int64 (cells + 1)); cells that are not used keep no vertex."""
    if semseg_key not in cells.vertex_labels:
        if len(cells.vertices):
            raise KeyError(semseg_key)
        lab = np.zeros(0, np.int32)
    else:
        lab = cells.vertex_labels[semseg_key]
    n_vert = np.diff(cells.vert_begin)
    ds = np.where(n_vert < 5e6, max(1, int(ds_vertices) // 10), int(ds_vertices))
    cell_of = np.repeat(np.arange(len(cells)), n_vert)
    local = np.arange(len(cells.vertices)) - cells.vert_begin[cell_of]
    keep = np.asarray(used, bool)[cell_of] & (local % ds[cell_of] == 0)
    keep &= ~np.isin(lab, np.asarray(list(ignore_labels or []), np.int64))
    begin = np.concatenate(([0], np.cumsum(np.bincount(cell_of[keep], minlength=len(cells))))).astype(np.int64)
    return cells.vertices[keep], lab[keep], begin


def collect_properties_from_ssv_partners(syn_ssv, cells: CellTable, scaling=None, syn_ids=None, k=None, ds_vertices=None, ignore_labels=None,
                                         pred_key_ax=None, n_embedding=None, sym_thresh=None, device=None) -> SynSsvProperties:
    """``collect_properties_from_ssv_partners`` (:44-106) with its workers ``_collect_properties_from_ssv_partners_thread`` (:109-174)
    and ``_from_cell_to_syn_dict`` (:177-229) on the ``SynSsvTable`` of ``combine_and_split_syn`` (``neuron_partners``, ``rep_coords``,
    ``syn_type_sym_ratio``) and a ``CellTable``.  For every synapse and partner: the spine label by a vote over the `k` nearest of the
    partner cell's mesh vertices (``semseg_for_coords``), the compartment (`pred_key_ax`) and ``latent_morph`` of the nearest
    skeleton node (``attr_for_coords``), the cell type and the spine-head volume stored for `syn_ids` (default: the row number).
    All cells go through two calls of ``sd_syn_props_knn``; the node attributes are gathered on the device.  The defaults come from
    ``config['spines']['semseg2coords_spines']``, ``config['compartments']``, ``config['tcmn']`` and ``config['cell_objects']``.

    A cell without mesh vertices gets zeros in every column; one without skeleton nodes -1 and inf; a skeleton without the key -1
    (``latent_morph``: inf).  ValueError: a partner cell that is not in the table, a cell whose vertices are all ignored.
    Not built: storages, ``cache_syn.pkl`` files, batch jobs; k <= 64.  No CPU fallback."""
    from .. import _dev as D
    from .. import global_params
    cfg = global_params.config
    if scaling is None:
        scaling = cfg['scaling']
    sp = cfg['spines']['semseg2coords_spines']
    k = sp['k'] if k is None else k
    ds_vertices = sp['ds_vertices'] if ds_vertices is None else ds_vertices
    ignore_labels = sp['ignore_labels'] if ignore_labels is None else ignore_labels
    if pred_key_ax is None:
        comp = cfg['compartments']
        pred_key_ax = '{}_avg{}'.format(comp['view_properties_semsegax']['semseg_key'], comp['dist_axoness_averaging'])
    m = int(cfg['tcmn']['ndim_embedding'] if n_embedding is None else n_embedding)
    sym_thresh = cfg['cell_objects']['sym_thresh'] if sym_thresh is None else sym_thresh
    if not isinstance(cells, CellTable):
        raise TypeError('cells must be a CellTable')
    _check_positive_int(k=k, ds_vertices=ds_vertices)
    if int(k) > L.SD_SYN_PROPS_MAX_K:
        raise ValueError(f'k = {k}: at most {L.SD_SYN_PROPS_MAX_K} neighbours per query')
    scale = _check_scaling32(scaling)
    if 'latent_morph' in cells.node_attrs and cells.node_attrs['latent_morph'].shape[1] != m:
        raise ValueError(f"latent_morph holds {cells.node_attrs['latent_morph'].shape[1]} values per node, ndim_embedding is {m}")
    n = len(syn_ssv)
    partners = np.ascontiguousarray(syn_ssv.neuron_partners, dtype=np.uint64).reshape(n, 2)
    rep = np.ascontiguousarray(syn_ssv.rep_coords, dtype=np.int32).reshape(n, 3)
    ratio = np.asarray(syn_ssv.syn_type_sym_ratio, np.float64).reshape(-1)
    syn_ids = np.arange(n, dtype=np.uint64) if syn_ids is None else np.ascontiguousarray(syn_ids, dtype=np.uint64).reshape(-1)
    if len(ratio) != n or len(syn_ids) != n:
        raise ValueError(f'{n} synapses, {len(ratio)} syn_type_sym_ratio, {len(syn_ids)} syn_ids')
    side_cell_id = partners.reshape(-1)
    row, known = _cell_rows(cells, side_cell_id)
    if not known.all():
        s = int(np.flatnonzero(~known)[0])
        raise ValueError(f'Could not find the partner cell {int(side_cell_id[s])} of synssv with ID {int(syn_ids[s // 2])} in the cell table.')
    props = dict(partner_axoness=np.zeros(2 * n, np.int32), partner_spiness=np.zeros(2 * n, np.int32), partner_celltypes=np.zeros(2 * n, np.int32),
                 partner_spineheadvol=np.zeros(2 * n, np.float32), latent_morph=np.zeros((2 * n, m), np.float32))
    sign = np.where(ratio > sym_thresh, -1, 1).astype(np.int64)
    if n:
        used = np.zeros(len(cells), bool)
        used[row] = True
        has_mesh = np.diff(cells.vert_begin) > 0
        has_skel = np.diff(cells.node_begin) > 0
        sides = np.flatnonzero(has_mesh[row])                    # the others keep their zeros (:144-152)
        q_xyz = np.repeat(rep.astype(np.float64) * scale, 2, 0)  # np.array(coords) * self.scaling
        if len(sides):
            verts, lab, begin = spine_vertices(cells, used & has_mesh, 'spiness', ds_vertices, ignore_labels)
            empty = np.flatnonzero(used & has_mesh & (np.diff(begin) == 0))
            if len(empty):
                raise ValueError(f'every mesh vertex of cell {int(cells.ids[empty[0]])} carries an ignored label: no vertex to vote')
            props['partner_spiness'][sides] = segmented_knn(verts, begin, lab, row[sides], q_xyz[sides], int(k), device)
            props['partner_celltypes'][sides] = cells.celltypes[row[sides]]
            vol = np.full(len(sides), -1, np.float32)
            if cells.spinehead_vol is not None:
                sb, sid, sv = cells.spinehead_vol
                ids_all = np.unique(np.concatenate([sid, syn_ids]))                         # (cell row, syn_ssv id) as one integer
                if len(cells) * len(ids_all) >= 2 ** 62:
                    raise ValueError('spinehead_vol: cells x synapse ids do not fit 62 bits')
                have = np.repeat(np.arange(len(cells)), np.diff(sb)) * len(ids_all) + np.searchsorted(ids_all, sid)
                o = np.argsort(have, kind='stable')
                want = row[sides] * len(ids_all) + np.searchsorted(ids_all, syn_ids[sides // 2])
                if len(have):
                    j = np.minimum(np.searchsorted(have[o], want), len(have) - 1)
                    hit = have[o][j] == want
                    vol[hit] = sv[o][j[hit]]
            props['partner_spineheadvol'][sides] = vol
            props['partner_axoness'][sides] = -1
            props['latent_morph'][sides] = np.inf
            sk = sides[has_skel[row[sides]]]
            if len(sk):
                dev = D.device(device)
                near_d = D.up(_nearest_nodes(cells, used & has_mesh, row[sk], q_xyz[sk], scale, device), dev)
                if pred_key_ax in cells.node_attrs:
                    ax = D.down(D.up(cells.node_attrs[pred_key_ax], dev)[near_d])
                    ok = cells.node_attr_present[pred_key_ax][row[sk]]
                    props['partner_axoness'][sk[ok]] = ax[ok]
                if 'latent_morph' in cells.node_attrs:
                    lm = D.down(D.up(cells.node_attrs['latent_morph'], dev)[near_d])
                    ok = cells.node_attr_present['latent_morph'][row[sk]]
                    props['latent_morph'][sk[ok]] = lm[ok]
    return SynSsvProperties(partner_axoness=props['partner_axoness'].reshape(n, 2), partner_spiness=props['partner_spiness'].reshape(n, 2),
                            partner_celltypes=props['partner_celltypes'].reshape(n, 2),
                            partner_spineheadvol=props['partner_spineheadvol'].reshape(n, 2), latent_morph=props['latent_morph'].reshape(n, 2, m),
                            syn_sign=sign)


def conn_mat_header(n_embedding: int) -> str:
    """:1492-1498."""
    return ("x\ty\tz\tssv1\tssv2\tsize\tcomp1\tcomp2\tcelltype1\tcelltype2\tspiness1\tspiness2\tsynprob\tspinehead_vol1\tspinehead_vol2" +
            "".join(["\tlatentmorph1_{}".format(ix) for ix in range(n_embedding)]) +
            "".join(["\tlatentmorph2_{}".format(ix) for ix in range(n_embedding)]))


def export_matrix(syn_ssv, props: SynSsvProperties, syn_prob, mesh_area, dest_folder=None, threshold_syn=0, export_kzip: bool = False,
                  n_embedding=None) -> str:
    """``export_matrix`` (:1434-1499): ``dest_folder + '/conn_mat.csv'``, one row per synapse with ``syn_prob > threshold_syn``
    (None: ``config['cell_objects']['thresh_synssv_proba']``): x, y, z (``rep_coords``), the two cell ids, ``size = mesh_area / 2 *
    syn_sign``, compartments, cell types, spine labels, the probability, the spine-head volumes and the two embeddings, written by
    ``np.savetxt`` with tabs in its default format.  An existing file is renamed with a time stamp first.  -> the path.
    ``export_kzip=True`` raises NotImplementedError (the skeleton classes are not built).  Host only."""
    import datetime
    import os
    import time
    from .. import global_params
    cfg = global_params.config
    if export_kzip:
        raise NotImplementedError('export_matrix: the kzip export needs the skeleton classes, which are not built')
    if threshold_syn is None:
        threshold_syn = cfg['cell_objects']['thresh_synssv_proba']
    if dest_folder is None:
        dest_folder = cfg.working_dir + '/connectivity_matrix/'
    n = len(syn_ssv)
    syn_prob = np.asarray(syn_prob, np.float64).reshape(-1)
    area = np.asarray(mesh_area, np.float64).reshape(-1)
    if len(props) != n or len(syn_prob) != n or len(area) != n:
        raise ValueError(f'{n} synapses, {len(props)} property rows, {len(syn_prob)} probabilities, {len(area)} mesh areas')
    m_emb = props.latent_morph.shape[2] if n_embedding is None else int(n_embedding)
    if props.latent_morph.shape[2] != m_emb:
        raise ValueError(f'latent_morph holds {props.latent_morph.shape[2]} values, the header {m_emb}')
    os.makedirs(dest_folder, exist_ok=True)                      # the reference makes the parent only: its default ends with '/'
    dest_name = dest_folder + '/conn_mat'
    m = syn_prob > threshold_syn
    m_sizes = area[m] / 2
    m_sizes = np.multiply(m_sizes, np.asarray(props.syn_sign)[m]).reshape(-1)[:, None]
    table = np.concatenate([np.asarray(syn_ssv.rep_coords).reshape(n, 3)[m], np.asarray(syn_ssv.neuron_partners).reshape(n, 2)[m], m_sizes,
                            props.partner_axoness[m], props.partner_celltypes[m], props.partner_spiness[m], syn_prob[m][:, None],
                            props.partner_spineheadvol[m], props.latent_morph[m].reshape(int(m.sum()), -1)], axis=1)
    if os.path.isfile(dest_name + '.csv'):                       # do not overwrite previous files
        st = datetime.datetime.fromtimestamp(time.time()).strftime('%Y-%m-%d %H:%M:%S')
        os.rename(dest_name + '.csv', '{}_{}.csv'.format(dest_name, st))
    np.savetxt(dest_name + '.csv', table, delimiter='\t', header=conn_mat_header(m_emb))
    return dest_name + '.csv'


def calculate_spinehead_volume(cells: CellTable, sv_begin, sv_ids, syn_ids, syn_rep_coords, syn_cells, seg, scaling=None, ctx_vol=(200, 200, 100),
                               k=None, ignore_labels=None, semseg_key: str = 'spiness', ax_key=None, ds_vertices=None, device=None,
                               batch: int = 8, max_peaks=None):
    """``extract_spinehead_volume_mesh`` (reps/super_segmentation_helper.py:2068-2198, run per cell by ``exec_syns.run_spinehead_volume_calc``)
    for every cell of a ``CellTable`` at once, tables in memory.  Cell c owns the supervoxels ``sv_ids[sv_begin[c]:sv_begin[c + 1]]``;
    synapse i (`syn_ids` uint64, `syn_rep_coords` (n, 3) voxels) touches the cells ``syn_cells[i]`` (n, 2): it is one of the ``syn_ssv`` of
    each of them that is in the table (ids that are not are skipped: the reference runs per cell).  `seg`: the cell segmentation, a
    ``KnossosDataset`` (windows are read in spatial buckets kept on the device) or ``(volume (x, y, z) of 64-bit ids, origin)`` as an array
    or device tensor, zeros outside.

    Per cell: the synapses whose spine label (vote of the `k` nearest mesh vertices, ``semseg_for_coords``) is 1 and whose nearest skeleton
    node carries `ax_key` == 0 are spine-head synapses (:2114-2122); each gets a ``2 * ctx_vol`` window (``extraction/spinehead.py``).
    A cell without skeleton nodes or without `ax_key` has no spine-head synapse (its compartment reads -1, as for the partner properties;
    the reference fails inside ``attr_for_coords`` there).  Negative `semseg_key` labels raise: they cannot seed the flood (the reference
    would write them into its float marker volume).
    -> ``(sh_begin (cells + 1) int64, ids uint64, volumes float64 um^3)``: the triple ``CellTable(spinehead_vol=...)`` takes, per cell in
    the order of the synapses.  A window without a mesh vertex in its box gives no entry, one whose flood leaves no head voxel 0.0.

    ValueError (before any launch): bad shapes, a cell with synapses but without `semseg_key` labels (the reference's message); after the
    batch: a window without any voxel of the cell (the reference's message).  Defaults from ``config['scaling']``,
    ``config['spines']['semseg2coords_spines']`` and ``config['compartments']``.  k <= 64.  No CPU fallback."""
    from .. import global_params
    from . import spinehead as SH
    cfg = global_params.config
    if not isinstance(cells, CellTable):
        raise TypeError('cells must be a CellTable')
    sp = cfg['spines']['semseg2coords_spines']
    k = sp['k'] if k is None else k
    ds_vertices = sp['ds_vertices'] if ds_vertices is None else ds_vertices
    ignore_labels = list(sp['ignore_labels'] if ignore_labels is None else ignore_labels)
    if ax_key is None:
        comp = cfg['compartments']
        ax_key = '{}_avg{}'.format(comp['view_properties_semsegax']['semseg_key'], comp['dist_axoness_averaging'])
    _check_positive_int(k=k, ds_vertices=ds_vertices, batch=batch)
    if int(k) > L.SD_SYN_PROPS_MAX_K:
        raise ValueError(f'k = {k}: at most {L.SD_SYN_PROPS_MAX_K} neighbours per query')
    sc, ds = SH.check_scaling(cfg['scaling'] if scaling is None else scaling)
    ctx = np.array(ctx_vol)
    if ctx.shape != (3,) or ctx.dtype.kind not in 'iu' or np.any(ctx < 1):
        raise ValueError(f'ctx_vol must be three positive integers, got {ctx_vol}')
    n_cells = len(cells)
    sv_begin = np.ascontiguousarray(sv_begin, dtype=np.int64).reshape(-1)
    sv_ids = np.ascontiguousarray(sv_ids, dtype=np.uint64).reshape(-1)
    _check_offsets('calculate_spinehead_volume: sv_begin', sv_begin, n_cells, len(sv_ids))
    syn_ids = np.ascontiguousarray(syn_ids, dtype=np.uint64).reshape(-1)
    n = len(syn_ids)
    rep = np.ascontiguousarray(syn_rep_coords, dtype=np.int64).reshape(-1, 3)
    syn_cells = np.ascontiguousarray(syn_cells, dtype=np.uint64).reshape(-1, 2)
    if len(rep) != n or len(syn_cells) != n:
        raise ValueError(f'{n} syn_ids, {len(rep)} syn_rep_coords, {len(syn_cells)} syn_cells')
    if n and rep.min() < 0:
        raise ValueError('calculate_spinehead_volume: a representative coordinate is negative')
    if not hasattr(seg, 'load_seg') and not (isinstance(seg, (tuple, list)) and len(seg) == 2 and len(np.asarray(seg[1]).reshape(-1)) == 3):
        raise ValueError('seg must be a KnossosDataset or (volume, origin)')
    # (cell row, synapse) pairs: a synapse is a syn_ssv of each of its cells, once
    row, known = _cell_rows(cells, syn_cells.reshape(-1))
    known[1::2] &= ~(known[0::2] & (syn_cells[:, 0] == syn_cells[:, 1]))
    pair_syn, pair_row = np.flatnonzero(known) // 2, row[known]
    used = np.zeros(n_cells, bool)
    used[pair_row] = True
    n_vert = np.diff(cells.vert_begin)
    for c in np.flatnonzero(used):
        if semseg_key not in cells.vertex_labels or n_vert[c] == 0:
            raise ValueError(f'"{semseg_key}" not available in skeleton of SSO {int(cells.ids[c])}.')
        if sv_begin[c + 1] == sv_begin[c]:
            raise ValueError(f'cell {int(cells.ids[c])} has no supervoxel')
    if n and len(cells.vertex_labels.get(semseg_key, ())) and cells.vertex_labels[semseg_key].min() < 0:
        raise ValueError(f'negative "{semseg_key}" vertex labels cannot seed the flood')
    sh_ids, sh_vol, sh_count = [], [], np.zeros(n_cells, np.int64)
    if len(pair_syn):
        # the spine-head filter (:2114-2122) through the two segmented_knn paths of collect_properties_from_ssv_partners
        scale = np.asarray(sc, np.float32).astype(np.float64)
        q_xyz = rep[pair_syn].astype(np.float64) * scale
        verts, lab, begin = spine_vertices(cells, used, semseg_key, ds_vertices, ignore_labels)
        empty = np.flatnonzero(used & (np.diff(begin) == 0))
        if len(empty):
            raise ValueError(f'every mesh vertex of cell {int(cells.ids[empty[0]])} carries an ignored label: no vertex to vote')
        curr_sp = segmented_knn(verts, begin, lab, pair_row, q_xyz, int(k), device)
        curr_ax = np.full(len(pair_syn), -1, np.int64)
        has_ax = ax_key in cells.node_attrs
        sk = np.flatnonzero((np.diff(cells.node_begin) > 0)[pair_row] & (cells.node_attr_present[ax_key][pair_row] if has_ax else False))
        if len(sk):
            curr_ax[sk] = cells.node_attrs[ax_key][_nearest_nodes(cells, used, pair_row[sk], q_xyz[sk], scale, device)]
        head = (curr_sp == 1) & (curr_ax == 0)
        runner = None                                                # every cell has the same window shape: one set of device buffers
        for c in np.flatnonzero(used):
            sel = np.flatnonzero(head & (pair_row == c))
            if not len(sel):
                continue
            v = cells.vertices[cells.vert_begin[c]:cells.vert_begin[c + 1]] / sc          # sso.mesh[1].reshape(-1, 3) / scaling (:2106)
            sem = cells.vertex_labels[semseg_key][cells.vert_begin[c]:cells.vert_begin[c + 1]]
            keep = ~np.isin(sem, np.asarray(ignore_labels, np.int64))
            if runner is None:
                runner = SH.WindowRunner([len(SH.zoom_source_table(2 * int(ctx[a]), ds[a])) for a in range(3)], int(batch), max_peaks, device)
            res = SH.spinehead_windows(seg, sv_ids[sv_begin[c]:sv_begin[c + 1]], rep[pair_syn[sel]], v[keep], sem[keep], sc, ctx, int(k), runner.dev,
                                       int(batch), max_peaks, syn_ids[pair_syn[sel]], runner=runner)
            entry = res[:, 5] > 0
            sh_ids.append(syn_ids[pair_syn[sel]][entry])
            sh_vol.append(np.asarray(SH.head_volume(res[entry, 2], sc, ds), np.float64))
            sh_count[c] = int(entry.sum())
    return (np.concatenate(([0], np.cumsum(sh_count))).astype(np.int64), np.concatenate(sh_ids) if sh_ids else np.zeros(0, np.uint64),
            np.concatenate(sh_vol) if sh_vol else np.zeros(0, np.float64))
