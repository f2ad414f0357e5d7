"""Dataset-wide object properties and organelle -> cell overlap counts from KnossosDataset segmentations: step 1 of
``map_subcell_extract_props`` (/root/reference/syconn/proc/sd_proc.py:273-787).

MI355X shape of the work.  The reference turns every chunk into Python dictionaries and folds them into running dictionaries, id
by id, on the host (its worker loop :617-678 with ``merge_prop_dicts`` :1248-1273 and ``merge_map_dicts`` :1300-1322).  Here no
per-object data exists on the host before the dataset is finished:

* per chunk  ``sd_segstats_scan`` (one HBM-bound pass over the label volumes) fills device hash tables; ``sd_chunkprops_append`` /
  ``sd_chunkpairs_append`` turn them into RECORDS appended to device arrays -- applying the "purely inside the chunk and smaller than
  ``min_obj_vx``" filter from the tables' own bounding boxes (an id is on a face of the chunk exactly when its box touches that
  face: no sixfold ``np.unique`` over the faces) and adding the chunk origin;
* per dataset  ``sd_propmerge_objects`` / ``sd_propmerge_pairs``: stable radix sort by id + one segment per id (sizes add up, the
  representative coordinate is the last chunk's, bounding boxes stay one per chunk in chunk order);
* at the API edge the merged tables (``PropTable`` / ``MapTable``, plain numpy) become the dictionaries the reference's workers
  pickle for step 2.  ``convert_nvox2ratio_mapdict`` / ``invert_mdc`` have array forms there (``MapTable.ratios`` /
  ``MapTable.inverted``).

The four dictionary functions of the reference's module are kept by name and contract (in-place merge into the first element)
for callers that hold dictionaries; the chunk driver does not use them.  Not built: the batch-job machinery, the mesh caches and
step 2 (writing SegmentationObject storages) -- SyConn's storage layer, outside the dense-prediction path.

Pinned by tests/golden/g12_propmerge.npz (outputs of the reference's own functions, tests/golden/make_golden_propmerge.py)."""
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from ..handler.basics import kd_factory
from .records import OBJECT_FIELDS, Records, segment_offsets


# ---------------------------------------------------------------------------------------------------------------------------------
# merged tables (host, numpy) and their dictionary views
class PropTable:
    """Merged properties of one label volume kind: ``ids`` ascending (uint64), ``sizes`` (int64), ``rep_coords`` (n, 3),
    ``boxes`` (m, 2, 3) = every (chunk, id) box in id-major / chunk-minor order, ``box_begin`` (n + 1) offsets into ``boxes``."""

    def __init__(self, ids, sizes, rep_coords, boxes, box_begin):
        self.ids, self.sizes, self.rep_coords, self.boxes, self.box_begin = ids, sizes, rep_coords, boxes, box_begin

    def __len__(self):
        return len(self.ids)

    def as_dicts(self) -> List[dict]:
        """``[rep_coords, bounding_boxes, sizes]`` as the reference's workers return them: id -> [x, y, z], id -> list of
        [[min], [max + 1]] (one entry per chunk holding the id), id -> voxels."""
        keys = self.ids.tolist()
        per_id = np.split(self.boxes, self.box_begin[1:-1]) if len(keys) else []
        return [dict(zip(keys, self.rep_coords.tolist())), dict(zip(keys, (b.tolist() for b in per_id))),
                dict(zip(keys, self.sizes.tolist()))]


class MapTable:
    """Merged overlap counts of one organelle: rows (subcell id, cell id, voxels), ascending by subcell id, then cell id."""

    def __init__(self, sub_ids, cell_ids, counts):
        self.sub_ids, self.cell_ids, self.counts = sub_ids, cell_ids, counts

    def __len__(self):
        return len(self.sub_ids)

    @staticmethod
    def _nested(outer, inner, values) -> Dict[int, Dict[int, object]]:
        out: Dict[int, Dict[int, object]] = {}
        if len(outer) == 0:
            return out
        cut = np.flatnonzero(outer[1:] != outer[:-1]) + 1
        inner_l, values_l = inner.tolist(), values.tolist()
        for a, b in zip(np.concatenate(([0], cut)).tolist(), np.concatenate((cut, [len(outer)])).tolist()):
            out[int(outer[a])] = dict(zip(inner_l[a:b], values_l[a:b]))
        return out

    def as_dict(self) -> Dict[int, Dict[int, int]]:
        """subcell id -> cell id -> overlapping voxels."""
        return self._nested(self.sub_ids, self.cell_ids, self.counts)

    def ratios(self) -> np.ndarray:
        """Array form of ``convert_nvox2ratio_mapdict`` (sd_proc.py:1276-1285): every count divided by the mapped voxels of its
        subcellular object (float64, ``count / sum`` like the reference's division by a numpy integer)."""
        if len(self) == 0:
            return np.zeros(0, np.float64)
        heads = np.flatnonzero(np.concatenate(([True], self.sub_ids[1:] != self.sub_ids[:-1])))
        totals = np.add.reduceat(self.counts.astype(np.int64), heads)
        return self.counts / np.repeat(totals, np.diff(np.concatenate((heads, [len(self)]))))

    def inverted(self, values: Optional[np.ndarray] = None) -> Dict[int, Dict[int, object]]:
        """Array form of ``invert_mdc`` (sd_proc.py:1288-1297): cell id -> subcell id -> value (the counts, or e.g. ``ratios()``)."""
        values = self.counts if values is None else values
        order = np.lexsort((self.sub_ids, self.cell_ids))
        return self._nested(self.cell_ids[order], self.sub_ids[order], values[order])


# ---------------------------------------------------------------------------------------------------------------------------------
# device-side record accumulators
class _TableOverflow(Exception):
    """A hash table of ``sd_segstats_scan`` was too small for some chunk (seen late: the flags are read two chunks behind)."""

    def __init__(self, objects: bool, pairs: bool):
        super().__init__('segstats table overflow')
        self.objects, self.pairs = objects, pairs


class ChunkMerger:
    """Accumulates the per-chunk tables of one dataset pass on the device and merges them at the end.

    The host never waits for the chunk it has just queued: the append cursors and the overflow flags of the scans are copied to
    page-locked memory on a side stream after every chunk, and chunk k reads the copy posted after chunk k - 2 (complete by then,
    while the GPU still works on chunk k - 1).  Record arrays are kept large enough for what is known to be stored plus the
    pessimistic bound (a full table) of the two chunks in between."""
    LAG = 2

    def __init__(self, names: Sequence[str], min_obj_vx: dict, device, n_chunks: int, capacity: int = 1 << 16):
        import torch
        from .. import _dev as D
        self.device = torch.device(device)
        self.names = list(names)
        self.min_vx = {k: int(min_obj_vx.get(k, 1)) for k in ['sv'] + self.names}
        obj, pair = OBJECT_FIELDS, [('sub', 'int64', 1), ('cell', 'int64', 1), ('cnt', 'int64', 1)]
        n = len(self.names)
        self.counters = D.counters(self.device, 1 + 2 * n)                                      # cursors: cell, subs, pairs
        self.status = torch.zeros((max(int(n_chunks), 1), 2), dtype=torch.int32, device=self.device)      # overflow flags of every chunk's scan
        self.cell = Records(self.device, obj, capacity, self.counters[0:1])
        self.sub = [Records(self.device, obj, capacity, self.counters[1 + i:2 + i]) for i in range(n)]
        self.pairs = [Records(self.device, pair, capacity, self.counters[1 + n + i:2 + n + i]) for i in range(n)]
        self.n_chunks = 0
        self._side = torch.cuda.Stream(device=self.device)
        ring = self.LAG + 1
        self._host_counts = [torch.zeros(1 + 2 * n, dtype=torch.int64).pin_memory() for _ in range(ring)]
        self._host_status = [torch.zeros_like(self.status, device='cpu').pin_memory() for _ in range(ring)]
        self._posted = [torch.cuda.Event() for _ in range(ring)]
        self._known = np.zeros(1 + 2 * n, dtype=np.int64)      # cursor values as of the newest copy that has been read
        self._known_at = -1                                    # ... posted after this chunk

    def status_slot(self):
        """Where the scan of the next chunk writes its overflow flags (``DeviceScan.scan(status_out=...)``)."""
        return self.status[self.n_chunks]

    def _post(self, k: int):
        import torch
        r = k % (self.LAG + 1)
        ev = torch.cuda.current_stream(self.device).record_event()
        with torch.cuda.stream(self._side):
            self._side.wait_event(ev)
            self._host_counts[r].copy_(self.counters, non_blocking=True)
            self._host_status[r].copy_(self.status, non_blocking=True)
            self._posted[r].record(self._side)

    def _read(self, k: int):
        """Take in the copy posted after chunk k (waits for it); raises when a scan up to chunk k overflowed its tables."""
        if k <= self._known_at or k < 0:
            return
        r = k % (self.LAG + 1)
        self._posted[r].synchronize()
        self._known = self._host_counts[r].numpy().copy()
        self._known_at = k
        flags = self._host_status[r].numpy()[:k + 1]
        if flags.any():
            raise _TableOverflow(bool(flags[:, 0].any()), bool(flags[:, 1].any()))

    def add_chunk(self, scan, origin):
        """`scan`: a ``DeviceScan`` after ``scan(cell, subs, status_out=self.status_slot())`` over one chunk whose (x, y, z) origin in
        the dataset is `origin`."""
        from .. import _dev as D
        k, dev = self.n_chunks, self.device
        X, Y, Z = scan.shape
        ox, oy, oz = (int(v) for v in origin)
        cap_o, cap_p = scan.cap_obj, scan.cap_pair
        upper_o, upper_p = min(cap_o, X * Y * Z), min(cap_p, X * Y * Z)
        self._read(k - self.LAG)
        behind = k - 1 - self._known_at            # chunks appended since the counts that are known (at most LAG - 1 ... LAG)
        n = len(self.names)

        def settle(rec, idx, upper):
            rec.room_for(int(self._known[idx]) + behind * upper, upper)
        settle(self.cell, 0, upper_o)
        D.call('sd_chunkprops_append', dev, scan.cell_table, cap_o, X, Y, Z, ox, oy, oz, self.min_vx['sv'], *self.cell.ptrs(), self.cell.capacity,
               self.cell.cursor)
        for i, name in enumerate(self.names):
            tab = scan.sub_tables[i]
            settle(self.sub[i], 1 + i, upper_o)
            D.call('sd_chunkprops_append', dev, tab, cap_o, X, Y, Z, ox, oy, oz, self.min_vx[name], *self.sub[i].ptrs(), self.sub[i].capacity,
                   self.sub[i].cursor)
            settle(self.pairs[i], 1 + n + i, upper_p)
            D.call('sd_chunkpairs_append', dev, scan.ptabs[i], cap_p, tab, scan.cell_table, cap_o, X, Y, Z, self.min_vx[name],
                   *self.pairs[i].ptrs(), self.pairs[i].capacity, self.pairs[i].cursor)
        self._post(k)
        self.n_chunks += 1

    # -- end of the dataset ------------------------------------------------------------------------------------------------------
    def _scratch(self, n: int):
        """One scratch buffer for all merges of `finish` (sized for the largest record count)."""
        from .. import _dev as D, _lib as L
        need = L.load().sd_propmerge_temp_bytes(max(int(n), 1))
        if getattr(self, '_tmp', None) is None or self._tmp.numel() < need:
            self._tmp = D.empty(need, D.u8, self.device)
        return self._tmp

    def _merge_objects(self, rec: Records, n: int) -> PropTable:
        from .. import _dev as D
        assert n <= rec.capacity, 'record arrays overran (internal error: capacity bound)'
        if n == 0:
            return PropTable(np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros((0, 3), np.int64), np.zeros((0, 2, 3), np.int64),
                             np.zeros(1, np.int64))
        dev = self.device
        uniq, tot, rc = D.empty(n, D.i64, dev), D.empty(n, D.i64, dev), D.empty((n, 3), D.i32, dev)
        beg, bbs = D.empty(n, D.i32, dev), D.empty((n, 6), D.i32, dev)
        cnt = D.counters(dev, 1)
        tmp = self._scratch(n)
        a = rec.arrays
        D.call('sd_propmerge_objects', dev, a['ids'], a['sizes'], a['rc'], a['bb'], n, uniq, tot, rc, beg, bbs, cnt, tmp, tmp.numel())
        u = int(cnt.item())
        return PropTable(D.down(uniq, u, np.uint64), D.down(tot, u), D.down(rc, u).astype(np.int64),
                         D.down(bbs).astype(np.int64).reshape(n, 2, 3), segment_offsets(beg, u, n))

    def _merge_pairs(self, rec: Records, n: int) -> MapTable:
        from .. import _dev as D
        assert n <= rec.capacity, 'record arrays overran (internal error: capacity bound)'
        if n == 0:
            return MapTable(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int64))
        dev = self.device
        o_s, o_c, o_n = (D.empty(n, D.i64, dev) for _ in range(3))
        cnt = D.counters(dev, 1)
        tmp = self._scratch(n)
        a = rec.arrays
        D.call('sd_propmerge_pairs', dev, a['sub'], a['cell'], a['cnt'], n, o_s, o_c, o_n, cnt, tmp, tmp.numel())
        u = int(cnt.item())
        return MapTable(D.down(o_s, u, np.uint64), D.down(o_c, u, np.uint64), D.down(o_n, u))

    def finish(self):
        """-> (cell PropTable, {name: PropTable}, {name: MapTable})"""
        self._read(self.n_chunks - 1)              # every chunk's flags and the final cursors
        counts = [int(v) for v in self._known]
        n = len(self.names)
        self._scratch(max(counts) if counts else 1)
        return (self._merge_objects(self.cell, counts[0]), {nm: self._merge_objects(self.sub[i], counts[1 + i]) for i, nm in enumerate(self.names)},
                {nm: self._merge_pairs(self.pairs[i], counts[1 + n + i]) for i, nm in enumerate(self.names)})


# ---------------------------------------------------------------------------------------------------------------------------------
def map_subcell_extract_props(kd_seg_path: str, kd_organelle_paths: Dict[str, str], n_folders_fs: int = 1000,
                              n_folders_fs_sc: int = 1000, n_chunk_jobs: Optional[int] = None, n_cores: int = 1,
                              cube_of_interest_bb: Optional[Sequence] = None, chunk_size: Optional[Sequence[int]] = None,
                              log=None, overwrite=False, min_obj_vx: Optional[dict] = None, device=None, as_tables: bool = False,
                              chunk_loader: Optional[Callable] = None, table_capacity: Optional[int] = None):
    """Step 1 of the reference's function of this name (sd_proc.py:273-787): over a regular chunk grid (``fit_box_size=True``)
    read the cell segmentation and every organelle segmentation (``load_seg(...).swapaxes(0, 2)``, zeros beyond the dataset),
    gather per-object properties and organelle -> cell overlap counts, drop objects that lie purely inside a chunk and are
    smaller than ``config['cell_objects']['min_obj_vx'][name]``, and merge everything in dataset coordinates.

    Returns ``(cell_props, organelle_props, organelle_maps)``: ``[rc, bb, size]`` of the cell segmentation, ``{name: [rc, bb, size]}``
    and ``{name: {subcell id: {cell id: voxels}}}`` -- the dictionaries the reference's workers pickle for step 2; with
    ``as_tables=True`` the merged ``PropTable`` / ``MapTable`` objects instead (no per-object Python objects are built).
    ``chunk_loader(name, offset_xyz, size_xyz)`` (name ``'sv'`` = cell segmentation) may supply (x, y, z) label volumes, host or
    device, in the place of the KnossosDataset reads."""
    import torch
    from .. import global_params
    from ..extraction.find_object_properties import DeviceScan
    from ..knossos import ChunkDataset
    names = list(kd_organelle_paths.keys())
    kd = kd_factory(kd_seg_path)
    if chunk_loader is None:
        kds = {'sv': kd}
        for name, path in kd_organelle_paths.items():
            kds[name] = kd_factory(path)
            if not np.array_equal(kds[name].boundary, kd.boundary):
                raise ValueError("Data shape of subcellular structures '{}' differs from cell segmentation data. {} vs. {}".format(
                    name, kds[name].boundary, kd.boundary))

        def chunk_loader(name, offset, size):
            return np.ascontiguousarray(kds[name].load_seg(size=size, offset=offset, mag=1).swapaxes(0, 2))
    if min_obj_vx is None:
        min_obj_vx = global_params.config['cell_objects']['min_obj_vx']
    chunk_size = np.asarray([512, 512, 512] if chunk_size is None else chunk_size, dtype=np.int64)
    lo = np.zeros(3, dtype=np.int64) if cube_of_interest_bb is None else np.asarray(cube_of_interest_bb[0], dtype=np.int64)
    hi = np.asarray(kd.boundary, dtype=np.int64) if cube_of_interest_bb is None else np.asarray(cube_of_interest_bb[1], dtype=np.int64)
    cd = ChunkDataset()
    cd.initialize(kd, hi - lo, chunk_size, '', box_coords=lo, fit_box_size=True)
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    chunk_ids = sorted(cd.chunk_dict)
    nvox = int(np.prod(chunk_size))
    # table capacities: label volumes hold far fewer objects than voxels; a chunk that needs more is detected (two chunks late, the
    # host does not wait for the chunk it has just queued) and the pass is repeated with 4x the capacity
    cap_obj = cap_pair = 1 << max(10, int((table_capacity or min(2 * nvox, max(1 << 16, nvox // 256))) - 1).bit_length())
    with torch.cuda.device(device):
        while True:
            scan = DeviceScan(device, cap_obj, cap_pair)
            merger = ChunkMerger(names, min_obj_vx, device, len(chunk_ids))
            try:
                for ch_id in chunk_ids:
                    origin = np.asarray(cd.chunk_dict[ch_id].coordinates, dtype=np.int64)
                    subs = [chunk_loader(n, origin, chunk_size) for n in names]
                    scan.scan(chunk_loader('sv', origin, chunk_size), subs, status_out=merger.status_slot())
                    merger.add_chunk(scan, origin)
                cell_t, sub_t, map_t = merger.finish()
                break
            except _TableOverflow as e:
                if e.objects:
                    if cap_obj >= 2 * nvox:
                        raise RuntimeError('sd_segstats_scan: object table overflow at maximum capacity')
                    cap_obj *= 4
                if e.pairs:
                    cap_pair *= 4
    if as_tables:
        return cell_t, sub_t, map_t
    return cell_t.as_dicts(), {n: t.as_dicts() for n, t in sub_t.items()}, {n: t.as_dict() for n, t in map_t.items()}


def mesh_objects(kd_seg_path: str, kd_organelle_paths: Dict[str, str], cube_of_interest_bb: Optional[Sequence] = None,
                 chunk_size: Optional[Sequence[int]] = None, device=None, chunk_loader: Optional[Callable] = None,
                 generate_sv_mesh: bool = False, scaling: Optional[Sequence[float]] = None):
    """The meshing part of the reference's ``map_subcell_extract_props`` (sd_proc.py:687-770 per chunk, :957-964 over chunks) as a pass of
    its own: over the chunk grid and with the loader convention of ``map_subcell_extract_props`` above, every organelle chunk (and the
    cell chunk with `generate_sv_mesh`) is meshed by ``find_meshes_table(chunk, origin, pad=1, ds=config['meshes']['downsampling'][kind])``
    and the per-chunk tables are merged in ASCENDING CHUNK ORDER (the reference merges in the order of a dictionary of workers).
    Returns ``{kind: MeshTable}`` (the cell segmentation under ``'sv'``).  The size thresholds and the ``mesh_bb`` fallbacks of step 2
    are ``proc.meshes.mesh_props`` over the merged ``PropTable``."""
    import torch
    from .. import global_params
    from ..knossos import ChunkDataset
    from .meshes import MeshTable, find_meshes_table
    kinds = list(kd_organelle_paths.keys()) + (['sv'] if generate_sv_mesh else [])
    kd = kd_factory(kd_seg_path)
    if chunk_loader is None:
        kds = {'sv': kd}
        for name, path in kd_organelle_paths.items():
            kds[name] = kd_factory(path)
            if not np.array_equal(kds[name].boundary, kd.boundary):
                raise ValueError("Data shape of subcellular structures '{}' differs from cell segmentation data. {} vs. {}".format(
                    name, kds[name].boundary, kd.boundary))

        def chunk_loader(name, offset, size):
            return np.ascontiguousarray(kds[name].load_seg(size=size, offset=offset, mag=1).swapaxes(0, 2))
    downsampling = global_params.config['meshes']['downsampling']
    scaling = global_params.config['scaling'] if scaling is None else scaling
    chunk_size = np.asarray([512, 512, 512] if chunk_size is None else chunk_size, dtype=np.int64)
    lo = np.zeros(3, dtype=np.int64) if cube_of_interest_bb is None else np.asarray(cube_of_interest_bb[0], dtype=np.int64)
    hi = np.asarray(kd.boundary, dtype=np.int64) if cube_of_interest_bb is None else np.asarray(cube_of_interest_bb[1], dtype=np.int64)
    cd = ChunkDataset()
    cd.initialize(kd, hi - lo, chunk_size, '', box_coords=lo, fit_box_size=True)
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    pieces = {k: [] for k in kinds}
    with torch.cuda.device(device):
        for ch_id in sorted(cd.chunk_dict):
            origin = np.asarray(cd.chunk_dict[ch_id].coordinates, dtype=np.int64)
            for kind in kinds:
                chunk = chunk_loader(kind, origin, chunk_size)
                if isinstance(chunk, torch.Tensor) and chunk.dtype != torch.int64:
                    chunk = chunk.to(torch.int64)
                pieces[kind].append(find_meshes_table(chunk, origin, pad=1, ds=downsampling[kind], scaling=scaling, device=device))
        return {kind: MeshTable.merge(pieces[kind], device=device) for kind in kinds}


# ---------------------------------------------------------------------------------------------------------------------------------
# The reference's dictionary helpers, kept by name and contract for callers that hold dictionaries (the driver above works on
# tables).  Each merges IN PLACE into the first element, as sd_proc.py:1248-1322 do.
def merge_prop_dicts(prop_dicts: List[List[dict]], offset: Optional[np.ndarray] = None):
    """``prop_dicts[0]`` = running ``[rep_coords, bounding_boxes, sizes]`` (its second entry maps id -> list of boxes); every further
    triple is one chunk: its coordinates and boxes are shifted by `offset`, its representative coordinates replace earlier ones,
    its boxes are appended, its sizes added.  A triple without objects is skipped."""
    into_rc, into_bb, into_sz = prop_dicts[0]
    shift = np.zeros(3, dtype=np.int64) if offset is None else np.asarray(offset)
    for rc, bb, sz in prop_dicts[1:]:
        if not rc:
            continue
        keys = list(bb)
        boxes = (np.asarray([bb[k] for k in keys]).reshape(len(keys), 2, 3) + shift).tolist()
        rc_keys = list(rc)
        into_rc.update(zip(rc_keys, (np.asarray([rc[k] for k in rc_keys]).reshape(len(rc_keys), 3) + shift).tolist()))
        for k, box in zip(keys, boxes):
            into_bb.setdefault(k, []).append(box)
        for k, n in sz.items():
            into_sz[k] = into_sz.get(k, 0) + n


def merge_map_dicts(map_dicts):
    """``map_dicts[0]`` = running ``subcell id -> cell id -> voxels``; the others are added to it (an id new to the running
    dictionary contributes its inner dictionary itself, not a copy)."""
    into = map_dicts[0]
    for chunk_map in map_dicts[1:]:
        for sub_id, cells in chunk_map.items():
            known = into.get(sub_id)
            if known is None:
                into[sub_id] = cells
                continue
            for cell_id, n in cells.items():
                known[cell_id] = known.get(cell_id, 0) + n


def convert_nvox2ratio_mapdict(map_dc):
    """Overlap voxel counts -> fractions of each subcellular object's mapped voxels, in place (float64 true division)."""
    for cells in map_dc.values():
        counts = np.fromiter(cells.values(), dtype=np.int64, count=len(cells))
        cells.update(zip(list(cells), counts / counts.sum()))


def invert_mdc(mapping_dict):
    """``subcell id -> cell id -> value`` -> ``cell id -> subcell id -> value``."""
    out: Dict[int, dict] = {}
    for sub_id, cells in mapping_dict.items():
        for cell_id, value in cells.items():
            out.setdefault(cell_id, {})[sub_id] = value
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# view predictions per supervoxel (proc/sd_proc.py:1345-1432)
def _views_device(who, views, dev):
    """The per-object view arrays (host uint8 or device tensors, (n_i, C, nb_views, H, W)) as ONE device tensor and the partition."""
    import torch
    tens = []
    for k, v in enumerate(views):
        t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 5:
            raise ValueError(f'{who}: views[{k}] must be a uint8 array or tensor (n, C, nb_views, H, W)')
        tens.append(t)
    if not tens:
        raise ValueError(f'{who}: no views')
    if len({tuple(t.shape[1:]) for t in tens}) != 1:
        raise ValueError(f'{who}: the view arrays differ in channels, views per location or window')
    part_views = np.cumsum([0] + [len(t) for t in tens])
    return torch.cat([t.to(dev) for t in tens], 0), part_views


def predict_views(model, views, ch=None, pred_key=None, single_cc_only=False, verbose=False, return_proba=False, nb_cpus=1, background=1):
    """``predict_views`` (proc/sd_proc.py:1386-1427).  `views`: one uint8 array or device tensor (n_i, C, nb_views, H, W) per object.
    With `single_cc_only` every plane of channel 0 goes through ``single_conn_comp_img`` -- one ``sd_views_center_component`` call for
    the whole batch; for the two views of the glia model these are the reference's two calls per location --, with `background` as
    its background value: 1 as in the reference, whose call leaves ``single_conn_comp_img``'s default in place although the renderer
    paints 255.  Then ONE ``model.predict_proba`` call over all locations; -> with `return_proba` the list of per-object slices
    (n_i, classes); otherwise the slices are stored as ``so.attr_dict[pred_key]`` of the objects in `ch` (there is no storage layer, so
    `nb_cpus` has nothing to parallelise).  The caller's arrays are not modified (the reference filters them in place)."""
    from .. import _dev as D
    from .image import center_component_planes
    who = 'predict_views'
    views = list(views)
    if not return_proba:
        if ch is None or pred_key is None:
            raise ValueError(f'{who}: storing the probabilities needs the objects (ch) and pred_key')
        ch = list(ch)
        if len(ch) != len(views):
            raise ValueError(f'{who}: {len(views)} view arrays for {len(ch)} objects')
    dev = getattr(model, 'dev', None)
    dev = D.device(None) if dev is None else dev
    flat, part_views = _views_device(who, views, dev)
    assert len(part_views) == len(views) + 1
    if single_cc_only and len(flat):
        if flat.shape[1] == 1:
            center_component_planes(flat, background, out=flat)
        else:
            flat[:, 0] = center_component_planes(flat[:, 0].contiguous(), background)
    probas = model.predict_proba(flat, verbose=verbose)
    so_probas = [probas[part_views[ii]:part_views[ii + 1]] for ii in range(len(views))]
    if return_proba:
        return so_probas
    for so, prob in zip(ch, so_probas):
        so.attr_dict[pred_key] = prob


def predict_sos_views(model, sos, pred_key, nb_cpus=1, woglia=True, verbose=False, raw_only=False, single_cc_only=False, return_proba=False,
                      background=1):
    """``predict_sos_views`` (proc/sd_proc.py:1345-1383) over objects that have ``load_views(woglia=, raw_only=)`` and ``attr_dict``:
    ``predict_views`` in chunks of about 200 objects, cut round-robin as the reference cuts them (``chunkify``), so with `return_proba`
    the rows follow the chunks.  `raw_only` keeps channel 0 of a view array that has more."""
    from ..handler.basics import chunkify
    sos = list(sos)
    all_probas = []
    for ch in chunkify(sos, max(1, len(sos) // 200)):
        views = [sv.load_views(woglia=woglia, raw_only=raw_only) for sv in ch]
        if raw_only:
            views = [v[:, :1] if v.shape[1] > 1 else v for v in views]
        proba = predict_views(model, views, ch, pred_key, verbose=False, single_cc_only=single_cc_only, return_proba=return_proba,
                              nb_cpus=nb_cpus, background=background)
        if return_proba:
            all_probas.append(np.concatenate(proba))
    if return_proba:
        return np.concatenate(all_probas)
