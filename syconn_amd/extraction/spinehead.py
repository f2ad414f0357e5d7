"""Spine head volumes on the device: the per-window steps of ``extract_spinehead_volume_mesh``
(/root/reference/syconn/reps/super_segmentation_helper.py:2068-2198) as thin wrappers of the ``sd_spinehead_*`` entries, ``sd_edt_squared``,
``sd_marker_flood`` and ``sd_syn_props_knn``, and the batch driver behind ``cs_processing_steps.calculate_spinehead_volume``.

One window = one spine-head synapse: a ``2 * ctx_vol`` box of the cell segmentation, zoomed to isotropic voxels, masked to the cell's
supervoxels, holes filled; the squared distance transform; its local maxima (``peak_local_max``, restated, parity-UNPINNED); a vote of
the ``k`` nearest mesh vertices per maximum; the marker flood; the 6-connected ``label == 1`` object next to the synapse and its voxel
count.  Windows of a cell run in batches on one stream: the stages of every window are queued without reading anything back, the
vertices in the boxes of the whole batch are compacted in one call (their total is the one value read per batch before the vote), one
``sd_syn_props_knn`` call votes for all maxima of the batch, and the per-window results come back in one copy.  No CPU fallback."""
import numpy as np


BATCH = 8                    # windows per batch (device buffers are sized for this many)
REGION_VOX = 256             # windows read from a KnossosDataset are grouped into spatial buckets of this many voxels per axis: with the
                             # reference's 400 x 400 x 200 windows a region of 8-byte ids stays below 656 x 656 x 456 voxels = 1.6 GB
REGION_BYTES = 2 << 30       # a group whose bounding box holds more is read window by window


def zoom_source_table(n_in: int, ds) -> np.ndarray:
    """Source index of every output sample of ``scipy.ndimage.zoom(a, 1 / ds, order=0)`` along an axis of `n_in` samples (mode
    'constant', cval 0, grid_mode False), int32; -1 where scipy writes the constant.  scipy's own arithmetic: ``n_out = round(n_in *
    zoom)``, coordinate ``i * ((n_in - 1) / (n_out - 1))`` in double, beyond ``n_in - 1``: the constant, else ``floor(c + 0.5)``."""
    n_in = int(n_in)
    zoom = float(1 / ds)
    if n_in < 1 or not zoom > 0:
        raise ValueError(f'zoom_source_table: n_in = {n_in}, ds = {ds}')
    n_out = int(round(n_in * zoom))
    if n_out < 1:
        raise ValueError(f'zoom of {n_in} samples by 1 / {ds} leaves no sample')
    step = (n_in - 1) / (n_out - 1) if n_out > 1 else 1.0
    c = np.arange(n_out, dtype=np.float64) * np.float64(step)
    idx = np.floor(c + 0.5).astype(np.int64)
    return np.where(c > n_in - 1, -1, idx).astype(np.int32)


def plan_regions(offsets, size, batch, bucket=None, max_bytes=None):
    """How the windows at `offsets` (n, 3) of `size` voxels are read from a dataset: -> list of (window rows, lo, hi), one resident
    region [lo, hi) per entry and at most `batch` windows in it.  Windows are grouped by the bucket of `bucket` voxels per axis their
    offset falls in (as ``map_myelin2coords`` groups its nodes), so a region never exceeds ``bucket + size`` per axis; a group whose
    bounding box still holds more than `max_bytes` of 8-byte ids is read window by window."""
    bucket = REGION_VOX if bucket is None else int(bucket)
    max_bytes = REGION_BYTES if max_bytes is None else int(max_bytes)
    offsets = np.asarray(offsets, np.int64).reshape(-1, 3)
    size = np.asarray(size, np.int64)
    plan = []
    if not len(offsets):
        return plan
    _, inv = np.unique(np.floor_divide(offsets, bucket), axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    for g in range(int(inv.max()) + 1):
        rows = np.flatnonzero(inv == g)
        for b0 in range(0, len(rows), int(batch)):
            ix = rows[b0:b0 + int(batch)]
            lo, hi = offsets[ix].min(0), offsets[ix].max(0) + size
            if len(ix) > 1 and int(np.prod(hi - lo)) * 8 > max_bytes:
                plan.extend((ix[j:j + 1], offsets[ix[j]], offsets[ix[j]] + size) for j in range(len(ix)))
            else:
                plan.append((ix, lo, hi))
    return plan


class WindowRunner:
    """Device buffers for batches of up to `batch` windows of `shape` zoomed voxels and the stage calls on the current stream."""

    def __init__(self, shape, batch: int = BATCH, max_peaks=None, device=None):
        import torch
        from .. import _dev as D
        self.dev = D.device(device)
        self.X, self.Y, self.Z = (int(v) for v in shape)
        self.nvox = self.X * self.Y * self.Z
        if min(self.X, self.Y, self.Z) < 1 or self.nvox >= 2 ** 31 or max(self.X, self.Y, self.Z) > 18000:
            raise ValueError(f'window of {shape} voxels: every extent must be in 1..18000 and the volume below 2^31 voxels')
        self.batch = int(batch)
        self.cap = int(min(self.nvox, 1 << 20) if max_peaks is None else max_peaks)
        if self.batch < 1 or self.cap < 1 or self.batch * self.cap >= 2 ** 31:
            raise ValueError(f'batch = {batch}, max_peaks = {max_peaks}: need batch >= 1, max_peaks >= 1, batch * max_peaks < 2^31')
        B, dev, sh = self.batch, self.dev, (self.X, self.Y, self.Z)
        self.ws = D.scratch('sd_spinehead_workspace_bytes', dev, *sh)
        self.ws_bytes = self.ws.numel()
        self.mask = torch.empty(sh, dtype=torch.uint8, device=dev)
        self.filled = torch.empty((B,) + sh, dtype=torch.uint8, device=dev)
        self.d2 = torch.empty((B,) + sh, dtype=torch.int32, device=dev)
        self.peaks = torch.empty((B, self.cap, 3), dtype=torch.int32, device=dev)
        self.markers = torch.empty(sh, dtype=torch.int32, device=dev)
        self.flood = torch.empty(sh, dtype=torch.int32, device=dev)
        self.max_label = torch.zeros(1, dtype=torch.int32, device=dev)
        # one buffer, one copy back per batch: int32 (B, 8) per window = filled voxels, peaks, head voxels, chosen id, nb_obj; then the
        # eight int64 counters of the vote
        self.buf = torch.zeros(B * 4 + 8, dtype=torch.int64, device=dev)
        self.res32 = self.buf[:B * 4].view(torch.int32).view(B, 8)
        self.knn_counts = self.buf[B * 4:]
        self.q_slots, self.q_cell, self.q_xyz, self.votes = 0, None, None, None      # sized by the peak counts of a batch (vote)

    # -- stages; every one only queues work ---------------------------------------------------------------------------------------------
    def window_mask(self, seg_d, origin, offset, tabs, sv_d, out=None):
        from .. import _dev as D
        out = self.mask if out is None else out
        VX, VY, VZ = (int(v) for v in seg_d.shape)
        D.call('sd_spinehead_window_mask', self.dev, seg_d, VX, VY, VZ, D.i64x3(origin), D.i64x3(offset), *tabs, self.X, self.Y, self.Z, sv_d,
               int(sv_d.numel()), out)
        return out

    def fill_holes(self, mask, w):
        from .. import _dev as D
        D.call('sd_spinehead_fill_holes', self.dev, mask, self.X, self.Y, self.Z, self.filled[w], self.res32[w, 0:], self.ws, self.ws_bytes)
        return self.filled[w]

    def edt(self, w):
        from .. import _dev as D
        D.call('sd_edt_squared', self.dev, self.filled[w], self.X, self.Y, self.Z, self.d2[w], self.ws, self.ws_bytes)
        return self.d2[w]

    def find_peaks(self, w):
        from .. import _dev as D
        D.call('sd_spinehead_peaks', self.dev, self.filled[w], self.d2[w], self.X, self.Y, self.Z, self.peaks[w], self.cap, self.res32[w, 1:],
               self.ws, self.ws_bytes)

    def box_vertices(self, verts_d, labels_d, offsets, size):
        """The vertices inside the boxes of the windows at `offsets` (n, 3): (points float64 (m, 3) relative to their window, labels
        int32 (m), begin (n + 2) as a host array).  Reads `begin` and, in the same copy, the peak counts of the windows (``self.n_peaks``)
        back: the one synchronisation of a batch before its results."""
        import torch
        from .. import _dev as D
        n_win, n_verts = len(offsets), int(verts_d.shape[0])
        begin_d = D.counters(self.dev, n_win + 2)
        if n_verts == 0:
            self.n_peaks = np.zeros(n_win, np.int64)
            return torch.zeros((0, 3), dtype=torch.float64, device=self.dev), torch.zeros(0, dtype=torch.int32, device=self.dev), begin_d.cpu().numpy()
        if n_verts * n_win >= 2 ** 31:
            raise ValueError(f'{n_verts} vertices x {n_win} windows per batch: the product must stay below 2^31 (use a smaller batch)')
        off_d = D.up(np.asarray(offsets, dtype=np.int64), self.dev)
        tmp = D.scratch('sd_spinehead_box_vertices_temp_bytes', self.dev, n_verts, n_win)
        size_c = D.i32x3(size)
        f32 = int(verts_d.dtype == torch.float32)

        def call(stages, pts, lab, cap):
            D.call('sd_spinehead_box_vertices', self.dev, verts_d, f32, labels_d, n_verts, off_d, n_win, size_c, stages, begin_d, pts, lab, cap,
                   tmp, tmp.numel())
        call(1, None, None, 0)
        both = torch.cat([begin_d, self.res32[:n_win, 1].to(torch.int64)]).cpu().numpy()
        begin, self.n_peaks = both[:n_win + 2], both[n_win + 2:]
        total = int(begin[n_win])
        pts, lab = D.empty((total, 3), D.f64, self.dev), D.empty(total, D.i32, self.dev)
        if total:
            call(2, pts, lab, total)
        self._begin_d = begin_d
        return pts[:total], lab[:total], begin

    def vote(self, n_win, pts, lab, ds, k):
        """One ``sd_syn_props_knn`` call for the maxima of windows 0 .. n_win - 1 against the segmented vertex set of `box_vertices`;
        every window gets as many query slots as the largest peak count of the batch (read back with the vertex offsets)."""
        from .. import _dev as D
        slots = int(max(1, min(self.cap, int(self.n_peaks[:n_win].max()))))
        if self.q_cell is None or self.q_cell.numel() < n_win * slots:
            self.q_cell = D.empty(n_win * slots, D.i32, self.dev)
            self.q_xyz = D.empty((n_win * slots, 3), D.f64, self.dev)
            self.votes = D.empty(n_win * slots, D.i32, self.dev)
        self.q_slots = slots
        self._n_peaks_d = self.res32[:n_win, 1].contiguous()        # (a device-side copy: the counts of the batch as one array)
        D.call('sd_spinehead_queries', self.dev, self.peaks, self._n_peaks_d, n_win, self.cap, slots, D.f64x3(ds), self.q_cell, self.q_xyz)
        n_pts = int(pts.shape[0])
        tmp = D.scratch('sd_syn_props_knn_temp_bytes', self.dev, n_pts, n_win + 1)
        D.call('sd_syn_props_knn', self.dev, pts, 0, self._begin_d, n_win + 1, n_pts, lab, self.q_cell, self.q_xyz, n_win * slots, int(k), 3,
               self.votes, None, None, self.knn_counts, tmp, tmp.numel())
        self._knn_tmp = tmp

    def flood_select(self, w, c_rel, offset, scaling, objects=None):
        from .. import _dev as D
        v = self.votes[w * self.q_slots:]                          # (a window with more peaks than max_peaks raises after the batch)
        D.call('sd_spinehead_markers', self.dev, self.peaks[w], self.res32[w, 1:], v, self.q_slots, self.X, self.Y, self.Z, self.markers)
        D.call('sd_marker_flood', self.dev, self.d2[w], self.markers, self.filled[w], self.X, self.Y, self.Z, self.flood, self.max_label,
               self.ws, self.ws_bytes)
        D.call('sd_spinehead_select', self.dev, self.flood, self.X, self.Y, self.Z, D.i64x3(c_rel), D.i64x3(offset), D.f64x3(scaling), objects,
               self.res32[w, 2:], self.ws, self.ws_bytes)

    # -- one batch ----------------------------------------------------------------------------------------------------------------------
    def run_batch(self, seg_d, origin, offsets, tabs, sv_d, verts_d, labels_d, size, ds, k, c_rel, scaling, keep=None):
        """Windows at `offsets` (n <= batch, (n, 3) int64) -> host int64 (n, 6): filled voxels, peaks, head voxels, chosen id, nb_obj,
        vertices in the box (0: the reference writes no entry).  `keep`: an optional list that receives per-window dicts of the stage
        volumes (device tensors), for the tests."""
        n = len(offsets)
        assert 1 <= n <= self.batch
        self.buf.zero_()
        for w in range(n):
            mask = self.window_mask(seg_d, origin, offsets[w], tabs, sv_d)
            self.fill_holes(mask, w)
            self.edt(w)
            self.find_peaks(w)
            if keep is not None:
                keep.append(dict(mask=mask.clone()))
        pts, lab, begin = self.box_vertices(verts_d, labels_d, offsets, size)
        n_box = np.diff(begin[:n + 1])
        if len(pts):
            self.vote(n, pts, lab, ds, k)
        for w in range(n):
            if n_box[w] == 0:
                continue
            objects = self.flood.new_empty(self.flood.shape) if keep is not None else None
            self.flood_select(w, c_rel[w], offsets[w], scaling, objects)
            if keep is not None:
                keep[len(keep) - n + w].update(markers=self.markers.clone(), flood=self.flood.clone(), objects=objects)
        buf = self.buf.cpu().numpy()                              # the one copy back of the batch
        r32 = buf[:self.batch * 4].view(np.int32).reshape(self.batch, 8)
        if len(pts) and int(buf[self.batch * 4 + 7]):
            raise RuntimeError('sd_syn_props_knn: an offset, a cell row or a point row was out of range')
        out = np.zeros((n, 6), np.int64)
        out[:, :5] = r32[:n, :5]
        out[:, 5] = n_box
        if keep is not None:
            for w in range(n):
                m = int(min(out[w, 1], self.cap))
                keep[len(keep) - n + w].update(filled=self.filled[w].clone(), d2=self.d2[w].clone(), peaks=self.peaks[w, :m].clone(),
                                               votes=self.votes[w * self.q_slots:w * self.q_slots + m].clone() if n_box[w] else None,
                                               points=pts[begin[w]:begin[w + 1]].clone(), point_labels=lab[begin[w]:begin[w + 1]].clone())
        return out


def check_scaling(scaling):
    """The voxel size as the array ``SuperSegmentationObject.scaling`` is (``np.array(config['scaling'])``, its dtype kept: the
    reference's arithmetic follows from it) and ``ds = scaling[2] // scaling`` (:2125)."""
    sc = np.array(scaling)
    if sc.shape != (3,) or sc.dtype.kind not in 'iuf' or not np.all(np.isfinite(sc.astype(np.float64))) or not np.all(sc > 0):
        raise ValueError(f'scaling must be three positive voxel sizes, got {scaling}')
    ds = sc[2] // sc
    if not np.all(ds > 0):
        raise ValueError(f'scaling {scaling}: the z voxel size must be the largest (ds = scaling[2] // scaling > 0)')
    return sc, ds


def spinehead_windows(seg, sv_ids, rep_coords, verts_vox, vert_labels, scaling, ctx_vol, k, device=None, batch=BATCH, max_peaks=None,
                      syn_ids=None, keep=None, runner=None):
    """The loop of :2130-2198 for one cell: `rep_coords` (n, 3) of its spine-head synapses, `verts_vox` = ``mesh / scaling`` without the
    ignored labels (float32 or float64, as numpy made them) with `vert_labels`.  -> host int64 (n, 6) in the order of `rep_coords`, see
    ``WindowRunner.run_batch``.  `runner`: a ``WindowRunner`` of the same window shape to reuse (one per call otherwise).  A
    KnossosDataset is read region by region (``plan_regions``).  ValueError: a window whose filled mask is empty (the reference's
    message)."""
    import torch
    from .. import _dev as D
    dev = D.device(device)
    sc, ds = check_scaling(scaling)
    ctx = np.array(ctx_vol)
    if ctx.shape != (3,) or ctx.dtype.kind not in 'iu' or np.any(ctx < 1):
        raise ValueError(f'ctx_vol must be three positive integers, got {ctx_vol}')
    ctx = ctx.astype(np.int64)
    size = (2 * ctx).astype(np.int32)
    rep = np.ascontiguousarray(rep_coords, dtype=np.int64).reshape(-1, 3)
    n = len(rep)
    sv = np.unique(np.ascontiguousarray(sv_ids, dtype=np.uint64).reshape(-1))
    if not len(sv):
        raise ValueError('the cell has no supervoxel')
    syn_ids = np.arange(n, dtype=np.uint64) if syn_ids is None else np.asarray(syn_ids)
    tabs_h = [zoom_source_table(int(size[a]), ds[a]) for a in range(3)]
    shape = [len(t) for t in tabs_h]
    if runner is None or [runner.X, runner.Y, runner.Z] != shape or runner.batch != int(batch) or runner.dev != dev:
        runner = WindowRunner(shape, batch, max_peaks, dev)
    tabs = [D.up(t, dev) for t in tabs_h]
    sv_d = D.up(sv, dev)
    verts_vox = np.asarray(verts_vox)
    verts_d = D.up(np.asarray(verts_vox, dtype=np.float32 if verts_vox.dtype == np.float32 else np.float64).reshape(-1, 3), dev)
    labels_d = D.up(np.asarray(vert_labels, dtype=np.int32).reshape(-1), dev)
    offsets = np.maximum(rep - ctx, 0)                             # offset[offset < 0] = 0 (:2131-2132)
    c_rel = rep - offsets
    out = np.zeros((n, 6), np.int64)
    keeps = [] if keep is not None else None
    if hasattr(seg, 'load_seg'):                                   # bounded regions, each resident for the windows that share it
        plan = plan_regions(offsets, size, runner.batch)
    else:
        vol, origin = seg
        if isinstance(vol, np.ndarray):
            vol = torch.from_numpy(np.ascontiguousarray(vol).astype(np.uint64, copy=False).view(np.int64))
        if vol.dim() != 3 or vol.dtype not in (torch.int64, torch.uint64):
            raise ValueError('seg must be an (x, y, z) volume of 64-bit ids with its origin, or a KnossosDataset')
        seg_d = vol.to(dev).contiguous()
        plan = [(np.arange(b0, min(b0 + runner.batch, n)), None, None) for b0 in range(0, n, runner.batch)]
    order = np.concatenate([ix for ix, _, _ in plan]) if plan else np.zeros(0, np.int64)
    for ix, lo, hi in plan:
        if lo is not None:
            region = seg.load_seg(size=hi - lo, offset=lo, mag=1)  # (z, y, x), zeros outside the dataset
            seg_d = D.up(region.swapaxes(2, 0).astype(np.uint64, copy=False), dev)
            origin = lo
        out[ix] = runner.run_batch(seg_d, origin, offsets[ix], tabs, sv_d, verts_d, labels_d, size, ds.astype(np.float64), k, c_rel[ix],
                                   sc.astype(np.float64), keeps)
    if keep is not None:
        back = np.argsort(order)
        keep.extend(keeps[i] for i in back)
    for i in range(n):                                             # the reference stops at the first such window (:2144-2148)
        if out[i, 0] == 0:
            raise ValueError(f'Could not find segmentation at {offsets[i]} and size {size} for SSVs {sv}. syn_ssv ID: {syn_ids[i]}.')
    for i in range(n):
        if out[i, 0] == runner.nvox:
            raise ValueError(f'the window at {offsets[i]} lies completely inside the cell: the distance transform has no background to measure '
                             f'from (scipy leaves it undefined). syn_ssv ID: {syn_ids[i]}.')
        if out[i, 1] > runner.cap:
            raise RuntimeError(f'{out[i, 1]} distance maxima in the window at {offsets[i]}, room for {runner.cap}: raise max_peaks')
    return out


def head_volume(n_voxels, scaling, ds):
    """``n_voxels_spinehead * np.prod(scaling * ds) / 1e9`` (:2197) in the reference's dtypes, um^3."""
    return np.asarray(n_voxels) * np.prod(scaling * ds) / 1e9
