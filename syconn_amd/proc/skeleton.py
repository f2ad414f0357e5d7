"""Cell skeletons from labelled chunks (the reference's ``proc/skeleton.py``): the TEASAR tracing of a chunk on the device and the
tables it fills.  ``kimimaro`` is not part of the reference tree, so the tracing follows the rules written down in DESIGN.md section 7
(stated, not pinned); ``trace_chunk`` drives the device entries of ``csrc/sd_skeletonize.hip`` stage by stage.  numpy only on the host:
no scipy, no networkx.

The host post-processing restates the reference's own ``sparsify_skelcv``, ``sparsify_skeleton_fast``, ``stitch_skel_nx`` and the flow of
``kimimaro_mergeskels`` with their visiting orders (pinned by tests/golden/g33_skeleton_post.npz); ``downsample``, ``simple_merge`` and
``consolidate`` are cloudvolume's and therefore stated.  The chunk driver is ``exec/exec_skeleton.py: run_kimimaro_skeletonization``.

Not built: soma mode, ``fix_borders``, ``fill_holes``, ``kimimaro.postprocess``, non-integer anisotropy, the
mesh-based fallback ``create_sso_skeleton_fast``, storages and batch jobs."""
import numpy as np

_TEMP, _EMIT_TEMP = 'sd_skeletonize_temp_bytes', 'sd_skeletonize_emit_temp_bytes'      # the two scratch sizers of the chain
TEASAR_DEFAULTS = dict(scale=2, const=500, pdrf_exponent=4, pdrf_scale=100000, max_paths=100)      # proc/skeleton.py:57-67


class Skeleton:
    """``vertices`` float32 (n, 3) nm, ``edges`` int64 (m, 2), ``radii`` float32 (n,): the fields of ``cloudvolume.Skeleton`` the
    reference uses."""

    def __init__(self, vertices=None, edges=None, radii=None):
        self.vertices = np.zeros((0, 3), np.float32) if vertices is None else np.asarray(vertices, np.float32).reshape(-1, 3)
        self.edges = np.zeros((0, 2), np.int64) if edges is None else np.asarray(edges, np.int64).reshape(-1, 2)
        self.radii = np.zeros(len(self.vertices), np.float32) if radii is None else np.asarray(radii, np.float32).reshape(-1)
        if len(self.radii) != len(self.vertices):
            raise ValueError('Skeleton: one radius per vertex')
        if self.edges.size and (self.edges.min() < 0 or self.edges.max() >= len(self.vertices)):
            raise ValueError('Skeleton: an edge names a vertex that does not exist')


class SkeletonTable:
    """Skeletons of many cells as columns: ``ids`` uint64 ascending; cell k owns ``nodes[node_begin[k]:node_begin[k + 1]]`` (float32 nm),
    the ``radii`` of the same rows and ``edges[edge_begin[k]:edge_begin[k + 1]]`` (int64, node indices INSIDE the cell)."""

    def __init__(self, ids, nodes, node_begin, edges, edge_begin, radii):
        self.ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        self.nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 3)
        self.node_begin = np.ascontiguousarray(node_begin, np.int64).reshape(-1)
        self.edges = np.ascontiguousarray(edges, np.int64).reshape(-1, 2)
        self.edge_begin = np.ascontiguousarray(edge_begin, np.int64).reshape(-1)
        self.radii = np.ascontiguousarray(radii, np.float32).reshape(-1)
        n = len(self.ids)
        if len(self.node_begin) != n + 1 or len(self.edge_begin) != n + 1:
            raise ValueError('SkeletonTable: node_begin and edge_begin hold one offset per cell and one more')
        for name, b, total in (('node_begin', self.node_begin, len(self.nodes)), ('edge_begin', self.edge_begin, len(self.edges))):
            if b[0] != 0 or b[-1] != total or (np.diff(b) < 0).any():
                raise ValueError(f'SkeletonTable: {name} must ascend from 0 to the number of rows')
        if len(self.radii) != len(self.nodes):
            raise ValueError('SkeletonTable: one radius per node')
        if n > 1 and (self.ids[1:] <= self.ids[:-1]).any():
            raise ValueError('SkeletonTable: ids must ascend strictly')
        if len(self.edges):
            size = np.repeat(np.diff(self.node_begin), np.diff(self.edge_begin))
            if (self.edges < 0).any() or (self.edges >= size[:, None]).any():
                raise ValueError('SkeletonTable: an edge names a node outside its cell')

    @classmethod
    def empty(cls):
        return cls(np.zeros(0, np.uint64), np.zeros((0, 3), np.float32), [0], np.zeros((0, 2), np.int64), [0], np.zeros(0, np.float32))

    def __len__(self):
        return len(self.ids)

    def as_dict(self):
        return dict(ids=self.ids, nodes=self.nodes, node_begin=self.node_begin, edges=self.edges, edge_begin=self.edge_begin, radii=self.radii)

    def skeleton_of(self, cell_id) -> Skeleton:
        k = int(np.searchsorted(self.ids, np.uint64(cell_id)))
        if k >= len(self.ids) or self.ids[k] != np.uint64(cell_id):
            raise KeyError(cell_id)
        n0, n1, e0, e1 = self.node_begin[k], self.node_begin[k + 1], self.edge_begin[k], self.edge_begin[k + 1]
        return Skeleton(self.nodes[n0:n1].copy(), self.edges[e0:e1].copy(), self.radii[n0:n1].copy())

    @classmethod
    def from_skeletons(cls, skeletons: dict):
        """{cell id: Skeleton} -> table (cells in ascending id order)."""
        ids = sorted(int(i) for i in skeletons)
        if not ids:
            return cls.empty()
        sk = [skeletons[i] for i in ids]
        nb = np.concatenate(([0], np.cumsum([len(s.vertices) for s in sk])))
        eb = np.concatenate(([0], np.cumsum([len(s.edges) for s in sk])))
        return cls(ids, np.concatenate([s.vertices for s in sk]), nb, np.concatenate([s.edges for s in sk]), eb, np.concatenate([s.radii for s in sk]))

    @classmethod
    def merge(cls, tables):
        """The rows of several tables (the chunks of a volume) per cell, concatenated in the order given: the pieces of a cell stay apart
        (edges are shifted by the rows before them), what ``PrecomputedSkeleton.simple_merge`` does before the stitching."""
        tables = [t for t in tables if len(t)]
        if not tables:
            return cls.empty()
        ids = np.unique(np.concatenate([t.ids for t in tables]))
        nodes, radii, edges, nb, eb = [], [], [], [0], [0]
        for i in ids:
            n_cell = e_cell = 0
            for t in tables:
                k = int(np.searchsorted(t.ids, i))
                if k >= len(t.ids) or t.ids[k] != i:
                    continue
                n0, n1, e0, e1 = t.node_begin[k], t.node_begin[k + 1], t.edge_begin[k], t.edge_begin[k + 1]
                nodes.append(t.nodes[n0:n1]); radii.append(t.radii[n0:n1]); edges.append(t.edges[e0:e1] + n_cell)
                n_cell += n1 - n0; e_cell += e1 - e0
            nb.append(nb[-1] + n_cell); eb.append(eb[-1] + e_cell)
        return cls(ids, np.concatenate(nodes), nb, np.concatenate(edges), eb, np.concatenate(radii))

    def to_cell_columns(self, scaling):
        """``nodes`` in voxels (float64 nm / scaling), ``node_begin``, ``edges``, ``edge_begin``: the skeleton columns ``CellTable``,
        ``skeleton_majority_vote`` and ``map_myelin_global`` take."""
        s = np.asarray(scaling, np.float64).reshape(3)
        return dict(nodes=self.nodes.astype(np.float64) / s, node_begin=self.node_begin.copy(), edges=self.edges.copy(), edge_begin=self.edge_begin.copy())


def _integers(what, v, n, lo, hi):
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size != n or not np.isfinite(a).all() or (a != np.round(a)).any() or (a < lo).any() or (a > hi).any():
        raise ValueError(f'{what} must be {"an integer" if n == 1 else f"{n} integers"} in {lo} .. {hi} (anything else is not built)')
    return [int(x) for x in a]


def trace_chunk(seg, anisotropy, teasar_params=None, dust_threshold=1000, max_paths=None, device=None, stages=None, max_comps=None, max_nodes=None, timings=None):
    """The device chain over one label volume ``seg`` (uint64 (X, Y, Z): a host array, or a resident int64 / uint64-as-int64 tensor).
    Returns a dict per COMPONENT (26-connected, equal label, at least ``dust_threshold`` voxels; numbered from 1 in raster order of the
    first voxel, row c - 1): ``labels`` uint64, ``sizes``, ``void`` (the float64 walk did not descend: no result), ``node_begin`` /
    ``edge_begin`` int64 [n + 1], ``node_voxel`` int32 raster indices, ``vertices`` float32 nm, ``radii`` float32, ``edges`` int32
    (indices inside the component), and ``stats``: sweeps / tiles per relaxation.  With ``stages`` (a dict) every intermediate is copied
    into it: comp, d2, dbf, dbf_max, daf0, root, daf, daf_max, p, targets, dist_rounds, valid_rounds, parent.  With ``timings`` (a dict) the
    milliseconds between HIP events around every stage are added to it (the host's synchronisations in between included)."""
    import torch
    from .. import _dev as D
    from .. import _lib as L
    tp = dict(TEASAR_DEFAULTS)
    tp.update(teasar_params or {})
    w = _integers('anisotropy', anisotropy, 3, 1, L.SD_SKELETONIZE_MAX_ANISOTROPY)
    e = _integers('pdrf_exponent', tp['pdrf_exponent'], 1, 1, L.SD_SKELETONIZE_MAX_EXPONENT)[0]
    n_paths = int(tp['max_paths'] if max_paths is None else max_paths)
    if n_paths < 1:
        raise ValueError('max_paths must be at least 1')
    inv_scale, inv_const, pdrf_scale = float(np.float32(tp['scale'])), float(np.float32(tp['const'])), float(tp['pdrf_scale'])
    if not (np.isfinite([inv_scale, inv_const, pdrf_scale]).all() and inv_scale >= 0 and pdrf_scale >= 0):
        raise ValueError('scale, const and pdrf_scale must be finite, scale and pdrf_scale not negative')
    if int(dust_threshold) != dust_threshold or dust_threshold < 0:
        raise ValueError('dust_threshold must be a non-negative integer')
    dev = D.device(device if device is not None or not isinstance(seg, torch.Tensor) else seg.device)
    if isinstance(seg, torch.Tensor):
        if seg.dtype != torch.int64 or seg.dim() != 3:
            raise ValueError('seg: a resident volume is an int64 tensor (the bits of uint64) of three axes')
        seg_d = seg.to(dev).contiguous()
    else:
        seg = np.asarray(seg)
        if seg.ndim != 3 or seg.dtype.kind not in 'ui':
            raise ValueError('seg must be an integer volume of three axes')
        seg_d = D.up(seg.astype(np.uint64, copy=False), dev)
    X, Y, Z = (int(n) for n in seg_d.shape)
    cap = L.SD_SKELETONIZE_MAX_EXTENT
    if min(X, Y, Z) < 1 or max(X, Y, Z) > cap or X * Y * Z >= 2 ** 31:
        raise ValueError(f'seg: extents must be 1 .. {cap} with fewer than 2^31 voxels')
    nvox = X * Y * Z
    w_c = D.i32x3(w)
    events = []

    def tick(name):
        if timings is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(dev))
            events.append((name, e))

    def close_timings():
        if timings is not None:
            torch.cuda.synchronize(dev)
            for (_, a), (name, b) in zip(events[:-1], events[1:]):
                timings[name] = timings.get(name, 0.0) + a.elapsed_time(b)

    temp = D.scratch(_TEMP, dev, X, Y, Z)
    tick('start')
    counts = D.counters(dev)
    comp = D.empty(nvox, D.i32, dev)
    n_cap = int(max_comps) if max_comps else 4096
    while True:
        sizes, labels, first = D.empty(n_cap + 1, D.i64, dev), D.empty(n_cap + 1, D.i64, dev), D.empty(n_cap + 1, D.i32, dev)
        D.call('sd_skeletonize_components', dev, seg_d, X, Y, Z, int(dust_threshold), comp, sizes, labels, first, n_cap, counts, temp, temp.numel())
        c = D.down(counts)
        n = int(c[0])
        if not c[7]:
            break
        if max_comps:
            raise RuntimeError(f'trace_chunk: {n} components, max_comps = {max_comps}')
        n_cap = n
    out = dict(labels=D.down(labels, n + 1, np.uint64)[1:], sizes=D.down(sizes, n + 1)[1:], void=np.zeros(n, np.int32), node_begin=np.zeros(n + 1, np.int64),
               edge_begin=np.zeros(n + 1, np.int64), node_voxel=np.zeros(0, np.int32), vertices=np.zeros((0, 3), np.float32), radii=np.zeros(0, np.float32),
               edges=np.zeros((0, 2), np.int32), stats=[], shape=(X, Y, Z))
    if stages is not None:
        stages.update(comp=D.down(comp, nvox).reshape(X, Y, Z), sizes=D.down(sizes, n + 1).astype(np.uint64), labels=D.down(labels, n + 1, np.uint64),
                      first=D.down(first, n + 1))
        stages['sizes'][0], stages['labels'][0], stages['first'][0] = 0, 0, -1      # (entry 0 of the tables is not written)
    tick('components')
    if n == 0:
        close_timings()
        return out
    fg = int(out['sizes'].sum())
    d2, dbf, dbf_max = D.empty(nvox, D.i64, dev), D.empty(nvox, torch.float32, dev), D.empty(n + 1, torch.float32, dev)
    D.call('sd_skeletonize_d2', dev, comp, X, Y, Z, w_c, n, d2, dbf, dbf_max, counts, temp, temp.numel())
    tick('d2')
    if stages is not None:
        stages.update(d2=D.down(d2, nvox, np.uint64).reshape(X, Y, Z), dbf=D.down(dbf, nvox).reshape(X, Y, Z), dbf_max=D.down(dbf_max, n + 1))
    if D.down(counts)[1]:
        raise ValueError('trace_chunk: a component has no voxel of another component (or background) in the array: its distance to the boundary is undefined')

    def relax(field, pen):
        """Sweeps until no tile is dirty; bounded by the foreground voxels + 1."""
        counts.zero_()
        done, step = 0, 12
        while True:
            D.call('sd_skeletonize_relax', dev, comp, X, Y, Z, w_c, field, pen, step, counts, temp, temp.numel())
            c = D.down(counts)
            if c[6]:
                raise RuntimeError('trace_chunk: a tile passed its local relaxation bound')
            if c[3] == 0:
                break
            done += step
            if done > fg + 1:
                raise RuntimeError('trace_chunk: the relaxation passed its bound of foreground voxels + 1 sweeps')
            step = min(step * 2, L.SD_SKELETONIZE_MAX_SWEEPS)
        out['stats'].append((int(c[4]), int(c[5])))

    def field_from(src, f64):
        f = D.empty(nvox, D.f64 if f64 else torch.float32, dev)
        D.call('sd_skeletonize_field_start', dev, comp, X, Y, Z, src, n, f, int(f64), temp, temp.numel())
        return f

    keys, idx, val = D.empty(n + 1, D.i64, dev), D.empty(n + 1, D.i32, dev), D.empty(n + 1, torch.float32, dev)
    daf0 = field_from(first, False)
    relax(daf0, None)
    tick('daf0')
    root = D.empty(n + 1, D.i32, dev)
    D.call('sd_skeletonize_argmax', dev, comp, daf0, None, nvox, n, root, None, keys)
    daf = field_from(root, False)
    relax(daf, None)
    daf_max = D.empty(n + 1, torch.float32, dev)
    D.call('sd_skeletonize_argmax', dev, comp, daf, None, nvox, n, idx, daf_max, keys)
    tick('daf')
    m_host = np.array([float(x) ** 1.01 for x in D.down(dbf_max, n + 1)], np.float64)      # M = dbf_max ** 1.01, computed here: no pow on the device
    pen = D.empty(nvox, D.f64, dev)
    D.call('sd_skeletonize_penalty', dev, comp, dbf, daf, nvox, n, D.up(m_host, dev), daf_max, pdrf_scale, e, pen)
    tick('penalty')
    dist = field_from(root, True)
    relax(dist, pen)
    tick('dist_first')
    if stages is not None:
        stages.update(daf0=D.down(daf0, nvox).reshape(X, Y, Z), root=D.down(root, n + 1), daf=D.down(daf, nvox).reshape(X, Y, Z), daf_max=D.down(daf_max, n + 1),
                      p=D.down(pen, nvox).reshape(X, Y, Z), targets=[], dist_rounds=[], valid_rounds=[])
    del daf0
    valid, parent, void = D.empty(nvox, D.u8, dev), D.empty(nvox, D.i32, dev), D.empty(n + 1, D.i32, dev)
    valid[:nvox] = comp[:nvox] > 0
    parent.fill_(-1)
    void.zero_()
    rcounts = D.counters(dev)
    for rnd in range(n_paths):
        D.call('sd_skeletonize_argmax', dev, comp, daf, valid, nvox, n, idx, None, keys)
        tg = D.down(idx, n + 1)
        tg[0] = -1
        live = tg >= 0
        live[1:] &= D.down(void, n + 1)[1:] == 0
        if not live.any():
            break
        if stages is not None:
            t = tg.copy()
            t[~live] = -1
            stages['targets'].append(t)
        D.call('sd_skeletonize_round', dev, comp, X, Y, Z, w_c, dbf, dist, valid, parent, idx, root if rnd == 0 else None, sizes, n, inv_scale, inv_const, void,
               rcounts, temp, temp.numel())
        tick('round_target_walk_invalidate')
        relax(dist, pen)
        tick('round_relax')
        if stages is not None:
            stages['dist_rounds'].append(D.down(dist, nvox).reshape(X, Y, Z))
            stages['valid_rounds'].append(D.down(valid, nvox).reshape(X, Y, Z))
    rc = D.down(rcounts)
    if rc[1]:
        raise RuntimeError('trace_chunk: a walk passed its bound (the voxels of its component)')
    out['absorbed'] = int(rc[2])
    n_cap = int(max_nodes) if max_nodes else max(min(fg, 1 << 16), 1)
    while True:
        etemp = D.scratch(_EMIT_TEMP, dev, n_cap)
        nb, eb = D.empty(n + 2, D.i64, dev), D.empty(n + 2, D.i64, dev)
        nv, vx, rd, ed = D.empty(n_cap, D.i32, dev), D.empty((n_cap, 3), torch.float32, dev), D.empty(n_cap, torch.float32, dev), D.empty((n_cap, 2), D.i32, dev)
        D.call('sd_skeletonize_emit', dev, comp, X, Y, Z, w_c, parent, dbf, root, void, n, n_cap, nb, eb, nv, vx, rd, ed, counts, temp, temp.numel(), etemp,
               etemp.numel())
        need = int(D.down(counts)[0])
        if need <= n_cap:
            break
        if max_nodes:
            raise RuntimeError(f'trace_chunk: {need} nodes, max_nodes = {max_nodes}')
        n_cap = need
    tick('emit')
    close_timings()
    nb_h, eb_h = D.down(nb, n + 2)[1:], D.down(eb, n + 2)[1:]
    out.update(void=D.down(void, n + 1)[1:], node_begin=nb_h, edge_begin=eb_h, node_voxel=D.down(nv, need), vertices=D.down(vx, need), radii=D.down(rd, need),
               edges=D.down(ed, int(eb_h[-1])))
    if stages is not None:
        stages.update(parent=D.down(parent, nvox).reshape(X, Y, Z), void=D.down(void, n + 1))
    return out


def relabel_lookup(seg, sv_ids, ssv_ids):
    """``relabel_vol_nonexist2zero``: supervoxel -> cell through the lookup (``sv_ids`` ascending), 0 for a supervoxel that is not in it."""
    sv = np.asarray(sv_ids, np.uint64).reshape(-1)
    ssv = np.asarray(ssv_ids, np.uint64).reshape(-1)
    if len(sv) != len(ssv) or (len(sv) > 1 and (sv[1:] <= sv[:-1]).any()):
        raise ValueError('sv_ids must ascend strictly, with one cell id each')
    seg = np.asarray(seg).astype(np.uint64, copy=False)
    if not len(sv):
        return np.zeros_like(seg)
    k = np.minimum(np.searchsorted(sv, seg), len(sv) - 1)
    return np.where(sv[k] == seg, ssv[k], np.uint64(0))


def skeletonize_chunk_table(seg, anisotropy, offset_nm=0, teasar_params=None, dust_threshold=1000, sv_ids=None, ssv_ids=None, max_paths=100, device=None) -> SkeletonTable:
    """``kimimaro.skeletonize`` of one chunk as proc/skeleton.py:21-86 calls it, as a table: the optional supervoxel -> cell lookup, the
    device tracing, and the components of one cell joined into one row by concatenation (the merge stitches them).  ``offset_nm`` is
    added to the vertices (float32)."""
    import torch
    if sv_ids is not None:
        if isinstance(seg, torch.Tensor):
            sv = torch.as_tensor(np.asarray(sv_ids, np.uint64).view(np.int64), device=seg.device)
            if len(sv) > 1 and bool((sv[1:] <= sv[:-1]).any()):
                raise ValueError('sv_ids must ascend strictly and stay below 2^63 for a resident volume')
            ssv = torch.as_tensor(np.asarray(ssv_ids, np.uint64).view(np.int64), device=seg.device)
            k = torch.searchsorted(sv, seg.contiguous()).clamp_(max=max(len(sv) - 1, 0))
            seg = torch.where(sv[k] == seg, ssv[k], torch.zeros_like(seg)) if len(sv) else torch.zeros_like(seg)
        else:
            seg = relabel_lookup(seg, sv_ids, ssv_ids)
    r = trace_chunk(seg, anisotropy, teasar_params, dust_threshold, max_paths, device)
    labels, nb, eb = r['labels'], r['node_begin'], r['edge_begin']
    off = np.broadcast_to(np.asarray(offset_nm, np.float32), (3,))
    skels = {}
    for cell in np.unique(labels):
        rows = np.flatnonzero(labels == cell)
        rows = rows[nb[rows + 1] > nb[rows]]
        if not len(rows):
            continue
        shift = np.concatenate(([0], np.cumsum(nb[rows + 1] - nb[rows])))
        skels[int(cell)] = Skeleton(np.concatenate([r['vertices'][nb[c]:nb[c + 1]] for c in rows]) + off,
                                    np.concatenate([r['edges'][eb[c]:eb[c + 1]].astype(np.int64) + shift[k] for k, c in enumerate(rows)]),
                                    np.concatenate([r['radii'][nb[c]:nb[c + 1]] for c in rows]))
    return SkeletonTable.from_skeletons(skels)


# ---- host post-processing: proc/skeleton.py:76-224, proc/graphs.py:701-739, reps/super_segmentation_helper.py:650-705 --------------------
class _Graph:
    """The part of ``networkx.Graph`` the reference's skeleton functions lean on, with its orders: nodes and the neighbours of a node
    are kept in insertion order, removing a node keeps the order of the others, an edge that exists stays where it is."""

    def __init__(self):
        self.pos, self.rad, self.adj = {}, {}, {}

    @classmethod
    def of(cls, skel: Skeleton):
        g = cls()
        for k in range(len(skel.vertices)):
            g.pos[k], g.rad[k], g.adj[k] = skel.vertices[k], skel.radii[k], {}
        for a, b in skel.edges.tolist():
            g.add_edge(a, b)
        return g

    def add_edge(self, a, b):
        for n in (a, b):
            if n not in self.adj:
                raise ValueError('an edge names a node that does not exist')
        self.adj[a][b] = None
        self.adj[b][a] = None

    def remove_node(self, n):
        for m in list(self.adj[n]):
            if m != n:
                del self.adj[m][n]
        del self.adj[n], self.pos[n], self.rad[n]

    def edges(self):
        seen, out = set(), []
        for n, nb in self.adj.items():
            out += [(n, m) for m in nb if m not in seen]
            seen.add(n)
        return out

    def components(self):
        """Node lists in breadth-first order, components in the order of their first node."""
        seen, out = set(), []
        for s in self.adj:
            if s in seen:
                continue
            seen.add(s)
            comp, level = [s], [s]
            while level:
                nxt = []
                for v in level:
                    for u in self.adj[v]:
                        if u not in seen:
                            seen.add(u); comp.append(u); nxt.append(u)
                level = nxt
            out.append(comp)
        return out

    def skeleton(self) -> Skeleton:
        """``nxgraph2skelcv``: nodes renumbered in their order, edges in the order a walk over the nodes meets them."""
        new = {n: k for k, n in enumerate(self.adj)}
        edges = np.array([(new[a], new[b]) for a, b in self.edges()], np.int64).reshape(-1, 2)
        return Skeleton(np.array([self.pos[n] for n in self.adj], np.float32).reshape(-1, 3), edges, np.array([self.rad[n] for n in self.adj], np.float32))


def _sparsify(g: _Graph, scale, keep_straight, max_dist_thresh, min_dist_thresh):
    """The loop both sparsifiers share: nodes of degree 2, visited in the order of the Python ``set`` the reference builds from the degree
    table, are taken out (their neighbours joined) where `keep_straight(unit dot product)` holds and the neighbours are closer than
    `max_dist_thresh`, or closer than `min_dist_thresh` whatever the angle; repeated until a pass removes nothing."""
    scale = np.asarray(scale)
    trunc = lambda n: np.array([int(c) for c in g.pos[n]])
    removed = 1
    while removed:
        removed = 0
        for v in list({n for n, nb in g.adj.items() if len(nb) + (n in nb) == 2}):
            nb = list(g.adj[v])
            if len(nb) + (v in g.adj[v]) != 2:
                continue
            left, right = nb[0], nb[1]
            with np.errstate(all='ignore'):
                a, b = (trunc(left) - trunc(v)) * scale, (trunc(right) - trunc(v)) * scale
                dot = np.dot(a / np.linalg.norm(a), b / np.linalg.norm(b))
                dist = np.linalg.norm([int(g.pos[right][k] * scale[k]) - int(g.pos[left][k] * scale[k]) for k in range(3)])
                if (keep_straight(dot) and dist < max_dist_thresh) or dist <= min_dist_thresh:
                    g.remove_node(v)
                    g.add_edge(left, right)
                    removed += 1
    return g


def sparsify_skelcv(skel: Skeleton, scale=None, angle_thresh=135, max_dist_thresh=500, min_dist_thresh=50) -> Skeleton:
    """proc/skeleton.py:176-224."""
    if scale is None:
        from .. import global_params
        scale = global_params.config['scaling']
    return _sparsify(_Graph.of(skel), scale, lambda d: abs(np.arccos(np.clip(d, -1.0, 1.0)) * 180 / np.pi) > angle_thresh, max_dist_thresh,
                     min_dist_thresh).skeleton()


def sparsify_skeleton_fast(skel: Skeleton, scal=None, dot_prod_thresh=0.8, max_dist_thresh=500, min_dist_thresh=50) -> Skeleton:
    """reps/super_segmentation_helper.py:650-705 on a ``Skeleton`` (the reference takes and returns the graph)."""
    if scal is None:
        from .. import global_params
        scal = global_params.config['scaling']
    return _sparsify(_Graph.of(skel), scal, lambda d: abs(d) > dot_prod_thresh, max_dist_thresh, min_dist_thresh).skeleton()


def downsample(skel: Skeleton, factor: int = 10) -> Skeleton:
    """``cloudvolume.Skeleton.downsample`` is not in the reference tree; stated: branch and end points (degree != 2;
    in a bare ring the smallest index) are kept, and of the inner vertices of every unbranched run between two of them every
    `factor`-th, counted from the run's start -- runs are walked from the kept points in ascending index, neighbours in ascending index.
    Vertices keep their order; the kept neighbours of a run are joined."""
    factor = int(factor)
    if factor < 1:
        raise ValueError('downsample: factor must be at least 1')
    n = len(skel.vertices)
    nbrs = [[] for _ in range(n)]
    for a, b in skel.edges.tolist():
        if a != b and b not in nbrs[a]:
            nbrs[a].append(b); nbrs[b].append(a)
    nbrs = [sorted(x) for x in nbrs]
    fixed = np.array([len(x) != 2 for x in nbrs], bool)
    for comp in _Graph.of(Skeleton(skel.vertices, skel.edges, skel.radii)).components():
        if not fixed[comp].any():
            fixed[min(comp)] = True
    keep, edges, used = fixed.copy(), [], set()
    for s in np.flatnonzero(fixed).tolist():
        for first in nbrs[s]:
            if (s, first) in used:
                continue
            used.add((s, first))
            last, prev, cur, k = s, s, first, 0
            while not fixed[cur]:
                k += 1
                if k % factor == 0:
                    keep[cur] = True
                    edges.append((last, cur)); last = cur
                prev, cur = cur, (nbrs[cur][0] if nbrs[cur][0] != prev else nbrs[cur][1])
            used.add((cur, prev))
            edges.append((last, cur))
    new = np.cumsum(keep) - 1
    e = np.array([(new[a], new[b]) for a, b in edges], np.int64).reshape(-1, 2)
    return Skeleton(skel.vertices[keep], e, skel.radii[keep])


def stitch_skel_nx(skel: Skeleton) -> Skeleton:
    """proc/graphs.py:701-739 on arrays: while there are several components, one edge from the largest component (ties: the one whose
    first node comes first) to the nearest node of all the others, by squared distance of the int64-cast positions, the first minimum;
    vertices and radii stay, the new edges follow the old ones."""
    g = _Graph.of(skel)
    comps = g.components()
    if len(comps) <= 1:
        return skel
    pos = np.asarray(skel.vertices).astype(np.int64)
    edges = skel.edges.tolist()
    while len(comps) > 1:
        comps.sort(key=len, reverse=True)
        cur, rest = np.array(comps[0]), np.array([n for c in comps[1:] for n in c])
        best = None
        for s in range(0, len(cur), 1024):
            d = ((pos[cur[s:s + 1024], None, :] - pos[None, rest, :]) ** 2).sum(-1)
            k = int(np.argmin(d))
            if best is None or d.flat[k] < best[0]:
                best = (d.flat[k], int(cur[s + k // len(rest)]), int(rest[k % len(rest)]))
        g.add_edge(best[1], best[2])
        edges.append([best[1], best[2]])
        comps = g.components()
    return Skeleton(skel.vertices, edges, skel.radii)


def simple_merge(skeletons) -> Skeleton:
    """Concatenation with shifted edges (cloudvolume's ``simple_merge``; stated)."""
    skeletons = list(skeletons)
    if not skeletons:
        return Skeleton()
    shift = np.concatenate(([0], np.cumsum([len(s.vertices) for s in skeletons])))
    return Skeleton(np.concatenate([s.vertices for s in skeletons]), np.concatenate([s.edges + shift[k] for k, s in enumerate(skeletons)]),
                    np.concatenate([s.radii for s in skeletons]))


def consolidate(skel: Skeleton) -> Skeleton:
    """Equal vertices become one (cloudvolume's ``consolidate``; stated): the distinct vertices in lexicographic order with the radius of
    their first occurrence, edges renamed, self loops dropped, each edge once with its smaller end first, in ascending order."""
    if not len(skel.vertices):
        return skel
    verts, first, inv = np.unique(skel.vertices, axis=0, return_index=True, return_inverse=True)
    e = np.sort(inv.reshape(-1)[skel.edges], axis=1).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    e = np.unique(e, axis=0) if len(e) else e
    return Skeleton(verts, e, skel.radii[first])


def kimimaro_mergeskels(pieces, cell_id=None) -> Skeleton:
    """proc/skeleton.py:89-137 without ``kimimaro.postprocess`` (not built): the pieces of one cell (a list of ``Skeleton``, or a list of
    {cell id: [Skeleton]} dicts with `cell_id`) merged, duplicate vertices consolidated, the components stitched."""
    if cell_id is not None:
        pieces = [s for d in pieces for s in d.get(int(cell_id), [])]
    skel = consolidate(simple_merge(pieces))
    if not len(skel.vertices):
        return skel
    return _Graph.of(stitch_skel_nx(_Graph.of(skel).skeleton())).skeleton()


def _zoom0(seg, ds):
    """``ndimage.zoom(seg, 1 / ds, order=0)`` through the zoom table of the spine head code."""
    from ..extraction.spinehead import zoom_source_table
    for a in range(3):
        t = zoom_source_table(seg.shape[a], ds[a])
        taken = np.take(seg, np.maximum(t, 0), axis=a)
        shape = [1, 1, 1]
        shape[a] = len(t)
        seg = np.where((t >= 0).reshape(shape), taken, np.zeros((), seg.dtype))
    return seg


def kimimaro_skelgen(seg_or_kd, cube_size, cube_offset, nb_cpus=None, ssd=None, ds=None, dust_threshold=1000, scaling=None, sv_ids=None, ssv_ids=None,
                     teasar_params=None, device=None) -> dict:
    """proc/skeleton.py:21-86 -> {cell id: Skeleton}.  `seg_or_kd`: a label volume (X, Y, Z) in memory whose origin is voxel 0, or an object
    with ``load_seg(size=, offset=, mag=1)`` returning (z, y, x) and ``scales``.  `ssd`: an object with ``sv2ssv_ids(ids) -> dict``, or the
    sorted lookup `sv_ids` / `ssv_ids`; without either the labels are cells already.  `nb_cpus` has nothing to parallelise."""
    size, off = np.asarray(cube_size, np.int64), np.asarray(cube_offset, np.int64)
    if hasattr(seg_or_kd, 'load_seg'):
        seg = np.asarray(seg_or_kd.load_seg(size=size, offset=off, mag=1)).swapaxes(0, 2)
        scaling = np.asarray(seg_or_kd.scales[0]) if scaling is None else scaling
    else:
        vol = np.asarray(seg_or_kd)
        seg = np.zeros(tuple(size), vol.dtype)
        hi = np.minimum(off + size, vol.shape)
        lo = np.maximum(off, 0)
        if (hi > lo).all():
            seg[tuple(slice(l - o, h - o) for l, h, o in zip(lo, hi, off))] = vol[tuple(slice(l, h) for l, h in zip(lo, hi))]
    if scaling is None:
        from .. import global_params
        scaling = global_params.config['scaling']
    scaling = np.asarray(scaling, np.float64)
    ds_arr = np.ones(3) if ds is None else np.asarray(ds, np.float64)
    if ds is not None:
        seg = _zoom0(seg, ds_arr)
    if ssd is not None:
        lut = ssd.sv2ssv_ids(np.unique(seg))
        sv_ids = sorted(lut)
        ssv_ids = [lut[k] for k in sv_ids]
    table = skeletonize_chunk_table(np.ascontiguousarray(seg), scaling * ds_arr, 0, teasar_params, dust_threshold, sv_ids, ssv_ids,
                                    (teasar_params or {}).get('max_paths', TEASAR_DEFAULTS['max_paths']), device)
    shift = (off * scaling).astype(np.int32)
    out = {}
    for cell in table.ids.tolist():
        s = sparsify_skelcv(downsample(table.skeleton_of(cell), 10), scale=np.array([1, 1, 1]))
        s.vertices = s.vertices + shift
        out[int(cell)] = s
    return out
