"""Golden vectors for the spine head volumes, produced by the REFERENCE'S OWN ``extract_spinehead_volume_mesh``
(/root/reference/syconn/reps/super_segmentation_helper.py:2068-2198) and ``colorcode_vertices`` (reps/rep_helper.py:281-334), lifted by
AST at generation time and run unchanged on stand-in ``sso`` / ``kd`` objects with scipy: every numpy / scipy statement of the reference
(zoom, fill holes, EDT, label, unique / argmax, cKDTree, the slice around the synapse, the volume formula) is pinned.  Nothing compiled
and no reference text is stored: inputs and outputs only, as flat arrays.

    python tests/golden/make_golden_spinehead.py      ->  tests/golden/g22_spinehead.npz

Injected restatements, for what cannot run here: the two skimage calls (``peak_local_max`` by the rule in tests/_spinehead_ref.py,
``watershed`` = oracle.objseg_ref.watershed_ref on rint(distance^2)), the two Cython helpers (``in_bounding_box``,
``relabel_vol_nonexist2zero``), and the two ``sso`` methods ``semseg_for_coords`` / ``attr_for_coords`` (tests/_syn_props_ref.py, pinned
to the reference by golden g21).  ``np.bool`` (removed from numpy) is given back as ``bool``; ``cKDTree.query`` gets ``n_jobs`` forwarded
as ``workers``.

dtypes (decided by the reference, reps/rep_helper.py:466 and the mesh storage): ``sso.scaling = np.array(config['scaling'])`` is int64
for the integer voxel sizes of a config, ``sso.mesh[1]`` float32.  So ``verts = mesh / scaling`` is float64 (the float32 widened
exactly, one division in double), the box ``[offset + size / 2, size]`` float64 (``in_bounding_box`` then runs its double form, half
edges in C float), ``maxima * ds`` uint64 * int64 = float64 (exact), ``verts_bb - offset`` float64, and the volume
``n * prod(int64) / 1e9`` one float64 division.  The device does the division on the host with numpy (same statement) and everything
after it in float64, where the widening is exact.

Four cases (prefix a_, b_, c_, d_), each one small dataset with its own cells; a scene is drawn from a seeded generator and checked in
``main`` to contain what it is there for:
  a  scaling (10, 10, 20) -> ds (2, 2, 1), ctx_vol (12, 12, 6): windows of 24 x 24 x 12 voxels, 12^3 after the zoom;
  b  scaling (10, 10, 10) -> ds (1, 1, 1), ctx_vol (8, 8, 8): 16^3; a hollow ball cut by its window's far face;
  c  scaling (10, 10, 20), ctx_vol (15, 15, 8): 30 x 30 x 16 -> 15 x 15 x 16, the zoom drops the last x / y plane;
  d  scaling (10, 10, 10), ctx_vol (8, 8, 8), k 5: one window, two thin objects with equal counts in the slice around the synapse.
Checked over all cases: a window clipped at the dataset origin that takes the nearest-voxel fallback, a window overhanging the far
boundary, a closed hole that is filled, a hole open to the window border that is not, two or more head objects decided by count, by a count tie and by the
fallback, cells of one and of several supervoxels, a window with no vertex in its box, a one-voxel-thick mask (entry 0.0), an empty mask
(ValueError, a cell of its own), ``ignore_labels`` removing vertices, k above the vertices in a box, synapses rejected by the spiness
and by the axoness filter, a plateau of equal maxima; no fallback distance and no kNN distance ties.

Per case: ``scaling``, ``ctx_vol``, ``k``, ``vol`` (x, y, z) uint64 at origin 0; cells: ``cell_ids``, ``cell_sv_begin`` / ``cell_sv``,
``cell_verts`` float32 nm / ``cell_vert_begin`` / ``cell_spiness``, ``cell_nodes`` / ``cell_node_begin`` / ``cell_ax``; synapses:
``syn_ids``, ``syn_rep``, ``syn_cells`` (n, 2); results: ``sh_cell`` / ``sh_syn`` / ``sh_vol`` float64 (one row per entry), ``err_cells`` =
cells for which the reference raised its ValueError."""
import os
import sys
import types
from collections import Counter

import numpy as np
from scipy import ndimage, spatial

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden_cs import lift_function  # noqa: E402
import _spinehead_ref as R  # noqa: E402
import _syn_props_ref as SP  # noqa: E402
from oracle.objseg_ref import watershed_ref  # noqa: E402

REF = '/root/reference/syconn'
IGNORE, AX_KEY, DS_VERT = [4, 5], 'axoness_avg10000', 1


class Scene:
    """A dataset of `shape` mag-1 voxels; geometry is drawn in isotropic units of the z voxel and rendered through `ds`."""

    def __init__(self, seed, scaling, ctx, shape, k):
        self.rng = np.random.default_rng(seed)
        self.scaling, self.ctx, self.k = np.array(scaling), np.array(ctx), k
        self.ds = self.scaling[2] // self.scaling
        self.vol = np.zeros(shape, np.uint64)
        self.cells, self.syn = [], []
        g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).astype(np.float64)
        self.iso = (g + 0.5) / self.ds                          # voxel centres in isotropic units

    def ball(self, c, r):
        return ((self.iso - np.asarray(c, np.float64)) ** 2).sum(-1) <= r * r

    def stick(self, a, b, r):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        t = np.clip(((self.iso - a) @ (b - a)) / ((b - a) @ (b - a)), 0, 1)
        return ((self.iso - (a + t[..., None] * (b - a))) ** 2).sum(-1) <= r * r

    def cell(self, cid, sv, parts, node_ax=0, sparse=1, drop_box=None):
        """parts: list of (mask, spine label); later parts do not overwrite earlier ones.  Vertices = centres of the cell's surface voxels
        (nm, jittered on the 1/64 nm lattice), labelled by their part; every 7th vertex gets an ignored label."""
        rng = self.rng
        own = np.zeros(self.vol.shape, bool)
        lab = np.full(self.vol.shape, -1, np.int64)
        for m, l in parts:
            lab[m & ~own] = l
            own |= m
        own &= self.vol == 0
        ids = np.asarray(sv, np.uint64)
        self.vol[own] = ids[(np.indices(self.vol.shape)[0][own] // 7) % len(ids)]      # several supervoxels: slabs along x
        surf = own & ~ndimage.binary_erosion(own, border_value=1)
        pos = np.transpose(np.nonzero(surf))[::sparse]
        verts = (np.round(((pos + 0.5) * self.scaling + rng.uniform(-3, 3, pos.shape)) * 64) / 64).astype(np.float32)
        vl = lab[tuple(pos.T)]
        vl[::7] = rng.integers(4, 6, len(vl[::7]))
        if drop_box is not None:
            lo, hi = drop_box
            keep = ~np.all((pos >= lo) & (pos < hi), 1)
            verts, vl = verts[keep], vl[keep]
        core = np.transpose(np.nonzero(ndimage.binary_erosion(own)))
        nodes = core[:: max(1, len(core) // 12)] if len(core) else pos[:: max(1, len(pos) // 12)]
        ax = np.full(len(nodes), node_ax, np.int64)
        self.cells.append(dict(id=cid, sv_ids=ids, vertices=verts, vertex_labels={'spiness': vl.astype(np.int64)}, nodes=nodes.astype(np.int64),
                               node_attrs={AX_KEY: ax}, own=own))
        return self.cells[-1]

    def synapse(self, cid, rep, other=0):
        self.syn.append((1000 + 7 * len(self.syn), np.asarray(rep, np.int64), (cid, other)))


def iso2vox(s, p):
    return np.floor(np.asarray(p, np.float64) * s.ds).astype(np.int64)


def spiny_cell(s, cid, sv, base, heads, shaft_axis=0, **kw):
    """A shaft (label 2) through `base` along an axis, necks (label 0) and head balls (label 1); heads = [(centre, radius), ...]."""
    a, b = np.array(base, np.float64), np.array(base, np.float64)
    a[shaft_axis], b[shaft_axis] = -5, 500
    parts = [(s.ball(c, r), 1) for c, r in heads]
    for c, _ in heads:
        foot = np.array(base, np.float64)
        foot[shaft_axis] = c[shaft_axis]
        parts.append((s.stick(c, foot, 0.8), 0))
    parts.append((s.stick(a, b, 1.6), 2))
    return s.cell(cid, sv, parts, **kw)


def case_a(seed):
    s = Scene(seed, (10, 10, 20), (12, 12, 6), (64, 56, 28), 50)
    r = s.rng
    # cell 1 (three supervoxels): two heads close to each other on one shaft -> two head objects in one window; a hollow head
    h1, h2 = np.array([6.5, 6.0, 6.0]) + r.uniform(-.4, .4, 3), np.array([6.5, 6.0, 12.5]) + r.uniform(-.4, .4, 3)
    c1 = spiny_cell(s, 1, [11, 12, 13], (6.5, 13.0, 9.0), [(h1, 2.6), (h2, 2.6), ((20.0, 6.0, 8.0), 3.4)], shaft_axis=0)
    hollow = s.ball((20.0, 6.0, 8.0), 1.3) & c1['own']
    s.vol[hollow] = 0                                          # a closed hole
    # cell 2 (one supervoxel): far corner, overhanging windows; sparse mesh (k above the vertices in the box)
    s.cell(2, [21], [(s.ball((27.0, 24.5, 25.0), 2.6), 1), (s.stick((27.0, 24.5, 25.0), (27.0, 20.0, 22.0), 0.8), 0)], sparse=8)
    # cell 3: a sheet one voxel thick (in zoomed voxels) next to a head; its own cell so that the sheet window has label-1 vertices
    sheet = np.zeros(s.vol.shape, bool)
    sheet[44:60, 4:20, 6:7] = True
    s.cell(3, [31], [(sheet, 1)])
    # cell 4: no voxel where its synapse sits -> the reference raises; cell 5: axoness 1 everywhere -> rejected
    s.cell(4, [41], [(s.ball((14.0, 22.0, 20.0), 2.0), 1)])
    spiny_cell(s, 5, [51], (16.0, 24.0, 4.0), [((13.0, 24.0, 4.0), 2.0)], shaft_axis=1, node_ax=1)
    for rep in (iso2vox(s, h1), iso2vox(s, h2), iso2vox(s, (h1 + h2) / 2), iso2vox(s, h1 + (0, 0, -2)), iso2vox(s, (20.0, 6.0, 8.0)),
                iso2vox(s, (6.5, 13.0, 9.0)),                    # on the shaft: spiness 2, rejected
                iso2vox(s, (2.0, 4.0, 3.0))):                    # clipped at the origin
        s.synapse(1, rep)
    s.synapse(2, iso2vox(s, (27.0, 24.5, 25.0)), 5)
    s.synapse(2, iso2vox(s, (27.5, 26.0, 26.5)))
    s.synapse(3, (52, 12, 6))
    s.synapse(4, iso2vox(s, (14.0, 22.0, 20.0)) + (24, 0, 0))   # 24 voxels off: the window misses the cell, its vertices vote 1
    s.synapse(5, iso2vox(s, (13.0, 24.0, 4.0)))
    return s


def case_b(seed):
    s = Scene(seed, (10, 10, 10), (8, 8, 8), (36, 32, 30), 50)
    r = s.rng
    h1, h2, h3 = (np.array(p) + r.uniform(-.4, .4, 3) for p in ([5.0, 5.5, 5.0], [5.0, 5.5, 13.0], [12.5, 5.5, 9.0]))
    spiny_cell(s, 1, [11, 12], (9.0, 14.0, 9.0), [(h1, 2.8), (h2, 2.8), (h3, 2.2)], shaft_axis=2)
    # cell 2: a straight rod of constant thickness (a plateau of maxima) labelled 1, vertices removed around one synapse
    rod = s.stick((24.0, 2.0, 22.0), (24.0, 30.0, 22.0), 2.1)
    s.cell(2, [21], [(rod, 1)], drop_box=((0, 20, 0), (40, 40, 40)))
    for rep in (iso2vox(s, h1), iso2vox(s, h2), iso2vox(s, h3), iso2vox(s, (h1 + h2) / 2 + (0, -3, 1)), iso2vox(s, (3.0, 3.0, 3.0))):
        s.synapse(1, rep)
    s.synapse(2, (24, 8, 22))
    s.synapse(2, (24, 30, 22))                                # every vertex of its box was removed: no entry
    # cell 3 (drawn last: the cells above keep their random numbers): a hollow ball that the far x face of its window cuts through
    # the cavity -> inside the window the cavity is a hole OPEN to the window border, which binary_fill_holes leaves unfilled
    shell = s.ball((30.0, 24.0, 8.0), 4.2) & ~s.ball((30.0, 24.0, 8.0), 2.2)
    s.cell(3, [31], [(shell, 1)])
    s.synapse(3, (22, 24, 8))
    return s


def case_c(seed):
    s = Scene(seed, (10, 10, 20), (15, 15, 8), (70, 60, 30), 20)
    r = s.rng
    h1, h2 = np.array([8.0, 7.0, 7.0]) + r.uniform(-.4, .4, 3), np.array([8.0, 7.0, 15.0]) + r.uniform(-.4, .4, 3)
    spiny_cell(s, 1, [11, 12, 13, 14], (8.0, 15.0, 11.0), [(h1, 3.0), (h2, 3.0)], shaft_axis=0)
    spiny_cell(s, 2, [21], (30.0, 24.0, 24.0), [((30.0, 27.0, 27.0), 2.5)], shaft_axis=0)
    for rep in (iso2vox(s, h1), iso2vox(s, h2), iso2vox(s, (h1 + h2) / 2), iso2vox(s, (3.0, 3.0, 4.0))):
        s.synapse(1, rep)
    s.synapse(2, iso2vox(s, (30.0, 27.0, 27.0)))
    return s


def case_d(seed):
    """One window = the whole 16^3 dataset, c = (8, 8, 8): the slice [c - 10 : c + 11] wraps to [14:16] on every axis.  Two one-voxel
    lines (label 1) that are not 6-connected hold two voxels of that corner each: a count tie, the smaller id wins.  A ball (a third head object, outside the slice)
    keeps the image from being trivial."""
    s = Scene(seed, (10, 10, 10), (8, 8, 8), (16, 16, 16), 5)
    a, b = np.zeros(s.vol.shape, bool), np.zeros(s.vol.shape, bool)
    a[14, 14, 3:16] = True
    b[15, 15, 1:16] = True
    b[14, 15, 1] = b[14, 14, 1] = True
    s.cell(1, [11], [(a, 1), (b, 1), (s.ball((4.0, 4.0, 4.0), 2.4), 1)])
    s.synapse(1, (8, 8, 8))
    return s


# ---- the reference's function on stand-ins ------------------------------------------------------------------------------------------
class Tree:
    def __init__(self, data):
        self.t = spatial.cKDTree(data)

    def query(self, x, k=1, n_jobs=1, **kw):
        return self.t.query(x, k=k, workers=n_jobs if n_jobs else 1, **kw)


def lifted():
    if not hasattr(np, 'bool'):
        np.bool = bool
    log = types.SimpleNamespace(debug=lambda *a: None, info=lambda *a: None, error=lambda *a: None, warning=lambda *a: None)
    sp_ns = types.SimpleNamespace(cKDTree=Tree)
    ns_c = {'np': np, 'spatial': sp_ns, 'Counter': Counter, 'log_reps': log}
    exec('from typing import *', ns_c)
    colorcode = lift_function(REF + '/reps/rep_helper.py', 'colorcode_vertices', ns_c)

    def relabel_vol_nonexist2zero(vol, label_map):
        flat = vol.reshape(-1)
        for i in range(len(flat)):
            flat[i] = label_map.get(flat[i], 0)

    def peak_local_max(distance, footprint=None, labels=None):
        assert footprint.shape == (3, 3, 3) and footprint.all()
        return R.peak_local_max(np.rint(distance * distance).astype(np.int64), labels)

    def watershed(neg_distance, markers, mask=None):
        return watershed_ref(np.rint(neg_distance * neg_distance).astype(np.int64), markers.astype(np.int32), mask.astype(np.uint8))
    ns = {'np': np, 'ndimage': ndimage, 'spatial': sp_ns, 'log_reps': log, 'colorcode_vertices': colorcode, 'peak_local_max': peak_local_max,
          'watershed': watershed, 'in_bounding_box': lambda v, b: R.in_bounding_box(v, b).tolist(),
          'relabel_vol_nonexist2zero': relabel_vol_nonexist2zero, 'kd_factory': lambda kd: kd}
    exec('from typing import *', ns)
    return lift_function(REF + '/reps/super_segmentation_helper.py', 'extract_spinehead_volume_mesh', ns)


class Kd:
    def __init__(self, vol):
        self.vol = vol

    def load_seg(self, offset, size, mag=1):
        return R.load_window(self.vol, (0, 0, 0), offset, size).swapaxes(2, 0)      # (z, y, x) like knossos_utils


class Config(dict):
    kd_seg_path = None


def make_sso(s, cell, syn):
    cfg = Config(spines={'semseg2coords_spines': dict(k=s.k, ds_vertices=DS_VERT, ignore_labels=list(IGNORE))},
                 compartments={'view_properties_semsegax': {'semseg_key': 'axoness'}, 'dist_axoness_averaging': 10000})
    cfg.kd_seg_path = Kd(s.vol)
    mine = [x for x in syn if cell['id'] in x[2]]
    sso = types.SimpleNamespace(id=cell['id'], attr_dict={'x': 0}, scaling=np.array(list(s.scaling)), sv_ids=cell['sv_ids'], config=cfg, nb_cpus=1,
                                syn_ssv=[types.SimpleNamespace(id=i, rep_coord=rep) for i, rep, _ in mine],
                                mesh=(np.zeros(0, np.uint32), cell['vertices'].reshape(-1), np.zeros(0, np.float32)))
    sso.label_dict = lambda kind: cell['vertex_labels']
    scale = SP.scale64(s.scaling)

    def semseg_for_coords(coords, key, k, ds_vertices, ignore_labels):
        v, lab = SP.spine_points(cell, ds_vertices, ignore_labels, key)
        q = np.array(coords).astype(np.float64) * scale
        return SP.knn(v, [0, len(v)], lab, np.zeros(len(q), np.int64), q, min(k, len(v)))[0]

    def attr_for_coords(coords, attr_keys):
        q = np.array(coords).astype(np.float64) * scale
        j = SP.knn(cell['nodes'].astype(np.float64) * scale, [0, len(cell['nodes'])], None, np.zeros(len(q), np.int64), q, 1)[0]
        return [np.asarray(cell['node_attrs'][a])[j] for a in attr_keys]
    sso.semseg_for_coords, sso.attr_for_coords = semseg_for_coords, attr_for_coords
    return sso


def run_case(s, fn, seen):
    out = dict(scaling=s.scaling, ctx_vol=s.ctx, k=np.int64(s.k), vol=s.vol,
               cell_ids=np.array([c['id'] for c in s.cells], np.uint64),
               cell_sv_begin=np.concatenate(([0], np.cumsum([len(c['sv_ids']) for c in s.cells]))), cell_sv=np.concatenate([c['sv_ids'] for c in s.cells]),
               cell_verts=np.concatenate([c['vertices'] for c in s.cells]), cell_vert_begin=np.concatenate(([0], np.cumsum([len(c['vertices']) for c in s.cells]))),
               cell_spiness=np.concatenate([c['vertex_labels']['spiness'] for c in s.cells]),
               cell_nodes=np.concatenate([c['nodes'] for c in s.cells]), cell_node_begin=np.concatenate(([0], np.cumsum([len(c['nodes']) for c in s.cells]))),
               cell_ax=np.concatenate([c['node_attrs'][AX_KEY] for c in s.cells]),
               syn_ids=np.array([x[0] for x in s.syn], np.uint64), syn_rep=np.array([x[1] for x in s.syn], np.int64),
               syn_cells=np.array([x[2] for x in s.syn], np.uint64))
    sh_cell, sh_syn, sh_vol, err = [], [], [], []
    for cell in s.cells:
        sso = make_sso(s, cell, s.syn)
        mine = [x for x in s.syn if cell['id'] in x[2]]
        try:
            fn(sso, ctx_vol=tuple(int(v) for v in s.ctx))
            got = sso.attr_dict['spinehead_vol']
        except ValueError as e:
            assert 'Could not find segmentation' in str(e)
            err.append(cell['id'])
            seen.add('empty mask')
            continue
        # the restatement must agree, and tells which paths the scene takes
        stages = {}
        mine_ids, mine_rep = np.array([x[0] for x in mine], np.uint64), np.array([x[1] for x in mine], np.int64).reshape(-1, 3)
        ref = R.extract_spinehead_volume(cell, mine_ids, mine_rep, (s.vol, (0, 0, 0)), s.scaling, s.ctx, s.k, DS_VERT, IGNORE, AX_KEY, stages)
        assert {int(a): float(b) for a, b in got.items()} == {int(a): float(b) for a, b in ref.items()}, (cell['id'], got, ref)
        keep = R.spinehead_filter(cell, mine_rep, s.scaling, s.k, DS_VERT, IGNORE, AX_KEY) if len(mine) else np.zeros(0, bool)
        if len(mine) and not keep.all():
            seen.add('rejected by spiness' if np.any(np.asarray(cell['node_attrs'][AX_KEY]) == 0) else 'rejected by axoness')
        seen.add('one supervoxel' if len(cell['sv_ids']) == 1 else 'several supervoxels')
        if np.isin(cell['vertex_labels']['spiness'], IGNORE).any():
            seen.add('ignore_labels')
        for sid, st in stages.items():
            rep = mine_rep[list(mine_ids).index(sid)]
            note(s, st, rep, seen)
        for a, b in got.items():
            sh_cell.append(cell['id']); sh_syn.append(int(a)); sh_vol.append(float(b))
    out.update(sh_cell=np.array(sh_cell, np.uint64), sh_syn=np.array(sh_syn, np.uint64), sh_vol=np.array(sh_vol, np.float64), err_cells=np.array(err, np.uint64))
    return out


def note(s, st, rep, seen):
    size = 2 * s.ctx
    if np.any(rep - s.ctx < 0):
        seen.add('clipped at origin')
    if np.any(np.maximum(rep - s.ctx, 0) + size > s.vol.shape):
        seen.add('overhang')
    if (st['filled'] != st['mask']).any():
        seen.add('closed hole filled')
    bg, n_bg = ndimage.label(st['mask'] == 0)
    if n_bg > 1:                                                   # a pocket of background apart from the outside that reaches the window border
        border = np.ones(bg.shape, bool)
        border[1:-1, 1:-1, 1:-1] = False
        sizes = np.bincount(bg.ravel())
        for i in np.unique(bg[border]):
            if i > 0 and sizes[i] < sizes[1:].max() and not st['filled'][bg == i].any():
                seen.add('open hole unfilled')
    if not st['entry']:
        seen.add('no vertex in box')
        return
    pts = st['points']
    if 0 < len(pts) < s.k:
        seen.add('k above vertices')
    if len(st['peaks']) == 0:
        seen.add('no peaks')
        if st['n_voxels'] == 0:
            seen.add('entry 0.0')
    else:
        p = st['peaks']
        d = np.abs(p[:, None, :] - p[None, :, :]).max(-1)
        if np.any(d == 1):
            seen.add('plateau')
        q = p.astype(np.float64) * s.ds
        k1 = min(s.k + 1, len(pts))
        d2 = np.sort(SP.sq_dist(q, pts), 1)[:, :k1]
        assert not np.any(np.diff(d2, axis=1) == 0), 'a kNN distance tie'
    if st['nb_obj'] > 1:
        c = rep - np.maximum(rep - s.ctx, 0)
        ls = st['objects'][(c[0] - 10):(c[0] + 11), (c[1] - 10):(c[1] + 11), (c[2] - 10):(c[2] + 11)]
        ids, cnt = np.unique(ls[ls > 0], return_counts=True)
        if len(ids) == 0:
            seen.add('fallback')
            if np.any(c < 10):
                seen.add('fallback with c < 10 at the origin' if np.any(rep - s.ctx < 0) else 'fallback with c < 10')
            co = np.transpose(np.nonzero(st['objects']))
            d2 = (((co - c) * s.scaling.astype(np.float64)) ** 2).sum(1)
            near = np.unique(st['objects'][tuple(co[d2 == d2.min()].T)])
            assert len(near) == 1, 'a fallback distance tie'
        elif len(ids) > 1 and np.sum(cnt == cnt.max()) > 1:
            seen.add('count tie')
        elif len(ids) > 1:
            seen.add('count')
        else:
            seen.add('count (one object in the slice)')


WANT = ['clipped at origin', 'overhang', 'closed hole filled', 'open hole unfilled', 'count', 'count tie', 'fallback',
        'fallback with c < 10 at the origin', 'one supervoxel',
        'several supervoxels', 'no vertex in box', 'entry 0.0', 'empty mask', 'ignore_labels', 'k above vertices', 'rejected by spiness',
        'rejected by axoness', 'plateau']


def main(seeds=(1, 1, 1, 1), path=os.path.join(HERE, 'g22_spinehead.npz'), write=True):
    fn = lifted()
    seen, out = set(), {}
    for prefix, make, seed in (('a_', case_a, seeds[0]), ('b_', case_b, seeds[1]), ('c_', case_c, seeds[2]), ('d_', case_d, seeds[3])):
        s = make(seed)
        for key, v in run_case(s, fn, seen).items():
            out[prefix + key] = v
    # the zoom of case c drops its last plane (scipy's rounding, 30 -> 15 samples)
    z = ndimage.zoom(np.arange(1, 31), 1 / 2, order=0)
    assert z[-1] == 0 and len(z) == 15
    missing = [w for w in WANT if w not in seen]
    print('seen:', sorted(seen))
    print('missing:', missing)
    if write:
        assert not missing, missing
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), 'bytes')
    return missing


if __name__ == '__main__':
    main()
