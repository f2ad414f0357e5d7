"""Restatement in numpy and a small union-find of what csrc/sd_glia.hip computes (own code, independent of the device code): the rule of
``remove_glia_nodes`` (/root/reference/syconn/proc/graphs.py:278-360) for all cells of a graph at once, the split graphs of
``write_astrocyte_svgraph`` (proc/glia_splitting.py:77-161) and ``glia_pred_so`` / ``glia_proba_so`` (reps/segmentation_helper.py:32-78).
tests/test_glia_split_cpu.py checks it against the golden of the reference's own functions and against a networkx statement of the rule."""
import numpy as np

U = np.uint64
SKIP = -1


def ordered_norm(d):
    """sqrt(((dx dx) + dy dy) + dz dz) in float64, every operation rounded on its own; d (..., 3)."""
    d = np.asarray(d, np.float64)
    return np.sqrt(((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def roots(n, ea, eb, grp):
    """Per node the smallest node of its set after uniting the edges whose two ends have the same group other than SKIP."""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    g = grp.tolist()
    for a, b in zip(ea.tolist(), eb.tolist()):
        if g[a] == SKIP or g[a] != g[b]:
            continue
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], np.int64).reshape(n)


def root_sizes(root, grp, lo, hi):
    """Per node the size of its set (NaN for SKIP): the norm of the extent of the union of the boxes."""
    n = len(root)
    mn, mx = np.full((n, 3), np.inf), np.full((n, 3), -np.inf)
    part = grp != SKIP
    np.minimum.at(mn, root[part], lo[part])
    np.maximum.at(mx, root[part], hi[part])
    size = np.full(n, np.nan)
    r = np.flatnonzero(part & (root == np.arange(n)))
    size[r] = ordered_norm(mx[r] - mn[r])
    out = np.full(n, np.nan)
    out[part] = size[root[part]]
    return out


def csr(node_ids, root, cellroot, member):
    """Components of the member nodes by root: ascending by root, members ascending inside."""
    rows = np.flatnonzero(member)
    order = rows[np.argsort(root[rows], kind='stable')]
    r = root[order]
    head = np.flatnonzero(np.concatenate(([True], r[1:] != r[:-1]))) if len(r) else np.zeros(0, np.int64)
    return dict(cc_ids=node_ids[r[head]], cc_cell=node_ids[cellroot[r[head]]], sv_begin=np.concatenate((head, [len(r)])).astype(np.int64),
                sv_ids=node_ids[order])


def split_table(edges, sv_ids, boxes_nm, glia, T, nodes=None, cell_size=None, min_cell_size=None, sv_sizes=None):
    """-> dict with the outputs of ``sd_glia_split`` (node_*, cell_*, ncc_* / gcc_* tables as dicts ``neuron`` / ``glia``, the two edge
    arrays) and ``counts`` (16 slots as the device fills them).  Every node must be in the table."""
    edges = np.asarray(edges, U).reshape(-1, 2)
    extra = np.zeros(0, U) if nodes is None else np.asarray(nodes, U).reshape(-1)
    ids = np.asarray(sv_ids, U).reshape(-1)
    boxes = np.asarray(boxes_nm, np.float64).reshape(-1, 2, 3)
    node_ids = np.unique(np.concatenate([edges.reshape(-1), extra]))
    n = len(node_ids)
    row = np.searchsorted(ids, node_ids)
    assert n == 0 or ((row < len(ids)).all() and (ids[row] == node_ids).all()), 'a node is not in the table'
    cls = (np.asarray(glia).reshape(-1)[row] != 0).astype(np.int64)
    lo, hi = np.minimum(boxes[row, 0], boxes[row, 1]), np.maximum(boxes[row, 0], boxes[row, 1])
    ea, eb = np.searchsorted(node_ids, edges[:, 0]), np.searchsorted(node_ids, edges[:, 1])
    alive = np.ones(n, bool) if cell_size is None else ~(np.asarray(cell_size, np.float64).reshape(-1)[row] < min_cell_size)
    cellroot = roots(n, ea, eb, np.zeros(n, np.int64))
    # steps 1 and 2: components of one class
    root_b = roots(n, ea, eb, cls)
    size1 = root_sizes(root_b, cls, lo, hi)
    sig = size1 > T
    has_n, has_g = np.zeros(n, bool), np.zeros(n, bool)
    np.logical_or.at(has_n, cellroot, sig & (cls == 0))
    np.logical_or.at(has_g, cellroot, sig & (cls == 1))
    outcome = np.where(~has_n[cellroot], 1, np.where(~has_g[cellroot], 2, 3))
    # step 3
    tiny = (cls == 1) & (size1 < T)
    grp_c = np.where((outcome == 3) & ((cls == 0) | tiny), 0, SKIP)
    root_c = roots(n, ea, eb, grp_c)
    size2 = root_sizes(root_c, grp_c, lo, hi)
    stays = (grp_c != SKIP) & ~(size2 < T)
    fcls = np.where(outcome == 1, 1, np.where(outcome == 2, 0, np.where(stays, 0, 1)))
    root_d = roots(n, ea, eb, fcls)
    cells = np.flatnonzero(cellroot == np.arange(n))
    ok = lambda c: (fcls[ea] == c) & (fcls[eb] == c) & alive[ea] & alive[eb]
    out = dict(node_ids=node_ids, node_cell=node_ids[cellroot], node_class=fcls.astype(np.uint8), node_comp=node_ids[root_d], node_size1=size1,
               node_size2=size2, cell_ids=node_ids[cells], cell_outcome=outcome[cells].astype(np.uint8),
               neuron=csr(node_ids, root_d, cellroot, (fcls == 0) & alive), glia=csr(node_ids, root_d, cellroot, (fcls == 1) & alive),
               neuron_edges=edges[ok(0)], astrocyte_edges=edges[ok(1)])
    counts = np.zeros(16, np.int64)
    counts[[0, 1]] = n, len(cells)
    counts[[2, 3, 4, 5]] = len(out['neuron']['cc_ids']), len(out['neuron']['sv_ids']), len(out['glia']['cc_ids']), len(out['glia']['sv_ids'])
    counts[[6, 8]] = len(out['neuron_edges']), len(out['astrocyte_edges'])
    if sv_sizes is not None:
        counts[9] = int(np.asarray(sv_sizes, np.int64).reshape(-1)[row][(fcls == 1) & alive].sum())
    counts[13:16] = [(outcome[cells] == k).sum() for k in (1, 2, 3)]
    out['counts'] = counts
    return out


def as_lists(res):
    """Per cell (ascending) ``(neuron_ccs, glia_ccs)``, every component a sorted list of ints."""
    out = [([], []) for _ in res['cell_ids']]
    for k, t in enumerate((res['neuron'], res['glia'])):
        for c, a, b in zip(np.searchsorted(res['cell_ids'], t['cc_cell']), t['sv_begin'][:-1], t['sv_begin'][1:]):
            out[c][k].append(t['sv_ids'][a:b].tolist())
    return out


def glia_pred(probas, view_begin, thresh, point_model):
    """-> (classes uint8, means float64): the float64 sum in view order divided once; no views: class 0, mean NaN."""
    p = np.asarray(probas).reshape(-1)
    vb = np.asarray(view_begin, np.int64)
    cls, mean = np.zeros(len(vb) - 1, np.uint8), np.full(len(vb) - 1, np.nan)
    for i, (a, b) in enumerate(zip(vb[:-1], vb[1:])):
        if b == a:
            continue
        v = p[a:b].astype(np.float64)
        mean[i] = np.cumsum(v)[-1] / float(b - a)                                 # cumsum adds one after another
        if point_model:
            cls[i] = mean[i] >= thresh
        else:
            cls[i] = mean[i] > thresh and int((v > thresh).sum()) > int((b - a) * 0.7)
    return cls, mean


def random_cells(rng, n_cells, max_nodes=40):
    """Connected cells with self loops and duplicate edges on a 100 nm lattice: every squared diagonal is exact, so its
    correctly rounded root has one value."""
    edges, cells, nxt = [], [], 5
    ids, boxes, glia = [], [], []
    for _ in range(n_cells):
        n = int(rng.integers(1, max_nodes))
        cid = np.arange(nxt, nxt + n)
        nxt += n + int(rng.integers(1, 4))
        e = [(int(rng.integers(0, b)), b) for b in range(1, n)] + [tuple(rng.integers(0, n, 2).tolist()) for _ in range(int(rng.integers(0, n + 1)))]
        if n == 1 or rng.random() < 0.3:
            e.append((0, 0))
        e = np.array(e, np.int64).reshape(-1, 2)
        e = np.where(rng.random((len(e), 1)) < 0.5, e[:, ::-1], e)
        lo = rng.integers(0, 30, (n, 3)) * 100 * np.array([1, 0, 0]) + rng.integers(0, 2, (n, 3)) * 100
        hi = lo + rng.integers(0, 12, (n, 3)) * 100 * np.array([1, 1, 0])
        ids.append(cid); boxes.append(np.stack([lo, hi], 1)); glia.append(rng.random(n) < rng.choice([0.1, 0.5, 0.9]))
        edges.append(cid[e]); cells.append(cid)
    edges = np.concatenate(edges)
    return edges[rng.permutation(len(edges))].astype(U), np.concatenate(ids).astype(U), np.concatenate(boxes).astype(np.float64), np.concatenate(glia).astype(np.uint8), cells
