"""GPU: csrc/sd_cell_assembly.hip past one grid stride of every kernel (SD_CELLASM_GRID blocks of 256 items), on analytic inputs whose
answers are closed forms, not the restatement.  Every scratch is followed by a guard band that must stay untouched (tests/
_cell_assembly_gpu.py)."""
import numpy as np
import pytest

import _cell_assembly_gpu as D
from syconn_amd import _lib as L

pytestmark = pytest.mark.gpu
U = np.uint64
STRIDE = L.SD_CELLASM_GRID * 256


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_disjoint_paths(gpu):
    """Paths of 1 .. 900 nodes: path l owns the ids first(l) .. first(l) + l - 1, first(l) = 1 + l (l - 1) / 2; node p of it has the box
    [(10 p, l, 0), (10 p + 5, l + 1, 1)].  With scaling (2, 3, 4) the diagonal of path l is sqrt((2 (10 (l - 1) + 5))^2 + 9 + 16): an
    exactly representable sum under a correctly rounded root.  The threshold is the diagonal of path 100: 1 .. 100 go, 101 .. 900 stay."""
    lengths = np.arange(1, 901)
    first = 1 + lengths * (lengths - 1) // 2
    n = int(lengths.sum())
    assert n == 405450 and n - 900 == 404550 and n > STRIDE and n - 900 > STRIDE
    ids = np.arange(1, n + 1, dtype=U)
    path = np.repeat(lengths, lengths)                                              # the path of every node
    pos = np.arange(n) - np.repeat(first - 1, lengths)                              # its position inside
    sizes = (np.arange(n) % 7 + 1).astype(np.int64)
    lo = np.stack([10 * pos, path, np.zeros(n, np.int64)], 1)
    boxes = np.stack([lo, lo + np.array([5, 1, 1])], 1)
    rep = lo + 1
    inner = pos > 0
    edges = np.stack([ids[inner] - U(1), ids[inner]], 1)
    rng = np.random.default_rng(51)
    edges = edges[rng.permutation(len(edges))]                                      # a fixed pseudo-random order, either direction
    flip = rng.random(len(edges)) < 0.5
    edges[flip] = edges[flip][:, ::-1]
    diag = np.sqrt((2.0 * (10 * (lengths - 1) + 5)) ** 2 + 9.0 + 16.0)
    tab = D.table(gpu, ids, sizes, rep, np.arange(n + 1), boxes)
    rc, counts, got = D.components(gpu, edges, tab, (2, 3, 4), diag[99], True)
    assert rc == 0 and not counts[5:].any()
    kept = lengths > 100
    kept_node = path > 100
    assert same_bits(got['node_ids'], ids)
    assert same_bits(got['node_comp'], np.where(kept_node, np.repeat(first, lengths), 0).astype(U))
    assert same_bits(got['node_size'], np.repeat(diag, lengths))
    assert same_bits(got['ssv_ids'], first[kept].astype(U))
    assert same_bits(got['sv_begin'], np.concatenate(([0], np.cumsum(lengths[kept]))).astype(np.int64))
    assert same_bits(got['sv_ids'], ids[kept_node])
    assert same_bits(got['edges'], edges[kept_node[edges[:, 0].astype(np.int64) - 1]])
    assert got['total_size'] == int(sizes[kept_node].sum())
    # the properties of the kept cells, their lists reversed: the first supervoxel of a list is then the LAST node of the path
    sv_begin, sv_ids = got['sv_begin'], got['sv_ids']
    rev = (sv_begin[:-1] + sv_begin[1:] - 1).repeat(lengths[kept]) - np.arange(len(sv_ids))
    rc, counts, size, box, r = D.props(gpu, sv_begin, sv_ids[rev], tab)
    lk = lengths[kept]
    assert rc == 0 and not counts.any() and len(sv_ids) > STRIDE
    assert same_bits(size, np.add.reduceat(sizes[kept_node], sv_begin[:-1]))
    zero = np.zeros(len(lk), np.int64)
    assert same_bits(box, np.stack([np.stack([zero, lk, zero], 1), np.stack([10 * (lk - 1) + 5, lk + 1, zero + 1], 1)], 1).astype(np.int32))
    assert same_bits(r, np.stack([10 * (lk - 1) + 1, lk + 1, zero + 1], 1).astype(np.int32))


def test_exact_ratio_sums(gpu):
    """300,000 records over 1000 cells: every cell has 30 supervoxels (a shuffled list) and 10 organelles of 2^16 voxels of its own; the
    count of (cell c, organelle t, list position p) is 2^((p t + c + t) mod 14): every ratio and every partial sum is a multiple of
    2^-16 below 2^3, so the sum of a run is exact in any order and equals the integer sum / 2^16."""
    n_cells, n_sv, n_org = 1000, 30, 10
    rng = np.random.default_rng(52)
    sv = rng.choice(2 ** 62, n_cells * n_sv, replace=False).astype(U) * U(4) + U(3)
    sv_begin = np.arange(n_cells + 1) * n_sv
    ssv_ids = np.minimum.reduceat(sv, sv_begin[:-1])
    order = np.argsort(ssv_ids)                                                      # cells ascend by their smallest supervoxel
    sv = sv.reshape(n_cells, n_sv)[order].reshape(-1)
    c, t, p = np.meshgrid(np.arange(n_cells), np.arange(n_org), np.arange(n_sv), indexing='ij')
    count = (1 << ((p * t + c + t) % 14)).astype(np.int64)
    org_ids = (np.arange(n_cells * n_org, dtype=U) + U(1)) * U(2 ** 40)
    sub, rsv = org_ids[(c * n_org + t).reshape(-1)], sv[(c * n_sv + p).reshape(-1)]
    shuffle = rng.permutation(count.size)
    assert count.size == 300000 and count.size > STRIDE
    rc, counts, got = D.mapping(gpu, sv_begin, sv, sub[shuffle], rsv[shuffle], count.reshape(-1)[shuffle], org_ids, np.full(len(org_ids), 2 ** 16), 0.5, 0.9, 0)
    ratio = count.sum(2).reshape(-1) / 2.0 ** 16
    acc = (ratio > 0.5) & (ratio <= 0.9)
    assert rc == 0 and not counts[5:].any() and counts[0] == 300000 and counts[1] == len(org_ids) and counts[2] == acc.sum()
    assert acc.any() and (ratio > 0.9).any() and (ratio <= 0.5).any()
    assert same_bits(got['cell_begin'], (np.arange(n_cells + 1) * n_org).astype(np.int64)) and same_bits(got['ids'], org_ids)
    assert same_bits(got['ratios'], ratio) and same_bits(got['accepted'], acc)
    assert same_bits(got['acc_begin'], np.concatenate(([0], np.cumsum(acc.reshape(n_cells, n_org).sum(1)))).astype(np.int64))
    assert same_bits(got['acc_ids'], org_ids[acc])
    assert same_bits(got['org_n_cells'], acc.astype(np.int64))
    assert same_bits(got['org_first_cell'], np.where(acc, np.repeat(np.arange(n_cells), n_org), -1).astype(np.int64))


def test_synapses_past_one_stride(gpu):
    """150,000 synapses (300,000 half records) between 500 cells: synapse i joins cells i mod 500 and (7 i + 1) mod 500; every third is
    below the threshold.  The list of cell c: the kept i with i mod 500 == c ascending, then those with (7 i + 1) mod 500 == c."""
    n, n_cells = 150000, 500
    i = np.arange(n)
    ssv_ids = (np.arange(n_cells, dtype=U) + U(1)) * U(2 ** 50)
    a, b = i % n_cells, (7 * i + 1) % n_cells
    keep = i % 3 != 0
    ids = (i + 10 ** 12).astype(U)
    rc, counts, begin, out = D.synapses(gpu, ssv_ids, np.stack([ssv_ids[a], ssv_ids[b]], 1), keep, ids)
    ik = i[keep]
    s0, s1 = ik[np.argsort(a[keep], kind='stable')], ik[np.argsort(b[keep], kind='stable')]
    n0, n1 = np.bincount(a[keep], minlength=n_cells), np.bincount(b[keep], minlength=n_cells)
    want = np.concatenate([x for c0, c1 in zip(np.split(s0, np.cumsum(n0)[:-1]), np.split(s1, np.cumsum(n1)[:-1])) for x in (c0, c1)])
    assert rc == 0 and counts[7] == 0 and 2 * n > STRIDE and counts[0] == 2 * keep.sum()
    assert same_bits(begin, np.concatenate(([0], np.cumsum(n0 + n1))).astype(np.int64)) and same_bits(out, ids[want])
