"""Restatement in plain Python / numpy of what the cell assembly replaces in the reference, for the parts the golden
(tests/golden/make_golden_cell_assembly.py) cannot lift and for random inputs: the graph preparation and the four filter lines of
``run_create_rag`` (exec/exec_init.py:318-350; with ``strict=False`` the ``<`` of ``run_create_neuron_ssd``, :74-76), the size of
``create_ccsize_dict`` (proc/graphs.py:238-248), the cell attributes (reps/super_segmentation_object.py:713-727, :1148-1168), the
ratio normalisation of proc/sd_proc.py:1063-1084, the ``Counter`` sums and the decisions of proc/ssd_proc.py (:74-90, :220-232) and
``map_synssv_objects_thread`` (:329-341).  Object by object, as the reference: slow on purpose."""
from collections import Counter

import numpy as np


def merged_boxes(box_begin, boxes):
    """Per table id its one box [[min], [max]] over its chunk boxes (what a SegmentationDataset stores)."""
    boxes = np.asarray(boxes).reshape(-1, 2, 3)
    return [np.stack([boxes[a:b, 0].min(0), boxes[a:b, 1].max(0)]) for a, b in zip(box_begin[:-1], box_begin[1:])]


def components(edges, ids, sizes, box_begin, boxes, scaling, min_cc_size, strict=True):
    """-> dict(node_ids, node_comp, node_size, ssv_ids, sv_begin, sv_ids, edges, total_size); raises ValueError for a component
    without a box."""
    edges = np.asarray(edges, np.uint64).reshape(-1, 2)
    ids = [int(i) for i in ids]
    nodes = sorted((set(edges.reshape(-1).tolist()) | set(ids)) - {0})
    parent = {n: n for n in nodes}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in edges.tolist():
        if a and b:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    ccs = {}
    for n in nodes:
        ccs.setdefault(find(n), []).append(n)
    bbs = dict(zip(ids, (b * np.asarray(scaling) for b in merged_boxes(box_begin, boxes))))        # sd.load_numpy_data('bounding_box') * sd.scaling
    size_of = dict(zip(ids, (int(s) for s in sizes)))
    node_size = {}
    for cc in ccs.values():
        curr_bbs = [bbs[n] for n in cc if n in bbs]
        if len(curr_bbs) == 0:
            raise ValueError(f'Could not find a single bounding box for connected component with IDs: {cc}.')
        curr_bbs = np.concatenate(curr_bbs)
        cc_size = np.linalg.norm(np.max(curr_bbs, axis=0) - np.min(curr_bbs, axis=0), ord=2)
        for n in cc:
            node_size[n] = cc_size
    dropped = (lambda s: s <= min_cc_size) if strict else (lambda s: s < min_cc_size)
    kept = {root: cc for root, cc in ccs.items() if not dropped(node_size[root])}
    comp = {n: root for root, cc in kept.items() for n in cc}
    ssv_ids = sorted(kept)
    sv_ids = [n for root in ssv_ids for n in kept[root]]
    keep_edge = [bool(a and b and a in comp) for a, b in edges.tolist()]
    return dict(node_ids=np.array(nodes, np.uint64), node_comp=np.array([comp.get(n, 0) for n in nodes], np.uint64),
                node_size=np.array([node_size[n] for n in nodes], np.float64), ssv_ids=np.array(ssv_ids, np.uint64),
                sv_begin=np.concatenate(([0], np.cumsum([len(kept[r]) for r in ssv_ids]))).astype(np.int64), sv_ids=np.array(sv_ids, np.uint64),
                edges=edges[np.array(keep_edge, bool)].reshape(-1, 2), total_size=sum(size_of.get(n, 0) for n in sv_ids))


def explicit_cells(sv_begin, sv_ids):
    """Cells from explicit lists: id = the smallest supervoxel (``cc_dict[np.min(cc)] = cc``), cells ascending, lists as given."""
    lists = [np.asarray(sv_ids, np.uint64)[a:b] for a, b in zip(sv_begin[:-1], sv_begin[1:])]
    lists.sort(key=lambda cc: int(cc.min()))
    return (np.array([cc.min() for cc in lists], np.uint64), np.concatenate(([0], np.cumsum([len(cc) for cc in lists]))).astype(np.int64),
            np.concatenate(lists) if lists else np.zeros(0, np.uint64))


def cell_props(sv_begin, sv_ids, ids, sizes, rep_coords, box_begin, boxes, allow_missing=False):
    """-> size int64 (n), bounding_box int32 (n, 2, 3), rep_coord int32 (n, 3)."""
    row = {int(i): k for k, i in enumerate(ids)}
    mb = merged_boxes(box_begin, boxes)
    out_size, out_box, out_rep = [], [], []
    for a, b in zip(sv_begin[:-1], sv_begin[1:]):
        svs = [int(s) for s in sv_ids[a:b]]
        if not allow_missing and any(s not in row for s in svs):
            raise ValueError('supervoxel not in the table')
        known = [row[s] for s in svs if s in row]
        if len(known) == 0:
            out_size.append(0)
            out_box.append(np.zeros((2, 3), np.int32))
        else:
            bounding_boxes = [mb[k] for k in known]
            out_size.append(np.sum([sizes[k] for k in known]))
            out_box.append(np.stack([np.min(bounding_boxes, axis=0)[0], np.max(bounding_boxes, axis=0)[1]]).astype(np.int32))
        out_rep.append(np.asarray(rep_coords[row[svs[0]]] if svs and svs[0] in row else np.zeros(3), np.int32))
    return np.array(out_size, np.int64), np.array(out_box, np.int32).reshape(-1, 2, 3), np.array(out_rep, np.int32).reshape(-1, 3)


def sv_mapping_dicts(rec_sub, rec_sv, rec_count, org_ids, org_sizes):
    """sd_proc.py:1063-1084: supervoxel -> {organelle: count / size}; organelles outside the size table are dropped."""
    size_dc = dict(zip((int(i) for i in org_ids), org_sizes))
    md = {}
    for sub, sv, cnt in zip(rec_sub.tolist(), rec_sv.tolist(), rec_count):
        if sub not in size_dc:
            continue
        md.setdefault(sv, {})[sub] = cnt / size_dc[sub]
    return md


def aggregate(ssv_ids, sv_begin, sv_ids, sv_md):
    """ssd_proc.py:74-90 for one object type, lists sorted by organelle id.  -> cell_begin, ids, ratios"""
    begin, ids, ratios = [0], [], []
    for a, b in zip(sv_begin[:-1], sv_begin[1:]):
        mapping = Counter()
        for svid in sv_ids[a:b].tolist():
            dc = sv_md.get(svid, {})
            mapping += Counter(dict(zip(dc.keys(), dc.values())))
        for k in sorted(mapping):
            ids.append(k)
            ratios.append(mapping[k])
        begin.append(len(ids))
    return np.array(begin, np.int64), np.array(ids, np.uint64), np.array(ratios, np.float64)


def decide(ids, ratios, org_ids, org_sizes, lower_ratio, upper_ratio, sizethreshold):
    """ssd_proc.py:220-232 -> accepted flag per pair."""
    size_dc = dict(zip((int(i) for i in org_ids), org_sizes))
    id_mask = ratios > lower_ratio
    if upper_ratio < 1.:
        id_mask[ratios > upper_ratio] = False
    return np.array([bool(m) and size_dc[int(i)] > sizethreshold for i, m in zip(ids, id_mask)], bool)


def mapping(ssv_ids, sv_begin, sv_ids, rec_sub, rec_sv, rec_count, org_ids, org_sizes, lower_ratio, upper_ratio, sizethreshold):
    """-> dict(cell_begin, ids, ratios, accepted, acc_begin, acc_ids, org_n_cells, org_first_cell)."""
    in_cell = set(np.asarray(sv_ids).tolist())
    md = {sv: dc for sv, dc in sv_mapping_dicts(rec_sub, rec_sv, rec_count, org_ids, org_sizes).items() if sv in in_cell}
    cell_begin, ids, ratios = aggregate(ssv_ids, sv_begin, sv_ids, md)
    acc = decide(ids, ratios, org_ids, org_sizes, lower_ratio, upper_ratio, sizethreshold)
    acc_begin = np.concatenate(([0], np.cumsum(acc)))[cell_begin]
    cell_of = np.repeat(np.asarray(ssv_ids, np.uint64), np.diff(cell_begin))
    n_cells, first = np.zeros(len(org_ids), np.int64), np.zeros(len(org_ids), np.uint64)
    for i, c in zip(ids[acc].tolist(), cell_of[acc].tolist()):
        o = int(np.searchsorted(org_ids, np.uint64(i)))
        if n_cells[o] == 0:
            first[o] = c
        n_cells[o] += 1
    return dict(cell_begin=cell_begin, ids=ids, ratios=ratios, accepted=acc, acc_begin=acc_begin.astype(np.int64), acc_ids=ids[acc], org_n_cells=n_cells,
                org_first_cell=first)


def cell_synapses(ssv_ids, neuron_partners, syn_prob, syn_ids, syn_threshold):
    """ssd_proc.py:329-341 -> syn_begin, syn_ids."""
    synssv_ids = syn_ids[syn_prob > syn_threshold]
    ssv_partners = neuron_partners[syn_prob > syn_threshold]
    begin, out = [0], []
    for ssv_id in ssv_ids:
        curr_synssv_ids = synssv_ids[np.isin(ssv_partners[:, 0], ssv_id)]
        curr_synssv_ids = np.concatenate([curr_synssv_ids, synssv_ids[np.isin(ssv_partners[:, 1], ssv_id)]])
        out.append(curr_synssv_ids)
        begin.append(begin[-1] + len(curr_synssv_ids))
    return np.array(begin, np.int64), np.concatenate(out).astype(np.uint64) if out else np.zeros(0, np.uint64)
