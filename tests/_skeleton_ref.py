"""numpy / pure-Python restatement of the skeleton votes (the semantics csrc/sd_skeleton.hip reproduces), used by the CPU and the GPU
tests.  The distances come from a label-correcting search (a FIFO of nodes whose distance went down), NOT from Dijkstra's heap:
dist(v) is the least fixed point of dist[v] = min(dist[u] + w) over float64 sums that start at the source, so both give the same
bits; tests/golden/g23_skeleton.npz (networkx, through the reference's own functions) pins that."""
from collections import deque

import numpy as np


def edge_weights(nodes, edges, scaling):
    """weighted_graph's expression (super_segmentation_object.py:1440-1444) for one cell."""
    node_scaled = np.asarray(nodes) * scaling
    edge_coords = node_scaled[np.asarray(edges, np.int64).reshape(-1, 2)]
    return np.linalg.norm(edge_coords[:, 0] - edge_coords[:, 1], axis=1)


def adjacency(n, edges, weights):
    adj = [[] for _ in range(n)]
    for (a, b), w in zip(np.asarray(edges).reshape(-1, 2).tolist(), np.asarray(weights, np.float64).tolist()):
        adj[a].append((b, w))
        adj[b].append((a, w))
    return adj


def window(adj, src, max_dist):
    """{node: distance} of the nodes within max_dist of src."""
    dist, queue, queued = {src: 0.0}, deque([src]), {src}
    while queue:
        u = queue.popleft()
        queued.discard(u)
        for v, w in adj[u]:
            nd = dist[u] + w
            if nd > max_dist:
                continue
            if v not in dist or nd < dist[v]:
                dist[v] = nd
                if v not in queued:
                    queued.add(v)
                    queue.append(v)
    return dist


def smallest_most_frequent(values):
    cls, cnts = np.unique(values, return_counts=True)
    return cls[np.argmax(cnts)]


def majority_vote(nodes, node_begin, edges, edge_begin, labels, scaling, max_dist):
    """-> (vote per node in the dtype of labels, window size per node uint32), cell by cell."""
    labels = np.asarray(labels).reshape(-1)
    vote, reached = labels.copy(), np.zeros(len(labels), np.uint32)
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    for c in range(len(node_begin) - 1):
        n0, n1, e0, e1 = node_begin[c], node_begin[c + 1], edge_begin[c], edge_begin[c + 1]
        adj = adjacency(n1 - n0, edges[e0:e1], edge_weights(np.asarray(nodes)[n0:n1], edges[e0:e1], scaling))
        for s in range(n1 - n0):
            win = np.fromiter(window(adj, s, float(max_dist)), np.int64)
            vote[n0 + s] = smallest_most_frequent(labels[n0:n1][win])
            reached[n0 + s] = len(win)
    return vote, reached


def share_below_066(c1, total):
    """The integer form of `float32(c1) / total < 0.66`."""
    return 50 * c1 < 33 * total


def compartment_majority(node_begin, edges, edge_begin, labels, soma_label=2):
    labels = np.asarray(labels).reshape(-1)
    out = labels.copy()
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    for c in range(len(node_begin) - 1):
        n0, n1 = node_begin[c], node_begin[c + 1]
        lab = labels[n0:n1]
        parent = list(range(n1 - n0))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a
        for a, b in edges[edge_begin[c]:edge_begin[c + 1]].tolist():
            if lab[a] != soma_label and lab[b] != soma_label:
                parent[find(a)] = find(b)
        root = np.array([find(a) for a in range(n1 - n0)], np.int64)
        for r in np.unique(root[lab != soma_label]):
            members = np.flatnonzero((root == r) & (lab != soma_label))
            maj = smallest_most_frequent(lab[members])
            if maj == 1 and share_below_066(int((lab[members] == 1).sum()), len(members)):
                maj = 0
            out[n0 + members] = maj
    return out
