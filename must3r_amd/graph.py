"""Pair graph from retrieval scores (must3r/retrieval/graph.py:9-76), host numpy.

Both functions draw from ``np.random`` as the reference does -- one ``np.random.choice(n)`` for the first anchor -- so a seeded run
picks the same anchors and returns the same arrays.  Argmax ties go to the lowest index, as numpy's do.
"""
import numpy as np


def farthest_point_sampling(dist, N=None, dist_thresh=None):
    """Greedy farthest points of an n x n distance matrix -> (indices, distances).  The first index is random; each next one
    maximises the distance to the nearest index already taken.  Stops after N indices (default n) or, with ``dist_thresh``,
    once that distance falls below it.  ``distances[0]`` is 0."""
    if N is None and dist_thresh is None:
        raise ValueError("farthest_point_sampling: give N or dist_thresh")
    n = dist.shape[0]
    if N is None:
        N = n
    taken = [np.random.choice(n)]
    gaps = [0]
    nearest = np.array(dist[taken[0]], copy=True)   # min over the taken rows, kept up to date
    while len(taken) < N:
        best = nearest.argmax()
        gap = nearest[best]
        if dist_thresh is not None and gap < dist_thresh:
            break
        taken.append(best)
        gaps.append(gap)
        nearest = np.minimum(nearest, dist[best])
    return np.array(taken), np.array(gaps)


def make_pairs_fps(sim_mat, Na=20, tokK=1, dist_thresh=None):
    """Pairs (i, j) for pairwise reconstruction -> (list of pairs, anchor indices): all pairs among ``Na`` farthest-point anchors
    (in anchor order), each other image with its nearest anchor, and each image with its ``tokK`` nearest images."""
    dist_mat = 1 - sim_mat
    pairs = set()
    anchors = np.array([])
    if Na != 0:
        anchors, _ = farthest_point_sampling(dist_mat, N=Na, dist_thresh=dist_thresh)
        for a in range(len(anchors)):
            for b in range(a + 1, len(anchors)):
                pairs.add((anchors[a], anchors[b]))
        to_anchor = dist_mat[:, anchors]
        for i in range(to_anchor.shape[0]):
            if i in anchors:
                continue
            j = anchors[to_anchor[i].argmin()]
            p = (min(i, j), max(i, j))
            if p[0] != p[1] and p not in pairs:
                pairs.add(p)
    if tokK > 0:
        for i in range(dist_mat.shape[0]):
            for j in dist_mat[i].argsort()[:tokK]:
                p = (min(i, j), max(i, j))
                if p[0] != p[1] and p not in pairs:
                    pairs.add(p)
    return list(pairs), anchors
