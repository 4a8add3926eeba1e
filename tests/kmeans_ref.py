"""The reference arithmetic of the k-means update (csrc/asmk_train.hip, must3r_hip_kmeans_update) in numpy float64, with bounds that count the roundings of
a correct kernel.  With u = 2^-53 (fp64) and 2^-24 (the one fp32 rounding of the stored centroid):

    centroid   |got - ref| <= 2^-24 |ref| + (n_c + 1) u (sum_j |x_j|) / n_c     n_c - 1 fp64 additions in any fixed order, one division, against a reference
                                                                                whose own sum is off by as much; then the rounding to fp32
    dist[j]    |got - ref| <= (D + 2) u ref                                     per term one subtraction (exact operands) and one product, D - 1 additions of
                                                                                non-negative terms: relative to the sum itself
    objective  |got - fsum(dist_got)| <= M u sum(dist_got)                      the objective is by contract the sum of the dist the SAME call wrote, so the bound
                                                                                counts the M - 1 additions only (at M = 1 it is the element itself)
    counts     exact

``defect`` plants what a wrong kernel could do, for the CPU test that shows the bounds see it: ``"fp32"`` (the cluster sum accumulated in fp32),
``"drop_last"`` (the last row of every cluster left out of its sum, the count kept), ``"boundary"`` (every cluster's segment of the grouped rows starts and ends one
position late).  Shared by tests/test_asmk_train_host.py and tests/test_asmk_train_gpu.py.
"""
import math

import numpy as np

U64, U32 = 2.0 ** -53, 2.0 ** -24
DEFECTS = ("fp32", "drop_last", "boundary")


def _colsum(rows):
    """the exactly rounded column sums of a [n, D] float64 block (math.fsum): the reference's own sum carries one rounding"""
    return np.array([math.fsum(col) for col in rows.T]) if rows.shape[0] else np.zeros((rows.shape[1],))


def update(feat, centroids, ids, defect=None):
    """-> dict(new [K, D] float64 (before the fp32 rounding), counts int64 [K], dist [M], objective, new_bound [K, D], dist_bound [M])"""
    x, c, ids = np.asarray(feat, dtype=np.float64), np.asarray(centroids, dtype=np.float64), np.asarray(ids, dtype=np.int64)
    (M, D), K = x.shape, c.shape[0]
    assert ids.shape == (M,) and ids.min() >= 0 and ids.max() < K
    order = np.argsort(ids, kind="stable")
    counts = np.bincount(ids, minlength=K)
    start = np.concatenate([[0], np.cumsum(counts)])
    new, clean, scale = c.copy(), c.copy(), np.zeros((K, D))
    for k in range(K):
        n = int(counts[k])
        if n == 0:
            continue
        lo, hi = int(start[k]), int(start[k + 1])
        if defect == "boundary":
            lo, hi = min(lo + 1, M), min(hi + 1, M)
        rows = order[lo:hi]
        if defect == "drop_last":
            rows = rows[:-1]
        if defect == "fp32":
            acc = np.zeros((D,), dtype=np.float32)
            for r in rows:
                acc = acc + np.asarray(feat, dtype=np.float32)[r]
            tot = acc.astype(np.float64)
        else:
            tot = _colsum(x[rows])
        seg = x[order[int(start[k]):int(start[k + 1])]]
        new[k], clean[k], scale[k] = tot / n, _colsum(seg) / n, np.abs(seg).sum(axis=0)
    dist = ((x - c[ids]) ** 2).sum(axis=1)
    n_c = np.maximum(counts, 1)[:, None]
    new_bound = np.where(counts[:, None] > 0, U32 * np.abs(clean) + (n_c + 1) * U64 * scale / n_c, 0.0)
    return dict(new=new, counts=counts, dist=dist, objective=math.fsum(dist), new_bound=new_bound, dist_bound=(D + 2) * U64 * dist)


def objective_check(dist_got, objective_got):
    """(error, bound) of the objective against the exact sum of the dist the same call wrote"""
    d = np.asarray(dist_got, dtype=np.float64)
    tot = math.fsum(d)
    return abs(float(objective_got) - tot), d.shape[0] * U64 * tot


def reseed(counts, dist):
    """the empty-cluster rule of must3r_amd.asmk_train.reseed_empty -> (empty ids ascending, donor rows): the r-th empty cluster takes the row of r-th largest dist,
    ties to the lower row index"""
    empty = np.nonzero(np.asarray(counts) == 0)[0]
    d = np.asarray(dist, dtype=np.float64)
    donors = sorted(range(d.shape[0]), key=lambda j: (-d[j], j))[:len(empty)]
    return empty, np.asarray(donors, dtype=np.int64)
