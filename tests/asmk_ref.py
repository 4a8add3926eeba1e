"""ASMK restatement for the tests, written from the spec in must3r_amd/asmk.py and include/must3r_hip.h (ABI 11): binary kernel, no
idf, multiple assignment 1 (database) / 5 (query).  Distances in float64; residual sums sequential in fp32 (each difference rounded,
then added, rows ascending); sigma in fp32; scores accumulated in float64 in ascending word order."""
import numpy as np


def sq_dist(feat, centroids):
    """float64 squared L2 distances [M, K]"""
    x = np.asarray(feat, dtype=np.float64)
    c = np.asarray(centroids, dtype=np.float64)
    return (x * x).sum(1)[:, None] - 2.0 * x @ c.T + (c * c).sum(1)[None, :]


def topk(feat, centroids, k):
    """(ids int64 [M, k] ascending by fp64 distance, ties to the lower id; the distances [M, K])"""
    d = sq_dist(feat, centroids)
    return np.argsort(d, axis=1, kind="stable")[:, :k], d


def aggregate(feat, centroids, ids, offsets, k_use):
    """per image: (ascending words int64 [n_w], bits bool [n_w, D])"""
    feat = np.asarray(feat, dtype=np.float32)
    centroids = np.asarray(centroids, dtype=np.float32)
    ids = np.asarray(ids)[:, :k_use]
    out = []
    for i in range(len(offsets) - 1):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        sub = ids[lo:hi]
        words = np.unique(sub)
        bits = np.zeros((len(words), feat.shape[1]), dtype=bool)
        for a, w in enumerate(words):
            r = np.zeros(feat.shape[1], dtype=np.float32)
            for j in range(hi - lo):
                if np.any(sub[j] == w):
                    r = r + (feat[lo + j] - centroids[w])
            bits[a] = r > 0
        out.append((words, bits))
    return out


def pack_bits(bits):
    """bool [n, D] -> uint32 [n, D / 32], bit d % 32 of word d / 32"""
    b = np.asarray(bits, dtype=np.uint64).reshape(bits.shape[0], -1, 32)
    return (b << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def unpack_bits(words32, D):
    w = np.asarray(words32).astype(np.uint32).reshape(-1, D // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1, D)


def sigma(h, D, alpha, tau):
    s = np.float32(1.0) - np.float32(2.0 * h) / np.float32(D)
    return np.power(s, np.float32(alpha), dtype=np.float32) if s >= tau else np.float32(0.0)


def scores(query, database, D, alpha=3.0, tau=0.0, normalize=True):
    """float64 [n_q, n_d] from per-image (words, bits) lists"""
    out = np.zeros((len(query), len(database)), dtype=np.float64)
    for q, (wq, bq) in enumerate(query):
        pos_q = {int(w): a for a, w in enumerate(wq)}
        for d, (wd, bd) in enumerate(database):
            total = 0.0
            for b, w in enumerate(wd):
                a = pos_q.get(int(w))
                if a is None:
                    continue
                h = int(np.count_nonzero(bq[a] != bd[b]))
                total += float(sigma(h, D, alpha, tau))
            if normalize:
                total = (total / np.sqrt(len(wd)) / np.sqrt(len(wq))) if len(wd) and len(wq) else 0.0
            out[q, d] = total
    return out


def asmk_scores(feat, centroids, offsets, alpha=3.0, tau=0.0, normalize=True, ids=None):
    """the whole back-end: query side k = 5, database side k = 1 (both from one top-5 search)"""
    if ids is None:
        ids, _ = topk(feat, centroids, 5)
    db = aggregate(feat, centroids, ids, offsets, 1)
    q = aggregate(feat, centroids, ids, offsets, 5)
    return scores(q, db, np.asarray(feat).shape[1], alpha, tau, normalize)
