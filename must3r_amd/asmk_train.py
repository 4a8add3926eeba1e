"""Training the ASMK codebook on the GPU: Lloyd's k-means over the retrieval front-end's local features (asmk's ``train_codebook`` behind
processor.py:83-96, which runs faiss-gpu; there is no such thing on ROCm).

One iteration is three native calls: ``asmk.centroid_sqnorm`` and ``asmk.quantize(feat, C, 1)`` (the exact fp32-MFMA nearest-centroid search of the
retrieval mode, ties to the lower id), then ``kmeans_update`` (``must3r_hip_kmeans_update``, csrc/asmk_train.hip): exact counts, the centroid of every
cluster as the fp32 rounding of an fp64 sum taken sequentially in ascending row index, the fp64 distance of every row to its old centroid and the objective.
No floating-point atomics: the update is repeatable bit for bit, and a cluster's centroid depends on its own rows alone.  Grouping the rows by cluster is
``torch.sort(ids, stable=True)`` (plumbing).

PARITY UNPINNED upstream (asmk and faiss are not vendored by the reference): the rule for empty clusters lives in one named place,
``reseed_empty``; it is NOT faiss's split of the largest cluster.  The initial centroids (a seeded ``torch.randperm`` of the rows) are this module's own too.

``python -m must3r_amd.asmk_train --weights CKPT --retrieval CKPT --images DIR_OR_LIST --nclusters 64k --niter 20 [--out PATH]`` extracts the local
features of the images with the front-end of the retrieval checkpoint and writes the codebook ``Retriever`` loads.
"""
import argparse
import ctypes as C
import os
import pickle

import numpy as np
import torch

from . import _lib, asmk

EMPTY_RULE = "r-th empty cluster (ascending id) <- the row of r-th largest dist (ties: lower row index)"


def _f32(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"must3r_amd.asmk_train: {what} must be a CUDA tensor; the HIP path has no CPU fallback")
    if x.dim() != 2:
        raise ValueError(f"{what} must be a matrix, got {tuple(x.shape)}")
    return x.float().contiguous()


def kmeans_update(feat, centroids, ids, with_record=False):
    """(new_centroids fp32 [K, D], counts int32 [K], dist fp64 [M], objective fp64 [1]) of one assignment ``ids`` (int32 [M], or [M, k]: its first column,
    read in place through the row stride) against ``centroids``; include/must3r_hip.h has the contract.  The call reads one small record back (that is how an
    id outside [0, K) is refused): ``with_record`` appends it as ``(objective, number of empty clusters)`` host numbers."""
    x, c = _f32(feat, "feat"), _f32(centroids, "centroids")
    (M, D), K = x.shape, c.shape[0]
    if c.shape[1] != D:
        raise ValueError(f"feature dim {D} != centroid dim {c.shape[1]}")
    if not isinstance(ids, torch.Tensor) or not ids.is_cuda or ids.dtype != torch.int32 or ids.dim() not in (1, 2) or ids.shape[0] != M:
        raise ValueError(f"ids must be a CUDA int32 tensor [{M}] or [{M}, k]")
    col = ids if ids.dim() == 1 else ids[:, 0]
    if M and col.stride(0) < 1:
        col = col.contiguous()
    order = torch.sort(col, stable=True).indices   # int64: rows grouped by cluster, ascending row index inside a cluster
    new = torch.empty_like(c)
    counts = torch.empty((K,), dtype=torch.int32, device=x.device)
    dist = torch.empty((M,), dtype=torch.float64, device=x.device)
    objective = torch.empty((1,), dtype=torch.float64, device=x.device)
    rec = (C.c_double * 2)()
    lib = _lib.load()
    with torch.cuda.device(x.device):
        nbytes = lib.must3r_hip_kmeans_update_scratch_bytes(M, K)
        scratch = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=x.device)
        _lib.check(lib.must3r_hip_kmeans_update(x.data_ptr(), M, D, c.data_ptr(), K, col.data_ptr(), col.stride(0) if M > 1 else 1, order.data_ptr(),
                                                new.data_ptr(), counts.data_ptr(), dist.data_ptr(), objective.data_ptr(), rec, _lib.stream_ptr(x.device),
                                                scratch.data_ptr(), nbytes))
    out = (new, counts, dist, objective)
    return out + ((float(rec[0]), int(rec[1])),) if with_record else out


def reseed_empty(new_centroids, counts, dist, feat):
    """The empty-cluster rule (``EMPTY_RULE``; PARITY UNPINNED, module docstring), in place on ``new_centroids``: the r-th empty cluster, in ascending id,
    takes the row with the r-th largest ``dist``, ties to the lower row index.  The donor row stays in its old cluster's mean for this iteration.  Returns the
    (empty ids, donor rows) it used."""
    empty = torch.nonzero(counts == 0).flatten()
    donors = torch.sort(dist, descending=True, stable=True).indices[:empty.numel()]
    new_centroids[empty] = feat[donors]
    return empty, donors


def train_codebook(feat, K, niter=20, seed=0, init=None, verbose=False):
    """Lloyd's k-means -> (centroids fp32 [K, D] on the device, log).  ``K``: an int or asmk's size string (``'64k'``).  ``log[i]`` = dict(objective, empty) of
    iteration i's assignment (the objective against the centroids the iteration started from).  One host read per iteration: the update's record."""
    K = asmk.parse_nclusters(K)
    if not isinstance(feat, torch.Tensor) or feat.dim() != 2:
        raise ValueError("train_codebook: feat must be a [M, D] tensor")
    M, D = feat.shape
    if K < 1 or M < K:
        raise ValueError(f"train_codebook: {M} feature rows cannot seed {K} clusters")
    if D % 64:
        raise ValueError(f"train_codebook: the feature dim must be a multiple of 64 (the quantizer's condition), got {D}")
    x = _f32(feat, "feat")
    if init is None:
        perm = torch.randperm(M, generator=torch.Generator().manual_seed(int(seed)))[:K]
        cent = x[perm.to(x.device)].clone()
    else:
        cent = _f32(init, "init").clone()
        if tuple(cent.shape) != (K, D):
            raise ValueError(f"init must be [{K}, {D}], got {tuple(cent.shape)}")
    log = []
    for it in range(int(niter)):
        csq = asmk.centroid_sqnorm(cent, refresh=True)
        ids = asmk.quantize(x, cent, 1, c_sqnorm=csq)
        new, counts, dist, _, (objective, n_empty) = kmeans_update(x, cent, ids, with_record=True)
        if n_empty:
            reseed_empty(new, counts, dist, x)
        log.append(dict(objective=objective, empty=n_empty))
        if verbose:
            print(f"k-means iteration {it}: objective {objective:.9g}, {n_empty} empty clusters")
        cent = new
    return cent, log


def write_codebook(path, centroids):
    """``{"centroids": float32 [K, D]}`` as a pickle that names nothing outside ``asmk._PICKLE_GLOBALS`` (so ``asmk.read_codebook`` returns the same bits);
    a path ending ``.npy`` writes that array as ``.npy``."""
    path = os.fspath(path)
    c = centroids.detach().cpu().numpy() if isinstance(centroids, torch.Tensor) else np.asarray(centroids)
    c = np.ascontiguousarray(c, dtype=np.float32)
    if c.ndim != 2:
        raise ValueError(f"centroids must be [K, D], got {c.shape}")
    if path.lower().endswith(".npy"):
        with open(path, "wb") as f:
            np.save(f, c, allow_pickle=False)
        return path
    with open(path, "wb") as f:
        pickle.dump({"centroids": c}, f, protocol=2)   # protocol 2: every global is named in a GLOBAL opcode
    return path


def image_list(images):
    """a folder (its files, sorted), a text file naming one image per line, or a list of paths"""
    if isinstance(images, (list, tuple)):
        return [os.fspath(p) for p in images]
    if os.path.isdir(images):
        return [os.path.join(images, n) for n in sorted(os.listdir(images)) if os.path.isfile(os.path.join(images, n))]
    with open(images) as f:
        return [ln.strip() for ln in f if ln.strip()]


@torch.no_grad()
def local_features(encoder, frontend, files, image_size=512, device="cuda", max_bs=None, verbose=False):
    """The rows ``train_codebook`` clusters: ``forward_local`` of the encoder tokens of every image, as ``MUSt3R_Retriever`` forms them."""
    from .image import load_images
    from .inference import encoder_multi_ar
    from .retrieval import frontend_local_features
    views = load_images(files, size=image_size, patch_size=encoder.patch_size, verbose=verbose, device=device)
    true_shape = torch.stack([torch.from_numpy(b["true_shape"]) for b in views], dim=0)
    x, _ = encoder_multi_ar(encoder, [b["img"] for b in views], true_shape, verbose=verbose, max_bs=max_bs, device=device)
    feat, _ = frontend_local_features(frontend, [xi.unsqueeze(0).float() for xi in x], device)
    return feat


def main(argv=None):
    from .model import load_model
    from .retrieval import codebook_path, load_frontend
    ap = argparse.ArgumentParser(prog="python -m must3r_amd.asmk_train", description="train the ASMK codebook of a retrieval checkpoint on the GPU")
    ap.add_argument("--weights", required=True, help="MUSt3R checkpoint (its encoder produces the tokens)")
    ap.add_argument("--retrieval", required=True, help="retrieval checkpoint (whitening + projector of the front-end)")
    ap.add_argument("--images", required=True, help="a folder of images, or a text file with one path per line")
    ap.add_argument("--nclusters", default="64k")
    ap.add_argument("--niter", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--image_size", type=int, default=512)
    ap.add_argument("--max_bs", type=int, default=0)
    ap.add_argument("--out", default=None, help="default: the codebook path next to --retrieval")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    encoder, _ = load_model(a.weights, device=a.device, verbose=False)
    model, _ = load_frontend(a.retrieval, encoder, a.device)
    feat = local_features(encoder, model, image_list(a.images), image_size=a.image_size, device=a.device, max_bs=a.max_bs or None)
    print(f"{feat.shape[0]} local features of dim {feat.shape[1]}")
    cent, _ = train_codebook(feat, a.nclusters, niter=a.niter, seed=a.seed, verbose=True)
    out = write_codebook(a.out or codebook_path(a.retrieval), cent)
    print(f"wrote {out}")
    return out


if __name__ == "__main__":
    main()
