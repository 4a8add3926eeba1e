"""ASMK back-end of the retrieval mode: the scores ``MUSt3R_Retriever`` gets from asmk (demo/inference.py:48-60), on the GPU.

The reference builds an ``asmk_method.ASMKMethod`` with processor.py:88-94's parameters -- binary kernel, no idf, multiple
assignment 1 for the database and 5 for the query, ``similarity_threshold=0.0``, ``alpha=3.0``, ``topk=None`` -- and queries the
image set against itself.  Here that is three native calls (include/must3r_hip.h, ABI 11; csrc/asmk.hip):

* ``must3r_hip_asmk_quantize``: the 5 nearest centroids of every local feature (one search serves both sides: its first column
  is the database assignment), fp32 MFMA distances, exact ties to the lower centroid id;
* ``must3r_hip_asmk_aggregate`` (once per side): per image, the ascending distinct words and the sign bits of their residual sums;
* ``must3r_hip_asmk_scores``: sum over shared words of sigma(1 - 2 popcount(xor) / D), float64 [query, database].

PARITY UNPINNED upstream (asmk is not vendored by the reference): each of these lives in one named place --
the ``1/sqrt(|W|)`` normalisation (``ASMK(normalize=True)``), the tie order (``TIE_ORDER``, csrc/asmk.hip ``rank_before``) and the
codebook pickle's layout (``read_codebook``).
"""
import io
import os
import pickle

import numpy as np
import torch

from . import _lib

TIE_ORDER = "lower centroid id first"   # exact distance ties in the quantizer (csrc/asmk.hip rank_before)
DB_ASSIGNMENT, QUERY_ASSIGNMENT = 1, 5   # processor.py:91,93 multiple_assignment
MAX_PAIRS_PER_IMAGE = 4096               # (word, row) pairs one image's LDS sort holds: rows * QUERY_ASSIGNMENT <= 4096

# the only globals a codebook pickle may name: builtin containers and scalars, numpy's array and dtype reconstruction
_PICKLE_GLOBALS = {
    ("builtins", n) for n in ("dict", "list", "tuple", "set", "frozenset", "int", "float", "complex", "str", "bytes", "bytearray", "bool")
} | {
    (m, n) for m in ("numpy.core.multiarray", "numpy._core.multiarray") for n in ("_reconstruct", "scalar")
} | {("numpy", "ndarray"), ("numpy", "dtype"), ("_codecs", "encode")}


class CodebookRefused(pickle.UnpicklingError):
    """a codebook pickle that names a global outside ``_PICKLE_GLOBALS``; nothing of it ran"""


class _CodebookUnpickler(pickle.Unpickler):
    def __init__(self, f, path):
        super().__init__(f)
        self._path = path

    def find_class(self, module, name):
        if (module, name) not in _PICKLE_GLOBALS:
            raise CodebookRefused(f"{self._path}: the codebook pickle names {module}.{name}; only builtin containers and numpy "
                                         "arrays are accepted")
        return super().find_class(module, name)


def _float_matrices(obj, out):
    """every 2-D floating array in ``obj`` (dicts, lists, tuples), depth first"""
    if isinstance(obj, torch.Tensor):
        obj = obj.detach().cpu().numpy()
    if isinstance(obj, np.ndarray):
        if obj.ndim == 2 and np.issubdtype(obj.dtype, np.floating):
            out.append(obj)
    elif isinstance(obj, dict):
        for v in obj.values():
            _float_matrices(v, out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _float_matrices(v, out)
    return out


def _centroids_of(obj, path):
    if isinstance(obj, dict) and "centroids" in obj:
        found = _float_matrices(obj["centroids"], [])
        if len(found) == 1:
            return found[0]
    found = _float_matrices(obj, [])
    if len(found) != 1:
        raise ValueError(f"{path}: expected exactly one 2-D floating array (the centroids), found {len(found)}")
    return found[0]


def parse_nclusters(n):
    """ckpt_args.nclusters -> int: ``65536``, ``'65536'`` or ``'64k'`` (asmk's size string)"""
    if isinstance(n, str):
        s = n.strip().lower()
        return int(s[:-1]) * 1024 if s.endswith("k") else int(s)
    return int(n)


def read_codebook(path, nclusters=None):
    """The ASMK codebook next to a retrieval checkpoint (processor.py:83-96 ``train_codebook(None, cache_path=...)``) as a host numpy
    ``[K, D]`` array.  Accepted layouts (PARITY UNPINNED: asmk's own pickle layout is not vendored upstream): a pickle, read by an
    unpickler that resolves nothing but builtin containers and numpy arrays, holding one 2-D floating array, under a ``centroids``
    key if it has one; a ``.npy`` file; a ``.pt`` tensor or dict of tensors (``weights_only``).  Anything else is refused with the
    file's name.  ``nclusters`` (checkpoint ``args.nclusters``, e.g. ``'64k'``) is checked against K."""
    path = os.fspath(path)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"ASMK codebook not found: {path}")
    ext = os.path.splitext(path)[1].lower()
    try:
        if ext == ".npy":
            obj = np.load(path, allow_pickle=False)
        elif ext in (".pt", ".pth"):
            obj = torch.load(path, map_location="cpu", weights_only=True)
        else:
            with open(path, "rb") as f:
                obj = _CodebookUnpickler(io.BytesIO(f.read()), path).load()
    except CodebookRefused:
        raise
    except Exception as e:
        raise ValueError(f"{path}: not a readable codebook ({type(e).__name__}: {e})") from None
    c = _centroids_of(obj, path)
    if nclusters is not None and parse_nclusters(nclusters) != c.shape[0]:
        raise ValueError(f"{path}: the codebook has {c.shape[0]} centroids, the checkpoint asks for {nclusters}")
    return c


def load_codebook(path, nclusters=None, device="cuda"):
    """``read_codebook`` as a CUDA fp32 ``[K, D]`` tensor whose squared norms are computed once (``centroid_sqnorm``)."""
    c = read_codebook(path, nclusters)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("must3r_amd.asmk.load_codebook: device must be CUDA; the HIP path has no CPU fallback")
    t = torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).to(device)
    centroid_sqnorm(t)
    return t


def _cuda_f32(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"must3r_amd.asmk: {what} must be a CUDA tensor; the HIP path has no CPU fallback")
    return x.float().contiguous()


def centroid_sqnorm(codebook, refresh=False):
    """|c|^2 of every centroid (``must3r_hip_asmk_centroid_sqnorm``), cached on the codebook tensor together with its version counter: an
    in-place update of the tensor (``copy_``, ``[...] =``, a reload into it) is seen and the norms are recomputed.  Writes through ``.data``
    bypass the version counter (as they do for autograd): pass ``refresh=True`` after them."""
    cached = getattr(codebook, "_asmk_sqnorm", None)
    if cached is not None and not refresh and cached[0] == codebook._version:
        return cached[1]
    c = _cuda_f32(codebook, "codebook")
    K, D = c.shape
    out = torch.empty((K,), dtype=torch.float32, device=c.device)
    with torch.cuda.device(c.device):
        _lib.check(_lib.load().must3r_hip_asmk_centroid_sqnorm(c.data_ptr(), K, D, out.data_ptr(), _lib.stream_ptr(c.device)))
    codebook._asmk_sqnorm = (codebook._version, out)
    return out


def quantize(feat, codebook, k, c_sqnorm=None):
    """ids int32 [M, k]: the k nearest centroids of each row of ``feat`` [M, D], ascending by squared L2 (ties: ``TIE_ORDER``)."""
    x, c = _cuda_f32(feat, "feat"), _cuda_f32(codebook, "codebook")
    M, D = x.shape
    K = c.shape[0]
    if c.shape[1] != D:
        raise ValueError(f"feature dim {D} != codebook dim {c.shape[1]}")
    csq = centroid_sqnorm(codebook) if c_sqnorm is None else c_sqnorm
    ids = torch.empty((M, k), dtype=torch.int32, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        nbytes = lib.must3r_hip_asmk_quantize_scratch_bytes(M, K, k)
        scratch = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=x.device)
        _lib.check(lib.must3r_hip_asmk_quantize(x.data_ptr(), M, c.data_ptr(), csq.data_ptr(), K, D, k, ids.data_ptr(), scratch.data_ptr(),
                                                nbytes, _lib.stream_ptr(x.device)))
    return ids


def _offsets(offsets, M):
    off = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64).reshape(-1)
    if off.size < 1 or off[0] != 0 or off[-1] != M or np.any(np.diff(off) < 0):
        raise ValueError(f"offsets must rise from 0 to the number of feature rows {M}, got {off.tolist()[:8]}...")
    return off


def aggregate(feat, codebook, ids, offsets, k_use):
    """Per image and side: (words int32 [M * k_use], bits int32 [M * k_use, D / 32] (uint32 bit patterns), counts int32 [n]); image i's
    ascending words and their residual sign bits start at slot ``offsets[i] * k_use``."""
    x, c = _cuda_f32(feat, "feat"), _cuda_f32(codebook, "codebook")
    M, D = x.shape
    off = _offsets(offsets, M)
    n = off.size - 1
    rows = int(np.diff(off).max()) if n else 0
    if rows * k_use > MAX_PAIRS_PER_IMAGE:
        raise ValueError(f"an image has {rows} local features; with multiple assignment {k_use} that is more than the "
                         f"{MAX_PAIRS_PER_IMAGE} (word, row) pairs the per-image sort holds (the reference uses nfeat = 300)")
    if not isinstance(ids, torch.Tensor) or ids.dim() != 2 or ids.shape[0] != M or not 1 <= k_use <= ids.shape[1]:
        raise ValueError(f"ids must be a [{M}, k >= {k_use}] tensor of centroid ids (one row per feature), got "
                         f"{tuple(ids.shape) if isinstance(ids, torch.Tensor) else type(ids).__name__}")
    if ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"ids must be an integer tensor, got {ids.dtype}")
    ids = ids.to(device=x.device, dtype=torch.int32).contiguous()
    K = c.shape[0]
    words = torch.empty((M * k_use,), dtype=torch.int32, device=x.device)
    bits = torch.empty((M * k_use, D // 32), dtype=torch.int32, device=x.device)
    counts = torch.empty((n,), dtype=torch.int32, device=x.device)
    off_dev = torch.from_numpy(off.astype(np.int32)).to(x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().must3r_hip_asmk_aggregate(x.data_ptr(), c.data_ptr(), K, D, ids.data_ptr(), ids.shape[1], k_use,
                                                         off_dev.data_ptr(), n, rows, words.data_ptr(), bits.data_ptr(), counts.data_ptr(),
                                                         _lib.stream_ptr(x.device)))
    bad = torch.nonzero(counts < 0).flatten()
    if bad.numel():   # the kernel refused these images before reading any centroid row through their ids
        raise ValueError(f"aggregate: images {bad.tolist()[:8]} have centroid ids outside [0, {K})")
    return words, bits, counts


def scores_from_aggregates(query, database, offsets, k_query, k_db, D, alpha=3.0, similarity_threshold=0.0, normalize=True):
    """float64 [n, n] (row = query image, column = database image) from two ``aggregate`` results over the same images."""
    (wq, bq, cq), (wd, bd, cd) = query, database
    n = cq.shape[0]
    dev = wq.device
    off_dev = torch.as_tensor(np.asarray(offsets, dtype=np.int32), device=dev)
    out = torch.empty((n, n), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().must3r_hip_asmk_scores(wq.data_ptr(), bq.data_ptr(), cq.data_ptr(), off_dev.data_ptr(), k_query, n,
                                                      wd.data_ptr(), bd.data_ptr(), cd.data_ptr(), off_dev.data_ptr(), k_db, n, D,
                                                      float(alpha), float(similarity_threshold), 1 if normalize else 0, out.data_ptr(),
                                                      _lib.stream_ptr(dev)))
    return out


class ASMK:
    """asmk_method.ASMKMethod as MUSt3R_Retriever uses it (processor.py:88-96, demo/inference.py:54-58), binary kernel without idf.
    ``normalize``: divide each score by sqrt(|W_d|) sqrt(|W_q|) (PARITY UNPINNED upstream; module docstring)."""

    def __init__(self, codebook, alpha=3.0, similarity_threshold=0.0, normalize=True, binary=True, use_idf=False,
                 multiple_assignment=(DB_ASSIGNMENT, QUERY_ASSIGNMENT)):
        if not binary or use_idf or tuple(multiple_assignment) != (DB_ASSIGNMENT, QUERY_ASSIGNMENT):
            raise NotImplementedError("must3r_amd.asmk offers the binary kernel without idf, multiple assignment (1, 5), as the "
                                      "reference's retriever configures it (processor.py:88-94)")
        self.codebook = codebook if isinstance(codebook, torch.Tensor) else load_codebook(codebook)
        if self.codebook.dim() != 2 or self.codebook.shape[1] % 64:
            raise ValueError(f"codebook must be [K, D] with D a multiple of 64, got {tuple(self.codebook.shape)}")
        centroid_sqnorm(self.codebook)
        self.alpha, self.similarity_threshold, self.normalize = float(alpha), float(similarity_threshold), bool(normalize)

    def scores(self, feat, offsets):
        """feat [M, D] (CUDA) with image i on rows [offsets[i], offsets[i+1]) -> device float64 [n, n], row = query, column = database."""
        x = _cuda_f32(feat, "feat")
        off = _offsets(offsets, x.shape[0])
        n = off.size - 1
        if x.shape[0] == 0:
            return torch.zeros((n, n), dtype=torch.float64, device=x.device)
        ids = quantize(x, self.codebook, QUERY_ASSIGNMENT)
        db = aggregate(x, self.codebook, ids, off, DB_ASSIGNMENT)
        q = aggregate(x, self.codebook, ids, off, QUERY_ASSIGNMENT)
        return scores_from_aggregates(q, db, off, QUERY_ASSIGNMENT, DB_ASSIGNMENT, x.shape[1], self.alpha, self.similarity_threshold,
                                      self.normalize)

    def scores_numpy(self, feat, offsets):
        return self.scores(feat, offsets).cpu().numpy()
