"""Retrieval front-end on the encoder tokens -- drop-in for the model part of must3r/retrieval/model.py (:59-183).

``Whitener`` and ``RetrievalModel`` keep the reference's constructor arguments, attribute names and state-dict keys
(``prewhiten.m/p`` and ``postwhiten.m/p`` in float64, ``projector.{i}.weight/bias``), so ``load_state_dict`` of a
reference retrieval checkpoint works unchanged; ``forward_local`` / ``forward_global`` take the encoder tokens
``x [B,N,C]`` (cuda fp32) like the reference's (demo/inference.py:40).  Every stage is a native call: float64 centre +
PCA projection (``must3r_hip_affine``, fp64 MFMA; ``Whitener(l2norm=dim)`` -> ``must3r_hip_l2_normalize``), the projector Linears (fp32
MFMA, exact products; hidden layers of a multi-layer projector: ``must3r_hip_layernorm_act_f32``), token attention
(``must3r_hip_row_norm``), top-k selection + gather (``must3r_hip_topk_gather``) or weighted sum pooling
(``must3r_hip_weighted_spoc``).  No CPU fallback.

``Retriever`` / ``MUSt3R_Retriever`` (processor.py:62-96, demo/inference.py:31-60) add the back-end: the checkpoint's front-end, the
ASMK codebook next to it and ``must3r_amd.asmk.ASMK`` (quantize, aggregate and score on the GPU, ABI 11), so the encoder tokens
become the reference's N x N score matrix without leaving the device.

The two learnt artefacts next to the encoder are made here too, so that a model trained with this package can be served in the retrieval mode.  The PCA
whitening (``pcawhitenlearn_shrinkage``, retrieval/model.py:18-35): ``WhiteningStats`` accumulates the shifted second moments of the features on the device
(``must3r_hip_cov_accumulate``: fp64 MFMA, exactly symmetric, no atomics), ``finish`` / ``learn_whitening`` / ``Whitener.learn_`` take the one D x D matrix to
the host for ``numpy.linalg.eigh``.  The ASMK codebook (k-means) is ``must3r_amd.asmk_train``.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib


def _tokens(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"must3r_amd.retrieval: {what} must be a CUDA tensor; the HIP path has no CPU fallback")
    return x.float().contiguous()


def affine(x, sub, B, b_transposed, bias=None, resid=None, double=False):
    """out = (x - sub) @ B (+ bias) (+ resid) over the last dimension, fp32 in / out; float64 inside when ``double``."""
    x = _tokens(x, "x")
    K = x.shape[-1]
    N = B.shape[0] if b_transposed else B.shape[1]
    M = x.numel() // K
    td = torch.float64 if double else torch.float32
    dev = x.device
    subd = None if sub is None else sub.detach().to(device=dev, dtype=td).reshape(-1).contiguous()
    Bd = B.detach().to(device=dev, dtype=td).contiguous()
    biasd = None if bias is None else bias.detach().to(device=dev, dtype=td).contiguous()
    residd = None if resid is None else _tokens(resid, "resid")
    out = torch.empty((*x.shape[:-1], N), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().must3r_hip_affine(1 if double else 0, x.data_ptr(), None if subd is None else subd.data_ptr(), Bd.data_ptr(),
                                                 1 if b_transposed else 0, None if biasd is None else biasd.data_ptr(),
                                                 None if residd is None else residd.data_ptr(), out.data_ptr(), M, N, K, _lib.stream_ptr(x.device)))
    return out


class Whitener(nn.Module):
    """retrieval/model.py:59-79."""

    def __init__(self, dim, l2norm=None):
        super().__init__()
        self.m = nn.Parameter(torch.zeros((1, dim)).double())
        self.p = nn.Parameter(torch.eye(dim, dim).double())
        self.l2norm = l2norm

    @torch.no_grad()
    def forward(self, x):
        out = affine(x, self.m, self.p, b_transposed=False, double=True).view(x.shape)
        if self.l2norm is not None:
            out = l2_normalize(out, self.l2norm)   # the reference normalises the float64 product (:77-78); here its fp32 rounding
        return out.to(x.dtype)

    @torch.no_grad()
    def learn_(self, x_or_stats, s=1.0):
        """Write the whitening learnt from features ``x`` [..., dim] (or from a ``WhiteningStats`` fed in chunks) into ``m`` and ``p``, in place."""
        m, P = x_or_stats.finish(s) if isinstance(x_or_stats, WhiteningStats) else learn_whitening(x_or_stats, s)
        if tuple(P.shape) != tuple(self.p.shape):
            raise ValueError(f"the statistics are of dim {P.shape[0]}, the whitener of dim {self.p.shape[0]}")
        self.m.copy_(torch.from_numpy(m).to(self.m.device))
        self.p.copy_(torch.from_numpy(P).to(self.p.device))
        return self


class WhiteningStats:
    """Running fp64 statistics of features for ``pcawhitenlearn_shrinkage`` (retrieval/model.py:18-35), on the device: with the shift fixed at the first
    chunk (its fp64 column mean) and u = double(x) - shift, ``S = sum u u^T``, ``s = sum u``, ``n`` = rows (``must3r_hip_cov_accumulate``).  Chunks of any size;
    the state after different chunkings agrees to rounding, not bit for bit (the sums associate differently)."""

    def __init__(self, dim, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("must3r_amd.retrieval.WhiteningStats: device must be CUDA; the HIP path has no CPU fallback")
        if dim < 1 or dim % 16:
            raise ValueError(f"WhiteningStats: dim must be a positive multiple of 16, got {dim}")
        self.dim, self.device = int(dim), device
        self.S = torch.zeros((dim, dim), dtype=torch.float64, device=device)
        self.s = torch.zeros((dim,), dtype=torch.float64, device=device)
        self.n = torch.zeros((1,), dtype=torch.float64, device=device)
        self.shift = None

    @torch.no_grad()
    def add(self, x):
        x = _tokens(x, "x")
        if x.shape[-1] != self.dim:
            raise ValueError(f"WhiteningStats of dim {self.dim} fed rows of {x.shape[-1]}")
        x = x.reshape(-1, self.dim)
        M = x.shape[0]
        if M == 0:
            return self
        if self.shift is None:
            self.shift = (x.sum(dim=0, dtype=torch.float64) / M).contiguous()
        lib = _lib.load()
        with torch.cuda.device(x.device):
            nbytes = lib.must3r_hip_cov_accumulate_scratch_bytes(M, self.dim)
            scratch = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=x.device)
            _lib.check(lib.must3r_hip_cov_accumulate(x.data_ptr(), M, self.dim, self.shift.data_ptr(), self.S.data_ptr(), self.s.data_ptr(), self.n.data_ptr(),
                                                     _lib.stream_ptr(x.device), scratch.data_ptr(), nbytes))
        return self

    def finish(self, s=1.0):
        """-> (m [1, dim], P [dim, dim]) float64 numpy, the return value of ``pcawhitenlearn_shrinkage(X, s)``"""
        if self.shift is None:
            raise ValueError("WhiteningStats.finish: no rows were added")
        return whitening_from_stats(self.S.cpu().numpy(), self.s.cpu().numpy(), float(self.n.item()), self.shift.cpu().numpy(), s)


def whitening_from_stats(S, s_sum, n, shift, s=1.0):
    """The host part of the whitening: d = s_sum / n, m = shift + d, Xcov = S / n - d d^T, then retrieval/model.py:27-35 with ``numpy.linalg.eigh`` on the
    symmetric matrix (``eig`` there; on a symmetric matrix the same decomposition up to the sign of each eigenvector, with orthogonality guaranteed)."""
    d = s_sum / n
    m = (shift + d)[None, :]
    Xcov = S / n - np.outer(d, d)
    eigval, eigvec = np.linalg.eigh(Xcov)
    order = eigval.argsort()[::-1]
    eigval = eigval[order]
    eigvec = eigvec[:, order]
    eigval = np.clip(eigval, a_min=1e-14, a_max=None)
    P = np.dot(np.linalg.inv(np.diag(np.power(eigval, 0.5 * s))), eigvec.T)
    return m, P.T


def learn_whitening(x, s=1.0):
    """``pcawhitenlearn_shrinkage(x, s)`` of CUDA fp32 features ``x`` [..., dim] in one call -> (m, P) float64 numpy."""
    x = _tokens(x, "x")
    return WhiteningStats(x.shape[-1], x.device).add(x).finish(s)


def l2_normalize(x, dim):
    """F.normalize(x, dim=dim) (eps 1e-12), in place on a contiguous fp32 tensor."""
    x = _tokens(x, "x")
    dim = dim % x.dim()
    outer = 1
    for d in x.shape[:dim]:
        outer *= d
    inner = 1
    for d in x.shape[dim + 1:]:
        inner *= d
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().must3r_hip_l2_normalize(x.data_ptr(), outer, x.shape[dim], inner, x.data_ptr(), _lib.stream_ptr(x.device)))
    return x


def layernorm_act(x, ln, gelu):
    """nn.LayerNorm ``ln`` (+ erf GELU) on fp32 rows."""
    x = _tokens(x, "x")
    Cd = x.shape[-1]
    if tuple(ln.normalized_shape) != (Cd,):
        raise ValueError(f"LayerNorm over {tuple(ln.normalized_shape)} on rows of {Cd}")
    dev = x.device
    w = None if ln.weight is None else ln.weight.detach().to(device=dev, dtype=torch.float32).contiguous()
    b = None if ln.bias is None else ln.bias.detach().to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty_like(x)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().must3r_hip_layernorm_act_f32(x.data_ptr(), None if w is None else w.data_ptr(), None if b is None else b.data_ptr(),
                                                            float(ln.eps), x.numel() // Cd, Cd, 1 if gelu else 0, out.data_ptr(), _lib.stream_ptr(x.device)))
    return out


def weighted_spoc(feat, attn):
    """retrieval/model.py:82-88."""
    feat, attn = _tokens(feat, "feat"), _tokens(attn, "attn")
    Bn, N, Cd = feat.shape
    out = torch.empty((Bn, Cd), dtype=torch.float32, device=feat.device)
    with torch.cuda.device(feat.device):
        _lib.check(_lib.load().must3r_hip_weighted_spoc(feat.data_ptr(), attn.data_ptr(), Bn, N, Cd, out.data_ptr(), _lib.stream_ptr(feat.device)))
    return out


def how_select_local(feat, attn, nfeat):
    """retrieval/model.py:91-101 -> (topk_features [B,k,C], topk_attn [B,k], topk_indices int64 [B,k]).

    Order: a stable descending sort of ``attn`` -- NaN first (as ``torch.topk`` ranks it), then the numbers descending; equal values, and NaNs among
    themselves, by lower index.  ``k = min(nfeat, N)``, with a negative ``nfeat`` a fraction of N."""
    feat, attn = _tokens(feat, "feat"), _tokens(attn, "attn")
    Bn, N, Cd = feat.shape
    if nfeat < 0:
        assert nfeat >= -1.0
        nfeat = int(-nfeat * N)
    else:
        nfeat = int(nfeat)
    k = min(nfeat, N)
    of = torch.empty((Bn, k, Cd), dtype=torch.float32, device=feat.device)
    oa = torch.empty((Bn, k), dtype=torch.float32, device=feat.device)
    oi = torch.empty((Bn, k), dtype=torch.int64, device=feat.device)
    with torch.cuda.device(feat.device):
        _lib.check(_lib.load().must3r_hip_topk_gather(feat.data_ptr(), attn.data_ptr(), Bn, N, Cd, k, of.data_ptr(), oa.data_ptr(), oi.data_ptr(),
                                                      _lib.stream_ptr(feat.device)))
    return of, oa, oi


class RetrievalModel(nn.Module):
    """retrieval/model.py:104-183 (inference part).  ``backbone`` is only used for its ``embed_dim`` (the reference's
    forward paths take encoder tokens, not images)."""

    def __init__(self, backbone, freeze_backbone=1, prewhiten=None, hdims=[1024], residual=False, postwhiten=None, featweights="l2norm",
                 nfeat=300, pretrained_retrieval=None):
        super().__init__()
        self.freeze_backbone = freeze_backbone
        try:
            self.backbone_dim = backbone.enc_embed_dim
        except Exception:
            self.backbone_dim = backbone.embed_dim
        self.prewhiten = nn.Identity() if prewhiten is None else Whitener(self.backbone_dim)
        self.prewhiten_freq = prewhiten
        self.residual = residual
        if residual:
            assert hdims[-1] == self.backbone_dim
        self.projector = self.build_projector(hdims, residual)
        self.dim = hdims[-1] if len(hdims) > 0 else self.backbone_dim
        self.postwhiten_freq = postwhiten
        self.postwhiten = nn.Identity() if postwhiten is None else Whitener(self.dim)
        if featweights != "l2norm":
            raise NotImplementedError(featweights)
        self.featweights = featweights
        self.nfeat = nfeat
        for prm in self.parameters():
            prm.requires_grad = False
        if pretrained_retrieval is not None:
            ckpt = torch.load(pretrained_retrieval, "cpu", weights_only=False)
            msg = self.load_state_dict(ckpt["model"], strict=False)
            assert len(msg.unexpected_keys) == 0 and all(k.startswith("backbone") or k.startswith("postwhiten") for k in msg.missing_keys)

    def build_projector(self, hdims, residual):   # retrieval/model.py:139-151: same modules, same state-dict keys
        d = self.backbone_dim
        if len(hdims) == 0:
            return nn.Identity()
        layers = []
        for h in hdims[:-1]:
            layers += [nn.Linear(d, h), nn.LayerNorm(h), nn.GELU()]
            d = h
        layers.append(nn.Linear(d, hdims[-1]))
        return nn.Sequential(*layers)

    def _project(self, pre):
        """projector(pre) (+ pre): every Linear one fp32 GEMM, LayerNorm + GELU of a hidden layer one kernel."""
        mods = list(self.projector)
        h = pre
        for i in range(0, len(mods) - 1, 3):
            lin, ln, act = mods[i], mods[i + 1], mods[i + 2]
            assert isinstance(lin, nn.Linear) and isinstance(ln, nn.LayerNorm) and isinstance(act, nn.GELU)
            h = layernorm_act(affine(h, None, lin.weight, b_transposed=True, bias=lin.bias), ln, gelu=True)
        lin = mods[-1]
        return affine(h, None, lin.weight, b_transposed=True, bias=lin.bias, resid=pre if self.residual else None)

    @torch.no_grad()
    def extract_features_and_attention(self, x):   # retrieval/model.py:165-172
        x = _tokens(x, "x")
        pre = x if isinstance(self.prewhiten, nn.Identity) else self.prewhiten(x)
        if isinstance(self.projector, nn.Identity):
            proj = pre if not self.residual else pre + pre
        else:
            proj = self._project(pre)
        Bn, N, Cd = proj.shape
        attention = torch.empty((Bn, N), dtype=torch.float32, device=proj.device)
        with torch.cuda.device(proj.device):
            _lib.check(_lib.load().must3r_hip_row_norm(proj.data_ptr(), Bn * N, Cd, attention.data_ptr(), _lib.stream_ptr(proj.device)))
        post = proj if isinstance(self.postwhiten, nn.Identity) else self.postwhiten(proj)
        return post, attention

    def forward_local(self, x):
        feat, attn = self.extract_features_and_attention(x)
        return how_select_local(feat, attn, self.nfeat)

    def forward_global(self, x):
        feat, attn = self.extract_features_and_attention(x)
        return weighted_spoc(feat, attn)

    def forward(self, x):
        return self.forward_global(x)


def codebook_path(modelname):
    """processor.py:83-86: ``<dir>/<checkpoint name without its last _part>_codebook.pkl``."""
    dname, bname = os.path.split(modelname)
    return os.path.join(dname, "_".join(bname.split("_")[:-1]) + "_codebook.pkl")


def load_frontend(modelname, backbone, device="cuda"):
    """processor.py:62-82: the retrieval front-end of a checkpoint on ``device`` -> (RetrievalModel, the checkpoint's args); no codebook is needed."""
    ckpt = torch.load(modelname, "cpu", weights_only=False)
    a = ckpt["args"]
    model = RetrievalModel(backbone, freeze_backbone=a.freeze_backbone, prewhiten=a.prewhiten,
                           hdims=list(map(int, a.hdims.split("_"))) if len(a.hdims) > 0 else "",
                           residual=getattr(a, "residual", False), postwhiten=a.postwhiten, featweights=a.featweights,
                           nfeat=a.nfeat).to(device)
    msg = model.load_state_dict(ckpt["model"], strict=False)
    if not all(k.startswith("backbone") for k in msg.missing_keys) or len(msg.unexpected_keys) != 0:
        raise RuntimeError(f"{modelname}: missing {msg.missing_keys}, unexpected {msg.unexpected_keys}")
    return model, a


class Retriever:
    """processor.py:62-96 (construction): the retrieval front-end of a checkpoint and its ASMK codebook, on ``device``."""

    def __init__(self, modelname, backbone, device="cuda", verbose=True):
        from .asmk import ASMK, load_codebook
        if not os.path.isfile(modelname):
            raise FileNotFoundError(modelname)
        if backbone is None:
            raise ValueError("Retriever needs the encoder (backbone) the checkpoint was trained on")
        if verbose:
            print(f"Loading retrieval model from {modelname}")
        self.model, a = load_frontend(modelname, backbone, device)
        self.device = device
        self.imsize = a.imsize
        cb = codebook_path(modelname)
        if not os.path.isfile(cb):
            raise FileNotFoundError(f"ASMK codebook not found next to the checkpoint: {cb}")
        self.asmk = ASMK(load_codebook(cb, nclusters=getattr(a, "nclusters", None), device=device), alpha=3.0, similarity_threshold=0.0)


@torch.no_grad()
def frontend_local_features(model, enc, device, dim=None):
    """forward_local of every image's tokens ``enc[i]`` [1, N_i, C] through the front-end ``model``, images with equal token counts in one call ->
    (feat [M, C] on the device, offsets [n + 1]) with image i on rows [offsets[i], offsets[i+1]).  ``dim``: the width of an empty result."""
    groups = {}
    for i, e in enumerate(enc):
        groups.setdefault(tuple(e.shape[1:]), []).append(i)
    per_image = [None] * len(enc)
    for idx in groups.values():
        x = torch.cat([enc[i].to(device) for i in idx], dim=0)
        feat, _, _ = model.forward_local(x)
        for j, i in enumerate(idx):
            per_image[i] = feat[j]
    offsets = np.zeros((len(enc) + 1,), dtype=np.int64)
    offsets[1:] = np.cumsum([f.shape[0] for f in per_image])
    feat = torch.cat(per_image, dim=0) if per_image else torch.empty((0, model.dim if dim is None else dim), device=device)
    return feat.contiguous(), offsets


class MUSt3R_Retriever(Retriever):
    """demo/inference.py:31-60: encoder tokens of the images -> float64 numpy [n, n] scores (row = query, column = database)."""

    def local_features(self, enc, device):
        """``frontend_local_features`` of this retriever's front-end"""
        return frontend_local_features(self.model, enc, device, dim=self.asmk.codebook.shape[1])

    def __call__(self, enc, device):
        feat, offsets = self.local_features(enc, device)
        return self.asmk.scores_numpy(feat, offsets)
