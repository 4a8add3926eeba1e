"""The prediction head with a backward pass: ``MUSt3R._compute_prediction_head`` (decoder.py:149-156: ``norm_dec`` LayerNorm, ``head_dec.proj``
Linear D -> 7 * 16 * 16, pixel shuffle to ``[n, H, W, 7]``; blocks/head.py:63-72, tools/image.py:9-14) under ``torch.autograd``, the link between the
decoder's last-layer tokens and ``must3r_amd.train_losses``::

    head = PredictionHead.from_decoder(decoder)
    raw = head(tokens, true_shape)                                    # tokens.requires_grad or not
    loss, details = criterion(gt, train_losses.postprocess(raw, 'norm_exp'))
    loss.backward()                                                   # tokens.grad, head.*.grad
    train_optim.AdamW(head.parameters()).step()                       # the native step (must3r_amd/train_optim.py); torch.optim.AdamW works too

The forward is the native decoder's own head (the same two launches, ``must3r_hip_head_forward``) on operands packed from the fp32 parameters of the
call, so that an optimizer step is seen by the next forward.  The backward (``must3r_hip_head_grad``, include/must3r_hip.h ABI 19) runs fp32 operands on
the fp32 MFMA, recomputes the LayerNorm statistics from the tokens and reads the upstream gradient in place: the forward saves its five inputs and
nothing else.  Only the gradients that ``needs_input_grad`` asks for are computed.  First order only (``once_differentiable``); gradients come back
in the shape and dtype of their inputs.  CPU tensors raise.

A batch stored landscape may hold portrait views (the reference's ``transpose_to_landscape(head, activate=True)``, blocks/head.py:24-60; the training recipe's
``landscape_only=True``)::

    head = PredictionHead.from_decoder(decoder, landscape_only=True)
    raw = head(tokens, true_shape, img_shape=(H, W))                  # true_shape rows (H, W) or, for a portrait view, (W, H); raw [B, nimgs, H, W, 7]

Which views are portrait is computed on the device and read by the kernels (``must3r_hip_head_forward_many_ar`` / ``must3r_hip_head_grad_many_ar``, ABI 21,
additive): the head's two launches write every view with the landscape geometry, the tiles of the flagged views alone are then turned into their places, and
the backward reads the upstream gradient of those views through the same map.  Given ``img_shape`` the host reads nothing back.  ``landscape_only=False``, the
default, is the module as it was.
"""
import ctypes as C

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._train_common import _Affine, _back, _dev, _f32, _new, _Proj, _ptr, _scratch, _stream

PATCH, CHANNELS = 16, 7
OUT = CHANNELS * PATCH * PATCH
WGRAD_MAX_SPLITS, WGRAD_ROWS_PER_SPLIT = 16, 128


def wgrad_splits(rows):
    """Over how many blocks the weight gradient splits its sum over ``rows`` token rows (``must3r_hip_head_grad_splits``): a function of the
    row count alone, so that the order of the additions, and with it every bit of the result, is fixed by the shapes."""
    return max(1, min(WGRAD_MAX_SPLITS, -(-int(rows) // WGRAD_ROWS_PER_SPLIT))) if rows > 0 else 0


def _check_shapes(tokens, img_shape, norm_weight, norm_bias, proj_weight, proj_bias):
    H, W = int(img_shape[0]), int(img_shape[1])
    if H <= 0 or W <= 0 or H % PATCH or W % PATCH:
        raise ValueError(f"prediction_head: the image size {(H, W)} is not a positive multiple of {PATCH}")
    if tokens.ndim < 2:
        raise ValueError(f"prediction_head: tokens of shape {tuple(tokens.shape)}, expected [..., N, D]")
    N, D = int(tokens.shape[-2]), int(tokens.shape[-1])
    if N != (H // PATCH) * (W // PATCH):
        raise ValueError(f"prediction_head: {N} tokens per view do not match an image of {H} x {W} ({(H // PATCH) * (W // PATCH)} patches)")
    if tuple(norm_weight.shape) != (D,) or tuple(norm_bias.shape) != (D,) or tuple(proj_weight.shape) != (OUT, D) or tuple(proj_bias.shape) != (OUT,):
        raise ValueError(f"prediction_head: parameters of shapes {tuple(norm_weight.shape)}, {tuple(norm_bias.shape)}, {tuple(proj_weight.shape)}, "
                         f"{tuple(proj_bias.shape)} do not belong to tokens of width {D}")
    return H, W, N, D


def _check_transposed(transposed, n_views, H, Wimg, what):
    """The per-view portrait flags of a head call: int32 ``[n_views]`` on the device, as ``train_encoder.patch_rows`` takes them."""
    _dev(transposed, f"{what}: transposed")
    if transposed.dtype != torch.int32 or tuple(transposed.shape) != (n_views,):
        raise ValueError(f"{what}: transposed of dtype {transposed.dtype} and shape {tuple(transposed.shape)}, expected int32 [{n_views}]")
    if H > Wimg:
        raise ValueError(f"{what}: a batch with portrait flags is stored landscape; this one is {H} x {Wimg}")
    return transposed.contiguous()


def head_forward(x, gamma, beta, W, b, n_views, H, Wimg, eps=1e-6, dtype=_lib.F16, transposed=None):
    """``must3r_hip_head_forward`` on contiguous fp32 tensors: x [n_views * N, D] -> pointmaps [n_views, H, Wimg, 7].  ``transposed`` (int32 [n_views] on the
    device, non-zero = portrait view of a batch stored landscape): ``must3r_hip_head_forward_many_ar``."""
    lib = _lib.load()
    D = int(x.shape[-1])
    out = torch.empty((n_views, H, Wimg, CHANNELS), dtype=torch.float32, device=x.device)
    if transposed is not None:
        a = _lib.HeadForwardArArgs()
        a.x, a.gamma, a.beta, a.W, a.b = _ptr(x), _ptr(gamma), _ptr(beta), _ptr(W), _ptr(b)
        a.dtype, a.n_views, a.H, a.Wimg, a.D, a.eps = dtype, n_views, H, Wimg, D, eps
        a.pointmaps, a.transposed, a.stream = _ptr(out), _ptr(transposed), _stream(x.device)
        with torch.cuda.device(x.device):
            nbytes = lib.must3r_hip_head_forward_many_ar_scratch_bytes(n_views, H, Wimg, D)
            scratch = _scratch(nbytes, x.device)
            _lib.check(lib.must3r_hip_head_forward_many_ar(C.byref(a), _ptr(scratch), nbytes))
        return out
    with torch.cuda.device(x.device):
        nbytes = lib.must3r_hip_head_forward_scratch_bytes(n_views, H, Wimg, D)
        scratch = _scratch(nbytes, x.device)
        _lib.check(lib.must3r_hip_head_forward(dtype, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(W), _ptr(b), n_views, H, Wimg, D, eps, _ptr(out),
                                               _ptr(scratch), nbytes, _stream(x.device)))
    return out


def head_linear(y, W, b, n_views, H, Wimg, dtype=_lib.F16):
    """The Linear stage of the head alone (``must3r_hip_op_head_linear``): y fp32 [n_views * N, D], already normalised -> [n_views, H, Wimg, 7]."""
    lib = _lib.load()
    y, W, b = (_f32(_dev(t, n)) for t, n in ((y, "y"), (W, "W"), (b, "b")))
    D = int(y.shape[-1])
    out = torch.empty((n_views, H, Wimg, CHANNELS), dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        nbytes = lib.must3r_hip_head_forward_scratch_bytes(n_views, H, Wimg, D)
        scratch = _scratch(nbytes, y.device)
        _lib.check(lib.must3r_hip_op_head_linear(dtype, _ptr(y), _ptr(W), _ptr(b), n_views, H, Wimg, D, _ptr(out), _ptr(scratch), nbytes,
                                                 _stream(y.device)))
    return out


def head_grad(x, gamma, beta, W, G, n_views, H, Wimg, eps=1e-6, want=(True,) * 5, transposed=None):
    """``must3r_hip_head_grad`` on contiguous fp32 tensors: ``(dx, dgamma, dbeta, dW, db)``, ``None`` where ``want`` says so.  ``transposed``: as in
    ``head_forward`` (``must3r_hip_head_grad_many_ar``)."""
    lib = _lib.load()
    D, dev = int(x.shape[-1]), x.device
    want_dx, want_dg, want_dbeta, want_dw, want_db = want
    # dY lives in the dx buffer: the column sums of the LayerNorm backward need one even when the tokens are frozen
    dx = _new(want_dx or want_dg or want_dbeta, dev, *x.shape)
    dgamma, dbeta, dW, db = _new(want_dg, dev, D), _new(want_dbeta, dev, D), _new(want_dw, dev, OUT, D), _new(want_db, dev, OUT)
    ar = _lib.HeadGradArArgs() if transposed is not None else None
    a = ar.g if ar is not None else _lib.HeadGradArgs()
    a.x, a.gamma, a.beta, a.W, a.G = _ptr(x), _ptr(gamma), _ptr(beta), _ptr(W), _ptr(G)
    a.n_views, a.H, a.Wimg, a.D, a.eps = n_views, H, Wimg, D, eps
    a.dx, a.dgamma, a.dbeta, a.dW, a.db = _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(dW), _ptr(db)
    if ar is not None:
        ar.transposed, ar.stream = _ptr(transposed), _stream(dev)
        with torch.cuda.device(dev):
            nbytes = lib.must3r_hip_head_grad_many_ar_scratch_bytes(n_views, H, Wimg, D)
            scratch = _scratch(nbytes, dev)
            _lib.check(lib.must3r_hip_head_grad_many_ar(C.byref(ar), _ptr(scratch), nbytes))
        return (dx if want_dx else None), dgamma, dbeta, dW, db
    with torch.cuda.device(dev):
        nbytes = lib.must3r_hip_head_grad_scratch_bytes(n_views, H, Wimg, D)
        scratch = _scratch(nbytes, dev)
        _lib.check(lib.must3r_hip_head_grad(C.byref(a), _ptr(scratch), nbytes, _stream(dev)))
    return (dx if want_dx else None), dgamma, dbeta, dW, db


class _Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tokens, norm_weight, norm_bias, proj_weight, proj_bias, H, W, eps, dtype, transposed=None):
        D = int(tokens.shape[-1])
        lead = tuple(tokens.shape[:-2])
        n_views = tokens.numel() // (int(tokens.shape[-2]) * D)
        ctx.save_for_backward(tokens, norm_weight, norm_bias, proj_weight, proj_bias, *([transposed] if transposed is not None else []))
        ctx.geom = (n_views, H, W, eps)
        out = head_forward(_f32(tokens).view(-1, D), _f32(norm_weight), _f32(norm_bias), _f32(proj_weight), _f32(proj_bias), n_views, H, W, eps, dtype,
                           transposed)
        return out.view(*lead, H, W, CHANNELS)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        *saved, = ctx.saved_tensors
        flags = saved.pop() if len(saved) == 6 else None
        n_views, H, W, eps = ctx.geom
        x, gamma, beta, Wt, _ = (_f32(t) for t in saved)
        grads = head_grad(x.view(-1, x.shape[-1]), gamma, beta, Wt, _f32(grad_out), n_views, H, W, eps, want=tuple(ctx.needs_input_grad[:5]),
                          transposed=flags)
        return (*_back(grads, saved), None, None, None, None, None)


def prediction_head(tokens, img_shape, norm_weight, norm_bias, proj_weight, proj_bias, eps=1e-6, dtype=_lib.F16, transposed=None):
    """Raw pointmaps ``[..., H, W, 7]`` fp32 from the decoder's last-layer tokens ``[..., N, D]`` (before ``norm_dec``), ``img_shape = (H, W)`` shared
    by every view; differentiable at the tokens and the four parameters.  ``dtype``: the 16-bit operand type of the forward's split-precision
    products (``_lib.F16`` / ``_lib.BF16``), as in the native decoder.  ``transposed``: int32, one entry per view, on the device (the tensor
    ``train_encoder.patch_rows`` takes): a non-zero entry marks a portrait view of a batch stored landscape (``H <= W``), whose tokens are those of its own
    ``W/16 x H/16`` grid and whose pointmaps come back in the stored layout -- ``head(tokens[v], (W, H)).swapaxes(0, 1)``, the reference's
    ``transpose_to_landscape(head, activate=True)``.  The kernels read the flags; the host does not.  ``None``: no view is, the call is the one it was."""
    H, W, N, D = _check_shapes(tokens, img_shape, norm_weight, norm_bias, proj_weight, proj_bias)
    for t, what in ((tokens, "tokens"), (norm_weight, "norm_weight"), (norm_bias, "norm_bias"), (proj_weight, "proj_weight"), (proj_bias, "proj_bias")):
        _dev(t, what)
    if tokens.numel() == 0:
        raise ValueError("prediction_head: no tokens")
    inputs = (tokens, norm_weight, norm_bias, proj_weight, proj_bias)
    n_views = tokens.numel() // (N * D)
    if transposed is not None:
        transposed = _check_transposed(transposed.reshape(-1) if isinstance(transposed, torch.Tensor) else transposed, n_views, H, W, "prediction_head")
    if torch.is_grad_enabled() and any(t.requires_grad for t in inputs):
        return _Head.apply(*inputs, H, W, float(eps), int(dtype), transposed)
    out = head_forward(_f32(tokens).view(-1, D), *(_f32(t) for t in inputs[1:]), n_views, H, W, float(eps), int(dtype), transposed)
    return out.view(*tokens.shape[:-2], H, W, CHANNELS)


class _HeadDec(nn.Module):
    def __init__(self, dim, out):
        super().__init__()
        self.proj = _Proj(dim, out)


class PredictionHead(nn.Module):
    """``norm_dec`` and ``head_dec`` of the decoder as a trainable module; the parameters live under the reference's state-dict keys
    (``norm_dec.weight``, ``norm_dec.bias``, ``head_dec.proj.weight``, ``head_dec.proj.bias``) in fp32.  ``landscape_only``: the constructor value of the
    reference's decoder (blocks/head.py:24-60).  ``False``, the default: all views of a call share ``(H, W)`` (the reference's ``wrapper_no``).  ``True``, the
    training recipe's: the batch is stored landscape and a ``true_shape`` row of ``(W, H)`` marks a portrait view (``wrapper_yes``)."""

    def __init__(self, embed_dim=768, eps=1e-6, dtype=_lib.F16, landscape_only=False):
        super().__init__()
        self.embed_dim, self.eps, self.dtype, self.landscape_only = int(embed_dim), float(eps), int(dtype), bool(landscape_only)
        self.norm_dec = _Affine(self.embed_dim)
        self.head_dec = _HeadDec(self.embed_dim, OUT)

    @classmethod
    def from_decoder(cls, decoder, dtype=_lib.F16, landscape_only=False):
        """fp32 copies of a loaded decoder's four head tensors (the decoder itself is left alone, and so is its ``landscape_only``: the value is the caller's)."""
        w = decoder.norm_dec.weight
        head = cls(int(w.shape[0]), float(decoder.norm_dec.eps), dtype, landscape_only)
        with torch.no_grad():
            for dst, src in ((head.norm_dec.weight, w), (head.norm_dec.bias, decoder.norm_dec.bias),
                             (head.head_dec.proj.weight, decoder.head_dec.proj.weight), (head.head_dec.proj.bias, decoder.head_dec.proj.bias)):
                dst.copy_(src.detach().to(torch.float32))
        return head.to(w.device)

    def forward(self, tokens, true_shape, img_shape=None):
        """tokens ``[B, nimgs, N, D]`` (or ``[nimgs, N, D]``), true_shape ``[B, nimgs, 2]`` of (H, W) rows, all alike -> ``[B, nimgs, H, W, 7]``.

        With ``landscape_only=True`` the rows of true_shape are ``(H, W)`` or, for a portrait view, ``(W, H)`` of one stored size ``H <= W``, and the result is
        in the stored layout.  Which views are portrait is computed on the device (``height > width``) and read by the kernels.  ``img_shape``: the stored
        ``(H, W)``; with it nothing is read back to the host, and that the rows are ``(H, W)`` or ``(W, H)`` is then the caller's word (a precondition: a row
        that is neither is treated by its ``height > width`` alone).  Without it ``(H, W)`` is ``true_shape.min()`` / ``.max()`` on the host, as in the
        reference, and the rows are checked there.  ``img_shape`` is not looked at with ``landscape_only=False``."""
        if self.landscape_only:
            return self._forward_landscape_only(tokens, true_shape, img_shape)
        ts = torch.as_tensor(true_shape).reshape(-1, 2).cpu()
        H, W = int(ts[0, 0]), int(ts[0, 1])
        if not bool((ts == ts[0]).all()):
            raise ValueError("PredictionHead: all views of a call must share (H, W)")
        return prediction_head(tokens, (H, W), self.norm_dec.weight, self.norm_dec.bias, self.head_dec.proj.weight, self.head_dec.proj.bias,
                               self.eps, self.dtype)

    def _forward_landscape_only(self, tokens, true_shape, img_shape):
        ts = torch.as_tensor(true_shape).reshape(-1, 2)
        if img_shape is not None:
            H, W = int(img_shape[0]), int(img_shape[1])
        else:
            host = ts.cpu()
            H, W = int(host.min()), int(host.max())
            if not bool((((host[:, 0] == H) & (host[:, 1] == W)) | ((host[:, 0] == W) & (host[:, 1] == H))).all()):
                raise ValueError(f"PredictionHead(landscape_only=True): every row of true_shape must be ({H}, {W}) or ({W}, {H}), one stored size")
        if H > W:
            raise ValueError(f"PredictionHead(landscape_only=True): the batch is stored landscape; img_shape is {H} x {W}")
        params = (self.norm_dec.weight, self.norm_dec.bias, self.head_dec.proj.weight, self.head_dec.proj.bias)
        _check_shapes(tokens, (H, W), *params)                 # a bad shape is reported as such wherever the tensors live
        _dev(tokens, "tokens")
        ts = ts.to(tokens.device)
        flags = (ts[:, 0] > ts[:, 1]).to(torch.int32)          # on the device: nothing is read back
        return prediction_head(tokens, (H, W), self.norm_dec.weight, self.norm_dec.bias, self.head_dec.proj.weight, self.head_dec.proj.bias,
                               self.eps, self.dtype, flags)
