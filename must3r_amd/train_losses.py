"""The reference's training criterion with a backward pass: ``must3r_amd.losses`` under ``torch.autograd`` (must3r/engine/losses.py
``Regr3D`` / ``ConfLoss``, the dust3r leaves ``L21`` / ``Criterion`` / ``MultiLoss`` / ``Sum``) and the head activation
(engine/inference.py ``postprocess``), under the reference's names, so that the training recipe's criterion string evaluates in this
module's namespace::

    criterion = eval("ConfLoss(Regr3D(L21, norm_mode='?avg_dis', sky_loss_value=2, loss_in_log=False), alpha=0.2)", vars(train_losses))
    loss, details = criterion(gt, postprocess(raw, 'norm_exp'))
    loss.backward()                                       # -> raw.grad

The forward values are those of ``must3r_amd.losses``, bit for bit: the same fused passes run on the detached inputs.  The gradient has
a closed form (include/must3r_hip.h, ABI 16) and comes out of ``must3r_hip_metrics_loss_grad``, which recomputes the per-pixel chain from
the inputs instead of saving it: the direct term through the log map, the scale and the warp; the path through a normalisation factor
that was computed from the prediction itself (``avg_dis``, ``avg_log1p``, ``avg_warp-log1p``, ``sqrt_dis``; ``median_dis`` is detached
in the reference), which reaches every valid pixel of ``pts3d``, those beyond ``dist_clip`` included; and, in ``ConfLoss``, the
gradient at ``conf``.  No per-pixel tensor is materialised for ``ConfLoss`` or for the 'mean' / 'sum' reductions.  With
``reduction='none'`` the dense per-pixel losses are the outputs and torch does the boolean gather.

Where the reference differs: ground truth is read only under ``valid``, so NaN ground truth outside it (sky pixels) does not turn the
gradients into NaN as ``torch.where``'s backward does; the norm's gradient at a zero residual is 0 (as torch has it); and a
prediction point at exactly 0 gets no scale-path gradient, where the reference yields ``inf * 0 = NaN`` for ``sqrt_dis``.  The factor
of ``sqrt_dis`` is taken over the valid pixels (a NaN prediction under ``valid``, which ``nanmean`` would skip, is not provided for).

First order only: the backward passes are ``once_differentiable``.  Gradients come back in the dtype and shape of the input they
belong to.  Inputs that do not require grad take the forward-only route of ``must3r_amd.losses``.  CPU tensors raise.
"""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from . import losses as _L
from .losses import BaseCriterion, Criterion, MultiLoss, Sum  # noqa: F401  (the reference's names)
from .model import ActivationType

_SCALE_PATH = (_lib.NORM_AVG_DIS, _lib.NORM_AVG_LOG1P, _lib.NORM_SQRT_DIS)


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _detached(pred):
    return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in pred.items()}


def loss_grad_pass(args, kw, weighting, w_g, w_l, counts=None, own=None, norm_mode=None, with_conf=False):
    """The backward of ``losses.loss_pass(*args, **kw)`` (``must3r_hip_metrics_loss_grad``): ``(grad_pts [B,V,H,W,3], grad_local or None,
    grad_conf [B,V,H,W] or None)`` fp32.  ``weighting`` one of ``_lib.LOSS_W_*`` with ``w_g`` / ``w_l`` one-element device tensors
    (per-pixel [B,V,H,W] with ``LOSS_W_PIXEL``), ``counts`` the forward's; ``own`` host bool [B]: the scenes whose ``pr_scale`` is the
    ``norm_mode`` factor of their own prediction."""
    lib = _lib.load()
    a, keep, (B, V, H, W), dev = _L.loss_args(*args, **kw)
    g = _lib.MetricsLossGradArgs()
    w_g = _L._f32(w_g, "w_g")
    w_l = w_g if w_l is None else _L._f32(w_l, "w_l")
    want = (B, V, H, W) if weighting == _lib.LOSS_W_PIXEL else (1,)
    if tuple(w_g.shape) != want or tuple(w_l.shape) != want:
        raise ValueError(f"loss_grad_pass: weights of shape {tuple(w_g.shape)} / {tuple(w_l.shape)}, expected {want}")
    g.w_g, g.w_l, g.weighting = _L._ptr(w_g), _L._ptr(w_l), weighting
    g.counts = _L._ptr(counts)
    mode = _L.NORM_MODES.get(norm_mode) if norm_mode else None
    if own is not None and mode in _SCALE_PATH and bool(own.any()):      # ``own`` lives on the host
        own_dev = own.to(torch.uint8).to(dev)
        n_valid = _L._u8(args[3], "valid").reshape(B, -1).sum(dim=1, dtype=torch.int64)
        keep += [own_dev, n_valid]
        g.factor_mode, g.n_own, g.own_factor, g.n_valid = mode, int(own.sum()), _L._ptr(own_dev), _L._ptr(n_valid)
    has_local = kw.get('pr_local') is not None
    grad_pts = torch.empty((B, V, H, W, 3), dtype=torch.float32, device=dev)
    grad_local = torch.empty((B, V, H, W, 3), dtype=torch.float32, device=dev) if has_local else None
    grad_conf = torch.empty((B, V, H, W), dtype=torch.float32, device=dev) if with_conf else None
    g.grad_pts, g.grad_local, g.grad_conf = _L._ptr(grad_pts), _L._ptr(grad_local), _L._ptr(grad_conf)
    nbytes = lib.must3r_hip_metrics_loss_grad_scratch_bytes(B, V, H, W)
    if not nbytes:
        raise _lib.HipError(lib.must3r_hip_last_error().decode("utf-8", "replace"))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.must3r_hip_metrics_loss_grad(C.byref(a), C.byref(g), _L._ptr(scratch), nbytes, C.c_void_p(_lib.stream_ptr(dev))))
    return grad_pts, grad_local, grad_conf


class _Pass:
    """What the backward of one forward pass needs: the inputs of ``loss_pass``, the weighting, and how the upstream gradients of the
    outputs become the two weights.  It never holds the outputs themselves: they point to the graph node, which points here."""

    def __init__(self, args, kw, weighting, weights, counts=None, own=None, norm_mode=None, with_conf=False, route=None):
        self.args, self.kw, self.weighting, self.weights = args, kw, weighting, weights
        self.counts, self.own, self.norm_mode, self.with_conf = counts, own, norm_mode, with_conf
        self.route = route or (lambda gp, gl, gc, needs: (gp, gl, gc))

    def grads(self, gos, needs):
        w_g, w_l = self.weights(gos)
        return self.route(*loss_grad_pass(self.args, self.kw, self.weighting, w_g, w_l, counts=self.counts, own=self.own,
                                          norm_mode=self.norm_mode, with_conf=self.with_conf), needs)


class _Fused(torch.autograd.Function):
    """Attaches ``outs``, the outputs of a pass that has run on the detached inputs, to the graph of the inputs.  The inputs are saved
    only so that autograd notices an in-place change between forward and backward (the pass reads them again)."""

    @staticmethod
    def forward(ctx, run, outs, *inputs):
        ctx.run = run
        ctx.meta = [None if t is None else (t.shape, t.dtype) for t in inputs]
        ctx.save_for_backward(*(t for t in inputs if t is not None))
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *gos):
        ctx.saved_tensors                        # raises if an input was modified in place
        grads = ctx.run.grads(gos, ctx.needs_input_grad[2:])
        out = [None, None]
        for need, meta, g in zip(ctx.needs_input_grad[2:], ctx.meta, grads):
            out.append(g.reshape(meta[0]).to(meta[1]) if need and g is not None else None)
        return tuple(out)


class L21Loss(_L.L21Loss):
    """``||a - b||`` per point, differentiable in both arguments (the gradient at ``b`` is the negation of that at ``a``)."""

    def __call__(self, a, b):
        if not _wants_grad(a, b):
            return super().__call__(*(t.detach() if isinstance(t, torch.Tensor) else t for t in (a, b)))
        assert a.shape == b.shape and a.ndim >= 2 and a.shape[-1] == 3, f'Bad shape = {a.shape}'
        _L._dev(a, "a"), _L._dev(b, "b")
        if self.reduction not in ('none', 'sum', 'mean'):
            raise ValueError(f'bad {self.reduction=} mode')
        n = a.numel() // 3
        if n == 0:                               # nothing to launch: the empty reductions, attached to the inputs
            empty = ((a - b) * 0).sum(dim=-1).to(torch.float32)
            return empty if self.reduction == 'none' else (empty.sum() if self.reduction == 'sum' else empty.mean())
        none = self.reduction == 'none'
        args = self.pass_inputs(a.detach(), b.detach())
        out = _L.loss_pass(*args, per_pixel=none)
        weighting = _lib.LOSS_W_PIXEL if none else (_lib.LOSS_W_SCALAR if self.reduction == 'sum' else _lib.LOSS_W_MEAN)
        run = _Pass(args, {}, weighting,
                    (lambda gos: (gos[0].reshape(1, 1, 1, n), None)) if none else (lambda gos: (gos[0].reshape(1), None)),
                    counts=out[0], route=lambda gp, gl, gc, needs: (gp, -gp if needs[1] else None))
        return _Fused.apply(run, (self.pick(out, a.shape[:-1]),), a, b)[0]


L21 = L21Loss()


class Regr3D(_L.Regr3D):
    """``must3r_amd.losses.Regr3D`` with a backward pass at ``pred['pts3d']`` and ``pred['pts3d_local']``, for every reduction."""

    def compute_loss(self, gt, pred, **kw):
        inputs = (pred['pts3d'], pred.get('pts3d_local'))
        if not _wants_grad(*inputs):
            return super().compute_loss(gt, _detached(pred), **kw)
        if self.sky_loss_value > 0:
            assert self.criterion.reduction == 'none', 'sky_loss_value should be 0 if no conf loss'
        has_local = inputs[1] is not None
        none = self.criterion.reduction == 'none'
        args, akw, own = self.fused_inputs(gt, _detached(pred), **kw)
        out = _L.loss_pass(*args, per_pixel=none, **akw)
        figures = self.figures(out[0], out[1])
        common = dict(counts=out[0], own=own, norm_mode=self.norm_mode)
        if none:
            pix_g, pix_l, msk_g, msk_l = out[2]
            run = _Pass(args, akw, _lib.LOSS_W_PIXEL, lambda gos: (gos[0], gos[1]), **common)
            pix_g, pix_l = _Fused.apply(run, (pix_g, pix_l), *inputs)
            loss = self.assemble(figures, (pix_g, pix_l, msk_g, msk_l), has_local)
        else:
            k = 2 if self.criterion.reduction == 'sum' else 0
            run = _Pass(args, akw, _lib.LOSS_W_SCALAR if k else _lib.LOSS_W_MEAN, lambda gos: (gos[0][k:k + 1], gos[0][k + 1:k + 2]), **common)
            loss = self.assemble(_Fused.apply(run, (figures,), *inputs)[0], None, has_local)
        return loss, self.details(figures, has_local)


class ConfLoss(_L.ConfLoss):
    """``must3r_amd.losses.ConfLoss`` with a backward pass at ``pts3d``, ``pts3d_local`` and ``conf``; still one fused forward pass and
    one device->host read, and no per-pixel tensor besides the three gradients."""

    def compute_loss(self, gt, pred, **kw):
        inputs = (pred['pts3d'], pred.get('pts3d_local'), pred.get('conf'))
        if not _wants_grad(*inputs):
            return super().compute_loss(gt, _detached(pred), **kw)
        has_local, has_conf = inputs[1] is not None, inputs[2] is not None
        pixel_loss = self.pixel_loss
        args, akw, own = pixel_loss.fused_inputs(gt, _detached(pred), alpha=self.alpha, **kw)
        counts, sums = _L.loss_pass(*args, **akw)
        run = _Pass(args, akw, _lib.LOSS_W_CONF if has_conf else _lib.LOSS_W_MEAN, lambda gos: (gos[0][2:3], gos[0][3:4]),
                    counts=counts, own=own, norm_mode=pixel_loss.norm_mode, with_conf=has_conf)
        return self.result(_Fused.apply(run, (self.figures(counts, sums, has_conf),), *inputs)[0], has_local)


class _Activation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pointmaps, activation):
        from .engine import postprocess as forward_only
        out = forward_only(pointmaps.detach(), activation)
        ctx.save_for_backward(pointmaps)
        ctx.activation = _lib.ACT_LINEAR if activation == ActivationType.LINEAR else _lib.ACT_NORM_EXP
        return out["pts3d"], out["pts3d_local"], out["conf"]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_pts, g_local, g_conf):
        pointmaps, = ctx.saved_tensors
        pm = pointmaps.detach().float().contiguous()
        grads = [g.float().contiguous() for g in (g_pts, g_local, g_conf)]
        out = torch.empty_like(pm)
        lib = _lib.load()
        with torch.cuda.device(pm.device):
            _lib.check(lib.must3r_hip_postprocess_act_grad(pm.data_ptr(), ctx.activation, *(g.data_ptr() for g in grads), out.data_ptr(),
                                                           pm.numel() // 7, _lib.stream_ptr(pm.device)))
        return out.to(pointmaps.dtype), None


def postprocess(pointmaps, pointmaps_activation=ActivationType.NORM_EXP, compute_cam=False):
    """``must3r_amd.postprocess`` (pointmaps [..., 7] -> ``pts3d``, ``pts3d_local``, ``conf``), differentiable at ``pointmaps``: the
    backward (``must3r_hip_postprocess_act_grad``) recomputes from the raw head output, the forward saves nothing else."""
    if compute_cam:
        raise NotImplementedError("must3r_amd.train_losses.postprocess: compute_cam is not differentiable here; use must3r_amd.postprocess")
    from .engine import postprocess as forward_only
    if isinstance(pointmaps_activation, str):
        pointmaps_activation = ActivationType(pointmaps_activation)
    _L._dev(pointmaps, "pointmaps")
    if not _wants_grad(pointmaps):
        return forward_only(pointmaps, pointmaps_activation)
    pts3d, pts3d_local, conf = _Activation.apply(pointmaps, pointmaps_activation)
    return {"pts3d": pts3d, "pts3d_local": pts3d_local, "conf": conf}
