"""Forward values of the reference's loss family on the GPU (must3r/engine/losses.py ``Regr3D`` / ``ConfLoss``; must3r/tools/geometry.py
``normalize_pointcloud`` / ``apply_log_to_norm``; the dust3r leaves ``L21``, ``geotrf``, ``Criterion`` / ``MultiLoss`` / ``Sum`` as far as
these classes use them), under the reference's names and call signatures, so that the training recipe's criterion string evaluates in
this module's namespace::

    ConfLoss(Regr3D(L21, norm_mode='?avg_dis', sky_loss_value=2, loss_in_log=False), alpha=0.2)

Every scalar (``ConfLoss``'s loss and ``details``, ``Regr3D``'s ``details``, ``L21``'s mean, ``eval_metric``) comes out of the fused passes
of csrc/metrics.hip: one read of the inputs, rigid transforms and scales applied per pixel, fp64 sums per (scene, view) combined in a
fixed order.  Per-pixel tensors exist only where a caller asks for them (``reduction='none'``, ``get_all_pts3d``).  Forward only: a
``pred`` that requires grad raises (``must3r_amd.train_losses`` subclasses these criteria with a backward pass).  As everywhere in the package, CPU tensors raise; there is no fallback.

An empty selection has count 0 and mean NaN (``torch.mean`` of nothing); ``ConfLoss`` turns that into 0 as the reference does.
"""
import ctypes as C
from copy import copy, deepcopy

import torch

from . import _lib

NORM_MODES = {"avg_dis": _lib.NORM_AVG_DIS, "avg_log1p": _lib.NORM_AVG_LOG1P, "avg_warp-log1p": _lib.NORM_AVG_LOG1P,
              "sqrt_dis": _lib.NORM_SQRT_DIS, "median_dis": _lib.NORM_MEDIAN_DIS}


# ------------------------------------------------------------------------------------------------------------------------------------
# device passes
# ------------------------------------------------------------------------------------------------------------------------------------
def _dev(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"must3r_amd.losses: {what} must be a tensor on the GPU (there is no CPU path)")
    return t


def _f32(t, what):
    return _dev(t, what).detach().to(torch.float32).contiguous()


def _u8(t, what):
    t = _dev(t, what)
    return (t if t.dtype == torch.uint8 else t.to(torch.bool).to(torch.uint8)).contiguous()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _no_grad_input(pred):
    for k, v in pred.items():
        if isinstance(v, torch.Tensor) and v.requires_grad:
            raise NotImplementedError(f"must3r_amd.losses: pred['{k}'] requires grad, and the backward pass is not built "
                                      "(forward values only; training is out of scope)")


def loss_args(gt_pts, in_camera0, pr_pts, valid, w2c=None, pr_local=None, conf=None, sky=None, gt_scale=None, pr_scale=None,
              pr_warp=None, gt_warp=False, dist_clip=None, loss_in_log=False, sky_loss_value=0.0, alpha=0.0):
    """The argument block of ``must3r_hip_metrics_loss`` (and of its backward) without outputs: ``(block, keep, (B, V, H, W), device)``;
    ``keep`` holds the converted tensors, which must outlive the launch: only their addresses go into the block."""
    gt_pts, pr_pts = _f32(gt_pts, "gt_pts"), _f32(pr_pts, "pr_pts")
    if gt_pts.ndim != 5 or gt_pts.shape[-1] != 3 or pr_pts.shape != gt_pts.shape:
        raise ValueError(f"loss_pass: gt_pts {tuple(gt_pts.shape)} and pr_pts {tuple(pr_pts.shape)} must both be [B,V,H,W,3]")
    B, V, H, W, _ = gt_pts.shape
    dev = gt_pts.device
    keep = [gt_pts, pr_pts]

    def opt(t, conv, what, shape):
        if t is None:
            return None
        t = conv(t, what)
        if tuple(t.shape) != shape:
            raise ValueError(f"loss_pass: {what} has shape {tuple(t.shape)}, expected {shape}")
        keep.append(t)
        return t
    a = _lib.MetricsLossArgs()
    a.n_scenes, a.n_views, a.H, a.W = B, V, H, W
    a.gt_pts, a.pr_pts = _ptr(gt_pts), _ptr(pr_pts)
    a.in_camera0 = _ptr(opt(in_camera0, _f32, "in_camera0", (B, 4, 4)))
    a.w2c = _ptr(opt(w2c, _f32, "w2c", (B, V, 4, 4)))
    a.pr_local = _ptr(opt(pr_local, _f32, "pr_local", (B, V, H, W, 3)))
    a.conf = _ptr(opt(conf, _f32, "conf", (B, V, H, W)))
    a.valid = _ptr(opt(valid, _u8, "valid", (B, V, H, W)))
    a.sky = _ptr(opt(sky, _u8, "sky", (B, V, H, W)))
    a.gt_scale = _ptr(opt(gt_scale, _f32, "gt_scale", (B,)))
    a.pr_scale = _ptr(opt(pr_scale, _f32, "pr_scale", (B,)))
    a.pr_warp = _ptr(opt(pr_warp, _u8, "pr_warp", (B,)))
    a.gt_warp = 1 if gt_warp else 0
    a.has_dist_clip = 0 if dist_clip is None else 1
    a.dist_clip = 0.0 if dist_clip is None else float(dist_clip)
    a.loss_in_log = 2 if loss_in_log == 'before' else (1 if loss_in_log else 0)
    a.sky_loss_value, a.alpha = float(sky_loss_value), float(alpha)
    return a, keep, (B, V, H, W), dev


def loss_pass(gt_pts, in_camera0, pr_pts, valid, per_pixel=False, **kw):
    """One fused pass (``must3r_hip_metrics_loss``).  ``gt_pts`` [B,V,H,W,3] world points, ``in_camera0`` [B,4,4], ``pr_pts`` [B,V,H,W,3],
    ``valid`` [B,V,H,W]; the optional inputs as ``loss_args`` names them.  Returns ``(counts int64 [B,V,2], sums fp64 [B,V,4])`` on the
    device -- (global, local) and (l global, l local, conf-weighted global, conf-weighted local) -- plus ``(pix_g, pix_l, msk_g, msk_l)``
    with ``per_pixel``."""
    lib = _lib.load()
    a, keep, (B, V, H, W), dev = loss_args(gt_pts, in_camera0, pr_pts, valid, **kw)
    counts = torch.empty((B, V, 2), dtype=torch.int64, device=dev)
    sums = torch.empty((B, V, 4), dtype=torch.float64, device=dev)
    a.counts, a.sums = _ptr(counts), _ptr(sums)
    pix = None
    if per_pixel:
        pix = (torch.empty((B, V, H, W), dtype=torch.float32, device=dev), torch.empty((B, V, H, W), dtype=torch.float32, device=dev),
               torch.empty((B, V, H, W), dtype=torch.uint8, device=dev), torch.empty((B, V, H, W), dtype=torch.uint8, device=dev))
        a.pix_g, a.pix_l, a.msk_g, a.msk_l = (_ptr(t) for t in pix)
    nbytes = lib.must3r_hip_metrics_loss_scratch_bytes(B, V, H, W)
    if not nbytes:
        raise _lib.HipError(lib.must3r_hip_last_error().decode("utf-8", "replace"))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.must3r_hip_metrics_loss(C.byref(a), _ptr(scratch), nbytes, C.c_void_p(_lib.stream_ptr(dev))))
    return (counts, sums) + ((pix,) if per_pixel else ())


def norm_factor(pts, valid, norm_mode='avg_dis', trf=None, return_dist=False):
    """``normalize_pointcloud``'s ``norm_factor`` fp32 [B] of ``pts`` [B, ..., 3] over ``valid`` [B, ...] (all pixels when None),
    ``trf`` [B,4,4] applied first when given (``must3r_hip_metrics_factor``).  ``return_dist`` (``median_dis``): also the distances the
    select ran over, fp32 [B, N], NaN where not selected."""
    lib = _lib.load()
    if norm_mode not in NORM_MODES:
        nm, _, dm = norm_mode.partition('_')
        raise ValueError(f'bad norm_mode={nm!r}' if nm not in ('avg', 'median', 'sqrt') else f'bad dis_mode={dm!r}')
    mode = NORM_MODES[norm_mode]
    pts = _f32(pts, "pts")
    if pts.ndim < 3 or pts.shape[-1] != 3:
        raise ValueError(f"norm_factor: pts {tuple(pts.shape)} must be [B, ..., 3]")
    B = pts.shape[0]
    N = pts[0].numel() // 3
    dev = pts.device
    valid = torch.ones((B, N), dtype=torch.uint8, device=dev) if valid is None else _u8(valid, "valid").reshape(B, -1)
    if valid.shape[1] != N:
        raise ValueError("norm_factor: valid does not match pts")
    trf = None if trf is None else _f32(trf, "trf")
    if trf is not None and tuple(trf.shape) != (B, 4, 4):
        raise ValueError("norm_factor: trf must be [B,4,4]")
    factor = torch.empty((B,), dtype=torch.float32, device=dev)
    dist = torch.empty((B, N), dtype=torch.float32, device=dev) if mode == _lib.NORM_MEDIAN_DIS else None
    nbytes = lib.must3r_hip_metrics_factor_scratch_bytes(B, 1, 1, N, mode)
    if not nbytes:
        raise _lib.HipError(lib.must3r_hip_last_error().decode("utf-8", "replace"))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.must3r_hip_metrics_factor(_ptr(pts), _ptr(trf), _ptr(valid), B, 1, 1, N, mode, _ptr(factor), _ptr(dist),
                                                 _ptr(scratch), nbytes, C.c_void_p(_lib.stream_ptr(dev))))
    return (factor, dist) if return_dist else factor


def eval_metric(gt_pts, in_camera0, pr_pts, valid):
    """eval.py:133-150 for one prediction: ``(counts int64 [B,V], sums fp64 [B,V])`` of ``||geotrf(in_camera0, gt) - pred||`` over the
    valid pixels.  Per-view mean = sum / count; per-scene mean = sum over views / count over views (``reduce_metric``)."""
    counts, sums = loss_pass(gt_pts, in_camera0, pr_pts, valid)
    return counts[..., 0], sums[..., 0]


def reduce_metric(counts, sums):
    """-> (per view [B,V], per scene [B]) float32: the fp64 sum divided by the count, rounded once; NaN where the count is 0."""
    per_view = (sums / counts.to(torch.float64)).to(torch.float32)
    per_scene = (sums.sum(dim=1) / counts.sum(dim=1).to(torch.float64)).to(torch.float32)
    return per_view, per_scene


# ------------------------------------------------------------------------------------------------------------------------------------
# tools/geometry.py and the dust3r leaves, materialising (for callers that want the tensors)
# ------------------------------------------------------------------------------------------------------------------------------------
def geotrf(Trf, pts, ncol=None, norm=False):
    """dust3r.utils.geometry.geotrf for torch tensors: ``pts @ Trf[..., :d, :d]^T + Trf[..., :d, d]`` with ``Trf`` [B,d+1,d+1] broadcast
    over the middle dimensions of ``pts`` [B, ..., d]."""
    _dev(pts, "pts")
    Trf = _dev(Trf, "Trf").to(pts.dtype)
    d = pts.shape[-1]
    lead = Trf.shape[:-2]
    if Trf.shape[-1] != d + 1 or pts.shape[:len(lead)] != lead:
        raise ValueError(f"geotrf: Trf {tuple(Trf.shape)} does not match pts {tuple(pts.shape)}")
    flat = pts.reshape(*lead, -1, d)
    res = flat @ Trf[..., :d, :d].transpose(-1, -2) + Trf[..., None, :d, d]
    if norm:
        res = res / res[..., -1:]
        if norm != 1:
            res = res * norm
    res = res.reshape(pts.shape)
    return res if ncol is None else res[..., :ncol]


def apply_log_to_norm(xyz, dim=-1):
    d = _dev(xyz, "xyz").norm(dim=dim, keepdim=True)
    return xyz / d.clip(min=1e-8) * torch.log1p(d)


def apply_exp_to_norm(xyz, dim=-1):
    d = _dev(xyz, "xyz").norm(dim=dim, keepdim=True)
    return xyz / d.clip(min=1e-8) * torch.expm1(d)


def _warp(pts, valid):
    d = pts.norm(dim=-1, keepdim=True)
    if valid is not None:
        d = torch.where(valid.bool().unsqueeze(-1), d, torch.zeros_like(d))     # invalid_to_zeros
    return pts * (torch.log1p(d) / d.clip(min=1e-8))


def normalize_pointcloud(pts1, pts2, norm_mode='avg_dis', valid1=None, valid2=None, ret_factor=False):
    """tools/geometry.py:21-84.  The factor comes from the device pass (joint over ``pts1`` and ``pts2``); the division materialises."""
    assert pts1.ndim >= 3 and pts1.shape[-1] == 3
    assert pts2 is None or (pts2.ndim >= 3 and pts2.shape[-1] == 3)
    _dev(pts1, "pts1")
    B = pts1.shape[0]
    if pts2 is None:
        allp, allv = pts1, valid1
    else:
        _dev(pts2, "pts2")
        ones = [torch.ones(p.shape[:-1], dtype=torch.bool, device=p.device) if v is None else v.bool() for p, v in ((pts1, valid1), (pts2, valid2))]
        allp = torch.cat((pts1.reshape(B, -1, 3), pts2.reshape(B, -1, 3)), dim=1)
        allv = torch.cat((ones[0].reshape(B, -1), ones[1].reshape(B, -1)), dim=1)
    f = norm_factor(allp, allv, norm_mode)
    if norm_mode == 'avg_warp-log1p':
        pts1 = _warp(pts1, valid1)
        pts2 = None if pts2 is None else _warp(pts2, valid2)
    while f.ndim < pts1.ndim:
        f = f.unsqueeze(-1)
    res = pts1 / f
    if pts2 is not None:
        res = (res, pts2 / f)
    if ret_factor:
        res = (res, f) if not isinstance(res, tuple) else res + (f,)
    return res


# ------------------------------------------------------------------------------------------------------------------------------------
# dust3r.losses, as far as the reference's classes use it
# ------------------------------------------------------------------------------------------------------------------------------------
def Sum(*losses_and_masks):
    loss, mask = losses_and_masks[0]
    if loss.ndim > 0:
        return losses_and_masks                 # the loss of every pixel
    for loss2, mask2 in losses_and_masks[1:]:
        if loss2 is not None:
            loss = loss + loss2
    return loss


class BaseCriterion:
    def __init__(self, reduction='mean'):
        self.reduction = reduction

    def __repr__(self):
        return f'{type(self).__name__}()'


class L21Loss(BaseCriterion):
    """``||a - b||`` per point.  'mean' and 'sum' come out of the fused pass (fp64 sum, rounded once); 'none' asks it for the pixels."""

    def __call__(self, a, b):
        assert a.shape == b.shape and a.ndim >= 2 and a.shape[-1] == 3, f'Bad shape = {a.shape}'
        _no_grad_input(dict(a=a, b=b))
        _dev(a, "a"), _dev(b, "b")
        if self.reduction not in ('none', 'sum', 'mean'):
            raise ValueError(f'bad {self.reduction=} mode')
        n = a.numel() // 3
        if n == 0:
            empty = a.new_zeros(a.shape[:-1], dtype=torch.float32)
            return empty if self.reduction == 'none' else (empty.sum() if self.reduction == 'sum' else empty.mean())
        out = loss_pass(*self.pass_inputs(a, b), per_pixel=self.reduction == 'none')
        return self.pick(out, a.shape[:-1])

    @staticmethod
    def pass_inputs(a, b):
        """``a``, ``b`` [..., 3] as one view of one scene under the identity: the positional inputs of ``loss_pass``."""
        n = a.numel() // 3
        eye = torch.eye(4, dtype=torch.float32, device=a.device)[None]
        valid = torch.ones((1, 1, 1, n), dtype=torch.uint8, device=a.device)
        return b.reshape(1, 1, 1, n, 3), eye, a.reshape(1, 1, 1, n, 3), valid

    def pick(self, out, shape):
        n = torch.Size(shape).numel()
        if self.reduction == 'none':
            return out[2][0].reshape(shape)
        s = out[1][0, 0, 0]
        return (s if self.reduction == 'sum' else s / n).to(torch.float32)


L21 = L21Loss()


class Criterion:
    def __init__(self, criterion=None):
        assert isinstance(criterion, BaseCriterion), f'{criterion} is not a proper criterion!'
        self.criterion = copy(criterion)

    def get_name(self):
        return f'{type(self).__name__}({self.criterion})'

    def with_reduction(self, mode='none'):
        res = loss = deepcopy(self)
        while loss is not None:
            assert isinstance(loss, Criterion)
            loss.criterion.reduction = mode
            loss = loss._loss2
        return res


class MultiLoss:
    """dust3r.losses.MultiLoss as far as Regr3D / ConfLoss use it: ``compute_loss`` -> ``(loss, details)``, and the name the details carry."""

    def __init__(self):
        self._alpha = 1
        self._loss2 = None

    def compute_loss(self, *args, **kwargs):
        raise NotImplementedError()

    def get_name(self):
        raise NotImplementedError()

    def __repr__(self):
        name = self.get_name()
        if self._alpha != 1:
            name = f'{self._alpha:g}*{name}'
        if self._loss2:
            name = f'{name} + {self._loss2}'
        return name

    def __call__(self, *args, **kwargs):
        loss = self.compute_loss(*args, **kwargs)
        if isinstance(loss, tuple):
            loss, details = loss
        elif loss.ndim == 0:
            details = {self.get_name(): float(loss)}
        else:
            details = {}
        loss = loss * self._alpha
        if self._loss2:
            loss2, details2 = self._loss2(*args, **kwargs)
            loss = loss + loss2
            details |= details2
        return loss, details
    forward = __call__


# ------------------------------------------------------------------------------------------------------------------------------------
# must3r/engine/losses.py
# ------------------------------------------------------------------------------------------------------------------------------------
def _ratio(s, c):
    return s / c.to(torch.float64)


class Regr3D(Criterion, MultiLoss):
    def __init__(self, criterion, norm_mode='?avg_dis', sky_loss_value=2, loss_in_log=False):
        Criterion.__init__(self, criterion)
        MultiLoss.__init__(self)
        if not isinstance(criterion, L21Loss):
            raise NotImplementedError("must3r_amd.losses.Regr3D: the fused pass computes L21 only")
        self.loss_in_log = loss_in_log
        if norm_mode.startswith('?'):
            self.norm_all = False               # metric-scale scenes: predictions share the ground truth's factor
            self.norm_mode = norm_mode[1:]
        else:
            self.norm_all = True
            self.norm_mode = norm_mode
        self.sky_loss_value = sky_loss_value

    def _inputs(self, gt, pred):
        _no_grad_input(pred)
        device = _dev(pred['pts3d'], "pred['pts3d']").device
        gt_c2w = torch.stack([b['camera_pose'] for b in gt], dim=1).to(device)
        gt_w2c = torch.linalg.inv(gt_c2w)
        gt_pts3d = torch.stack([b['pts3d'] for b in gt], dim=1).to(device)
        valid = torch.stack([b['valid_mask'] for b in gt], dim=1).to(device)
        sky = torch.stack([b['sky_mask'] for b in gt], dim=1).to(device)
        is_metric = gt[0]['is_metric_scale']
        mask_host = (~is_metric if not self.norm_all else torch.ones_like(is_metric)).cpu()
        return device, gt_w2c, gt_pts3d, valid, sky, mask_host

    def _scales(self, gt_pts3d, in_camera0, pr_pts, valid, mask_host):
        """losses.py:62-79 as per-scene divisors: (gt_scale, pr_scale, pr_warp, gt_warp), None where nothing is normalised."""
        if not self.norm_mode:
            return None, None, None, False
        warp = self.norm_mode == 'avg_warp-log1p'
        gt_scale = norm_factor(gt_pts3d, valid, self.norm_mode, trf=in_camera0)
        mask = mask_host.to(gt_scale.device)
        if bool(mask_host.any()):
            pr_scale = torch.where(mask, norm_factor(pr_pts, valid, self.norm_mode), gt_scale)
        else:
            pr_scale = gt_scale
        return gt_scale, pr_scale, (mask if warp else None), warp

    def fused(self, gt, pred, dist_clip=None, alpha=0.0, per_pixel=False):
        """The device passes behind ``compute_loss``: ``(counts [B,V,2], sums [B,V,4][, pixels])`` of ``loss_pass``."""
        args, kw, _ = self.fused_inputs(gt, pred, dist_clip=dist_clip, alpha=alpha)
        return loss_pass(*args, per_pixel=per_pixel, **kw)

    def fused_inputs(self, gt, pred, dist_clip=None, alpha=0.0):
        """``(args, kw, mask_host)``: the inputs of ``loss_pass`` for this criterion, and the scenes normalised by their own factor."""
        device, gt_w2c, gt_pts3d, valid, sky, mask_host = self._inputs(gt, pred)
        in_camera0 = gt_w2c[:, 0].contiguous()
        pr_pts = _f32(pred['pts3d'], "pred['pts3d']").reshape(gt_pts3d.shape)
        pr_local = pred.get('pts3d_local')
        pr_local = None if pr_local is None else _f32(pr_local, "pred['pts3d_local']").reshape(gt_pts3d.shape)
        conf = pred.get('conf')
        conf = None if conf is None else _f32(conf, "pred['conf']").reshape(gt_pts3d.shape[:-1])
        gt_scale, pr_scale, pr_warp, gt_warp = self._scales(gt_pts3d, in_camera0, pr_pts, valid, mask_host)
        kw = dict(w2c=gt_w2c, pr_local=pr_local, conf=conf, sky=sky if self.sky_loss_value > 0 else None, gt_scale=gt_scale,
                  pr_scale=pr_scale, pr_warp=pr_warp, gt_warp=gt_warp, dist_clip=dist_clip, loss_in_log=self.loss_in_log,
                  sky_loss_value=self.sky_loss_value, alpha=alpha)
        return (gt_pts3d, in_camera0, pr_pts, valid), kw, (mask_host if self.norm_mode else None)

    def get_all_pts3d(self, gt, pred, dist_clip=None):
        """losses.py:22-84, materialised: everything normalised w.r.t. the camera of view 1."""
        device, gt_w2c, gt_pts3d, valid, sky_mask, mask_host = self._inputs(gt, pred)
        in_camera0 = gt_w2c[:, 0]
        gt_pts3d = gt_pts3d.to(torch.float32)
        gt_pts3d_local = geotrf(gt_w2c, gt_pts3d)
        gt_pts = geotrf(in_camera0, gt_pts3d)
        valid = valid.bool()
        if dist_clip is not None:
            valid_g = valid & (gt_pts.norm(dim=-1) <= dist_clip)
            valid_l = valid & (gt_pts3d_local.norm(dim=-1) <= dist_clip)
        else:
            valid_g = valid_l = valid
        pr_pts = pred['pts3d'].detach().clone().reshape(gt_pts.shape)
        pr_pts_local = pred['pts3d_local'].detach().clone().reshape(gt_pts.shape) if 'pts3d_local' in pred else None
        gt_scale, pr_scale, pr_warp, gt_warp = self._scales(gt_pts3d, in_camera0.contiguous(), pr_pts, valid, mask_host)
        if gt_scale is not None:
            bc = (-1, 1, 1, 1, 1)
            if gt_warp:
                gt_pts = _warp(gt_pts, valid)
                pr_pts = torch.where(pr_warp.view(bc), _warp(pr_pts, valid), pr_pts)
            gt_pts, gt_pts3d_local = gt_pts / gt_scale.view(bc), gt_pts3d_local / gt_scale.view(bc)
            pr_pts = pr_pts / pr_scale.view(bc)
            if pr_pts_local is not None:
                pr_pts_local = pr_pts_local / pr_scale.view(bc)
        sky_mask = sky_mask.bool()
        return gt_pts, gt_pts3d_local, pr_pts, pr_pts_local, valid_g, valid_l, sky_mask & ~valid_g, sky_mask & ~valid_l, {}

    def compute_loss(self, gt, pred, **kw):
        if self.sky_loss_value > 0:
            assert self.criterion.reduction == 'none', 'sky_loss_value should be 0 if no conf loss'
        has_local = 'pts3d_local' in pred
        none = self.criterion.reduction == 'none'
        out = self.fused(gt, pred, per_pixel=none, **kw)
        figures = self.figures(out[0], out[1])
        return self.assemble(figures, out[2] if none else None, has_local), self.details(figures, has_local)

    @staticmethod
    def figures(counts, sums):
        """fp32 [4]: the means of the global and of the local term, then their sums."""
        counts, sums = counts.sum(dim=(0, 1)), sums.sum(dim=(0, 1))
        return torch.cat((_ratio(sums[:2], counts).to(torch.float32), sums[:2].to(torch.float32)))

    def details(self, figures, has_local):
        host = figures.tolist()                  # the one device->host read
        self_name = type(self).__name__
        details = {self_name + '_pts3d': host[0]}
        if has_local:
            details[self_name + '_pts3d_local'] = host[1]
        return details

    def assemble(self, figures, pix, has_local):
        if pix is not None:
            pix_g, pix_l, msk_g, msk_l = pix
            msk_g, msk_l = msk_g.bool(), msk_l.bool()
            l1, l2 = pix_g[msk_g], (pix_l[msk_l] if has_local else None)
        else:
            msk_g = msk_l = None
            k = 2 if self.criterion.reduction == 'sum' else 0
            l1, l2 = figures[k], (figures[k + 1] if has_local else None)
        return Sum((l1, msk_g), (l2, msk_l))


class ConfLoss(MultiLoss):
    """Regression weighted by the learned confidence: ``l * conf - alpha * log(conf)``, averaged over the selected pixels of the global
    and of the local term, both sums taken in the same pass as the plain ones."""

    def __init__(self, pixel_loss, alpha=1):
        super().__init__()
        assert alpha > 0
        self.alpha = alpha
        self.pixel_loss = pixel_loss.with_reduction('none')

    def get_name(self):
        return f'ConfLoss({self.pixel_loss})'

    def compute_loss(self, gt, pred, **kw):
        has_local, has_conf = 'pts3d_local' in pred, 'conf' in pred
        counts, sums = self.pixel_loss.fused(gt, pred, alpha=self.alpha, **kw)
        return self.result(self.figures(counts, sums, has_conf), has_local)

    @staticmethod
    def figures(counts, sums, has_conf):
        """fp32 [4]: the plain means of the global and of the local term, then the confidence-weighted ones (the loss's two terms)."""
        counts, sums = counts.sum(dim=(0, 1)), sums.sum(dim=(0, 1))
        plain = _ratio(sums[:2], counts)
        weighted = _ratio(sums[2:], counts) if has_conf else plain
        weighted = torch.where(counts > 0, weighted, torch.zeros_like(weighted))      # nan protection (no selected pixel at all)
        return torch.cat((plain, weighted)).to(torch.float32)

    def result(self, host, has_local):
        values = host.tolist()                   # the one device->host read
        name = type(self.pixel_loss).__name__
        details = dict(conf_loss_g=values[2])
        details[name + '_pts3d'] = values[0]
        if has_local:
            details[name + '_pts3d_local'] = values[1]
            details['conf_loss_l'] = values[3]
        loss = host[2] + host[3] if has_local else host[2]
        return loss, details
