"""Yardstick of the checkpoint evaluation: the reference's eval.py loss loop, tools/geometry.py ``normalize_pointcloud`` and
engine/losses.py ``Regr3D`` / ``ConfLoss`` restated in torch, written from the reference's text (line numbers below) and from nothing
of must3r_amd.  Every function takes the tensors in whatever dtype it is given: fed fp32 inputs cast to fp64 (``to64``) it is the fp64
reference the tests compare against; fed fp32 it is what eval.py / train.py compute on the CPU.

The leaves the reference takes from dust3r are restated here from their call sites (dust3r is not a dependency and not on the build
machine, so parity with it is unpinned -- DESIGN.md section 5): ``L21`` = mean (or per point, ``reduction='none'``) of ``||a - b||``;
``geotrf`` = ``pts @ R^T + t``; ``invalid_to_zeros`` / ``invalid_to_nans``; ``Criterion.with_reduction`` / ``MultiLoss`` / ``Sum``.
"""
import math
from copy import copy, deepcopy

import numpy as np
import torch


def to64(x):
    if isinstance(x, torch.Tensor):
        return x.double() if x.is_floating_point() else x
    if isinstance(x, dict):
        return {k: to64(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(to64(v) for v in x)
    return x


# ---- dust3r leaves ---------------------------------------------------------------------------------------------------------------
def geotrf(Trf, pts, ncol=None, norm=False):
    """dust3r.utils.geometry.geotrf for tensors: Trf [..., d+1, d+1] applied to pts [..., (middle dims), d]."""
    d = pts.shape[-1]
    lead = Trf.ndim - 2
    flat = pts.reshape(*pts.shape[:lead], -1, d)
    res = flat @ Trf[..., :d, :d].transpose(-1, -2) + Trf[..., None, :d, d]
    assert not norm
    res = res.reshape(pts.shape)
    return res if ncol is None else res[..., :ncol]


def invalid_to_nans(arr, valid_mask, ndim=999):
    if valid_mask is not None:
        arr = arr.clone()
        arr[~valid_mask] = float('nan')
    if arr.ndim > ndim:
        arr = arr.flatten(-2 - (arr.ndim - ndim), -2)
    return arr


def invalid_to_zeros(arr, valid_mask, ndim=999):
    if valid_mask is not None:
        arr = arr.clone()
        arr[~valid_mask] = 0
        nnz = valid_mask.view(len(valid_mask), -1).sum(1)
    else:
        nnz = arr.numel() // len(arr) if len(arr) else 0
    if arr.ndim > ndim:
        arr = arr.flatten(-2 - (arr.ndim - ndim), -2)
    return arr, nnz


class BaseCriterion(torch.nn.Module):
    def __init__(self, reduction='mean'):
        super().__init__()
        self.reduction = reduction


class L21Loss(BaseCriterion):
    """``torch.norm(a - b, dim=-1)``; the mean of an empty selection is NaN, as ``torch.mean`` gives it."""

    def forward(self, a, b):
        assert a.shape == b.shape and a.ndim >= 2 and 1 <= a.shape[-1] <= 3, f'Bad shape = {a.shape}'
        dist = torch.norm(a - b, dim=-1)
        if self.reduction == 'none':
            return dist
        if self.reduction == 'sum':
            return dist.sum()
        assert self.reduction == 'mean'
        return dist.mean()


L21 = L21Loss()


def Sum(*losses_and_masks):
    loss, mask = losses_and_masks[0]
    if loss.ndim > 0:
        return losses_and_masks
    for loss2, mask2 in losses_and_masks[1:]:
        loss = loss + loss2
    return loss


class Criterion(torch.nn.Module):
    def __init__(self, criterion=None):
        super().__init__()
        assert isinstance(criterion, BaseCriterion)
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


class MultiLoss(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self._alpha = 1
        self._loss2 = None

    def compute_loss(self, *args, **kwargs):
        raise NotImplementedError()

    def get_name(self):
        raise NotImplementedError()

    def forward(self, *args, **kwargs):
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


# ---- must3r/tools/geometry.py ------------------------------------------------------------------------------------------------------
def apply_log_to_norm(xyz, dim=-1):                   # :7-11
    d = xyz.norm(dim=dim, keepdim=True)
    xyz = xyz / d.clip(min=1e-8)
    return xyz * torch.log1p(d)


def normalize_pointcloud(pts1, pts2, norm_mode='avg_dis', valid1=None, valid2=None, ret_factor=False):   # :21-84
    assert pts1.ndim >= 3 and pts1.shape[-1] == 3
    assert pts2 is None or (pts2.ndim >= 3 and pts2.shape[-1] == 3)
    norm_mode, dis_mode = norm_mode.split('_')
    if norm_mode == 'avg':
        nan_pts1, nnz1 = invalid_to_zeros(pts1, valid1, ndim=3)
        nan_pts2, nnz2 = invalid_to_zeros(pts2, valid2, ndim=3) if pts2 is not None else (None, 0)
        all_pts = torch.cat((nan_pts1, nan_pts2), dim=1) if pts2 is not None else nan_pts1
        all_dis = all_pts.norm(dim=-1)
        if dis_mode == 'dis':
            pass
        elif dis_mode == 'log1p':
            all_dis = torch.log1p(all_dis)
        elif dis_mode == 'warp-log1p':
            log_dis = torch.log1p(all_dis)
            warp_factor = log_dis / all_dis.clip(min=1e-8)
            H1, W1 = pts1.shape[1:-1]
            pts1 = pts1 * warp_factor[:, :W1 * H1].view(-1, H1, W1, 1)
            if pts2 is not None:
                H2, W2 = pts2.shape[1:-1]
                pts2 = pts2 * warp_factor[:, W1 * H1:].view(-1, H2, W2, 1)
            all_dis = log_dis
        else:
            raise ValueError(f'bad {dis_mode=}')
        norm_factor = all_dis.sum(dim=1) / (nnz1 + nnz2 + 1e-8)
    else:
        nan_pts1 = invalid_to_nans(pts1, valid1, ndim=3)
        nan_pts2 = invalid_to_nans(pts2, valid2, ndim=3) if pts2 is not None else None
        all_pts = torch.cat((nan_pts1, nan_pts2), dim=1) if pts2 is not None else nan_pts1
        all_dis = all_pts.norm(dim=-1)
        if norm_mode == 'median':
            norm_factor = all_dis.nanmedian(dim=1).values.detach()
        elif norm_mode == 'sqrt':
            norm_factor = all_dis.sqrt().nanmean(dim=1) ** 2
        else:
            raise ValueError(f'bad {norm_mode=}')
    norm_factor = norm_factor.clip(min=1e-8)
    while norm_factor.ndim < pts1.ndim:
        norm_factor = norm_factor.unsqueeze(-1)
    res = pts1 / norm_factor
    if pts2 is not None:
        res = (res, pts2 / norm_factor)
    if ret_factor:
        res = (res, norm_factor) if not isinstance(res, tuple) else res + (norm_factor,)
    return res


def _normalize_views(pts, norm_mode, valid):
    """losses.py:69 / :75 call normalize_pointcloud on [b, nimgs, H, W, 3] with ``pts2=None``: the warp branch's ``H1, W1 =
    pts1.shape[1:-1]`` only unpacks for 4-d input, so the views are folded into the rows first (same pixels, same order)."""
    b, n, H, W, _ = pts.shape
    res, f = normalize_pointcloud(pts.reshape(b, n * H, W, 3), None, norm_mode, valid.reshape(b, n * H, W), None, ret_factor=True)
    return res.reshape(pts.shape), f.reshape(b, 1, 1, 1, 1)


# ---- must3r/engine/losses.py -------------------------------------------------------------------------------------------------------
class Regr3D(Criterion, MultiLoss):
    def __init__(self, criterion, norm_mode='?avg_dis', sky_loss_value=2, loss_in_log=False):   # :10-20
        super().__init__(criterion)
        self.loss_in_log = loss_in_log
        if norm_mode.startswith('?'):
            self.norm_all = False
            self.norm_mode = norm_mode[1:]
        else:
            self.norm_all = True
            self.norm_mode = norm_mode
        self.sky_loss_value = sky_loss_value

    def get_all_pts3d(self, gt, pred, dist_clip=None):   # :22-84
        gt_c2w = torch.stack([b['camera_pose'] for b in gt], dim=1)
        gt_w2c = torch.linalg.inv(gt_c2w)
        in_camera0 = gt_w2c[:, 0]
        gt_pts3d = torch.stack([b['pts3d'] for b in gt], dim=1)
        gt_pts3d_local = geotrf(gt_w2c, gt_pts3d)
        gt_pts = geotrf(in_camera0, gt_pts3d)
        valid = torch.stack([b['valid_mask'] for b in gt], dim=1).clone()
        is_metric_scale = gt[0]['is_metric_scale'].clone()
        sky_mask = torch.stack([b['sky_mask'] for b in gt], dim=1).clone()
        if dist_clip is not None:
            valid_g = valid & (gt_pts.norm(dim=-1) <= dist_clip)
            valid_l = valid & (gt_pts3d_local.norm(dim=-1) <= dist_clip)
        else:
            valid_g = valid_l = valid
        pr_pts = pred['pts3d'].clone()
        pr_pts_local = pred['pts3d_local'].clone() if 'pts3d_local' in pred else None
        mask = ~is_metric_scale if not self.norm_all else torch.ones_like(is_metric_scale)
        if self.norm_mode and mask.any():
            pr_pts[mask], norm_factor_pred = _normalize_views(pr_pts[mask], self.norm_mode, valid[mask])
            if pr_pts_local is not None:
                pr_pts_local[mask] = pr_pts_local[mask] / norm_factor_pred
        if self.norm_mode:
            gt_pts, norm_factor = _normalize_views(gt_pts, self.norm_mode, valid)
            gt_pts3d_local = gt_pts3d_local / norm_factor
            pr_pts[~mask] = pr_pts[~mask] / norm_factor[~mask]
            if pr_pts_local is not None:
                pr_pts_local[~mask] = pr_pts_local[~mask] / norm_factor[~mask]
        sky_g = sky_mask & (~valid_g)
        sky_l = sky_mask & (~valid_l)
        return gt_pts, gt_pts3d_local, pr_pts, pr_pts_local, valid_g, valid_l, sky_g, sky_l, {}

    def compute_loss(self, gt, pred, **kw):               # :86-127
        gt_pts, gt_pts3d_local, pred_pts, pred_pts_local, mask_g, mask_l, sky_g, sky_l, monitoring = self.get_all_pts3d(gt, pred, **kw)
        if self.sky_loss_value > 0:
            assert self.criterion.reduction == 'none', 'sky_loss_value should be 0 if no conf loss'
            mask_g = mask_g | sky_g
            mask_l = mask_l | sky_l
        gt_pts = gt_pts[mask_g]
        if self.loss_in_log:
            gt_pts = apply_log_to_norm(gt_pts, dim=-1)
            pred_pts = apply_log_to_norm(pred_pts, dim=-1)
        pred_pts_m = pred_pts[mask_g]
        l1 = self.criterion(pred_pts_m, gt_pts)
        if pred_pts_local is not None:
            pred_pts_local = pred_pts_local[mask_l]
            gt_pts3d_local = gt_pts3d_local[mask_l]
            if self.loss_in_log and self.loss_in_log != 'before':
                gt_pts3d_local = apply_log_to_norm(gt_pts3d_local, dim=-1)
                pred_pts_local = apply_log_to_norm(pred_pts_local, dim=-1)
            l2 = self.criterion(pred_pts_local, gt_pts3d_local)
        else:
            l2 = None
        if self.sky_loss_value > 0:
            sky_value = torch.as_tensor(self.sky_loss_value, dtype=l1.dtype)
            l1 = torch.where(sky_g[mask_g], sky_value, l1)
            if l2 is not None:
                l2 = torch.where(sky_l[mask_l], sky_value, l2)
        self_name = type(self).__name__
        details = {self_name + '_pts3d': float(l1.mean())}
        if l2 is not None:
            details[self_name + '_pts3d_local'] = float(l2.mean())
        return Sum((l1, mask_g), (l2, mask_l)), (details | monitoring)


class ConfLoss(MultiLoss):
    def __init__(self, pixel_loss, alpha=1):              # :141-145
        super().__init__()
        assert alpha > 0
        self.alpha = alpha
        self.pixel_loss = pixel_loss.with_reduction('none')

    def get_name(self):
        return f'ConfLoss({self.pixel_loss})'

    def compute_loss(self, gt, pred, **kw):               # :153-186
        ((loss_g, msk_g), (loss_l, msk_l)), details = self.pixel_loss(gt, pred, **kw)
        if 'conf' not in pred:
            conf_loss_g = loss_g.mean() if loss_g.numel() > 0 else 0
            if loss_l is not None:
                conf_loss_l = loss_l.mean() if loss_l.numel() > 0 else 0
            else:
                conf_loss_l = 0
        else:
            conf_g = pred['conf'][msk_g]
            conf_loss_g = loss_g * conf_g - self.alpha * torch.log(conf_g)
            conf_loss_g = conf_loss_g.mean() if conf_loss_g.numel() > 0 else 0
            if loss_l is not None:
                conf_l = pred['conf'][msk_l]
                conf_loss_l = loss_l * conf_l - self.alpha * torch.log(conf_l)
                conf_loss_l = conf_loss_l.mean() if conf_loss_l.numel() > 0 else 0
            else:
                conf_loss_l = 0
        details_conf = dict(conf_loss_g=float(conf_loss_g), **details)
        if loss_l is not None:
            details_conf['conf_loss_l'] = float(conf_loss_l)
        return conf_loss_g + conf_loss_l, details_conf


# ---- eval.py -----------------------------------------------------------------------------------------------------------------------
def eval_schedule(num_views_dec, num_views_all, init_num_views, batch_num_views, render_once):
    """eval.py:116-124 -> (mem_batches, to_render)."""
    mem_batches = [min(init_num_views, num_views_dec)]
    while (sum_b := sum(mem_batches)) != num_views_dec:
        mem_batches.append(min(batch_num_views, num_views_dec - sum_b))
    to_render = list(range(num_views_dec, num_views_all)) if render_once else None
    return mem_batches, to_render


def eval_batch_losses(views, x_out_0, x_out, criterion=L21):
    """eval.py:100-150 for one batch: ``views`` the list of per-view dicts, ``x_out_0`` [B, num_views_dec, H, W, 3] or None, ``x_out``
    [B, num_views_all, H, W, 3].  Returns (first pass [num_views_dec][B], per image [num_views_all][B], global [B]) as lists of 0-dim
    tensors in the dtype of the inputs."""
    gt_c2w = torch.stack([b['camera_pose'] for b in views], dim=1)
    gt_w2c = torch.linalg.inv(gt_c2w)
    in_camera0 = gt_w2c[:, 0]
    gt_pts = torch.stack([b['pts3d'] for b in views], dim=1)
    gt_pts = geotrf(in_camera0, gt_pts)
    gt_valid = torch.stack([b['valid_mask'] for b in views], dim=1)
    B, num_views_all = gt_valid.shape[:2]
    first, imgs = [], [[] for _ in range(num_views_all)]
    if x_out_0 is not None:
        first = [[] for _ in range(x_out_0.shape[1])]
        for b in range(B):
            for i in range(x_out_0.shape[1]):
                first[i].append(criterion(gt_pts[b, i][gt_valid[b, i]], x_out_0[b, i][gt_valid[b, i]]))
    for b in range(B):
        for i in range(num_views_all):
            imgs[i].append(criterion(gt_pts[b, i][gt_valid[b, i]], x_out[b, i][gt_valid[b, i]]))
    glob = [criterion(gt_pts[b][gt_valid[b]], x_out[b][gt_valid[b]]) for b in range(B)]
    return first, imgs, glob


def result_str(num_views_dec, losses_firstpass, losses_imgs, losses_all):
    """eval.py:152-159 on lists of float32 scalars."""
    s = f'{num_views_dec=}\n'
    if len(losses_firstpass) > 0 and len(losses_firstpass[0]) > 0:
        for i in range(num_views_dec):
            s += f'first pass {i} - mean = {np.mean(losses_firstpass[i])}, median = {np.median(losses_firstpass[i])}\n'
    for i in range(len(losses_imgs)):
        s += f'{i} - mean = {np.mean(losses_imgs[i])}, median = {np.median(losses_imgs[i])}\n'
    s += f'global - mean = {np.mean(losses_all)}, median = {np.median(losses_all)}\n'
    return s


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def random_rigid(g, n, scale=1.0):
    q, _ = torch.linalg.qr(torch.randn((n, 3, 3), generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.linalg.det(q)).view(n, 1, 1)
    T = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    T[:, :3, :3] = q
    T[:, :3, 3] = torch.randn((n, 3), generator=g, dtype=torch.float64) * scale
    return T.float()


def make_case(B, V, H, W, seed, scale=1.0, valid_frac=0.7, sky_frac=0.0, local=True, conf=True, metric=None, poison=False, ties=False,
              empty_view=None, full_view=None):
    """Seeded ground truth and prediction in the reference's formats: ``gt`` a list of V dicts (camera_pose [B,4,4], pts3d [B,H,W,3]
    world, valid_mask, sky_mask [B,H,W] bool, is_metric_scale [B] bool), ``pred`` a dict (pts3d, pts3d_local [B,V,H,W,3], conf
    [B,V,H,W] > 1).  ``poison``: NaN / inf ground truth under the mask; ``ties``: coordinates on a coarse grid, so many distances tie."""
    g = torch.Generator().manual_seed(seed)
    c2w = random_rigid(g, B * V, scale).view(B, V, 4, 4)
    local_pts = torch.randn((B, V, H, W, 3), generator=g) * scale
    local_pts[..., 2] = local_pts[..., 2].abs() + 0.5 * scale
    if ties:
        local_pts = torch.round(local_pts * 2) / 2
    world = geotrf(c2w, local_pts)
    if ties:
        world = torch.round(world * 2) / 2
    valid = torch.rand((B, V, H, W), generator=g) < valid_frac
    sky = (torch.rand((B, V, H, W), generator=g) < sky_frac) & ~valid if sky_frac > 0 else torch.zeros_like(valid)
    if sky_frac > 0:                                     # some labelled sky pixels also carry 3-d points (losses.py:81-83)
        sky |= (torch.rand((B, V, H, W), generator=g) < 0.02) & valid
    if empty_view is not None:
        valid[empty_view] = False
    if full_view is not None:
        valid[full_view] = True
    bad = torch.rand((B, V, H, W), generator=g)          # drawn whether used or not: poison changes nothing else of a case
    if poison:
        world = world.clone()
        world[(bad < 0.3) & ~valid] = float('nan')
        world[(bad > 0.7) & ~valid] = float('inf')
    w2c = torch.linalg.inv(c2w.double())
    in_cam0 = w2c[:, :1]
    pr = (geotrf((in_cam0 @ c2w.double()).float(), local_pts) + 0.05 * scale * torch.randn((B, V, H, W, 3), generator=g)) * 1.3
    metric = torch.zeros(B, dtype=torch.bool) if metric is None else torch.as_tensor(metric, dtype=torch.bool)
    gt = [dict(camera_pose=c2w[:, v].contiguous(), pts3d=world[:, v].contiguous(), valid_mask=valid[:, v].contiguous(),
               sky_mask=sky[:, v].contiguous(), is_metric_scale=metric) for v in range(V)]
    pred = dict(pts3d=pr.contiguous())
    if local:
        pred['pts3d_local'] = ((local_pts + 0.05 * scale * torch.randn((B, V, H, W, 3), generator=g)) * 1.3).contiguous()
    if conf:
        pred['conf'] = 1.0 + torch.exp(torch.randn((B, V, H, W), generator=g))
    return gt, pred


def scene_of(gt, pred, k):
    """Scene ``k`` of a batch as a batch of one."""
    gt1 = [{key: v[k:k + 1].clone() for key, v in b.items()} for b in gt]
    return gt1, {key: v[k:k + 1].clone() for key, v in pred.items()}


def to_device(gt, pred, device):
    return [{k: v.to(device) for k, v in b.items()} for b in gt], {k: v.to(device) for k, v in pred.items()}


def max_abs(gt, pred):
    """Largest finite absolute coordinate or translation of a case: the ``S`` of the tolerance."""
    vals = []
    for b in gt:
        p = b['pts3d'][b['valid_mask']]
        vals += [p.abs().max() if p.numel() else torch.tensor(0.0), b['camera_pose'][:, :3].abs().max()]
    vals += [pred['pts3d'].abs().max()] + ([pred['pts3d_local'].abs().max()] if 'pts3d_local' in pred else [])
    return float(torch.stack([v.double() for v in vals]).max())


# ---- tolerance ---------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24          # unit roundoff of fp32
OPS_L21 = 9             # rigid transform: the fp32 inverse's own rounding (1) and a 4-term dot product per component (4); difference (1);
                        # norm: squares, sums, sqrt (3)
OPS_SCALE = 2           # the factor's own rounding to fp32 and the division by it
OPS_WARP = 4            # norm, log1p, the quotient log1p(d) / d, the product
OPS_LOG = 4             # apply_log_to_norm: norm, log1p, quotient, product
LIBM_MARGIN = 2.0       # log1p / log of the device (and of the CPU's libm) are not correctly rounded


def min_factor(gt, pred, norm_mode):
    """Smallest norm_factor (fp64 restatement) a case is divided by: ground truth and prediction, all scenes."""
    mode = norm_mode[1:] if norm_mode.startswith('?') else norm_mode
    if not mode:
        return 1.0
    gt64, pred64 = to64(gt), to64(pred)
    w2c = torch.linalg.inv(torch.stack([b['camera_pose'] for b in gt64], dim=1))
    gt_pts = geotrf(w2c[:, 0], torch.stack([b['pts3d'] for b in gt64], dim=1))
    valid = torch.stack([b['valid_mask'] for b in gt64], dim=1)
    f = torch.cat([_normalize_views(p, mode, valid)[1].flatten() for p in (gt_pts, pred64['pts3d'])])
    f = f[~f.isnan()]
    return float(f.min()) if f.numel() else 1.0


def tolerance(S, scaled=False, warp=False, log=False, factor=1.0, conf_max=None, alpha=0.0, libm=None):
    """Bound on |fp32 figure - fp64 figure| for a mean of per-pixel L21 losses, from the roundings on the path alone (the fp64
    accumulation adds nothing at these sizes).  Every fp32 operation on the path contributes at most ``U`` times the magnitude of what
    it produces, and nothing on the path exceeds ``S_eff = S / factor``: ``S`` is the largest absolute coordinate or translation of the
    case (the fused transform cancels translations, so the error is absolute in the scene's scale and not relative to the loss),
    ``factor`` the smallest normalisation factor.  The norm, the log map (its derivative is at most 1) and the mean are 1-Lipschitz,
    so the per-pixel bound ``n_ops U S_eff`` holds for the mean: a mean is no further off than its worst pixel.  With ``conf_max`` the
    figure is ``l c - alpha log c``: ``c`` times the bound on ``l`` plus three roundings of magnitudes ``c l`` and ``alpha |log c|``, with
    ``l <= 2 sqrt(3) S_eff``.  Figures that go through log1p / log carry the margin ``LIBM_MARGIN``."""
    ops = OPS_L21 + (OPS_SCALE if scaled else 0) + (OPS_WARP if warp else 0) + (OPS_LOG if log else 0)
    s_eff = S / factor
    b = ops * U * s_eff
    uses_libm = (warp or log or conf_max is not None) if libm is None else libm
    if conf_max is not None:
        b = conf_max * b + 3 * U * (conf_max * 2 * math.sqrt(3) * s_eff + alpha * abs(math.log(conf_max)))
    return b * (LIBM_MARGIN if uses_libm else 1.0)


def factor_tolerance(S, mode):
    """The same reasoning for normalize_pointcloud's factor: transform (5) + norm (3) + the final rounding (1), + 2 for log1p / sqrt and
    for the square of sqrt_dis; the median is an order statistic, 1-Lipschitz in the sup norm of the distances."""
    extra = {'avg_dis': 0, 'median_dis': 0, 'avg_log1p': 2, 'avg_warp-log1p': 2, 'sqrt_dis': 4}[mode]
    return (9 + extra) * U * S * (LIBM_MARGIN if 'log1p' in mode else 1.0)
