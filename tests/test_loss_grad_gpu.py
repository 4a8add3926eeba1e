"""GPU (-m gpu): the backward pass of the loss family and of the head activation -- csrc/metrics.hip ``must3r_hip_metrics_loss_grad`` and
csrc/misc.hip ``must3r_hip_postprocess_act_grad`` through must3r_amd.train_losses -- against the yardstick tests/metrics_ref.py under
torch autograd on the CPU, fed the fp32 inputs cast to fp64.  For the activation the two formulas are restated here in fp64.

Tolerance, per case and per gradient tensor, not fixed in advance: ``e_gpu`` = max |GPU gradient - fp64 gradient|, ``e_ref`` the same
for the yardstick's own fp32 autograd on the CPU; required ``e_gpu <= 4 e_ref + 32 2^-24 max|g64|``.  Both fp32 paths divide by the
same small distances, so they share the conditioning; the factor 4 covers the differently ordered, equally long fp32 chains (the fused
rigid transform, the inverse's rounding), the floor the cases where the CPU happens to be exact.  Every case's figures are printed
before they are asserted and go, as a table, to the file M3R_LOSS_GRAD_TABLE names (kept as profiles/loss_grad_parity.txt).

The exact conditions (zeros outside the selections, no scale path where the reference detaches, poison, determinism, the forward's
bits, linearity in the upstream scalar) have no tolerance.  Masks for them come from the forward kernel itself (``per_pixel``).
"""
import functools
import os

import pytest
import torch

import metrics_ref as R
from must3r_amd import losses as L
from must3r_amd import train_losses as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
ALPHA = 0.2
NORM_MODES = ['', '?avg_dis', 'avg_dis', '?median_dis', 'median_dis', 'sqrt_dis', 'avg_log1p', '?avg_warp-log1p', 'avg_warp-log1p']
LOGS = [False, True, 'before']
CLIP = 6.0
_rows = []


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    path = os.environ.get("M3R_LOSS_GRAD_TABLE")
    if _rows and path:
        with open(path, "w") as f:
            f.write("# tests/test_loss_grad_gpu.py: per case and gradient tensor, e_gpu = max |GPU - fp64|, e_ref = max |fp32 CPU autograd - fp64|, both in\n"
                    "# units of 2^-24 max|g64|; bound = 4 e_ref + 32; ratio = e_gpu / bound\n")
            f.write(f"{'case':<70}{'tensor':<13}{'max|g64|':>12}{'e_gpu':>10}{'e_ref':>10}{'ratio':>8}\n")
            for r in _rows:
                f.write(f"{r[0]:<70}{r[1]:<13}{r[2]:>12.4e}{r[3]:>10.2f}{r[4]:>10.2f}{r[5]:>8.3f}\n")


def _case(H, W, B=3, V=3, poison=False, metric=(True, False, False), empty_view=(1, 2), **kw):
    return R.make_case(B, V, H, W, H + W, scale=2.0, sky_frac=0.1, metric=list(metric), empty_view=empty_view, poison=poison, **kw)


def _crit(ns, norm_mode, log, kind='conf', reduction='mean'):
    if kind == 'conf':
        return ns.ConfLoss(ns.Regr3D(ns.L21, norm_mode=norm_mode, sky_loss_value=2, loss_in_log=log), alpha=ALPHA)
    return ns.Regr3D(ns.L21Loss(reduction=reduction), norm_mode=norm_mode, sky_loss_value=0, loss_in_log=log)


def _scalar(loss, weights):
    """The scalar a case differentiates: the loss itself, or, for ``reduction='none'``, the per-pixel losses against fixed dense weights."""
    if isinstance(loss, torch.Tensor):
        return loss
    total = 0
    for (l, m), w in zip(loss, weights):
        if l is not None:
            w = w.to(l)
            total = total + (l * w[m.to(w.device)]).sum()
    return total


def _grads(crit, gt, pred, kw, weights=None, scale=1.0):
    leaves = {k: v.clone().requires_grad_(True) for k, v in pred.items()}
    loss, details = crit(gt, leaves, **kw)
    scalar = _scalar(loss, weights)
    (scale * scalar).backward()
    return {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in leaves.items()}, scalar.detach(), details


def _weights(gt, pred):
    g = torch.Generator().manual_seed(11)
    shape = pred['pts3d'].shape[:-1]
    return torch.rand(shape, generator=g) + 0.5, torch.rand(shape, generator=g) + 0.5


@functools.lru_cache(maxsize=None)
def _reference(H, W, norm_mode, log, clip, kind='conf', reduction='mean', local=True, conf=True, B=3, V=3, metric=(True, False, False),
               empty_view=(1, 2)):
    """(gt, pred, g64, g32): the case and the yardstick's gradients in fp64 and in fp32, computed once and shared."""
    gt, pred = _case(H, W, B=B, V=V, local=local, conf=conf, metric=metric, empty_view=empty_view)
    kw = {} if clip is None else dict(dist_clip=clip)
    weights = _weights(gt, pred) if reduction == 'none' else None
    g64 = _grads(_crit(R, norm_mode, log, kind, reduction), R.to64(gt), R.to64(pred), kw, weights)[0]
    g32 = _grads(_crit(R, norm_mode, log, kind, reduction), gt, pred, kw, weights)[0]
    return gt, pred, g64, g32


def _gpu(crit, gt, pred, kw, weights=None, scale=1.0):
    gt_d, pred_d = R.to_device(gt, pred, DEV)
    grads, loss, details = _grads(crit, gt_d, pred_d, kw, None if weights is None else [w.to(DEV) for w in weights], scale)
    return {k: v.cpu() for k, v in grads.items()}, loss.cpu(), details


def _compare(tag, got, g64, g32):
    bad = []
    for k in g64:
        assert got[k].dtype == torch.float32 and got[k].shape == g64[k].shape
        assert bool(torch.isfinite(g64[k]).all()), (tag, k, "the fp64 yardstick is not finite")
        m = float(g64[k].abs().max())
        e_gpu = float((got[k].double() - g64[k]).abs().max())
        e_ref = float((g32[k].double() - g64[k]).abs().max())
        bound = 4 * e_ref + 32 * U * m
        unit = U * m if m > 0 else 1.0
        ratio = e_gpu / bound if bound > 0 else (0.0 if e_gpu == 0 else float('inf'))
        _rows.append((tag, k, m, e_gpu / unit, e_ref / unit, ratio))
        print(f"{tag} {k}: max|g64| {m:.4e} e_gpu {e_gpu / unit:.2f} e_ref {e_ref / unit:.2f} (units of 2^-24 max|g64|) e_gpu / bound {ratio:.3f}")
        if not e_gpu <= bound:
            bad.append((k, e_gpu, e_ref, bound))
    assert not bad, (tag, bad)


def _selections(gt, pred, clip, norm_mode=''):
    """(vg, vl, sel_g, sel_l) bool [B,V,H,W] on the CPU as the forward kernel selects: valid within the clip; those or sky."""
    gt_d, pred_d = R.to_device(gt, pred, DEV)
    kw = {} if clip is None else dict(dist_clip=clip)
    plain = L.Regr3D(L.L21Loss(reduction='none'), norm_mode=norm_mode, sky_loss_value=0).fused(gt_d, pred_d, per_pixel=True, **kw)[2]
    sky = L.Regr3D(L.L21Loss(reduction='none'), norm_mode=norm_mode, sky_loss_value=2).fused(gt_d, pred_d, per_pixel=True, **kw)[2]
    return plain[2].bool().cpu(), plain[3].bool().cpu(), sky[2].bool().cpu(), sky[3].bool().cpu()


# ---------------------------------------------------------------------------------------------------------------------------------
# parity with the yardstick's autograd
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, CLIP])
@pytest.mark.parametrize("log", LOGS, ids=str)
@pytest.mark.parametrize("norm_mode", NORM_MODES)
@pytest.mark.parametrize("H,W", [(7, 13), (33, 37)])
def test_confloss_gradients(H, W, norm_mode, log, clip):
    """(7,13): a tail shorter than one 4-pixel group and unaligned bases; (33,37): two chunks per view.  Scene 0 is metric (no factor of
    its own under '?...'), view (1,2) has no valid pixel, 10 % sky."""
    gt, pred, g64, g32 = _reference(H, W, norm_mode, log, clip)
    kw = {} if clip is None else dict(dist_clip=clip)
    got, _, _ = _gpu(_crit(T, norm_mode, log), gt, pred, kw)
    _compare(f"ConfLoss {H}x{W} norm={norm_mode!r} log={log} clip={clip}", got, g64, g32)


@pytest.mark.parametrize("local,conf", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("norm_mode,log", [('?avg_dis', False), ('avg_warp-log1p', True), ('sqrt_dis', 'before')])
def test_confloss_gradients_pred_variants(norm_mode, log, local, conf):
    gt, pred, g64, g32 = _reference(33, 37, norm_mode, log, CLIP, local=local, conf=conf)
    assert ('pts3d_local' in pred) == local and ('conf' in pred) == conf
    got, _, _ = _gpu(_crit(T, norm_mode, log), gt, pred, dict(dist_clip=CLIP))
    _compare(f"ConfLoss 33x37 norm={norm_mode!r} log={log} local={local} conf={conf}", got, g64, g32)


def test_confloss_gradients_stride_loop():
    """49 152 pixels per view: more than the 32 x 1024 a view's blocks cover in one step."""
    args = (192, 256, '?avg_dis', False, CLIP)
    kw = dict(B=1, V=2, metric=(False,), empty_view=None)
    gt, pred, g64, g32 = _reference(*args, **kw)
    got, _, _ = _gpu(_crit(T, '?avg_dis', False), gt, pred, dict(dist_clip=CLIP))
    _compare("ConfLoss 1x2x192x256 norm='?avg_dis' log=False clip=6.0", got, g64, g32)


@pytest.mark.parametrize("reduction", ['mean', 'sum', 'none'])
@pytest.mark.parametrize("norm_mode,log", [('', False), ('avg_dis', True), ('?avg_log1p', 'before'), ('sqrt_dis', False)])
def test_regr3d_gradients(norm_mode, log, reduction):
    """Regr3D alone (sky_loss_value 0, as the reference asserts without a conf loss).  'none': the dense per-pixel losses are the
    Function's outputs, the gather is torch's, and the backward receives dense per-pixel weights (fixed random ones here)."""
    gt, pred, g64, g32 = _reference(33, 37, norm_mode, log, CLIP, kind='regr', reduction=reduction)
    weights = _weights(gt, pred) if reduction == 'none' else None
    got, _, _ = _gpu(_crit(T, norm_mode, log, 'regr', reduction), gt, pred, dict(dist_clip=CLIP), weights)
    assert float(got['conf'].abs().max()) == 0.0
    _compare(f"Regr3D 33x37 norm={norm_mode!r} log={log} reduction={reduction}", got, g64, g32)


@pytest.mark.parametrize("reduction", ['mean', 'sum', 'none'])
def test_l21_gradients(reduction):
    g = torch.Generator().manual_seed(4)
    a, b, w = torch.randn((5, 11, 3), generator=g), torch.randn((5, 11, 3), generator=g), torch.rand((5, 11), generator=g) + 0.5

    def run(crit, a, b, w):
        a, b = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        out = crit(a, b)
        (out * w).sum().backward() if reduction == 'none' else out.backward()
        return dict(a=a.grad.cpu(), b=b.grad.cpu())
    g64 = run(R.L21Loss(reduction=reduction), a.double(), b.double(), w.double())
    g32 = run(R.L21Loss(reduction=reduction), a, b, w)
    got = run(T.L21Loss(reduction=reduction), a.to(DEV), b.to(DEV), w.to(DEV))
    assert torch.equal(got['b'], -got['a'])
    _compare(f"L21 reduction={reduction}", got, g64, g32)
    half = T.L21(a.to(DEV).half().requires_grad_(True), b.to(DEV))
    assert half.grad_fn is not None


def _act64(raw, activation):
    """engine/inference.py:19-27, tools/geometry.py:14-18 in the dtype of ``raw``."""
    def norm_exp(x):
        d = x.norm(dim=-1, keepdim=True)
        return x / d.clip(min=1e-8) * torch.expm1(d)
    f = norm_exp if activation == 'norm_exp' else (lambda x: x)
    return dict(pts3d=f(raw[..., 0:3]), pts3d_local=f(raw[..., 3:6]), conf=1 + torch.exp(raw[..., 6]))


@pytest.mark.parametrize("activation", ['norm_exp', 'linear'])
def test_chain_raw_head_output_to_loss(activation):
    """raw [2,2,33,37,7] -> activation -> ConfLoss -> backward: raw.grad against the fp64 chain; one raw pixel is exactly 0 in 0:3."""
    gt, _ = _case(33, 37, B=2, V=2, metric=(True, False), empty_view=(1, 1))
    g = torch.Generator().manual_seed(21)
    raw = torch.randn((2, 2, 33, 37, 7), generator=g) * 0.5
    raw[..., 6] = torch.rand((2, 2, 33, 37), generator=g) * 2 - 1
    valid = torch.stack([b['valid_mask'] for b in gt], dim=1)
    where = valid[1, 0].nonzero()[0]
    raw[1, 0, where[0], where[1], 0:3] = 0

    def run(ns, act, raw, gt):
        raw = raw.clone().requires_grad_(True)
        loss, _ = _crit(ns, '?avg_dis', False)(gt, act(raw), dist_clip=CLIP)
        loss.backward()
        return dict(raw=raw.grad.cpu())
    g64 = run(R, lambda r: _act64(r, activation), raw.double(), R.to64(gt))
    g32 = run(R, lambda r: _act64(r, activation), raw, gt)
    got = run(T, lambda r: T.postprocess(r, activation), raw.to(DEV), R.to_device(gt, {}, DEV)[0])
    assert bool(torch.isfinite(got['raw']).all())
    _compare(f"chain {activation} 2x2x33x37", got, g64, g32)


def test_activation_gradient_alone():
    """Both activations against the fp64 formulas with random upstream gradients; a zero vector gets a zero gradient."""
    g = torch.Generator().manual_seed(22)
    raw = torch.randn((3, 7, 13, 7), generator=g)
    raw[0, 0, 0, 0:3] = 0
    ups = dict(pts3d=torch.randn((3, 7, 13, 3), generator=g), pts3d_local=torch.randn((3, 7, 13, 3), generator=g), conf=torch.randn((3, 7, 13), generator=g))
    for activation in ('norm_exp', 'linear'):
        def run(act, raw, ups):
            raw = raw.clone().requires_grad_(True)
            out = act(raw)
            sum((out[k] * ups[k]).sum() for k in ups).backward()
            return dict(raw=raw.grad.cpu())
        g64 = run(lambda r: _act64(r, activation), raw.double(), {k: v.double() for k, v in ups.items()})
        g32 = run(lambda r: _act64(r, activation), raw, ups)
        got = run(lambda r: T.postprocess(r, activation), raw.to(DEV), {k: v.to(DEV) for k, v in ups.items()})
        if activation == 'norm_exp':
            assert float(got['raw'][0, 0, 0, 0:3].abs().max()) == 0.0
        _compare(f"activation {activation} 3x7x13", got, g64, g32)


# ---------------------------------------------------------------------------------------------------------------------------------
# exact conditions
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(7, 13), (33, 37)])
@pytest.mark.parametrize("norm_mode", ['', '?avg_dis', 'median_dis', 'avg_dis'])
def test_zeros_outside_the_selections(H, W, norm_mode):
    gt, pred = _case(H, W)
    vg, vl, sel_g, sel_l = _selections(gt, pred, CLIP, norm_mode)
    valid = torch.stack([b['valid_mask'] for b in gt], dim=1)
    got, _, _ = _gpu(_crit(T, norm_mode, False), gt, pred, dict(dist_clip=CLIP))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert float(got['conf'][~(sel_g | sel_l)].abs().max()) == 0.0                       # unselected pixels
    assert float(got['pts3d_local'][~vl].abs().max()) == 0.0                             # sky pixels included
    assert float(got['pts3d'][~valid].abs().max()) == 0.0                                # unselected and pure sky pixels
    assert bool((sel_g & ~vg).any()) and bool((valid & ~vg).any())
    no_scale_path = {'': [0, 1, 2], '?avg_dis': [0], 'median_dis': [0, 1, 2], 'avg_dis': []}[norm_mode]
    for b in range(3):
        beyond = got['pts3d'][b][valid[b] & ~vg[b]]
        assert beyond.numel() > 0
        if b in no_scale_path:                                                           # metric scene under '?', detached median, no norm
            assert float(got['pts3d'][b][~vg[b]].abs().max()) == 0.0
        else:                                                                            # the scale path reaches valid pixels beyond the clip
            assert bool((beyond.abs().sum(dim=-1) > 0).all())
    assert float(got['pts3d'][1, 2].abs().max()) == 0.0 and float(got['pts3d_local'][1, 2].abs().max()) == 0.0   # the view without a valid pixel
    assert not bool(valid[1, 2].any())
    assert float(got['conf'][1, 2][~sel_g[1, 2]].abs().max()) == 0.0


def test_zero_residual_gives_zero_point_gradients():
    """Identity poses, no normalisation, pred == gt bitwise: l = 0, the point gradients are exactly 0 and everything is finite."""
    gt, pred = _case(33, 37)
    eye = torch.eye(4).repeat(3, 1, 1)
    for b in gt:
        b['camera_pose'] = eye.clone()
    world = torch.stack([b['pts3d'] for b in gt], dim=1)
    pred['pts3d'], pred['pts3d_local'] = world.clone(), world.clone()
    got, loss, _ = _gpu(_crit(T, '', False), gt, pred, {})
    assert all(bool(torch.isfinite(v).all()) for v in got.values()) and bool(torch.isfinite(loss))
    assert float(got['pts3d'].abs().max()) == 0.0 and float(got['pts3d_local'].abs().max()) == 0.0
    assert float(got['conf'].abs().max()) > 0.0


@pytest.mark.parametrize("norm_mode", ['avg_dis', 'sqrt_dis'])
def test_zero_prediction_point_is_finite(norm_mode):
    gt, pred = _case(7, 13)
    valid = torch.stack([b['valid_mask'] for b in gt], dim=1)
    where = valid.nonzero()[:3]
    for i in where:
        pred['pts3d'][tuple(i)] = 0
    got, loss, _ = _gpu(_crit(T, norm_mode, True), gt, pred, {})
    assert all(bool(torch.isfinite(v).all()) for v in got.values()) and bool(torch.isfinite(loss))


@pytest.mark.parametrize("norm_mode,log", [('?avg_dis', False), ('avg_warp-log1p', True)])
def test_poison_determinism_forward_bits_and_linearity(norm_mode, log):
    gt, pred = _case(33, 37)
    kw = dict(dist_clip=CLIP)
    crit = _crit(T, norm_mode, log)
    got, loss, details = _gpu(crit, gt, pred, kw)
    # ground truth is never read outside valid: NaN / inf there changes no bit
    gt_p, pred_p = _case(33, 37, poison=True)
    assert bool(torch.stack([b['pts3d'] for b in gt_p], dim=1).isnan().any())
    got_p, loss_p, details_p = _gpu(crit, gt_p, pred_p, kw)
    assert all(bool(torch.isfinite(v).all()) for v in got_p.values())
    assert all(torch.equal(got[k], got_p[k]) for k in got) and torch.equal(loss, loss_p) and details == details_p
    # the same call twice: the same bits
    again, loss_a, _ = _gpu(crit, gt, pred, kw)
    assert all(torch.equal(got[k], again[k]) for k in got) and torch.equal(loss, loss_a)
    # the forward is that of must3r_amd.losses
    gt_d, pred_d = R.to_device(gt, pred, DEV)
    loss_f, details_f = _crit(L, norm_mode, log)(gt_d, pred_d, **kw)
    assert torch.equal(loss, loss_f.cpu()) and details == details_f and list(details) == list(details_f)
    # inputs that do not require grad take the forward-only route
    loss_n, details_n = crit(gt_d, pred_d, **kw)
    assert loss_n.grad_fn is None and torch.equal(loss_n.cpu(), loss) and details_n == details
    # linear in the upstream scalar to 1 ulp
    tripled, _, _ = _gpu(crit, gt, pred, kw, scale=3.0)
    for k in got:
        a, b = tripled[k], 3 * got[k]
        assert bool(((a == 0) == (b == 0)).all()) and bool((torch.sign(a) == torch.sign(b)).all())
        nz = b != 0
        assert int((a[nz].view(torch.int32) - b[nz].view(torch.int32)).abs().max()) <= 1, k


def test_dtypes_second_order_and_cpu():
    gt, pred = _case(7, 13)
    gt_d, pred_d = R.to_device(gt, pred, DEV)
    leaves = dict(pts3d=pred_d['pts3d'].half().requires_grad_(True), pts3d_local=pred_d['pts3d_local'].double().requires_grad_(True),
                  conf=pred_d['conf'].clone().requires_grad_(True))
    crit = _crit(T, '?avg_dis', False)
    loss, _ = crit(gt_d, leaves)
    assert loss.grad_fn is not None and loss.dtype == torch.float32
    grads = torch.autograd.grad(loss * loss, list(leaves.values()), create_graph=True)     # the upstream gradient 2 loss depends on the leaves
    assert [g.dtype for g in grads] == [torch.float16, torch.float64, torch.float32]
    assert [g.shape for g in grads] == [v.shape for v in leaves.values()]
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):
        grads[0].float().sum().backward()
    raw = torch.randn((7, 13, 7), device=DEV, requires_grad=True)
    out = T.postprocess(raw, 'norm_exp')
    g, = torch.autograd.grad((out['pts3d'] ** 2).sum(), raw, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):
        g.sum().backward()
    with pytest.raises(NotImplementedError):
        T.postprocess(raw, 'norm_exp', compute_cam=True)
