"""GPU (-m gpu): the checkpoint evaluation -- csrc/metrics.hip through must3r_amd.losses and must3r_amd.evaluate -- against the fp64
yardstick tests/metrics_ref.py (pinned to the reference's own text by tests/test_metrics_host.py).  Nothing of the reference is read.

Tolerance (``metrics_ref.tolerance`` / ``factor_tolerance``), derived and not tuned: kernel and yardstick see the same fp32 inputs, the
kernel accumulates in fp64, so the only differences are the fp32 roundings per pixel.  Every fp32 operation contributes at most
``2^-24`` times the magnitude of its result, and no intermediate exceeds ``S_eff = S / factor`` -- ``S`` the largest absolute
coordinate or translation of the case (the fused rigid transform cancels translations, so the error is absolute in the scene's scale,
not relative to the loss), ``factor`` the smallest normalisation factor of the case (fp64 yardstick).  Operations on the path:
transform 5 (the fp32 4x4 inverse's rounding, then a 4-term dot product per component), difference 1, norm 3 -> 9 for eval.py's plain
metric; +2 when scaled (the factor's
rounding, the division); +4 with the warp (norm, log1p, quotient, product); +4 with the log map.  Norm, log map and mean are
1-Lipschitz, so ``n_ops 2^-24 S_eff`` bounds every per-pixel loss and therefore every mean.  A conf-weighted figure ``l c - alpha log c``
gets ``c_max`` times that plus three roundings of ``c_max l_max`` and ``alpha log c_max``.  Paths through the device's log1p / log,
which are not correctly rounded, are asserted with a margin of 2.  The same bound holds for the reference's own fp32 arithmetic on
the CPU (tests/test_metrics_host.py asserts it; observed ratios there: 0.009 for eval.py's samples, 0.012 for Regr3D / ConfLoss, 0.12
for the factors), so it is a property of the number format, not of the code under test.
"""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import metrics_ref as R
from must3r_amd import _lib
from must3r_amd import evaluate as E
from must3r_amd import losses as L
from must3r_amd.synthetic import SyntheticScenes

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _close(tag, got, want, bound):
    """a NaN expected is a NaN asserted"""
    got, want = float(got), float(want)
    print(f"{tag}: got {got!r} want {want!r} |diff| / bound = {abs(got - want) / bound if want == want else float('nan'):.4f}")
    if want != want:
        assert got != got, (tag, got, want)
    else:
        assert abs(got - want) <= bound, (tag, got, want, bound)


def _stacked(gt, device=DEV):
    c2w = torch.stack([b['camera_pose'] for b in gt], dim=1).to(device)
    w2c = torch.linalg.inv(c2w)
    pts = torch.stack([b['pts3d'] for b in gt], dim=1).to(device)
    valid = torch.stack([b['valid_mask'] for b in gt], dim=1).to(device)
    return w2c, pts, valid


def _eval_metric(gt, pred):
    w2c, pts, valid = _stacked(gt)
    counts, sums = L.eval_metric(pts, w2c[:, 0].contiguous(), pred['pts3d'].to(DEV), valid)
    return counts, sums


def _check_eval_metric(gt, pred):
    counts, sums = _eval_metric(gt, pred)
    per_view, per_scene = L.reduce_metric(counts, sums)
    B, V = counts.shape
    _, imgs, glob = R.eval_batch_losses(R.to64(gt), None, pred['pts3d'].double())
    valid = torch.stack([b['valid_mask'] for b in gt], dim=1)
    assert torch.equal(counts.cpu(), valid.flatten(2).sum(-1))
    tol = R.tolerance(R.max_abs(gt, pred))
    for b in range(B):
        for i in range(V):
            _close(f"view {b},{i}", per_view[b, i], imgs[i][b], tol)
        _close(f"scene {b}", per_scene[b], glob[b], tol)
    return counts, sums


# ---------------------------------------------------------------------------------------------------------------------------------
# eval.py's metric
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(7, 13), (33, 37), (32, 64)])
def test_eval_metric_small_shapes(H, W):
    """H W not a multiple of 4 or 64: the scalar tails and the unaligned view bases; a view with no valid pixel (count 0, NaN), a fully
    valid one, NaN / inf ground truth under the mask."""
    gt, pred = R.make_case(3, 4, H, W, seed=H + W, local=False, conf=False, empty_view=(1, 2), full_view=(2, 0), poison=True)
    counts, sums = _check_eval_metric(gt, pred)
    assert int(counts[1, 2]) == 0 and float(sums[1, 2]) == 0.0 and int(counts[2, 0]) == H * W
    assert math.isnan(float(L.reduce_metric(counts, sums)[0][1, 2]))
    # the poison changes nothing: the same case with finite values under the mask gives the same bits
    gt2, pred2 = R.make_case(3, 4, H, W, seed=H + W, local=False, conf=False, empty_view=(1, 2), full_view=(2, 0), poison=False)
    c2, s2 = _eval_metric(gt2, pred2)
    assert torch.equal(counts, c2) and torch.equal(sums, s2)


def test_eval_metric_8x20_views_of_384x512():
    gt, pred = R.make_case(8, 20, 384, 512, seed=5, local=False, conf=False, empty_view=(1, 3), full_view=(2, 4), poison=True)
    counts, sums = _check_eval_metric(gt, pred)
    c2, s2 = _eval_metric(gt, pred)
    assert torch.equal(counts, c2) and torch.equal(sums, s2)
    assert math.isnan(float(L.reduce_metric(counts, sums)[0][1, 3])) and int(counts[2, 4]) == 384 * 512


def test_l21_is_the_fused_pass():
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn((5, 11, 3), generator=g), torch.randn((5, 11, 3), generator=g)
    want = torch.norm(a.double() - b.double(), dim=-1)
    tol = R.tolerance(float(torch.maximum(a.abs().max(), b.abs().max())))
    _close("mean", L.L21(a.to(DEV), b.to(DEV)), want.mean(), tol)
    none = L.L21Loss(reduction='none')(a.to(DEV), b.to(DEV))
    assert none.shape == (5, 11) and float((none.cpu().double() - want).abs().max()) <= tol
    assert math.isnan(float(L.L21(a[:0].to(DEV), b[:0].to(DEV))))


# ---------------------------------------------------------------------------------------------------------------------------------
# normalize_pointcloud
# ---------------------------------------------------------------------------------------------------------------------------------
MODES = ["avg_dis", "avg_log1p", "avg_warp-log1p", "sqrt_dis", "median_dis"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,W,ties", [(7, 13, False), (33, 37, True), (96, 128, False)])
def test_norm_factor_modes(mode, H, W, ties):
    gt, pred = R.make_case(3, 3, H, W, seed=H, scale=2.0, ties=ties, empty_view=(1, 0))
    valid = torch.stack([b['valid_mask'] for b in gt], dim=1)
    valid[2] = False                                        # a scene with nothing valid: 1e-8 (avg), NaN (sqrt, median)
    pts = pred['pts3d']
    want = R._normalize_views(pts.double(), mode, valid)[1].flatten()
    got = L.norm_factor(pts.to(DEV), valid.to(DEV), mode).cpu()
    tol = R.factor_tolerance(float(pts.abs().max()), mode)
    for b in range(3):
        _close(f"{mode} scene {b}", got[b], want[b], tol)
    # with the rigid transform fused: the ground truth's factor
    w2c, gpts, _ = _stacked(gt)
    want = R._normalize_views(R.geotrf(w2c[:, 0].cpu().double(), gpts.cpu().double()), mode, valid)[1].flatten()
    got = L.norm_factor(gpts, valid.to(DEV), mode, trf=w2c[:, 0].contiguous()).cpu()
    for b in range(3):
        _close(f"{mode} gt scene {b}", got[b], want[b], R.factor_tolerance(R.max_abs(gt, pred), mode))
    # the materialising wrapper: same factor, points divided by it (warped first in warp-log1p)
    res, f = L.normalize_pointcloud(pts[:, 0].to(DEV), pts[:, 1].to(DEV), mode, valid[:, 0].to(DEV), valid[:, 1].to(DEV), ret_factor=True)[::2]
    want = R.normalize_pointcloud(pts[:, 0].double(), pts[:, 1].double(), mode, valid[:, 0], valid[:, 1], ret_factor=True)
    fmin = float(want[2][:2].min())
    ok = valid[:2, 0]
    assert float((res.cpu().double() - want[0])[:2][ok].abs().max()) <= R.tolerance(float(pts.abs().max()), scaled=True, warp='warp' in mode,
                                                                                   factor=fmin)
    assert f.shape == want[2].shape


@pytest.mark.parametrize("ties", [False, True])
def test_median_is_the_lower_median_of_the_kernels_own_distances(ties):
    """Exact: the radix select returns one of the distances the pass itself computed -- the element of rank (n - 1) // 2, torch's
    nanmedian -- whatever the ties."""
    gt, pred = R.make_case(4, 5, 33, 37, seed=9, ties=ties, empty_view=(3, 1))
    valid = torch.stack([b['valid_mask'] for b in gt], dim=1)
    valid[1, :, :, :] = False
    valid[1, 2, 5, 6] = True                                # one element
    valid[2, :, :, :] = False
    valid[2, 0, 0, :2] = True                               # two elements: the lower one
    pts = torch.stack([b['pts3d'] for b in gt], dim=1)    # with ties: world points on a grid of 0.5, so few distinct distances
    f, dist = L.norm_factor(pts.to(DEV), valid.to(DEV), 'median_dis', return_dist=True)
    assert dist.shape == (4, 5 * 33 * 37) and torch.equal(~dist.isnan().cpu(), valid.flatten(1))
    assert torch.equal(f, dist.nanmedian(dim=1).values)
    d = dist.cpu()
    for b in range(4):
        own = np.sort(d[b][~d[b].isnan()].numpy())
        assert float(f[b]) == float(own[(len(own) - 1) // 2])
    if ties:
        assert len(np.unique(d[0][~d[0].isnan()].numpy())) < int(valid[0].sum()) // 2
    none = torch.zeros_like(valid[:1])
    f0 = L.norm_factor(pts[:1].to(DEV), none.to(DEV), 'median_dis')
    assert math.isnan(float(f0[0]))


# ---------------------------------------------------------------------------------------------------------------------------------
# Regr3D / ConfLoss
# ---------------------------------------------------------------------------------------------------------------------------------
def _tolerances(gt, pred, norm_mode, loss_in_log, alpha):
    S = R.max_abs(gt, pred)
    mode = norm_mode.lstrip('?')
    fmin = R.min_factor(gt, pred, norm_mode)
    kw = dict(scaled=bool(mode), warp='warp' in mode, log=bool(loss_in_log), factor=fmin)
    plain = R.tolerance(S, libm=bool(loss_in_log) or 'log1p' in mode, **kw)
    conf = R.tolerance(S, conf_max=float(pred['conf'].max()), alpha=alpha, **kw) if 'conf' in pred else plain
    return plain, conf


def _check_confloss(gt, pred, norm_mode, loss_in_log, sky_loss_value=2, alpha=0.2, **kw):
    want_l, want_d = R.ConfLoss(R.Regr3D(R.L21, norm_mode=norm_mode, sky_loss_value=sky_loss_value, loss_in_log=loss_in_log),
                                alpha=alpha)(R.to64(gt), R.to64(pred), **kw)
    crit = L.ConfLoss(L.Regr3D(L.L21, norm_mode=norm_mode, sky_loss_value=sky_loss_value, loss_in_log=loss_in_log), alpha=alpha)
    g, p = R.to_device(gt, pred, DEV)
    got_l, got_d = crit(g, p, **kw)
    assert list(got_d) == list(want_d)
    plain, conf = _tolerances(gt, pred, norm_mode, loss_in_log, alpha)
    for k in want_d:
        _close(f"{norm_mode} log={loss_in_log} {kw} {k}", got_d[k], want_d[k], conf if k.startswith('conf') else plain)
    _close("loss", got_l, want_l, 2 * conf)
    return crit, g, p, got_l, got_d


@pytest.mark.parametrize("loss_in_log", [False, True, 'before'])
@pytest.mark.parametrize("norm_mode", ['?avg_dis', 'avg_dis', '?median_dis', 'sqrt_dis', 'avg_log1p', '?avg_warp-log1p', 'avg_warp-log1p'])
def test_confloss_modes_on_a_mixed_batch(norm_mode, loss_in_log):
    """metric and non-metric scenes in one batch, with and without the leading '?', sky pixels, NaN / inf ground truth under the mask"""
    gt, pred = R.make_case(4, 3, 33, 37, seed=21, sky_frac=0.1, metric=[True, False, False, True], poison=True)
    _check_confloss(gt, pred, norm_mode, loss_in_log)
    _check_confloss(gt, pred, norm_mode, loss_in_log, dist_clip=3.0)


@pytest.mark.parametrize("local,conf", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("H,W", [(7, 13), (33, 37)])
def test_confloss_optional_inputs(local, conf, H, W):
    gt, pred = R.make_case(3, 2, H, W, seed=H, sky_frac=0.1, local=local, conf=conf, metric=[False, True, False], poison=True,
                           empty_view=(0, 1), full_view=(1, 0))
    _check_confloss(gt, pred, '?avg_dis', False)
    _check_confloss(gt, pred, '?avg_dis', True, dist_clip=2.5)
    _check_confloss(gt, pred, '', 'before', sky_loss_value=0)                     # no normalisation, no sky term


def test_confloss_nothing_selected_is_zero():
    """ConfLoss's nan protection: no selected pixel at all -> 0, while Regr3D's detail is the NaN of an empty mean."""
    gt, pred = R.make_case(2, 2, 7, 13, seed=1, valid_frac=0.0)
    _, _, _, loss, details = _check_confloss(gt, pred, '?avg_dis', False)
    assert float(loss) == 0.0 and details['conf_loss_g'] == 0.0 and math.isnan(details['Regr3D_pts3d'])


def test_regr3d_per_pixel_route_and_details():
    """``reduction='none'``: the per-pixel tensors a caller asks for -- same masks as the yardstick, values within the per-pixel bound --
    and ``get_all_pts3d``; the criterion string of the training recipe evaluates in the module's namespace."""
    gt, pred = R.make_case(3, 2, 33, 37, seed=8, sky_frac=0.1, metric=[True, False, False], poison=True)
    crit = eval("ConfLoss(Regr3D(L21, norm_mode='?avg_dis', sky_loss_value=2, loss_in_log=False), alpha=0.2)", vars(L))
    g, p = R.to_device(gt, pred, DEV)
    ref = R.Regr3D(R.L21, norm_mode='?avg_dis', sky_loss_value=2, loss_in_log=False).with_reduction('none')
    ((w1, wmg), (w2, wml)), wd = ref.compute_loss(R.to64(gt), R.to64(pred), dist_clip=3.0)
    ((l1, mg), (l2, ml)), d = crit.pixel_loss.compute_loss(g, p, dist_clip=3.0)
    plain, _ = _tolerances(gt, pred, '?avg_dis', False, 0.2)
    assert torch.equal(mg.cpu(), wmg) and torch.equal(ml.cpu(), wml) and l1.dtype == torch.float32
    assert float((l1.cpu().double() - w1).abs().max()) <= plain and float((l2.cpu().double() - w2).abs().max()) <= plain
    assert list(d) == list(wd)
    for k in wd:
        _close(k, d[k], wd[k], plain)
    want = ref.get_all_pts3d(R.to64(gt), R.to64(pred), dist_clip=3.0)
    got = crit.pixel_loss.get_all_pts3d(g, p, dist_clip=3.0)
    for i in (4, 5, 6, 7):
        assert torch.equal(got[i].cpu(), want[i])
    for i, m in ((0, 4), (1, 5), (2, 4), (3, 5)):
        assert float((got[i].cpu().double() - want[i])[want[m]].abs().max()) <= plain


# ---------------------------------------------------------------------------------------------------------------------------------
# determinism and batch invariance
# ---------------------------------------------------------------------------------------------------------------------------------
def test_same_inputs_twice_and_scene_alone_give_equal_bits():
    gt, pred = R.make_case(4, 3, 96, 128, seed=31, sky_frac=0.1, metric=[True, False, False, True], poison=True)
    reg = L.Regr3D(L.L21, norm_mode='?avg_dis', sky_loss_value=2, loss_in_log=True).with_reduction('none')
    g, p = R.to_device(gt, pred, DEV)
    a, b = reg.fused(g, p, alpha=0.2, dist_clip=3.0), reg.fused(g, p, alpha=0.2, dist_clip=3.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for mode in MODES:
        f1 = L.norm_factor(p['pts3d'], torch.stack([v['valid_mask'] for v in g], 1), mode)
        f2 = L.norm_factor(p['pts3d'], torch.stack([v['valid_mask'] for v in g], 1), mode)
        assert torch.equal(f1, f2)
    for k in range(4):
        g1, p1 = R.to_device(*R.scene_of(gt, pred, k), DEV)
        c1, s1 = reg.fused(g1, p1, alpha=0.2, dist_clip=3.0)
        assert torch.equal(c1[0], a[0][k]) and torch.equal(s1[0], a[1][k]), k
        for mode in MODES:
            valid = torch.stack([v['valid_mask'] for v in g], 1)
            assert torch.equal(L.norm_factor(p1['pts3d'], valid[k:k + 1], mode)[0], L.norm_factor(p['pts3d'], valid, mode)[k]), (k, mode)
    w2c, pts, valid = _stacked(gt)
    ca, sa = L.eval_metric(pts, w2c[:, 0].contiguous(), p['pts3d'], valid)
    for k in range(4):
        c1, s1 = L.eval_metric(pts[k:k + 1].contiguous(), w2c[k:k + 1, 0].contiguous(), p['pts3d'][k:k + 1].contiguous(), valid[k:k + 1].contiguous())
        assert torch.equal(c1[0], ca[k]) and torch.equal(s1[0], sa[k])


# ---------------------------------------------------------------------------------------------------------------------------------
# evaluate() end to end
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("render_once", [False, True])
def test_evaluate_end_to_end_on_synthetic_scenes(tmp_path, monkeypatch, render_once):
    from torch.utils.data import DataLoader
    from must3r_amd.config import SMALL
    from test_model_gpu import build
    enc, dec = build(SMALL, "fp16wa")
    dataset = SyntheticScenes(3, 4, 224, 224, seed=2)
    loader = DataLoader(dataset, batch_size=2, shuffle=False)
    recorded = []
    real_inference, real_postprocess = E.inference, E.postprocess

    def inference(*a, **kw):
        out = real_inference(*a, **kw)
        recorded.append(dict(mem_batches=list(a[4]), to_render=kw.get('to_render'), raw=out, post=[]))
        return out

    def postprocess(x, **kw):
        out = real_postprocess(x, **kw)
        recorded[-1]['post'].append({k: v.clone() for k, v in out.items()})
        return out
    monkeypatch.setattr(E, "inference", inference)
    monkeypatch.setattr(E, "postprocess", postprocess)
    out_file = str(tmp_path / "out" / "eval.txt")
    results = E.evaluate(enc, dec, loader, render_once=render_once, eval_memory_num_views=[2, 3], output=out_file)
    assert [r.num_views_dec for r in results] == [2, 3] and len(recorded) == 4
    text = open(out_file).read()
    assert text == "".join(E.format_results(r) for r in results)
    it = iter(recorded)
    S = 0.0
    for res in results:
        nd, V = res.num_views_dec, 4
        assert (res.mem_batches, res.to_render) == R.eval_schedule(nd, V, 2, 1, render_once)
        first64, imgs64, all64 = [[] for _ in range(nd)], [[] for _ in range(V)], []
        for views in loader:
            rec = next(it)
            assert (rec['mem_batches'], rec['to_render']) == (res.mem_batches, res.to_render)
            x0, x = rec['post'][0]['pts3d'].cpu(), rec['post'][1]['pts3d'].cpu()
            if render_once:
                assert x.shape[1] == V - nd
                x = torch.cat((x0, x), dim=1)
            assert x0.shape[1] == nd and x.shape[1] == V
            S = max(S, R.max_abs(views, dict(pts3d=torch.cat((x0, x), dim=1))))
            f, i, a = R.eval_batch_losses(R.to64(views), x0.double(), x.double())
            for k in range(nd):
                first64[k] += f[k]
            for k in range(V):
                imgs64[k] += i[k]
            all64 += a
        tol = R.tolerance(S)
        assert res.global_.dtype == np.float32 and len(res.first_pass) == nd and len(res.per_image) == V
        for got, want in ((res.first_pass, first64), (res.per_image, imgs64), ([res.global_], [all64])):
            for gv, wv in zip(got, want):
                assert len(gv) == len(wv) == len(dataset)
                for gs, ws in zip(gv, wv):
                    _close("sample", gs, ws, tol)
        # the text parses back to the aggregates of the same numbers
        block = E.format_results(res)
        nums = [float(v) for v in re.findall(r"= ([-+.0-9e]+|nan|inf)", block.split("\n", 1)[1])]
        rows = list(res.first_pass) + list(res.per_image) + [res.global_]
        assert block.startswith(f"num_views_dec={nd}\n") and len(nums) == 2 * len(rows)
        for r, (mean, median) in zip(rows, zip(nums[::2], nums[1::2])):
            assert np.float32(mean) == np.mean(r) and np.float32(median) == np.median(r)


# ---------------------------------------------------------------------------------------------------------------------------------
# the C entry points refuse bad arguments without launching
# ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    B, V, H, W = 2, 3, 8, 12
    dev = torch.device(DEV)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    gt, pr, cam, valid = f32(B, V, H, W, 3), f32(B, V, H, W, 3), torch.eye(4, device=dev).repeat(B, 1, 1), torch.ones((B, V, H, W), dtype=torch.uint8, device=dev)
    counts = torch.full((B, V, 2), -7, dtype=torch.int64, device=dev)
    sums = torch.full((B, V, 4), -7.0, dtype=torch.float64, device=dev)
    nbytes = lib.must3r_hip_metrics_loss_scratch_bytes(B, V, H, W)
    assert nbytes > 0
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    def args(**over):
        a = _lib.MetricsLossArgs()
        a.n_scenes, a.n_views, a.H, a.W = B, V, H, W
        a.gt_pts, a.in_camera0, a.pr_pts, a.valid = gt.data_ptr(), cam.data_ptr(), pr.data_ptr(), valid.data_ptr()
        a.counts, a.sums = counts.data_ptr(), sums.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def refused(rc, word):
        msg = lib.must3r_hip_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)
    sc, stream = C.c_void_p(scratch.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    refused(lib.must3r_hip_metrics_loss(None, sc, nbytes, stream), "null")
    for name in ("gt_pts", "in_camera0", "pr_pts", "valid", "counts", "sums"):
        refused(lib.must3r_hip_metrics_loss(C.byref(args(**{name: None})), sc, nbytes, stream), "null")
    refused(lib.must3r_hip_metrics_loss(C.byref(args()), None, nbytes, stream), "null")
    refused(lib.must3r_hip_metrics_loss(C.byref(args(n_views=0)), sc, nbytes, stream), "n_views")
    refused(lib.must3r_hip_metrics_loss(C.byref(args(n_scenes=-1)), sc, nbytes, stream), "n_scenes")
    refused(lib.must3r_hip_metrics_loss(C.byref(args()), sc, nbytes - 1, stream), "scratch too small")
    refused(lib.must3r_hip_metrics_loss(C.byref(args(pr_local=pr.data_ptr())), sc, nbytes, stream), "w2c")
    refused(lib.must3r_hip_metrics_loss(C.byref(args(loss_in_log=3)), sc, nbytes, stream), "loss_in_log")
    refused(lib.must3r_hip_metrics_loss(C.byref(args(pix_g=pr.data_ptr())), sc, nbytes, stream), "per-pixel")
    assert lib.must3r_hip_metrics_loss_scratch_bytes(B, 0, H, W) == 0 and "n_views" in lib.must3r_hip_last_error().decode()
    # the factor pass
    factor = torch.full((B,), -7.0, dtype=torch.float32, device=dev)
    dist = f32(B, V * H * W)
    for mode in range(4):
        fb = lib.must3r_hip_metrics_factor_scratch_bytes(B, V, H, W, mode)
        assert fb > 0
        fs = torch.zeros(fb, dtype=torch.uint8, device=dev)
        call = lambda **o: lib.must3r_hip_metrics_factor(*[o.get(k, d) for k, d in (  # noqa: E731
            ("pts", gt.data_ptr()), ("trf", None), ("valid", valid.data_ptr()), ("B", B), ("V", V), ("H", H), ("W", W), ("mode", mode),
            ("factor", factor.data_ptr()), ("dist", dist.data_ptr()), ("scratch", fs.data_ptr()), ("bytes", fb))], stream)
        for name in ("pts", "valid", "factor", "scratch"):
            refused(call(**{name: None}), "null")
        refused(call(V=0), "n_views")
        refused(call(bytes=fb - 1), "scratch too small")
        refused(call(mode=7), "unknown mode")
    refused(lib.must3r_hip_metrics_factor(gt.data_ptr(), None, valid.data_ptr(), B, V, H, W, _lib.NORM_MEDIAN_DIS, factor.data_ptr(), None,
                                          fs.data_ptr(), fb, stream), "distance buffer")
    assert lib.must3r_hip_metrics_factor_scratch_bytes(B, V, H, W, 9) == 0
    torch.cuda.synchronize()
    # nothing was launched: the outputs still hold their fill
    assert bool((counts == -7).all()) and bool((sums == -7.0).all()) and bool((factor == -7.0).all())
    # and the same arguments, all valid, run
    _lib.check(lib.must3r_hip_metrics_loss(C.byref(args()), sc, nbytes, stream))
    torch.cuda.synchronize()
    assert bool((counts[..., 0] == H * W).all()) and bool((sums == 0).all())
