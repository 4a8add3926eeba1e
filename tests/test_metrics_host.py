"""Host side of the checkpoint evaluation (must3r_amd.evaluate, must3r_amd.losses' host logic, inference.concat_preds), no GPU needed,
skipped when the reference checkout is absent.  It pins tests/metrics_ref.py -- the fp64 yardstick of the GPU tests -- to the
reference's own program text, read at test time:

* ``must3r.tools.geometry`` and ``must3r.engine.losses`` are imported with this test's dust3r leaves (``metrics_ref``'s ``geotrf``,
  ``invalid_to_zeros`` / ``invalid_to_nans``, ``L21`` / ``Criterion`` / ``MultiLoss`` / ``Sum``) registered in ``sys.modules`` and restored
  afterwards;
* the ``__main__`` body of eval.py is compiled out of its source with ``ast``, its two ``'cuda'`` constants rebound to ``'cpu'``, and run
  with recording stand-ins for ``load_model``, ``inference``, ``postprocess``, ``get_pointmaps_activation`` and the dataset.

Tolerance (``metrics_ref.tolerance``): the reference computes in fp32, the yardstick in fp64 on the same fp32 inputs, so they differ by
the fp32 roundings per pixel alone: ``n_ops * 2^-24 * S`` with ``S`` the largest absolute coordinate or translation of the case and
``n_ops`` the fp32 operations on the path (9 for the plain L21 of eval.py: the fp32 inverse 1, the 4-term dot products of the transform 4,
the difference 1, the norm 3; +2 scale, +4 warp, +4 log map), times 2 where log1p / log
are on the path.  Observed on this CPU for the committed (seeded) inputs: eval.py's per-sample losses reach 0.009 of the bound
(largest ratio |fp32 - fp64| / bound over every printed sample), ``Regr3D`` / ``ConfLoss`` figures 0.012, ``normalize_pointcloud``
factors 0.12 (sqrt_dis; 0.07 avg_dis, 0.08 median_dis, 0.017 the log1p modes): the reference's own arithmetic sits well inside it, as a mean of many per-pixel errors must.
"""
import argparse
import ast
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

import metrics_ref as R
from must3r_amd import evaluate as E
from must3r_amd import inference as I
from must3r_amd import losses as L
from must3r_amd.synthetic import SyntheticScenes

from oracle.ref_shims import REFERENCE_ROOT

REF_EVAL = os.path.join(REFERENCE_ROOT, "eval.py")
REF_INFERENCE = os.path.join(REFERENCE_ROOT, "must3r", "engine", "inference.py")
pytestmark = pytest.mark.skipif(not os.path.exists(REF_EVAL), reason="the reference checkout is not present")


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's modules with this test's leaves
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def ref_modules():
    """(must3r.tools.geometry, must3r.engine.losses) imported from the reference with the restated dust3r leaves."""
    from oracle import ref_shims
    ref_shims.install()
    names = ("dust3r.utils.misc", "dust3r.utils.geometry", "dust3r.losses", "must3r.tools.geometry", "must3r.engine.losses",
             "must3r.tools.path_to_dust3r")
    saved = {n: sys.modules.get(n) for n in names}

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    mod("dust3r.utils.misc", invalid_to_zeros=R.invalid_to_zeros, invalid_to_nans=R.invalid_to_nans)
    mod("dust3r.utils.geometry", geotrf=R.geotrf)
    mod("dust3r.losses", Criterion=R.Criterion, L21=R.L21, MultiLoss=R.MultiLoss, Sum=R.Sum)
    for n in names[3:]:
        sys.modules.pop(n, None)
    try:
        yield importlib.import_module("must3r.tools.geometry"), importlib.import_module("must3r.engine.losses")
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


def _ratio(got, want, bound):
    if want != want:
        assert got != got, (got, want)
        return 0.0
    return abs(got - want) / bound


@pytest.mark.parametrize("mode", ["avg_dis", "avg_log1p", "avg_warp-log1p", "sqrt_dis", "median_dis"])
def test_normalize_pointcloud_restatement(ref_modules, mode):
    geometry, _ = ref_modules
    worst = 0.0
    for seed, scale in ((1, 1.0), (2, 10.0)):
        gt, pred = R.make_case(3, 2, 9, 11, seed=seed, scale=scale, ties=seed == 2)
        pts1, pts2 = pred['pts3d'][:, 0], pred['pts3d'][:, 1]
        v1, v2 = gt[0]['valid_mask'], gt[1]['valid_mask']
        S = float(pred['pts3d'].abs().max())
        for second in (False, True):
            a = (pts1, pts2 if second else None, mode, v1, v2 if second else None)
            ref = geometry.normalize_pointcloud(*a, ret_factor=True)
            mine = R.normalize_pointcloud(*R.to64(a), ret_factor=True)
            assert len(ref) == len(mine) == (3 if second else 2)
            for r, m in zip(ref, mine):
                assert r.shape == m.shape and r.dtype == torch.float32 and m.dtype == torch.float64
            f_ref, f_mine = ref[-1].flatten(), mine[-1].flatten()
            for b in range(3):
                worst = max(worst, _ratio(float(f_ref[b]), float(f_mine[b]), R.factor_tolerance(S, mode)))
            fmin = float(f_mine.min())
            tol = R.tolerance(S, scaled=True, warp='warp' in mode, factor=fmin) if fmin > 0 else 0
            assert float((ref[0].double() - mine[0]).abs().max()) <= tol
    print(f"normalize_pointcloud {mode}: worst |fp32 - fp64| / bound = {worst:.4f}")
    assert worst <= 1.0


def test_log_maps_restatement(ref_modules):
    geometry, _ = ref_modules
    x = torch.randn((5, 7, 3), generator=torch.Generator().manual_seed(3)) * 4
    assert torch.equal(geometry.apply_log_to_norm(x), R.apply_log_to_norm(x))
    assert torch.equal(geometry.apply_log_to_norm(x.double()), R.apply_log_to_norm(x.double()))


CASES = [dict(norm_mode='?avg_dis', loss_in_log=False), dict(norm_mode='avg_dis', loss_in_log=True),
         dict(norm_mode='?median_dis', loss_in_log='before'), dict(norm_mode='sqrt_dis', loss_in_log=False),
         dict(norm_mode='?avg_log1p', loss_in_log=True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['norm_mode']}-{c['loss_in_log']}")
@pytest.mark.parametrize("local,conf,clip", [(True, True, None), (False, True, 3.0), (True, False, 3.0)])
def test_regr3d_confloss_restatement(ref_modules, case, local, conf, clip):
    """The reference's Regr3D / ConfLoss in fp32 against the restatement in fp64: same keys, same masks, figures within the bound.
    (``avg_warp-log1p`` is left to the GPU tests: the reference's own Regr3D cannot run it, normalize_pointcloud's warp branch unpacks
    ``H1, W1 = pts1.shape[1:-1]`` and losses.py hands it five dimensions.)"""
    _, ref_losses = ref_modules
    gt, pred = R.make_case(4, 3, 9, 11, seed=7, sky_frac=0.1, local=local, conf=conf, metric=[True, False, False, True], poison=True)
    kw = {} if clip is None else dict(dist_clip=clip)
    S, alpha = R.max_abs(gt, pred), 0.2
    fmin = R.min_factor(gt, pred, case['norm_mode'])
    log = bool(case['loss_in_log'])
    ref = ref_losses.ConfLoss(ref_losses.Regr3D(R.L21, sky_loss_value=2, **case), alpha=alpha)
    mine = R.ConfLoss(R.Regr3D(R.L21, sky_loss_value=2, **case), alpha=alpha)
    gt_ref, pred_ref = [{k: v.clone() for k, v in b.items()} for b in gt], {k: v.clone() for k, v in pred.items()}
    loss_ref, det_ref = ref(gt_ref, pred_ref, **kw)
    loss_mine, det_mine = mine(R.to64(gt), R.to64(pred), **kw)
    assert list(det_ref) == list(det_mine)
    cmax = float(pred['conf'].max()) if conf else None
    tol_plain = R.tolerance(S, scaled=True, log=log, factor=fmin, libm=log or 'log1p' in case['norm_mode'])
    tol_conf = R.tolerance(S, scaled=True, log=log, factor=fmin, conf_max=cmax, alpha=alpha) if conf else tol_plain
    worst = 0.0
    for k in det_ref:
        worst = max(worst, _ratio(det_ref[k], det_mine[k], tol_conf if k.startswith('conf') else tol_plain))
    worst = max(worst, _ratio(float(loss_ref), float(loss_mine), 2 * tol_conf))
    print(f"Regr3D/ConfLoss {case} local={local} conf={conf} clip={clip}: worst |fp32 - fp64| / bound = {worst:.4f}")
    assert worst <= 1.0
    # the per-pixel route: same masks, per-pixel values within the per-pixel bound
    (l1r, mgr), (l2r, mlr) = ref.pixel_loss(gt_ref, pred_ref, **kw)[0]
    (l1m, mgm), (l2m, mlm) = mine.pixel_loss(R.to64(gt), R.to64(pred), **kw)[0]
    assert torch.equal(mgr, mgm) and torch.equal(mlr, mlm) and (l2r is None) == (l2m is None) == (not local)
    assert float((l1r.double() - l1m).abs().max()) <= tol_plain
    if local:
        assert float((l2r.double() - l2m).abs().max()) <= tol_plain


# ---------------------------------------------------------------------------------------------------------------------------------
# eval.py's own loop
# ---------------------------------------------------------------------------------------------------------------------------------
class _Cuda2Cpu(ast.NodeTransformer):
    def __init__(self):
        self.n = 0

    def visit_Constant(self, node):
        if node.value == 'cuda':
            self.n += 1
            return ast.copy_location(ast.Constant('cpu'), node)
        return node


def _compile_eval_body():
    tree = ast.parse(open(REF_EVAL).read())
    parser = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_args_parser")
    main = next(n for n in tree.body if isinstance(n, ast.If) and isinstance(n.test, ast.Compare) and
                getattr(n.test.left, "id", None) == "__name__")
    rebind = _Cuda2Cpu()
    body = [rebind.visit(n) for n in main.body]
    assert rebind.n == 2
    mod = ast.fix_missing_locations(ast.Module(body=[parser] + body, type_ignores=[]))
    return compile(mod, REF_EVAL, "exec")


def _ref_concat_preds():
    tree = ast.parse(open(REF_INFERENCE).read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "concat_preds")
    ns = dict(torch=torch)
    exec(compile(ast.Module(body=[node], type_ignores=[]), REF_INFERENCE, "exec"), ns)
    return ns["concat_preds"]


class _Recorder:
    """Stand-ins for the model side of eval.py: canned predictions per scene, every call to ``inference`` recorded."""

    def __init__(self, dataset, batch_size):
        g = torch.Generator().manual_seed(99)
        n, V, H, W = len(dataset), dataset.n_views, dataset.H, dataset.W
        gt = torch.stack([torch.stack([v['pts3d'] for v in dataset[i]]) for i in range(n)])
        pose = torch.stack([torch.stack([v['camera_pose'] for v in dataset[i]]) for i in range(n)])
        cam0 = R.geotrf(torch.linalg.inv(pose[:, 0]), torch.nan_to_num(gt))
        self.first = cam0 + 0.10 * torch.randn(cam0.shape, generator=g)
        self.render = cam0 + 0.05 * torch.randn(cam0.shape, generator=g)
        self.batch_size, self.n_batches = batch_size, -(-n // batch_size)
        self.calls, self.batches = [], []

    def load_model(self, chkpt, encoder=None, decoder=None, device=None):
        assert device == 'cpu'
        return "encoder", "decoder"

    def inference(self, encoder, decoder, imgs, true_shape, mem_batches, verbose=False, max_bs=None, to_render=None):
        assert (encoder, decoder) == ("encoder", "decoder") and imgs.device.type == 'cpu'
        k = len(self.calls) % self.n_batches
        self.calls.append((list(mem_batches), None if to_render is None else list(to_render)))
        sl = slice(k * self.batch_size, k * self.batch_size + imgs.shape[0])
        nd = sum(mem_batches)
        x0 = self.first[sl, :nd].clone()
        x = self.render[sl].clone() if to_render is None else self.render[sl][:, to_render].clone()
        self.batches.append((x0, self.render[sl].clone() if to_render is None else torch.cat((x0, x), dim=1)))
        return x0, x

    @staticmethod
    def postprocess(x, pointmaps_activation=None):
        assert pointmaps_activation == "activation"
        return dict(pts3d=x, conf=torch.ones(x.shape[:-1]))


def _run_body(code, dataset, rec, argv, monkeypatch):
    from torch.utils.data import DataLoader
    ns = dict(__name__="__main__", os=os, torch=torch, np=np, argparse=argparse, tqdm=lambda x: x, DataLoader=DataLoader,
              toggle_memory_efficient_attention=lambda on: None, load_model=rec.load_model, inference=rec.inference,
              postprocess=rec.postprocess, concat_preds=_ref_concat_preds(), get_pointmaps_activation=lambda dec: "activation",
              apply_log_to_norm=R.apply_log_to_norm, L21=R.L21, geotrf=R.geotrf, DATASET=dataset)
    monkeypatch.setattr(sys, "argv", ["eval.py"] + argv)
    exec(code, ns)
    return ns


@pytest.mark.parametrize("render_once", [False, True])
@pytest.mark.parametrize("sweep", [None, [2, 4]])
def test_eval_body_against_restatement_and_format(tmp_path, monkeypatch, render_once, sweep):
    """eval.py's ``__main__`` body on the CPU: its float32 losses against the fp64 restatement, its ``result_str`` against
    ``format_results`` fed its own losses, its ``mem_batches`` / ``to_render`` against ``eval_schedule``."""
    dataset = SyntheticScenes(5, 4, 12, 16, seed=3)
    V, bs = 4, 2
    code = _compile_eval_body()
    out = str(tmp_path / "res" / "eval.txt")
    common = ["--chkpt", "none", "--dataset", "DATASET", "--num_workers", "0", "--batch_size", str(bs), "--output", out, "--loss_in_log"]
    common += ["--render_once"] if render_once else []
    nds = list(range(2, V + 1)) if sweep is None else sweep
    # the whole sweep in one run: the file holds every result_str
    rec = _Recorder(dataset, bs)
    _run_body(code, dataset, rec, common + ([] if sweep is None else ["--eval_memory_num_views"] + [str(v) for v in sweep]), monkeypatch)
    whole = open(out).read()
    os.remove(out)
    expect_calls = []
    for nd in nds:
        expect_calls += [E.eval_schedule(nd, V, 2, 1, render_once)] * rec.n_batches
    assert [(m, t) for m, t in rec.calls] == [(m, t) for m, t in expect_calls]
    assert [E.eval_schedule(nd, V, 2, 1, render_once) for nd in nds] == [R.eval_schedule(nd, V, 2, 1, render_once) for nd in nds]
    # one num_views_dec at a time: the body's lists of float32 losses are left in its namespace
    S = max(float(torch.nan_to_num(torch.stack([v['pts3d'] for v in dataset[i]])).abs().max()) for i in range(len(dataset)))
    S = max(S, max(float(torch.stack([v['camera_pose'] for v in dataset[i]])[:, :3].abs().max()) for i in range(len(dataset))))
    tol = R.tolerance(S)
    text, worst = "", 0.0
    for nd in nds:
        rec = _Recorder(dataset, bs)
        ns = _run_body(code, dataset, rec, common + ["--eval_memory_num_views", str(nd)], monkeypatch)
        os.remove(out)
        lf, li, la = ns["losses_firstpass"], ns["losses_imgs"], ns["losses_all"]
        assert all(t.dtype == torch.float32 and t.ndim == 0 for t in la)
        res = E.result_from_losses(nd, [[float(t) for t in v] for v in lf[:nd]], [[float(t) for t in v] for v in li], [float(t) for t in la])
        assert E.format_results(res) == ns["result_str"] == R.result_str(nd, lf, li, la)
        text += ns["result_str"]
        # the restatement, fp64, batch by batch
        from torch.utils.data import DataLoader
        first64, imgs64, all64 = [[] for _ in range(nd)], [[] for _ in range(V)], []
        for views, (x0, x) in zip(DataLoader(dataset, batch_size=bs, shuffle=False), rec.batches):
            f, i, a = R.eval_batch_losses(R.to64(views), x0.double(), x.double())
            for k in range(nd):
                first64[k] += f[k]
            for k in range(V):
                imgs64[k] += i[k]
            all64 += a
        for got, want in ((lf[:nd], first64), (li, imgs64), ([la], [all64])):
            for gv, wv in zip(got, want):
                assert len(gv) == len(wv) == len(dataset)
                for gs, ws in zip(gv, wv):
                    worst = max(worst, _ratio(float(gs), float(ws), tol))
    assert text == whole
    print(f"eval.py body render_once={render_once} sweep={sweep}: worst |fp32 - fp64| / bound = {worst:.4f} (bound {tol:.3e}, S {S:.2f})")
    assert worst <= 1.0


def test_format_results_numbers():
    """float32 in, the reference's float32 reprs out; NaN samples print as nan; no first-pass lines without a first pass."""
    res = E.result_from_losses(2, [[1.5, 2.5], [0.1, 0.3]], [[1.0, 3.0], [2.0, 2.0], [float('nan'), 1.0]], [5.701168060302734, 1.0])
    text = E.format_results(res)
    lines = text.splitlines()
    assert lines[0] == "num_views_dec=2" and lines[1] == "first pass 0 - mean = 2.0, median = 2.0"
    assert lines[2] == f"first pass 1 - mean = {np.mean(np.float32([0.1, 0.3]))}, median = {np.median(np.float32([0.1, 0.3]))}"
    assert lines[5] == "2 - mean = nan, median = nan"
    assert lines[6] == f"global - mean = {np.mean(np.float32([5.701168060302734, 1.0]))}, median = {np.median(np.float32([5.701168060302734, 1.0]))}"
    assert E.format_results(E.result_from_losses(3, [], [[1.0]], [1.0])) == "num_views_dec=3\n0 - mean = 1.0, median = 1.0\nglobal - mean = 1.0, median = 1.0\n"


# ---------------------------------------------------------------------------------------------------------------------------------
# parser, concat_preds, data sources, host-side refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _parser_table(parser):
    out = {}
    for a in parser._actions:
        if isinstance(a, argparse._HelpAction):
            continue
        out[tuple(a.option_strings)] = dict(dest=a.dest, default=a.default, choices=None if a.choices is None else list(a.choices),
                                            required=a.required, type=a.type, nargs=a.nargs, const=a.const, kind=type(a).__name__)
    return out


def test_parser_equals_reference():
    tree = ast.parse(open(REF_EVAL).read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_args_parser")
    ns = dict(argparse=argparse)
    exec(compile(ast.Module(body=[node], type_ignores=[]), REF_EVAL, "exec"), ns)
    ref_parser, nat_parser = ns["get_args_parser"](), E.get_args_parser()
    ref, nat = _parser_table(ref_parser), _parser_table(nat_parser)
    assert list(ref) == list(nat)
    assert ref == nat
    assert ref_parser.prog == nat_parser.prog and ref_parser.add_help == nat_parser.add_help
    help_text = next(a.help for a in nat_parser._actions if a.dest == "loss_in_log")
    assert "do not depend" in help_text


def test_concat_preds_equals_reference():
    g = torch.Generator().manual_seed(0)
    out0 = dict(pts3d=torch.randn((2, 3, 4, 5, 3), generator=g), conf=torch.randn((2, 3, 4, 5), generator=g), only0=torch.zeros(1))
    out = dict(pts3d=torch.randn((2, 2, 4, 5, 3), generator=g), conf=torch.randn((2, 2, 4, 5), generator=g), only1=torch.ones(2, 2))
    want = _ref_concat_preds()({k: v.clone() for k, v in out0.items()}, {k: v.clone() for k, v in out.items()})
    got = I.concat_preds(out0, out)
    assert got is out and list(got) == list(want)
    assert all(torch.equal(got[k], want[k]) for k in want) and got['pts3d'].shape[1] == 5


def test_npz_scenes_roundtrip(tmp_path):
    from torch.utils.data import DataLoader
    dataset = SyntheticScenes(3, 3, 10, 14, seed=5)
    for i in range(len(dataset)):
        E.NpzScenes.save(str(tmp_path / f"scene_{i:03d}.npz"), dataset[i])
    for source in (str(tmp_path), str(tmp_path / "scene_*.npz")):
        stored = E.NpzScenes(source)
        assert len(stored) == 3 and len(stored[0]) == 3
        a = next(iter(DataLoader(dataset, batch_size=3, shuffle=False)))
        b = next(iter(DataLoader(stored, batch_size=3, shuffle=False)))
        for va, vb in zip(a, b):
            assert list(va) == list(vb)
            for k in va:
                assert va[k].dtype == vb[k].dtype and va[k].shape == vb[k].shape
                assert torch.equal(torch.nan_to_num(va[k].float()), torch.nan_to_num(vb[k].float()))
                assert torch.equal(va[k].float().isnan(), vb[k].float().isnan())
    assert len(E.NpzScenes(str(tmp_path), num_views=2)[1]) == 2
    with pytest.raises(FileNotFoundError):
        E.NpzScenes(str(tmp_path / "nothing_*.npz"))
    ns = E.dataset_namespace()
    assert ns["NpzScenes"] is E.NpzScenes and ns["SyntheticScenes"] is SyntheticScenes
    assert len(eval("SyntheticScenes(2, 3, 8, 8, seed=1)", ns)) == 2


def test_synthetic_scenes_are_consistent():
    """World points are the camera pose applied to points in front of the camera; invalid pixels are NaN; a scene is reproducible."""
    d = SyntheticScenes(2, 3, 12, 16, seed=1)
    a, b = d[1], SyntheticScenes(2, 3, 12, 16, seed=1)[1]
    for va, vb in zip(a, b):
        assert torch.equal(va['valid_mask'], vb['valid_mask']) and torch.equal(torch.nan_to_num(va['pts3d']), torch.nan_to_num(vb['pts3d']))
        local = R.geotrf(torch.linalg.inv(va['camera_pose'])[None], va['pts3d'][None])[0]
        assert bool((local[va['valid_mask']][:, 2] > 1.0).all()) and bool(va['pts3d'][~va['valid_mask']].isnan().all())
        assert not bool((va['sky_mask'] & va['valid_mask']).any())


def test_cpu_tensors_and_grad_are_refused():
    gt, pred = R.make_case(1, 2, 4, 5, seed=0)
    crit = eval("ConfLoss(Regr3D(L21, norm_mode='?avg_dis', sky_loss_value=2, loss_in_log=False), alpha=0.2)", vars(L))
    assert crit.alpha == 0.2 and crit.pixel_loss.criterion.reduction == 'none' and crit.pixel_loss.norm_mode == 'avg_dis'
    assert not crit.pixel_loss.norm_all and L.L21.reduction == 'mean'
    with pytest.raises(RuntimeError, match="GPU"):
        crit(gt, pred)
    with pytest.raises(RuntimeError, match="GPU"):
        L.L21(pred['pts3d'], pred['pts3d'])
    with pytest.raises(RuntimeError, match="GPU"):
        L.normalize_pointcloud(pred['pts3d'][:, 0], None, 'avg_dis', gt[0]['valid_mask'])
    pred['pts3d'].requires_grad_(True)
    with pytest.raises(NotImplementedError, match="backward pass is not built"):
        crit(gt, pred)
