"""``python -m must3r_amd.evaluate``: the reference's eval.py -- the pointmap regression error of a checkpoint per view and per scene
against ground truth -- with its option names, defaults, loop and output text.

For every ``num_views_dec`` of the sweep (eval.py:85-164): the first ``num_views_dec`` views build the memory (``mem_batches`` from
``init_num_views`` / ``batch_num_views``), all views (or, with ``render_once``, only the unseen ones, the seen ones taken from the first
pass through ``concat_preds``) are rendered, and ``L21(geotrf(in_camera0, gt)[valid], pred[valid])`` is taken per view of the first
pass, per view of the render and per scene.  The reference does that with ``B * (num_views_dec + num_views_all + 1)`` boolean-mask
gathers, each followed by ``.cpu()``; here a batch's metric is ``batch_metric``: one fused pass per prediction tensor
(``losses.eval_metric``, csrc/metrics.hip) whose [B, V] fp64 sums and counts stay on the device; the host reads them once per
``num_views_dec``.  Each per-sample loss is the fp64 sum divided by the count, rounded once to float32; ``format_results`` aggregates
them with ``np.mean`` / ``np.median`` on float32 arrays, as the reference does on its float32 scalars, so the text matches it
character for character for the same numbers.

Data: ``evaluate`` takes any re-iterable of batches in the reference's view format (a list of ``num_views_all`` dicts of batched
tensors: ``img`` [B,3,H,W], ``true_shape`` [B,2], ``camera_pose`` [B,4,4], ``pts3d`` [B,H,W,3], ``valid_mask`` [B,H,W]).  ``--dataset`` is
evaluated in a namespace that offers ``SyntheticScenes`` (must3r_amd.synthetic), ``NpzScenes`` (below) and, when it can be imported,
everything of ``must3r.datasets``.

``NpzScenes`` layout: one ``.npz`` per scene, every array stacked over the scene's V views -- ``img`` float32 [V,3,H,W] (ImgNorm range
[-1,1]), ``true_shape`` int32 [V,2], ``camera_pose`` float32 [V,4,4] (camera to world), ``pts3d`` float32 [V,H,W,3] (world), ``valid_mask``
bool [V,H,W]; optional ``sky_mask`` bool [V,H,W] (default all False) and ``is_metric_scale`` bool scalar (default True).
"""
import argparse
import glob as _glob
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import losses
from .engine import postprocess
from .inference import concat_preds, inference
from .synthetic import SyntheticScenes


def get_args_parser():
    parser = argparse.ArgumentParser('MUSt3R eval', add_help=False)
    parser.add_argument('--output', default=None)
    parser.add_argument('--encoder', default=None, type=str)
    parser.add_argument('--decoder', default=None)
    parser.add_argument('--init_num_views', default=2, type=int, help="number of views to use when initializing the memory")
    parser.add_argument('--batch_num_views', default=1, type=int, help="number of views to use at once when updating the memory")
    parser.add_argument('--max_batch_size', default=None, type=int, help="max batch size for encoder/renderer")
    parser.add_argument('--render_once', action='store_true', default=False)
    parser.add_argument('--loss_in_log', action='store_true', default=False,
                        help="accepted as in the reference, which computes the log-mapped ground truth and never uses it: "
                             "the printed figures do not depend on this flag")
    parser.add_argument('--chkpt', required=True, type=str, help="path to weights")
    parser.add_argument('--eval_memory_num_views', default=None, nargs='+', type=int,
                        help="number of views to use when updating the memory")
    parser.add_argument('--verbose', action='store_true', default=False)
    parser.add_argument('--dataset', required=True, type=str, help="test set")
    parser.add_argument('--num_workers', default=8, type=int, help="data loader workers")
    parser.add_argument('--batch_size', default=8, type=int, help="scenes per batch")
    return parser


class NpzScenes:
    """Scenes stored one ``.npz`` each (layout in the module docstring); ``path_or_glob``: a directory, a glob pattern or one file."""

    KEYS = ("img", "true_shape", "camera_pose", "pts3d", "valid_mask")

    def __init__(self, path_or_glob, num_views=None):
        if os.path.isdir(path_or_glob):
            path_or_glob = os.path.join(path_or_glob, "*.npz")
        self.files = sorted(_glob.glob(path_or_glob))
        if not self.files:
            raise FileNotFoundError(f"NpzScenes: no .npz scene matches {path_or_glob!r}")
        self.num_views = num_views

    def set_epoch(self, epoch):
        pass

    def __len__(self):
        return len(self.files)

    def __getitem__(self, idx):
        with np.load(self.files[idx]) as z:
            missing = [k for k in self.KEYS if k not in z]
            if missing:
                raise KeyError(f"{self.files[idx]}: missing {missing}")
            arrays = {k: z[k] for k in z.files}
        V = arrays["img"].shape[0] if self.num_views is None else self.num_views
        if V > arrays["img"].shape[0]:
            raise ValueError(f"{self.files[idx]}: {arrays['img'].shape[0]} views stored, {V} asked for")
        sky = arrays.get("sky_mask")
        metric = bool(arrays["is_metric_scale"]) if "is_metric_scale" in arrays else True
        views = []
        for v in range(V):
            views.append(dict(img=torch.from_numpy(arrays["img"][v].astype(np.float32)),
                              true_shape=torch.from_numpy(arrays["true_shape"][v].astype(np.int32)),
                              camera_pose=torch.from_numpy(arrays["camera_pose"][v].astype(np.float32)),
                              pts3d=torch.from_numpy(arrays["pts3d"][v].astype(np.float32)),
                              valid_mask=torch.from_numpy(arrays["valid_mask"][v].astype(bool)),
                              sky_mask=torch.from_numpy((np.zeros_like(arrays["valid_mask"][v]) if sky is None else sky[v]).astype(bool)),
                              is_metric_scale=torch.tensor(metric)))
        return views

    @staticmethod
    def save(path, views):
        """One scene (a list of per-view dicts of unbatched tensors) -> ``path``."""
        def stack(k):
            return np.stack([np.asarray(v[k]) for v in views])
        arrays = {k: stack(k) for k in NpzScenes.KEYS}
        if "sky_mask" in views[0]:
            arrays["sky_mask"] = stack("sky_mask")
        if "is_metric_scale" in views[0]:
            arrays["is_metric_scale"] = np.asarray(bool(views[0]["is_metric_scale"]))
        np.savez(path, **arrays)
        return path


def eval_schedule(num_views_dec, num_views_all, init_num_views=2, batch_num_views=1, render_once=False):
    """eval.py:116-124 -> ``(mem_batches, to_render)``."""
    mem_batches = [min(init_num_views, num_views_dec)]
    while (sum_b := sum(mem_batches)) != num_views_dec:
        mem_batches.append(min(batch_num_views, num_views_dec - sum_b))
    to_render = list(range(num_views_dec, num_views_all)) if render_once else None
    return mem_batches, to_render


def batch_metric(views, x_out_0, x_out, device=None):
    """The metric stage of one batch (eval.py:100-150) on the device.  ``views``: the batch's list of per-view dicts; ``x_out_0``
    [B, num_views_dec, H, W, 3] or None; ``x_out`` [B, num_views_all, H, W, 3].  Returns ``(first, full)``, each ``(counts int64 [B,V],
    sums fp64 [B,V])`` (``first`` None without a first pass).  Nothing is read back."""
    device = device or x_out.device
    gt_c2w = torch.stack([b['camera_pose'] for b in views], dim=1).to(device)
    in_camera0 = torch.linalg.inv(gt_c2w)[:, 0].contiguous()
    gt_pts = torch.stack([b['pts3d'] for b in views], dim=1).to(device)
    gt_valid = torch.stack([b['valid_mask'] for b in views], dim=1).to(device)
    B, V, H, W, _ = gt_pts.shape
    full = losses.eval_metric(gt_pts, in_camera0, x_out.reshape(B, V, H, W, 3), gt_valid)
    first = None
    if x_out_0 is not None and x_out_0.shape[1] > 0:
        n0 = x_out_0.shape[1]
        first = losses.eval_metric(gt_pts[:, :n0].contiguous(), in_camera0, x_out_0.reshape(B, n0, H, W, 3), gt_valid[:, :n0].contiguous())
    return first, full


@dataclass
class EvalResult:
    """The per-sample float32 losses of one ``num_views_dec``: ``first_pass[i]`` / ``per_image[i]`` hold one value per scene for view
    ``i``, ``global_`` one per scene (eval.py's ``losses_firstpass`` / ``losses_imgs`` / ``losses_all``)."""
    num_views_dec: int
    first_pass: list = field(default_factory=list)
    per_image: list = field(default_factory=list)
    global_: np.ndarray = None
    mem_batches: list = None
    to_render: list = None


def format_results(result):
    """eval.py:152-159, character for character."""
    num_views_dec = result.num_views_dec
    result_str = f'{num_views_dec=}\n'
    if len(result.first_pass) > 0 and len(result.first_pass[0]) > 0:
        for i in range(num_views_dec):
            result_str += (f'first pass {i} - mean = {np.mean(result.first_pass[i])}, '
                           f'median = {np.median(result.first_pass[i])}\n')
    for i in range(len(result.per_image)):
        result_str += f'{i} - mean = {np.mean(result.per_image[i])}, median = {np.median(result.per_image[i])}\n'
    result_str += f'global - mean = {np.mean(result.global_)}, median = {np.median(result.global_)}\n'
    return result_str


def _as_f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def result_from_losses(num_views_dec, first_pass, per_image, global_):
    """An ``EvalResult`` from per-sample float32 losses given as nested sequences (for callers that computed them elsewhere)."""
    return EvalResult(num_views_dec, [_as_f32(v) for v in first_pass], [_as_f32(v) for v in per_image], _as_f32(global_))


@torch.no_grad()
def evaluate(encoder, decoder, batches, init_num_views=2, batch_num_views=1, max_batch_size=None, render_once=False,
             eval_memory_num_views=None, pointmaps_activation=None, verbose=False, device='cuda', output=None, num_views_all=None,
             print_results=False):
    """eval.py:79-164.  ``batches`` is iterated once per ``num_views_dec`` (a DataLoader or a list of batches).  Returns the list of
    ``EvalResult`` of the sweep; ``output``: file the formatted results are appended to."""
    if pointmaps_activation is None:
        from .model import get_pointmaps_activation
        pointmaps_activation = get_pointmaps_activation(decoder, verbose=False)
    if iter(batches) is batches:
        batches = list(batches)
    if num_views_all is None:
        num_views_all = len(next(iter(batches)))
    if output is not None and os.path.dirname(output):
        os.makedirs(os.path.dirname(output), exist_ok=True)
    sweep = list(range(init_num_views, num_views_all + 1)) if eval_memory_num_views is None else list(eval_memory_num_views)
    results = []
    for num_views_dec in sweep:
        mem_batches, to_render = eval_schedule(num_views_dec, num_views_all, init_num_views, batch_num_views, render_once)
        pending = []                                  # per batch: device tensors only
        for views in batches:
            assert len(views) == num_views_all
            imgs = torch.stack([b['img'] for b in views], dim=1).to(device)
            true_shape = torch.stack([b['true_shape'] for b in views], dim=1).to(torch.int64)   # stays where it is: both modules read (H, W) as host integers
            x_out_0, x_out = inference(encoder, decoder, imgs, true_shape, mem_batches, verbose=verbose, max_bs=max_batch_size,
                                       to_render=to_render)
            x_out_0 = postprocess(x_out_0, pointmaps_activation=pointmaps_activation)
            x_out = postprocess(x_out, pointmaps_activation=pointmaps_activation)
            if to_render is not None:
                x_out = concat_preds(x_out_0, x_out)
            pending.append(batch_metric(views, x_out_0['pts3d'], x_out['pts3d'], device=imgs.device))
        full_c = torch.cat([f[1][0] for f in pending])
        full_s = torch.cat([f[1][1] for f in pending])
        per_view, per_scene = losses.reduce_metric(full_c, full_s)
        packed = [per_view, per_scene[:, None]]
        if pending and pending[0][0] is not None:
            packed.append(losses.reduce_metric(torch.cat([f[0][0] for f in pending]), torch.cat([f[0][1] for f in pending]))[0])
        host = torch.cat(packed, dim=1).cpu().numpy()  # the one device->host read of this num_views_dec
        V = num_views_all
        res = EvalResult(num_views_dec, [_as_f32(host[:, V + 1 + i]) for i in range(host.shape[1] - V - 1)],
                         [_as_f32(host[:, i]) for i in range(V)], _as_f32(host[:, V]), mem_batches, to_render)
        results.append(res)
        text = format_results(res)
        if print_results:
            print(text)
        if output is not None:
            with open(output, 'a') as fid:
                fid.write(text)
    return results


def dataset_namespace():
    ns = dict(NpzScenes=NpzScenes, SyntheticScenes=SyntheticScenes, np=np, torch=torch)
    try:
        import must3r.datasets as ref_datasets
        ns.update({k: v for k, v in vars(ref_datasets).items() if not k.startswith('_')})
    except Exception:
        pass
    return ns


def main(argv=None):
    from torch.utils.data import DataLoader
    from .model import get_pointmaps_activation, load_model
    args = get_args_parser().parse_args(argv)
    print('Loading pretrained: ', args.chkpt)
    encoder, decoder = load_model(args.chkpt, encoder=args.encoder, decoder=args.decoder, device='cuda')
    pointmaps_activation = get_pointmaps_activation(decoder)
    dataset = eval(args.dataset, dataset_namespace())  # noqa: S307 -- same contract as the reference (eval.py:73)
    if hasattr(dataset, 'set_epoch'):
        dataset.set_epoch(0)
    num_views_all = len(dataset[0])
    dataloader = DataLoader(dataset, batch_size=args.batch_size, shuffle=False, num_workers=args.num_workers)
    return evaluate(encoder, decoder, dataloader, init_num_views=args.init_num_views, batch_num_views=args.batch_num_views,
                    max_batch_size=args.max_batch_size, render_once=args.render_once, eval_memory_num_views=args.eval_memory_num_views,
                    pointmaps_activation=pointmaps_activation, verbose=args.verbose, output=args.output, num_views_all=num_views_all,
                    print_results=True)


if __name__ == "__main__":
    main()
