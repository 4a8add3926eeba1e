"""The backward pass of the loss family and of the head activation (csrc/metrics.hip ``must3r_hip_metrics_loss_grad``, csrc/misc.hip
``must3r_hip_postprocess_act_grad``; must3r_amd.train_losses) against the reference's method (tests/metrics_ref.py ``ConfLoss`` in fp32
under torch autograd, on the same GPU and the same tensors).  One JSON line per size (append them to profiles/loss_grad_bench.jsonl).
Sizes: 8 and 28 scenes x 20 views of 384 x 512.

  (a) kernels, device events, as a fraction of 6.3 TB/s beside the forward pass (0.71, profiles/metrics_bench.jsonl):
      the forward pass of the full ConfLoss (42 useful bytes per pixel: 12 ground truth, 12 + 12 predictions, 4 conf, 2 masks);
      the backward without a scale path (gradient kernel alone: 42 read + 28 written) and with one ('avg_dis', every scene normalised by
      its own factor: + the reduction pass, which skips the sky mask: 41 read; its share is the difference of the two, both timed
      around the C entry point alone on preallocated buffers, so it also holds the per-scene final kernel and the scale-path term's work
      in the gradient kernel: the kernels one by one are in the rocprofv3 run); the activation backward (28 raw + 28 upstream gradients read, 28 written)
  (b) wall clock of forward + backward of ``ConfLoss(Regr3D(L21, norm_mode='?avg_dis', sky_loss_value=2), alpha=0.2)`` through
      train_losses, beside the yardstick.  The yardstick is the reference's method, never the code under test.

Timings: ``warmup`` runs, then ``rounds`` rounds: median, min and max.  Per-kernel times: run with --kernels-only under
``rocprofv3 --kernel-trace --stats`` (a separate run; profiles/loss_grad_kernel_stats.txt).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_ref as R  # noqa: E402
from must3r_amd import _lib, losses as L, train_losses as T  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12
H, W, V = 384, 512, 20
RECIPE = "ConfLoss(Regr3D(L21, norm_mode='?avg_dis', sky_loss_value=2, loss_in_log=False), alpha=0.2)"


def _stats(xs, **kw):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), rounds=len(xs), **kw)


def make_batch(B, seed=0):
    """seeded, generated on the device: world points in front of moving cameras, 70 % valid, sky among the rest, conf = 1 + exp(randn)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    c2w = R.random_rigid(torch.Generator().manual_seed(seed), B * V).view(B, V, 4, 4).to(DEV)
    pts = torch.randn((B, V, H, W, 3), generator=g, device=DEV)
    pr = pts + 0.05 * torch.randn((B, V, H, W, 3), generator=g, device=DEV)
    pl = torch.randn((B, V, H, W, 3), generator=g, device=DEV)
    conf = 1.0 + torch.exp(torch.randn((B, V, H, W), generator=g, device=DEV))
    r = torch.rand((B, V, H, W), generator=g, device=DEV)
    valid, sky = r < 0.7, r > 0.9
    w2c = torch.linalg.inv(c2w)
    return dict(c2w=c2w, w2c=w2c, cam0=w2c[:, 0].contiguous(), pts=pts, pr=pr, pl=pl, conf=conf, valid=valid, sky=sky)


def _events(fn, args):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def grad_call(pos, kw, counts, scale_path):
    """The backward entry point on preallocated buffers: nothing but ``must3r_hip_metrics_loss_grad`` inside the timed call.  With
    ``scale_path`` every scene has a factor of its own ('avg_dis'), so the reduction launches run too."""
    import ctypes as C
    lib = _lib.load()
    a, keep, (B, V, H, W), dev = L.loss_args(*pos, **kw)
    one = torch.ones((1,), device=dev)
    outs = [torch.empty((B, V, H, W, 3), device=dev), torch.empty((B, V, H, W, 3), device=dev), torch.empty((B, V, H, W), device=dev)]
    g = _lib.MetricsLossGradArgs()
    g.w_g = g.w_l = one.data_ptr()
    g.weighting, g.counts = _lib.LOSS_W_CONF, counts.data_ptr()
    g.grad_pts, g.grad_local, g.grad_conf = (t.data_ptr() for t in outs)
    if scale_path:
        own = torch.ones((B,), dtype=torch.uint8, device=dev)
        n_valid = pos[3].reshape(B, -1).sum(dim=1, dtype=torch.int64)
        keep += [own, n_valid]
        g.factor_mode, g.n_own, g.own_factor, g.n_valid = _lib.NORM_AVG_DIS, B, own.data_ptr(), n_valid.data_ptr()
    nbytes = lib.must3r_hip_metrics_loss_grad_scratch_bytes(B, V, H, W)
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(_lib.stream_ptr(dev))
    keep += [one, outs, scratch, counts]

    def call(_keep=keep):
        _lib.check(lib.must3r_hip_metrics_loss_grad(C.byref(a), C.byref(g), scratch.data_ptr(), nbytes, stream))
    return call


def bench_kernels(b, args):
    B = b["pts"].shape[0]
    n_pix = B * V * H * W
    valid8, sky8 = b["valid"].to(torch.uint8), b["sky"].to(torch.uint8)
    scale = L.norm_factor(b["pr"], valid8, "avg_dis")
    pos = (b["pts"], b["cam0"], b["pr"], valid8)
    out = {}

    def figure(name, fn, bytes_per_pixel):
        st = _stats(_events(fn, args), unit="ms")
        nbytes = bytes_per_pixel * n_pix
        out[name] = dict(ms=st, bytes=int(nbytes), bytes_per_pixel=bytes_per_pixel,
                         fraction_of_6p3_TBps=nbytes / (st["median"] * 1e-3) / HBM_BYTES_PER_S)
    # the recipe's criterion (no log map, no clip), and everything on (log map on both terms, dist_clip)
    for tag, extra in (("recipe", dict(loss_in_log=False)), ("all_on", dict(dist_clip=3.0, loss_in_log=True))):
        kw = dict(w2c=b["w2c"], pr_local=b["pl"], conf=b["conf"], sky=sky8, gt_scale=scale, pr_scale=scale, sky_loss_value=2.0, alpha=0.2, **extra)
        counts, _ = L.loss_pass(*pos, **kw)
        figure(f"loss_pass_confloss_{tag}", lambda: L.loss_pass(*pos, **kw), 42)
        figure(f"loss_grad_confloss_{tag}", grad_call(pos, kw, counts, False), 42 + 28)
        figure(f"loss_grad_confloss_scale_path_{tag}", grad_call(pos, kw, counts, True), 41 + 42 + 28)
        red = out[f"loss_grad_confloss_scale_path_{tag}"]["ms"]["median"] - out[f"loss_grad_confloss_{tag}"]["ms"]["median"]
        out[f"scale_path_reduction_{tag}"] = dict(ms_median_by_difference=red, bytes_per_pixel=41,
                                                  fraction_of_6p3_TBps=41 * n_pix / (red * 1e-3) / HBM_BYTES_PER_S if red > 0 else None)
    raw = torch.randn((B, V, H, W, 7), device=DEV)
    ups = [torch.randn((B, V, H, W, 3), device=DEV), torch.randn((B, V, H, W, 3), device=DEV), torch.randn((B, V, H, W), device=DEV)]
    grad_raw = torch.empty_like(raw)
    lib, stream = _lib.load(), _lib.stream_ptr(raw.device)
    for name, act in (("activation_grad_norm_exp", _lib.ACT_NORM_EXP), ("activation_grad_linear", _lib.ACT_LINEAR)):
        figure(name, lambda: _lib.check(lib.must3r_hip_postprocess_act_grad(raw.data_ptr(), act, ups[0].data_ptr(), ups[1].data_ptr(),
                                                                            ups[2].data_ptr(), grad_raw.data_ptr(), n_pix, stream)), 56 + 28)
    return out


def _wall(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def bench_step(b, args):
    B = b["pts"].shape[0]
    metric = torch.arange(B) % 2 == 0
    gt = [dict(camera_pose=b["c2w"][:, v], pts3d=b["pts"][:, v], valid_mask=b["valid"][:, v], sky_mask=b["sky"][:, v], is_metric_scale=metric.to(DEV))
          for v in range(V)]
    leaves = {k: b[s].clone().requires_grad_(True) for k, s in (("pts3d", "pr"), ("pts3d_local", "pl"), ("conf", "conf"))}

    def step(crit, gt):
        for v in leaves.values():
            v.grad = None
        loss, details = crit(gt, leaves)
        loss.backward()
        return float(loss.detach()), {k: v.grad for k, v in leaves.items()}
    native = eval(RECIPE, vars(T))
    yard = eval(RECIPE, vars(R))
    gt_native = [dict(v, is_metric_scale=metric) for v in gt]           # the host reads the metric flags
    loss_n, g_n = step(native, gt_native)
    g_n = {k: v.clone() for k, v in g_n.items()}
    loss_y, g_y = step(yard, gt)
    rec = dict(native_s=_stats(_wall(lambda: step(native, gt_native), args.rounds, args.warmup), unit="s"),
               yardstick_torch_s=_stats(_wall(lambda: step(yard, gt), args.yardstick_rounds, 1), unit="s"),
               loss_native=loss_n, loss_yardstick=loss_y,
               max_abs_grad_difference={k: float((g_n[k] - g_y[k]).abs().max()) for k in g_n},
               max_abs_grad={k: float(g_y[k].abs().max()) for k in g_n})
    rec["speedup_median"] = rec["yardstick_torch_s"]["median"] / rec["native_s"]["median"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="*", default=[8, 28])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--yardstick-rounds", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true", help="figure (a) alone, e.g. under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    f = open(args.out, "a") if args.out else None
    for B in args.scenes:
        b = make_batch(B)
        rec = dict(figure="loss_grad", scenes=B, views=V, H=H, W=W, pixels=B * V * H * W, kernels=bench_kernels(b, args))
        if not args.kernels_only:
            rec["step"] = bench_step(b, args)
        line = json.dumps(rec)
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()
        del b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
