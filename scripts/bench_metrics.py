"""Checkpoint evaluation (csrc/metrics.hip; must3r_amd.losses, must3r_amd.evaluate) against the reference's method (tests/metrics_ref.py:
boolean-mask gathers and a ``.cpu()`` per loss, run in fp32 on the same GPU through torch).  One JSON line per figure (append them to
profiles/metrics_bench.jsonl).  Sizes: 8 and 28 scenes x 20 views of 384 x 512 (28 x 20 is the benched step's size).

  (a) kernels, device events: the loss pass as eval.py's metric (25 useful bytes per pixel: 12 ground truth, 12 prediction, 1 mask)
      and as the full ConfLoss (42: + 12 local prediction, 4 conf, 1 sky; dist_clip and loss_in_log on), and the factor pass per norm
      mode (13; median_dis 25: + 4 written and 2 x 4 read back by the select passes); their fraction of 6.3 TB/s
  (b) the metric stage of one ``evaluate`` batch, wall clock: ``evaluate.batch_metric`` (first pass + render) + ``reduce_metric`` + the
      one device->host read, beside the reference's loop on the same tensors.  The yardstick is the reference's method, never the code
      under test.
  (c) ``evaluate`` on SyntheticScenes with MUSt3R_512 random-init weights, 20-view scenes: views/s of the whole loop, the share of it
      spent outside ``inference``, and ``engine.run_scenes`` alone on the same batch

Timings: ``warmup`` runs, then ``rounds`` rounds: median, min and max.  Per-kernel times: run with --kernels-only under
``rocprofv3 --kernel-trace --stats`` (a separate run; profiles/metrics_kernel_stats.txt).
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
from must3r_amd import evaluate as E, losses as L  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12
H, W, V = 384, 512, 20


def _stats(xs, **kw):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), rounds=len(xs), **kw)


def _emit(rec, f):
    line = json.dumps(rec)
    print(line, flush=True)
    if f:
        f.write(line + "\n")
        f.flush()


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


def bench_kernels(b, args):
    B = b["pts"].shape[0]
    n_pix = B * V * H * W
    valid8, sky8 = b["valid"].to(torch.uint8), b["sky"].to(torch.uint8)
    scale = torch.full((B,), 1.7, device=DEV)
    out = {}

    def figure(name, fn, bytes_per_pixel):
        st = _stats(_events(fn, args), unit="ms")
        nbytes = bytes_per_pixel * n_pix
        out[name] = dict(ms=st, bytes=int(nbytes), bytes_per_pixel=bytes_per_pixel,
                         fraction_of_6p3_TBps=nbytes / (st["median"] * 1e-3) / HBM_BYTES_PER_S)
    figure("loss_pass_eval_metric", lambda: L.loss_pass(b["pts"], b["cam0"], b["pr"], valid8), 25)
    figure("loss_pass_confloss", lambda: L.loss_pass(b["pts"], b["cam0"], b["pr"], valid8, w2c=b["w2c"], pr_local=b["pl"], conf=b["conf"],
                                                     sky=sky8, gt_scale=scale, pr_scale=scale, dist_clip=3.0, loss_in_log=True,
                                                     sky_loss_value=2.0, alpha=0.2), 42)
    for mode in ("avg_dis", "avg_log1p", "sqrt_dis", "median_dis"):
        figure("factor_pass_" + mode, lambda: L.norm_factor(b["pts"], valid8, mode, trf=b["cam0"]), 25 if mode == "median_dis" else 13)
    return out


def views_of(b):
    B = b["pts"].shape[0]
    return [dict(camera_pose=b["c2w"][:, v], pts3d=b["pts"][:, v], valid_mask=b["valid"][:, v]) for v in range(V)]


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


def bench_metric_stage(b, args):
    views = views_of(b)
    x0, x = b["pl"][:, :V].contiguous(), b["pr"]         # a full first pass (num_views_dec = V) and the render

    def native():
        first, full = E.batch_metric(views, x0, x)
        pv, ps = L.reduce_metric(*full)
        fv = L.reduce_metric(*first)[0]
        return torch.cat((pv, ps[:, None], fv), dim=1).cpu()

    def yardstick():
        return R.eval_batch_losses(views, x0, x, criterion=lambda p, q: R.L21(p, q).cpu())
    got = native()
    f, i, a = yardstick()
    want = torch.tensor([[float(i[v][s]) for v in range(V)] + [float(a[s])] + [float(f[v][s]) for v in range(V)] for s in range(got.shape[0])])
    rec = dict(native_s=_stats(_wall(native, args.rounds, args.warmup), unit="s"),
               yardstick_torch_s=_stats(_wall(yardstick, args.yardstick_rounds, 1), unit="s"),
               max_abs_difference=float((got - want).abs().max()), losses=int(got.numel()))
    rec["speedup_min"] = rec["yardstick_torch_s"]["min"] / rec["native_s"]["min"]
    return rec


def bench_evaluate(B, args):
    from torch.utils.data import DataLoader
    import must3r_amd.model as M
    from must3r_amd import synthetic as S
    from must3r_amd.config import MUST3R_512
    from must3r_amd.engine import run_scenes
    cfg = MUST3R_512
    enc = M.Dust3rEncoder(img_size=(cfg.img_size,) * 2, embed_dim=cfg.enc_dim, depth=cfg.enc_depth, num_heads=cfg.enc_heads)
    dec = M.MUSt3R(img_size=(cfg.img_size,) * 2, enc_embed_dim=cfg.enc_dim, embed_dim=cfg.dec_dim, depth=cfg.dec_depth, num_heads=cfg.dec_heads,
                   feedback_type="single_mlp", memory_mode="kv", landscape_only=False)
    enc.load_state_dict(S.make_encoder_state_dict(cfg, 0), strict=True)
    dec.load_state_dict(S.make_decoder_state_dict(cfg, 0), strict=True)
    enc, dec = enc.to(DEV).eval(), dec.to(DEV).eval()
    batches = list(DataLoader(S.SyntheticScenes(B, V, H, W, seed=0), batch_size=B, shuffle=False))
    inside = [0.0]
    real = E.inference

    def timed(*a, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = real(*a, **kw)
        torch.cuda.synchronize()
        inside[0] += time.perf_counter() - t0
        return out
    E.inference = timed
    try:
        def run():
            return E.evaluate(enc, dec, batches, eval_memory_num_views=[V], device=DEV)
        for _ in range(args.warmup):
            run()
        total, shares = [], []
        for _ in range(args.rounds):
            inside[0] = 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = run()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            total.append(dt)
            shares.append(1.0 - inside[0] / dt)
    finally:
        E.inference = real
    imgs = torch.stack([v["img"] for v in batches[0]], dim=1).to(DEV)
    ts = torch.tensor([[H, W]] * V, dtype=torch.int64)
    fwd = _wall(lambda: run_scenes(enc, dec, imgs, ts), args.rounds, args.warmup)
    st = _stats(total, unit="s")
    return dict(evaluate_s=st, views_per_s=B * V / st["median"], share_outside_inference=_stats(shares),
                run_scenes_s=_stats(fwd, unit="s"), run_scenes_views_per_s=B * V / float(np.median(fwd)),
                global_mean=float(np.mean(res[0].global_)), precision=str(dec.precision))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="*", default=[8, 28])
    ap.add_argument("--evaluate-scenes", type=int, nargs="*", default=[8])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--yardstick-rounds", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true", help="figure (a) alone, e.g. under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    f = open(args.out, "a") if args.out else None
    for B in args.scenes:
        b = make_batch(B)
        rec = dict(figure="metrics", scenes=B, views=V, H=H, W=W, pixels=B * V * H * W, kernels=bench_kernels(b, args))
        if not args.kernels_only:
            rec["metric_stage"] = bench_metric_stage(b, args)
        _emit(rec, f)
        del b
        torch.cuda.empty_cache()
    if not args.kernels_only:
        for B in args.evaluate_scenes:
            _emit(dict(figure="evaluate", scenes=B, views=V, H=H, W=W, **bench_evaluate(B, args)), f)


if __name__ == "__main__":
    main()
