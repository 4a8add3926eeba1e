"""The ground truth of a training batch from depth on the device (csrc/train_data.hip; must3r_amd.train_data) beside two other routes to the same tensors, and
the cost of the training loop around its parts (must3r_amd.train), on one GPU in one run.  One JSON line per run (append it to
profiles/train_data_bench.jsonl).

  (a) ``must3r_hip_gt_from_depth`` through its C entry point on preallocated buffers, ``--scenes`` x ``--views`` views (28 x 20) of ``--height`` x ``--width``
      (384 x 512), in four forms -- fp32 or uint16 depth, all or half of the views flagged portrait -- alternated inside every round: ``--launches``
      launches between two device events, per launch, and the bytes a form has to move (depth in, pts3d and the two masks out: 18 or 16 bytes a pixel)
      against the 6.3 TB/s the project uses for a float4 copy.  Beside it the fractions the project records for the metrics pass (0.71) and the export
      kernels (0.38), and two launches of the same arithmetic with outputs omitted (the masks alone: 6 bytes a pixel; pts3d alone: 16), which show what
      the stores cost, and torch's fill and copy of the pts3d buffer (stores alone; a plain copy) as the roofs of this run.
  (b) the same formula as torch tensor expressions on the GPU (tests/train_data_ref.py's, on device tensors), host clock around a synchronise.
  (c) the reference's route: ``pts3d``, ``valid_mask`` and ``sky_mask`` built on the host, stacked per view and uploaded as ``losses.Regr3D._inputs`` does.
      The upload is counted; the numpy formula is not (it belongs to the loader's workers).
  (d) one iteration of ``train_one_epoch`` -- one scene of ``--loop-views`` views (10) at the released geometry under ``--amp bf16``, ``mem_dropout=0.1`` --
      beside the sum of its parts measured alone in this run: encoder forward, decoder forward + backward, activation + loss forward + backward, the
      optimizer's two passes.  The difference is what the loop itself costs (the batch's upload and ground truth, ``select_batch``, the logger).  The parent
      of this script has no loop: the figure is a first record, not a comparison.

Timings: ``warmup`` runs, then ``rounds`` rounds: median, min and max.  Clocks are not pinned and the machine is shared: the record says so.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from must3r_amd import _lib, train as T, train_block as TB, train_data as TD, train_dropout as TDrop, train_encoder as TE, train_losses as TL  # noqa: E402
from must3r_amd import train_optim as TO  # noqa: E402
from must3r_amd.inference import concat_preds  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12
RECORDED_FRACTIONS = dict(metrics_loss_pass=0.71, export_kernels=0.38)


def _stats(xs, **kw):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), rounds=len(xs), **kw)


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


def _inputs(V, H, W, g):
    depth = 0.5 + 4.5 * torch.rand((V, H, W), generator=g, device=DEV)
    pick = torch.rand((V, H, W), generator=g, device=DEV)
    depth[pick < 0.1] = 0.0
    depth[pick > 0.95] = -1.0
    f = 0.9 * max(H, W)
    K = torch.tensor([[f, 0.0, W / 2 + 0.3], [0.0, f, H / 2 - 0.2], [0.0, 0.0, 1.0]], device=DEV).repeat(V, 1, 1)
    Q, _ = torch.linalg.qr(torch.randn((V, 3, 3), generator=g, device=DEV))
    pose = torch.eye(4, device=DEV).repeat(V, 1, 1)
    pose[:, :3, :3], pose[:, :3, 3] = Q, torch.randn((V, 3), generator=g, device=DEV)
    raw = (depth.clamp(min=0.0) * 1000.0).round().clamp(0, 65535).to(torch.int32).to(torch.uint16)
    scale = torch.tensor([1000.0, 1.0], device=DEV).repeat(V, 1)
    return depth, raw, scale, K, pose


def bench_kernel(args, depth, raw, scale, K, pose):
    """(a): the four forms alternated inside every round"""
    lib = _lib.load()
    V, H, W = depth.shape
    P = V * H * W
    pts = torch.empty((V, H, W, 3), dtype=torch.float32, device=DEV)
    valid, sky = torch.empty((V, H, W), dtype=torch.uint8, device=DEV), torch.empty((V, H, W), dtype=torch.uint8, device=DEV)
    flags = {"all": torch.ones((V,), dtype=torch.int32, device=DEV), "half": (torch.arange(V, device=DEV) % 2).to(torch.int32)}
    calls, nbytes = {}, {}
    for form, (d, s, per_pixel) in (("fp32", (depth, None, 18)), ("uint16", (raw, scale, 16))):
        for which, fl in flags.items():
            a = _lib.GtArgs()
            a.depth, a.depth_scale, a.K, a.c2w, a.transposed = d.data_ptr(), None if s is None else s.data_ptr(), K.data_ptr(), pose.data_ptr(), fl.data_ptr()
            a.pts3d, a.valid, a.sky = pts.data_ptr(), valid.data_ptr(), sky.data_ptr()
            a.V, a.Hs, a.Ws, a.depth_u16 = V, H, W, int(s is not None)
            a.stream = _lib.stream_ptr(torch.device(DEV))
            name = f"{form}_{which}_flagged"
            calls[name] = (lambda a=a: _lib.check(lib.must3r_hip_gt_from_depth(C.byref(a))))
            nbytes[name] = float(per_pixel) * P
    # the same arithmetic with outputs omitted: what the stores cost (fp32 depth, half of the views flagged)
    for name, keep, per_pixel in (("fp32_half_flagged_masks_only", ("valid", "sky"), 6), ("fp32_half_flagged_pts3d_only", ("pts3d",), 16)):
        a = _lib.GtArgs()
        a.depth, a.K, a.c2w, a.transposed = depth.data_ptr(), K.data_ptr(), pose.data_ptr(), flags["half"].data_ptr()
        for key, t in (("pts3d", pts), ("valid", valid), ("sky", sky)):
            setattr(a, key, t.data_ptr() if key in keep else None)
        a.V, a.Hs, a.Ws, a.depth_u16 = V, H, W, 0
        a.stream = _lib.stream_ptr(torch.device(DEV))
        calls[name] = (lambda a=a: _lib.check(lib.must3r_hip_gt_from_depth(C.byref(a))))
        nbytes[name] = float(per_pixel) * P
    # the write roof beside them: torch's fill of the pts3d buffer, stores alone (12 bytes a pixel), and its copy of it (12 read, 12 written)
    other = torch.empty_like(pts)
    calls["torch_fill_of_pts3d"], nbytes["torch_fill_of_pts3d"] = (lambda: pts.zero_()), 12.0 * P
    calls["torch_copy_of_pts3d"], nbytes["torch_copy_of_pts3d"] = (lambda: other.copy_(pts)), 24.0 * P
    us = {k: [] for k in calls}
    for r in range(args.warmup + args.rounds):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                call()
            e1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                us[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    out = dict(launches_per_round=args.launches, recorded_fractions_of_6p3_TBps=RECORDED_FRACTIONS)
    for name, xs in us.items():
        st = _stats(xs, unit="us per launch")
        out[name] = dict(bytes=nbytes[name], us=st, fraction_of_6p3_TBps=nbytes[name] / (st["median"] * 1e-6) / HBM_BYTES_PER_S,
                         fraction_of_6p3_TBps_min_max=[nbytes[name] / (st["max"] * 1e-6) / HBM_BYTES_PER_S, nbytes[name] / (st["min"] * 1e-6) / HBM_BYTES_PER_S])
    return out


def _torch_formula(depth, K, pose, flags):
    """tests/train_data_ref.py's expressions on device tensors"""
    V, Hs, Ws = depth.shape
    r = torch.arange(Hs, device=DEV).view(1, Hs, 1).expand(V, Hs, Ws)
    c = torch.arange(Ws, device=DEV).view(1, 1, Ws).expand(V, Hs, Ws)
    fl = (flags != 0).view(V, 1, 1)
    u, v = torch.where(fl, r, c), torch.where(fl, c, r)
    k = lambda i, j: K[:, i, j].view(V, 1, 1).to(torch.float64)
    zd = depth.to(torch.float64)
    x = ((u.to(torch.float64) - k(0, 2)) * zd / k(0, 0)).to(torch.float32)
    y = ((v.to(torch.float64) - k(1, 2)) * zd / k(1, 1)).to(torch.float32)
    e = lambda i, j: pose[:, i, j].view(V, 1, 1)
    pts = torch.stack([((e(i, 0) * x + e(i, 1) * y) + e(i, 2) * depth) + e(i, 3) for i in range(3)], dim=-1)
    return pts, (depth > 0) & torch.isfinite(pts).all(dim=-1), depth < 0


def bench_routes(args, depth, K, pose, native):
    """(b) and (c), alternated with the kernel's wrapper in every round"""
    B, n = args.scenes, args.views
    V, H, W = depth.shape
    flags = (torch.arange(V, device=DEV) % 2).to(torch.int32)
    ts = torch.where(flags.view(V, 1) != 0, torch.tensor([[W, H]], device=DEV), torch.tensor([[H, W]], device=DEV)).view(B, n, 2)
    pts, valid, sky = _torch_formula(depth, K, pose, flags)
    same = not bool(((pts.view(torch.int32) != native[0].view(torch.int32)) & ~(pts.isnan() & native[0].isnan())).any())
    same = same and bool(torch.equal(valid, native[1].bool())) and bool(torch.equal(sky, native[2].bool()))
    host = [dict(pts3d=pts.view(B, n, H, W, 3)[:, i].cpu(), valid_mask=valid.view(B, n, H, W)[:, i].cpu(), sky_mask=sky.view(B, n, H, W)[:, i].cpu())
            for i in range(n)]
    del pts, valid, sky
    d4, K4, p4 = depth.view(B, n, H, W), K.view(B, n, 3, 3), pose.view(B, n, 4, 4)

    def wrapper():
        TD.ground_truth(d4, K4, p4, ts)

    def formula():
        _torch_formula(depth, K, pose, flags)

    def upload():
        for key in ("pts3d", "valid_mask", "sky_mask"):
            torch.stack([b[key] for b in host], dim=1).to(DEV)
    fns = dict(native_wrapper=wrapper, torch_expressions=formula, host_built_stack_and_upload=upload)
    secs = {k: [] for k in fns}
    for r in range(args.warmup + args.rounds):
        for name, fn in fns.items():
            s = _wall(fn, 1, 0)
            if r >= args.warmup:
                secs[name] += s
    out = {k: _stats(v, unit="s") for k, v in secs.items()}
    out["torch_expressions_equal_the_kernels_bits"] = same
    out["upload_bytes"] = 14.0 * V * H * W
    for k in ("torch_expressions", "host_built_stack_and_upload"):
        out[f"{k}_over_native_median"] = out[k]["median"] / out["native_wrapper"]["median"]
        out[f"{k}_beyond_the_spreads"] = out[k]["min"] > out["native_wrapper"]["max"]
    return out


class _Features:
    """an encoder that hands out what it was given: the decoder's share of a step alone"""

    def __init__(self, x, pos):
        self.x, self.pos = x, pos

    def __call__(self, img, true_shape):
        return self.x, self.pos


def bench_loop(args):
    """(d)"""
    n, H, W = args.loop_views, args.height, args.width
    torch.manual_seed(0)
    enc = TE.Dust3rEncoder(img_size=(H, W), embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, patch_embed="ManyAR_PatchEmbed").to(DEV)
    dec = TDrop.CausalMUSt3R(landscape_only=True, mem_dropout=0.1, enc_embed_dim=1024, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0,
                             feedback_type="single_mlp", memory_mode="norm_y").to(DEV)
    a = T.get_args_parser().parse_args(["--dataset", "SyntheticDepthScenes", "--amp", "bf16", "--accum_iter", "1", "--lr", "1e-5", "--print_freq", "1000",
                                        "--epochs", "100", "--warmup_epochs", "1"])
    crit = eval(a.criterion, vars(TL) | {"args": a})
    opt = TO.AdamW(TO.get_parameter_groups(dec, enc.depth, a.weight_decay), lr=a.lr, betas=(0.9, 0.95))
    scaler = TO.LossScaler()
    from torch.utils.data import DataLoader
    batch = next(iter(DataLoader(TD.SyntheticDepthScenes(1, n, H, W, seed=1, portrait_every=4, memory_num_views=n // 2), batch_size=1)))

    def loop():
        T.train_one_epoch(enc, dec, crit, [batch], opt, DEV, 1, scaler, a)
    loop_s = _wall(loop, args.rounds, args.warmup)
    # the parts, on the tensors of the same iteration
    imgs, ts, gt = TD.collate_views(batch, DEV)
    rng = np.random.default_rng(a.seed + 1)
    imgs, ts, mnv, to_skip, to_render, skip_batches, mem_batches = T.select_batch(DEV, a, rng, int(batch[0]["memory_num_views"][0]), 1 / a.epochs, imgs, ts, n)
    assert to_skip == 0 and to_render is None

    def encoder():
        with torch.no_grad(), TB.amp("bf16"):
            return enc(imgs.view(n, 3, H, W), ts.view(n, 2))
    x, pos = encoder()
    feats = _Features(x, pos)
    with TB.amp("bf16"):
        p0, pts = TE.inference(feats, dec, imgs, ts, mem_batches)
    G0, G = torch.randn_like(p0) * 1e-7, torch.randn_like(pts) * 1e-7

    def decoder():
        dec.zero_grad(set_to_none=True)
        with TB.amp("bf16"):
            q0, q = TE.inference(feats, dec, imgs, ts, mem_batches)
        torch.autograd.backward([q0, q], [G0, G])
    raw0, raw = p0.detach().clone().requires_grad_(True), pts.detach().clone().requires_grad_(True)
    truth = list(gt[:mnv]) + list(gt)

    def loss():
        raw0.grad = raw.grad = None
        pred = concat_preds(TL.postprocess(raw0, "norm_exp"), TL.postprocess(raw, "norm_exp"))
        crit(truth, pred)[0].backward()
    decoder()

    def optimizer():
        opt.step(control=opt.grad_norm(scaler=scaler))
    parts = dict(encoder_forward=encoder, decoder_forward_backward=decoder, activation_loss_forward_backward=loss, optimizer_norm_and_step=optimizer)
    out = {k: _stats(_wall(fn, args.rounds, args.warmup), unit="s") for k, fn in parts.items()}
    total = sum(v["median"] for v in out.values())
    out.update(loop_iteration=_stats(loop_s, unit="s"), sum_of_parts_median=total, mem_batches=[int(m) for m in mem_batches], views=n,
               geometry="encoder D 1024 / 16 heads / 24 layers, decoder D 768 / 12 heads / 12 layers, amp bf16, mem_dropout 0.1, decoder trained")
    out["loop_minus_parts_median"] = out["loop_iteration"]["median"] - total
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=28)
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--loop-views", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true", help="figure (a) alone, e.g. under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--no-loop", action="store_true", help="without figure (d)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_data: needs a GPU (no CPU fallback)")
    V, H, W = args.scenes * args.views, args.height, args.width
    g = torch.Generator(device=DEV).manual_seed(0)
    depth, raw, scale, K, pose = _inputs(V, H, W, g)
    rec = dict(figure="train_data", scenes=args.scenes, views=args.views, H=H, W=W, pixels=V * H * W,
               conditions="clocks not pinned, shared machine; medians with min and max; forms alternated inside every round; (a) device events around the C "
                          "entry point on preallocated buffers, (b)-(d) host clock around a synchronise")
    rec["kernel"] = bench_kernel(args, depth, raw, scale, K, pose)
    print(json.dumps(dict(kernel=rec["kernel"])), file=sys.stderr, flush=True)          # progress; the record is the one line on stdout
    if not args.kernel_only:
        flags = (torch.arange(V, device=DEV) % 2).to(torch.int32)
        native = TD.gt_from_depth(depth, K, pose, flags)[:3]
        rec["routes"] = bench_routes(args, depth, K, pose, native)
        print(json.dumps(dict(routes=rec["routes"])), file=sys.stderr, flush=True)
        del native
        if not args.no_loop:
            del depth, raw
            torch.cuda.empty_cache()
            rec["loop"] = bench_loop(args)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
