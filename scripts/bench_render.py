"""Scene rendering (csrc/render.hip; must3r_amd.render.SceneRenderer) against two other forms of the same arithmetic on the same tensors.  One JSON
line per case (append them to profiles/render_bench.jsonl).

Scenes: 200 views of 384 x 512 (39.3 M points, the export's benchmark size) and one view; points uniform in the cube [-1, 1]^3, conf = 1 + exp(randn),
threshold 1.05 (nearly every point is kept: the heaviest case for the z-buffer).  Cases: a 512 x 384 target, one camera and a batch of 120 orbit cameras,
point sizes 1 and 4.

  hip     SceneRenderer.render: all cameras in one native call per scratch chunk, device events around the call (memset of the keys, splat, resolve)
  torch   the composed form: the same projection as fp64 tensor expressions, then scatter_reduce_(..., "amin") on int64 keys, camera after camera
  numpy   the restatement tests/render_ref.py, the views spread over 16 host threads, for ONE camera only (the yardstick of what a host would do)

hip and torch alternate inside every round, so drift hits both; `rounds` rounds after `warmup`: median, min and max (a torch form that takes more than
--slow-form-s per run is timed in the first 3 rounds only; its `rounds` field says so).  The images of hip and torch are
compared once per case (bit-equal index and depth).  bytes_read is what the splat has to read once (conf and points, 16 bytes per source pixel); its rate
against 6.3 TB/s is a lower bound for the splat launch, because the time is the whole call's.  Per-kernel times: run with --hip-only under
`rocprofv3 --kernel-trace --stats` (a separate run).
"""
import argparse
import concurrent.futures
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_ref as RR  # noqa: E402
from must3r_amd import render as Rn  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12
THR = 1.05
W, H = 512, 384
I64_MAX = torch.iinfo(torch.int64).max


def _stats(xs, **kw):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), rounds=len(xs), **kw)


def _emit(rec, f):
    line = json.dumps(rec)
    print(line, flush=True)
    if f:
        f.write(line + "\n")
        f.flush()


def make_views(V):
    g = torch.Generator(device=DEV).manual_seed(0)
    conf = 1.0 + torch.exp(torch.randn((V, 384, 512), generator=g, device=DEV))
    pts = torch.rand((V, 384, 512, 3), generator=g, device=DEV) * 2 - 1
    rgb = torch.rand((V, 384, 512, 3), generator=g, device=DEV)
    return conf, pts, rgb


def torch_form(conf, pts, cam, thr, ps):
    """-> (depth fp32 [H, W] with +inf where empty, index int64 [H, W] with -1 there) of one camera; identity view matrices, so A = w2c"""
    A = torch.as_tensor(np.asarray(cam.w2c, dtype=np.float64), device=DEV)
    c, p = conf.reshape(-1), pts.reshape(-1, 3)
    x, y, z = (p[:, a].double() for a in range(3))
    X = [((A[a, 0] * x + A[a, 1] * y) + A[a, 2] * z) + A[a, 3] for a in range(3)]
    Z = X[2]
    iz = 1.0 / Z
    u, v = cam.fx * (X[0] * iz) + cam.cx, cam.fy * (X[1] * iz) + cam.cy
    half = 0.5 * (ps - 1)
    c0, r0 = torch.floor(u - half), torch.floor(v - half)
    keep = (c >= thr) & torch.isfinite(p).all(dim=1) & torch.isfinite(u) & torch.isfinite(v) & (Z >= float(np.float32(cam.z_near))) & (Z <= float(np.float32(cam.z_far)))
    keep &= (c0 < cam.W) & (c0 + ps > 0) & (r0 < cam.H) & (r0 + ps > 0)
    idx = keep.nonzero().squeeze(1)
    key = (Z[idx].float().view(torch.int32).long() << 32) | idx           # Z > 0: the int32 view is positive and orders as the value does
    c0, r0 = c0[idx].long(), r0[idx].long()
    zbuf = torch.full((cam.H * cam.W,), I64_MAX, dtype=torch.int64, device=DEV)
    for dr in range(ps):
        for dc in range(ps):
            r, q = r0 + dr, c0 + dc
            ok = (r >= 0) & (r < cam.H) & (q >= 0) & (q < cam.W)
            zbuf.scatter_reduce_(0, (r * cam.W + q)[ok], key[ok], "amin")
    hit = zbuf != I64_MAX
    depth = torch.where(hit, (zbuf >> 32).to(torch.int32).view(torch.float32), torch.full_like(zbuf, float("inf"), dtype=torch.float32))
    index = torch.where(hit, zbuf & 0xFFFFFFFF, torch.full_like(zbuf, -1))
    return depth.view(cam.H, cam.W), index.view(cam.H, cam.W)


def numpy_form(views, cam, thr, ps, threads=16):
    """the restatement with the views spread over `threads` host threads: a z-buffer per view, then the minimum over them"""
    bases = np.cumsum([0] + [v[0].size for v in views])

    def one(i):
        pix, keys, _ = RR.contenders([views[i]], RR.identity(1), cam, thr, ps)
        part = np.full(cam.H * cam.W, RR.EMPTY, dtype=np.uint64)
        np.minimum.at(part, pix, keys + np.uint64(bases[i]))
        return part

    with concurrent.futures.ThreadPoolExecutor(threads) as pool:
        zbuf = np.full(cam.H * cam.W, RR.EMPTY, dtype=np.uint64)
        for part in pool.map(one, range(len(views))):
            np.minimum(zbuf, part, out=zbuf)
    return zbuf


def _index64(index):
    """uint32 with 0xFFFFFFFF for empty -> int64 with -1 there"""
    i32 = index.view(torch.int32)
    return torch.where(i32 == -1, -1, i32.long() & 0xFFFFFFFF)


def _events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def bench_case(V, tensors, renderer, cams, ps, args, f):
    conf, pts, _ = tensors
    n_pix = conf.numel()
    rec = dict(figure="render", views=V, pixels=n_pix, target=[W, H], cameras=len(cams), point_size=ps, thr=THR)
    hip = lambda: renderer.render(cams, THR, ps)                                 # noqa: E731
    tor = lambda: [torch_form(conf, pts, c, THR, ps) for c in cams]              # noqa: E731
    torch_rounds = args.rounds
    for _ in range(args.warmup):
        images = hip()
        if not args.hip_only:
            t0 = time.perf_counter()
            ref = tor()
            torch.cuda.synchronize()
            if time.perf_counter() - t0 > args.slow_form_s:      # a slow composed form is timed in fewer rounds; its `rounds` field says so
                torch_rounds = min(args.rounds, 3)
    torch.cuda.synchronize()
    if not args.hip_only:
        same = all(torch.equal(im["depth"], d) and torch.equal(_index64(im["index"]), i) for im, (d, i) in zip(images, ref))
        rec["hip_equals_torch_form"] = bool(same)
        del ref
    rec["covered_share"] = float(np.mean([float((im["index"].view(torch.int32) != -1).float().mean()) for im in images]))
    del images
    ms_hip, ms_torch = [], []
    for r in range(args.rounds):
        ms_hip.append(_events(hip)[0])
        if not args.hip_only and r < torch_rounds:
            ms_torch.append(_events(tor)[0])
    rec["hip_ms"] = _stats(ms_hip, unit="ms")
    rec["bytes_read"] = 16 * n_pix
    rec["hip_read_rate_fraction_of_6p3_TBps"] = 16 * n_pix / (rec["hip_ms"]["median"] * 1e-3) / HBM_BYTES_PER_S
    if not args.hip_only:
        rec["torch_ms"] = _stats(ms_torch, unit="ms")
        rec["torch_over_hip_median"] = rec["torch_ms"]["median"] / rec["hip_ms"]["median"]
        # a difference counts only beyond the spreads
        rec["hip_faster_beyond_spreads"] = rec["hip_ms"]["max"] < rec["torch_ms"]["min"]
    if len(cams) == 1 and not args.hip_only and args.numpy_rounds > 0:
        views = [(conf[i].cpu().numpy(), pts[i].cpu().numpy(), None) for i in range(V)]
        secs = []
        for _ in range(args.numpy_rounds):
            t0 = time.perf_counter()
            zbuf = numpy_form(views, cams[0], THR, ps)
            secs.append(time.perf_counter() - t0)
        got = renderer.render(cams, THR, ps, want=("index",))[0]["index"].cpu().numpy().reshape(-1)
        rec["hip_equals_numpy_form"] = bool(np.array_equal(got, (zbuf & np.uint64(0xFFFFFFFF)).astype(np.uint32)))
        rec["numpy_16_threads_s"] = _stats(secs, unit="s")
    _emit(rec, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="*", default=[200, 1])
    ap.add_argument("--cameras", type=int, nargs="*", default=[1, 120])
    ap.add_argument("--point-sizes", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--numpy-rounds", type=int, default=2)
    ap.add_argument("--slow-form-s", type=float, default=4.0, help="a torch form slower than this per run is timed in 3 rounds")
    ap.add_argument("--hip-only", action="store_true", help="the native form alone, e.g. under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    f = open(args.out, "a") if args.out else None
    orbit = Rn.orbit_box(np.full(3, -1.0), np.full(3, 1.0), np.eye(4), 120, W, H)
    for V in args.views:
        tensors = make_views(V)
        renderer = Rn.SceneRenderer([(tensors[0][i], tensors[1][i], tensors[2][i]) for i in range(V)], None, device=DEV)
        for n in args.cameras:
            for ps in args.point_sizes:
                bench_case(V, tensors, renderer, orbit[:n], ps, args, f)
        del renderer, tensors
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
