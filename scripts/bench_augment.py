"""The training augmentation on the device (csrc/train_augment.hip; must3r_amd.train_augment) beside the host path it replaces, on one GPU in one run.  One
JSON line per run (append it to profiles/augment_bench.jsonl).

The workload is one training batch: ``--scenes`` x ``--views`` views (28 x 10), raw frames of ``--height`` x ``--width`` (1168 x 1752) with fp32 depth, every third
one portrait, already resident on the device as uint8 (as after a decoder), to 512 x 384 with ``aug_crop`` 16 and ColorJitter(0.5, 0.5, 0.5, 0.1) on.

  (a) ``train_augment.augment_views`` on the batch: host clock around a synchronise -- the geometry chain of every view on the host, the tables, the launches.
  (b) its launches one by one between device events, on the tables of the same batch: ``must3r_hip_resample`` (one call, PIL_LANCZOS: every frame shrinks),
      ``must3r_hip_augment_color`` (two passes: jitter on means contrast, hence the sums pass) and ``must3r_hip_augment_depth``, each through its C entry point on
      a table, scratch and outputs prepared beforehand (the entry point's own host work -- checks, device table, upload -- is inside its interval), beside the
      bytes it has to move as a fraction of the 6.3 TB/s the project uses for a float4 copy.  Counted: resample 3 bytes per pixel of the first crop in and 12
      per output pixel out (the intermediate between its two passes is not counted); colour 12 in per pass and 12 out: 36; depth 4 in and 4 out.
  (c) the same batch through tests/augment_ref.py's Pillow path (``view_ref``: crop, resize, ImageEnhance, HSV, ImgNorm, the depth gather in numpy) on
      ``--threads`` host threads (16), then the stack and upload of its results.  This stands in for the reference's loader; the frames start on the host there.

Forms alternated inside every round; ``warmup`` runs, then ``rounds`` rounds: median, min and max.  Clocks are not pinned and the machine is shared.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_ref as AR  # noqa: E402
from must3r_amd import _lib, image as IM, train_augment as TA  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12


def _stats(xs, **kw):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), rounds=len(xs), **kw)


def _batch(args):
    g = torch.Generator(device=DEV).manual_seed(0)
    frames, depths, Ks = [], [], []
    for v in range(args.scenes * args.views):
        H, W = (args.width, args.height) if v % 3 == 2 else (args.height, args.width)
        frames.append(torch.randint(0, 256, (H, W, 3), generator=g, device=DEV, dtype=torch.uint8))
        d = 0.5 + 4.5 * torch.rand((H, W), generator=g, device=DEV)
        d[: H // 4][d[: H // 4] > 4.5] = -1.0
        depths.append(d)
        sign = -1.0 if v % 2 else 1.0
        Ks.append(np.array([[0.9 * max(H, W), 0.0, W / 2 + sign * 0.06 * W], [0.0, 0.9 * max(H, W), H / 2 - sign * 0.04 * H], [0.0, 0.0, 1.0]]))
    gen = torch.Generator().manual_seed(1)
    jps = [TA.get_jitter_params(0.5, 0.5, 0.5, 0.1, generator=gen) for _ in frames]
    return frames, depths, Ks, jps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=28)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--height", type=int, default=1168)
    ap.add_argument("--width", type=int, default=1752)
    ap.add_argument("--aug-crop", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-host", action="store_true", help="without figure (c), e.g. under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs a GPU (no CPU fallback)")
    res = (512, 384)
    frames, depths, Ks, jps = _batch(args)
    V = len(frames)

    def native():
        return TA.augment_views(frames, depths, Ks, res, rng=np.random.default_rng(2), aug_crop=args.aug_crop, jitter_params=jps)

    # (b): the tables of the same batch, the launches between events
    rng = np.random.default_rng(2)
    geoms = [TA.crop_resize_geometry(f.shape[1], f.shape[0], K, res, rng, args.aug_crop) for f, K in zip(frames, Ks)]
    Hs, Ws = TA.stored_shape(geoms)
    assert {g.mode for g in geoms} == {_lib.RESAMPLE_PIL_LANCZOS}
    descs, views, off = [], [], 0
    for f, g, jp in zip(frames, geoms, jps):
        H, W = int(f.shape[0]), int(f.shape[1])
        w, h = g.out
        descs.append(IM._desc(f, _lib.IMG_U8_HWC, 3, H, W, W * 3, 0, (g.crop1[1], g.crop1[0], g.size1[1], g.size1[0]), (g.resized[1], g.resized[0]),
                              (g.window[1], g.window[0], h, w), off))
        views.append(dict(offset=off, h=h, w=w, portrait=g.portrait, order=jp[0], factors=jp[1], flags=(1, 1, 1, 1)))
        off += 3 * h * w
    mid = torch.empty((off,), dtype=torch.float32, device=DEV)
    img = torch.empty((V, 3, Hs, Ws), dtype=torch.float32, device=DEV)
    dep = torch.empty((V, Hs, Ws), dtype=torch.float32, device=DEV)
    P = V * Hs * Ws
    lib = _lib.load()
    arr = (_lib.ImageDesc * V)(*descs)
    nbytes = lib.must3r_hip_image_scratch_bytes(_lib.RESAMPLE_PIL_LANCZOS, arr, V)
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    stream = _lib.stream_ptr(torch.device(DEV))
    color, depth = TA.prepare_color(mid, views, Hs, Ws, out=img), TA.prepare_depth(depths, geoms, Hs, Ws, out=dep)
    launches = dict(resample_pil_lanczos=(lambda: _lib.check(lib.must3r_hip_resample(_lib.RESAMPLE_PIL_LANCZOS, arr, V, mid.data_ptr(), scratch.data_ptr(), nbytes,
                                                                                     stream)),
                                          float(sum(3 * g.size1[0] * g.size1[1] for g in geoms) + 12 * P)),
                    augment_color=(color.run, 36.0 * P), augment_depth=(depth.run, 8.0 * P))

    # (c): the host path
    host = None
    if not args.no_host:
        host = [(f.cpu().numpy(), d.cpu().numpy()) for f, d in zip(frames, depths)]
        pool = ThreadPoolExecutor(args.threads)

    def pillow():
        rng = np.random.default_rng(2)
        seeds = [np.random.default_rng(rng.integers(1 << 31)) for _ in range(V)]      # a generator per view: the threads draw independently
        out = list(pool.map(lambda i: AR.view_ref(host[i][0], host[i][1], Ks[i], res, seeds[i], args.aug_crop, (jps[i][0], jps[i][1], (1, 1, 1, 1)), True),
                            range(V)))
        t1 = time.perf_counter()
        up = [torch.stack([o[k] for o in out]).to(DEV) for k in ("img", "depthmap", "camera_intrinsics", "true_shape")]
        torch.cuda.synchronize()
        return up, time.perf_counter() - t1

    total, upload, host_s = [], [], []
    us = {k: [] for k in launches}
    for r in range(args.warmup + args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        native()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        if r >= args.warmup:
            total.append(t)
        for name, (call, _) in launches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                us[name].append(e0.elapsed_time(e1) * 1e3)
        if host is not None:
            t0 = time.perf_counter()
            _, up_s = pillow()
            t = time.perf_counter() - t0
            if r >= args.warmup:
                host_s.append(t)
                upload.append(up_s)
    rec = dict(figure="augment", scenes=args.scenes, views=args.views, raw_H=args.height, raw_W=args.width, portrait_views=sum(g.portrait for g in geoms),
               Hs=Hs, Ws=Ws, aug_crop=args.aug_crop, jitter="ColorJitter(0.5, 0.5, 0.5, 0.1), all four operations on every view",
               conditions="clocks not pinned, shared machine; medians with min and max; forms alternated inside every round; (a), (c) host clock around a "
                          "synchronise, (b) device events around each entry point on preallocated outputs; no counters were taken")
    rec["native_augment_views"] = _stats(total, unit="s")
    rec["launches"] = {}
    for name, (_, nbytes) in launches.items():
        st = _stats(us[name], unit="us")
        rec["launches"][name] = dict(bytes=nbytes, us=st, fraction_of_6p3_TBps=nbytes / (st["median"] * 1e-6) / HBM_BYTES_PER_S,
                                     fraction_of_6p3_TBps_min_max=[nbytes / (st["max"] * 1e-6) / HBM_BYTES_PER_S, nbytes / (st["min"] * 1e-6) / HBM_BYTES_PER_S])
    dev_us = sum(v["us"]["median"] for v in rec["launches"].values())
    rec["launches_sum_us_median"] = dev_us
    rec["resampler_share_of_launches"] = rec["launches"]["resample_pil_lanczos"]["us"]["median"] / dev_us
    if host is not None:
        rec["pillow_path"] = dict(threads=args.threads, total=_stats(host_s, unit="s"), upload_of_results=_stats(upload, unit="s"))
        rec["pillow_over_native_median"] = rec["pillow_path"]["total"]["median"] / rec["native_augment_views"]["median"]
        rec["pillow_beyond_the_spreads"] = rec["pillow_path"]["total"]["min"] > rec["native_augment_views"]["max"]
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
