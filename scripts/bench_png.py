"""The PNG decoder on the device (csrc/png.hip; must3r_amd.png) beside Pillow on the host, on one GPU and the same machine in one run.  One JSON line per
workload (append them to profiles/png_bench.jsonl; ``--out`` does).

Two workloads, both encoded by Pillow at its default level:

  depth  ``--depth-frames`` (280) 16-bit grey 1168 x 1752 files.  The generator: millimetres of a smooth surface, ``2000 + 1500 * sin(x / 211 + 0.1 i) *
         cos(y / 173) + 0.5 * x``, plus uniform noise in the low three bits, with 2 % of the pixels in holes (rectangles of 24 x 16 set to 0), seeded per frame.
         Decoded by ``png.decode_gray``.
  rgb    ``--rgb-frames`` (200) RGB 1920 x 1080 files: tests/jpeg_ref.py's synthetic field plus noise, shifted per frame.  Decoded by ``png.decode_images`` in
         chunks of ``image.LOAD_CHUNK_BYTES`` (the default) and in one call.

Per workload, alternated inside every round: (a) the native batch -- parse, pinned upload of the IDAT bytes, the launches; host clock around a synchronise;
(b) Pillow on 1 host thread and on ``--threads`` (16), then the pinned asynchronous upload of every frame and one synchronise: upload included on both sides;
(c) one file alone through (a), its result waited for: the latency; (d) one round of (a) under torch's profiler: device time per kernel.

``warmup`` runs, then ``rounds`` rounds: median, min and max.  Clocks are not pinned and the machine is shared.
"""
import argparse
import io
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
import jpeg_ref as R  # noqa: E402
from must3r_amd import png  # noqa: E402

DEV = "cuda:0"


def _stats(xs, **kw):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)), rounds=len(xs), **kw)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def depth_frame(i, w=1752, h=1168):
    rng = np.random.default_rng(1000 + i)
    yy, xx = np.mgrid[0:h, 0:w]
    d = 2000 + 1500 * np.sin(xx / 211 + 0.1 * i) * np.cos(yy / 173) + 0.5 * xx + rng.integers(0, 8, (h, w))
    d = d.astype(np.uint16)
    for _ in range(int(0.02 * w * h / (24 * 16))):
        x, y = int(rng.integers(0, w - 24)), int(rng.integers(0, h - 16))
        d[y:y + 16, x:x + 24] = 0
    return d


def _encode(arr):
    import PIL.Image
    buf = io.BytesIO()
    PIL.Image.fromarray(arr).save(buf, "PNG")
    return buf.getvalue()


def _pillow_one(args):
    import PIL.Image
    data, rgb = args
    im = PIL.Image.open(io.BytesIO(data))
    if rgb:
        im = im.convert("RGB")
    im.load()
    return np.asarray(im)


def measure(name, datas, rgb, native_forms, args, pool):
    dev = torch.device(DEV)
    want = _pillow_one((datas[3 % len(datas)], rgb))
    png.reset_path_record()
    (got,) = (png.decode_images if rgb else png.decode_gray)([datas[3 % len(datas)]], DEV, check=True)
    got = got.cpu().numpy() if rgb else got.cpu().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want), "the decoder is not bit-equal to Pillow on this workload"

    def pillow(threads):
        arrs = list(pool.map(_pillow_one, [(d, rgb) for d in datas])) if threads > 1 else [_pillow_one((d, rgb)) for d in datas]
        return [png._upload(a, dev) for a in arrs]

    single = (lambda d: png.decode_images([d], DEV)) if rgb else (lambda d: png.decode_gray([d], DEV))
    t = {k: [] for k in (*native_forms, "pillow_1", "pillow_n", "single")}
    for r in range(args.warmup + args.rounds):
        row = {k: _timed(fn) for k, fn in native_forms.items()}
        row.update(pillow_n=_timed(lambda: pillow(args.threads)), single=_timed(lambda: single(datas[r % len(datas)])), pillow_1=_timed(lambda: pillow(1)))
        if r >= args.warmup:
            for k, v in row.items():
                t[k].append(v)
    kernels = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            next(iter(native_forms.values()))()
            torch.cuda.synchronize()
        kernels = {}
        for e in prof.key_averages():
            us = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
            if "png_" in e.key and us:
                kernels[e.key.split("(")[0].split("::")[-1]] = dict(us=float(us), calls=int(e.count))
        kernels = kernels or None
    except Exception as e:      # noqa: BLE001
        kernels = dict(error=repr(e))
    n = len(datas)
    info = png.probe(datas[0])
    rec = dict(figure="png_decode", workload=name, frames=n, width=info["width"], height=info["height"], mode=info["mode"],
               file_bytes_mean=float(np.mean([len(d) for d in datas])), inflated_bytes=info["inflated_bytes"], host_threads=args.threads, paths=png.path_record(),
               conditions="clocks not pinned, shared machine; medians with min and max; forms alternated inside every round; host clock around a synchronise; "
                          "upload included on both sides; Pillow on this machine's CPU",
               pillow_1_thread=_stats(t["pillow_1"], unit="s"), pillow_n_threads=_stats(t["pillow_n"], unit="s"), single_file=_stats(t["single"], unit="s"),
               kernels_one_round=kernels)
    for k in native_forms:
        rec[k] = _stats(t[k], unit="s")
        rec[k + "_vs_pillow_n_threads"] = ("faster" if rec[k]["max"] < rec["pillow_n_threads"]["min"] else
                                           "slower" if rec[k]["min"] > rec["pillow_n_threads"]["max"] else "the spreads overlap")
    one = [_timed(lambda: _pillow_one((datas[r % n], rgb))) for r in range(args.rounds)]
    rec["pillow_single_file"] = _stats(one, unit="s")
    rec["single_file_vs_pillow"] = ("faster" if rec["single_file"]["max"] < min(one) else "slower" if rec["single_file"]["min"] > max(one) else "the spreads overlap")
    rec["frames_per_s"] = {k: n / rec[k]["median"] for k in (*native_forms, "pillow_1_thread", "pillow_n_threads")}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth-frames", type=int, default=280)
    ap.add_argument("--rgb-frames", type=int, default=200)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png: needs a GPU (no CPU fallback)")
    pool = ThreadPoolExecutor(args.threads)
    lines = []
    if args.depth_frames:
        datas = list(pool.map(lambda i: _encode(depth_frame(i)), range(args.depth_frames)))
        lines.append(json.dumps(measure("depth", datas, False, dict(native_batch=lambda: png.decode_gray(datas, DEV)), args, pool)))
        print(lines[-1], flush=True)
    if args.rgb_frames:
        base = [R.synthetic(1920, 1080, 10 + i, noise=6.0) for i in range(4)]
        rgbs = list(pool.map(lambda i: _encode(np.roll(base[i % 4], (7 * i, 13 * i), (0, 1))), range(args.rgb_frames)))
        forms = dict(native_batch=lambda: png.decode_images(rgbs, DEV, chunk_bytes=2 << 30), native_default_chunks=lambda: png.decode_images(rgbs, DEV))
        lines.append(json.dumps(measure("rgb", rgbs, True, forms, args, pool)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
